"""csrc/fft_loss.hip -- srk_fft_loss_fwd_bwd, the frequency loss (L1 of the rfft2 half spectrum, value and gradient) -- through the C ABI
on guarded memory, and what is built on it: ops.fft_loss_fwd_bwd, training.make_loss(fft_weight=...), a graphed HAT step and the
finetune_swinir flags.  The fp64 reference is tests/fft_loss_ref.py, pinned to torch in tests/test_fft_loss_ref.py.

Bounds (u = 2^-24; the kernel as built: every product is a k-ordered fmaf chain on the fp32-input MFMA, steps padded with exact zeros).

  forward, per component of D of one plane:  tau = 2 K u sum_plane |d|,  K = W + 2 H.
    Stage 1 is a chain of W fmaf over x with twiddles rounded once (relative u): |err T[y][v]| <= (W + 1) u sum_x |d[y][x]|; d itself
    carries the u of the fp32 subtraction.  Stage 2 is a chain of 2 H over y of |twiddle| <= 1 times T:
    |err D| <= (2 H + 1) u sum_y |T| + sum_y |err T| <= (W + 2 H + 3) u sum_plane |d| <= tau (W + 2 H >= 3).
    The inputs of the bounded cases keep every component outside the structural bins further than tau from zero (asserted on the
    reference, allowed count 0), so every sign the kernel takes is the reference's and G is exact.
  gradient, per element:  2 K' u s / N * sum_plane (|G_re| + |G_im|) + 4 u max|g|,  K' = 2 H + 2 Wh + 2.
    Stage 3 (chain 2 H over u, twiddles rounded once): |err P_re| + |err P_im| <= (2 H + 1) u sqrt(2) sum_u (|G_re| + |G_im|) for one v.
    Stage 4 (chain 2 Wh over v): |err g| <= sum_v [(2 Wh + 1) u (|P_re| + |P_im|) + |err P_re| + |err P_im|] with
    |P_re| + |P_im| <= sqrt(2) sum_u (|G_re| + |G_im|): together sqrt(2) (2 H + 2 Wh + 2) u sum_plane, below 2 K' u sum_plane.  The
    coefficient alpha s / N is rounded once and multiplied once: 2 u of the entry; 4 u leaves room for the compounding.
  value:  s * mean_plane(tau) + 2 Ks u L,  Ks = 33 + 6 + ceil(P / 256) + 8 + 2.
    Every one of the N components is off by at most its plane's tau; the sum is a chain of a lane's 2 x 16 accumulators (one addition
    inside each term), the wave butterfly 6, a finishing thread's ceil(P / 256) of the P per-wave partials, its butterfly 6 and four
    waves 2, the multiplication by the rounded s / N.

Worst ratios error / bound are printed per case (pytest -s) and recorded in DESIGN.md 7s."""
import functools
import math

import pytest
import torch

import fft_loss_ref as R
from guarded import Guarded

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
E_SHAPE, E_NULL, E_UNSUPPORTED = -1, -2, -3
PAD = 4096          # NaN floats before and after every operand and the workspace


def _lib():
    from tpu_superresolution_amd._lib import lib
    return lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


class Padded:
    """n floats on the device with PAD quiet NaNs on either side (an operand: a read past its ends poisons the result; the workspace:
    a write past its ends is seen)"""

    def __init__(self, n, fill=None):
        self.n = n
        self.raw = torch.full((n + 2 * PAD,), float("nan"), dtype=torch.float32, device="cuda")
        if fill is not None:
            self.raw[PAD:PAD + n] = fill.reshape(-1).float().cuda()
        self.before = self.raw.clone()

    @property
    def ptr(self):
        return self.raw.data_ptr() + 4 * PAD

    def assert_guards(self, what):
        a, b = self.raw.view(torch.int32), self.before.view(torch.int32)
        assert torch.equal(a[:PAD], b[:PAD]) and torch.equal(a[PAD + self.n:], b[PAD + self.n:]), f"{what}: written outside its {self.n} floats"


def _ws_floats(shape):
    B, C, H, W = shape
    Wh = W // 2 + 1
    tiles = -(-H // 64) * -(-Wh // 32)          # one partial per stage-2 wave: 64 rows u x 32 columns v
    return 2 * H + 2 * W + B * C * tiles + B * C * H * W + 4 * B * C * H * Wh


def _call(x, y, shape, dptr, ortho=0, alpha=1.0, accumulate=0, value=None, loss=None, ws=None):
    B, C, H, W = shape
    ptr = lambda t: t if t is None or isinstance(t, int) else (t.ptr if isinstance(t, (Padded, Guarded)) else t.data_ptr())          # noqa: E731
    if ws is None:
        ws = Padded(int(_lib().srk_fft_loss_workspace(B, C, H, W)) // 4)
    rc = _lib().srk_fft_loss_fwd_bwd(ptr(x), ptr(y), ptr(ws), B, C, H, W, ortho, alpha, ptr(dptr), accumulate, ptr(value), ptr(loss), _stream())
    if isinstance(ws, Padded):
        torch.cuda.synchronize()
        ws.assert_guards(f"workspace {shape}")
    return rc


def _coef(shape, norm, alpha=1.0):
    """alpha s / N and s / N as the host forms them: in fp64, rounded once"""
    B, C, H, W = shape
    s = 1.0 / math.sqrt(float(H) * float(W)) if norm == "ortho" else 1.0
    n = 2.0 * B * C * H * (W // 2 + 1)
    return float(torch.tensor(alpha * s / n, dtype=torch.float64).float()), s, n


def _run(pred, target, shape, norm="backward"):
    """overwrite call with alpha 1 on guarded memory -> (d_x fp32 on the host, value fp32 [1] on the host)"""
    B, C, H, W = shape
    assert int(_lib().srk_fft_loss_workspace(B, C, H, W)) == 4 * _ws_floats(shape)
    x, y = Padded(pred.numel(), pred), Padded(target.numel(), target)
    out = Guarded("f32", B * C * H, W, W)
    value = torch.full((1,), float("nan"), device="cuda")
    assert _call(x, y, shape, out, int(norm == "ortho"), value=value) == 0
    out.assert_guards(f"fft loss {shape}")
    return out.data().view(shape), value.cpu()


# ---- exact cases ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1, 1, 1), (1, 1, 4, 1), (1, 1, 2, 4), (2, 3, 4, 4)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("norm", R.NORMS)
def test_integer_inputs_are_exact(shape, norm):
    """H, W in {1, 2, 4}: every twiddle is 0 or +-1, so D and the adjoint sum are integers and d_x is one rounded product"""
    g = torch.Generator().manual_seed(sum(shape))
    target = torch.randint(-3, 4, shape, generator=g).float()
    pred = target + torch.randint(-3, 4, shape, generator=g).float()
    got, value = _run(pred, target, shape, norm)
    v64, g64 = R.fft_loss_ref(pred, target, norm)
    coef, s, n = _coef(shape, norm)
    ints = torch.round(g64 * n / s)
    assert float((ints - g64 * n / s).abs().max()) <= 1e-9
    want = (ints.float() * torch.tensor(coef, dtype=torch.float32))          # one fp32 product
    assert torch.equal(got, want), (got, want)          # bit-equal (a zero of either sign is a zero)
    assert abs(float(value) - float(v64)) <= 2 * U * float(v64)


# ---- impulse, identical images ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,a", [((1, 1, 12, 20), 0.75), ((1, 2, 9, 15), -1.5)], ids=["12x20", "9x15"])
def test_impulse_known_answer(shape, a):
    """d = a delta(0, 0): L = |a| / 2 and d_x[y, x] = sign(a) / N * H [y == 0] sum_{v < Wh} cos(2 pi v x / W): Hermitian doubling or a
    wrong range of v changes the row"""
    B, C, H, W = shape
    Wh = W // 2 + 1
    target = torch.rand(shape, generator=torch.Generator().manual_seed(4))
    target[..., 0, 0] = 0.25
    pred = target.clone()
    pred[..., 0, 0] = 0.25 + a
    got, value = _run(pred, target, shape)
    n = 2 * B * C * H * Wh
    x = torch.arange(W, dtype=torch.float64)
    row = sum(torch.cos(2 * math.pi * v * x / W) for v in range(Wh)) * (math.copysign(1.0, a) * H / n)
    want = torch.zeros(shape, dtype=torch.float64)
    want[..., 0, :] = row
    bound = 2 * (2 * H + 2 * Wh + 2) * U * (H * Wh) / n + 4 * U * float(want.abs().max())
    err = float((got.double() - want).abs().max())
    print(f"impulse {shape}: gradient err {err:.3e} / bound {bound:.3e} = {err / bound:.3f}")
    assert err <= bound
    assert abs(float(value) - abs(a) / 2) <= 64 * U * abs(a) / 2


def test_identical_images_give_exact_zeros():
    shape = (2, 3, 12, 20)
    t = torch.rand(shape, generator=torch.Generator().manual_seed(5))
    got, value = _run(t.clone(), t, shape)
    assert float(value) == 0.0 and float(got.abs().max()) == 0.0


# ---- sign-stable inputs: per-element bounds ---------------------------------------------------------------------------------------------
RANDOM = [(s, seed) for s in [(2, 3, 12, 20), (1, 3, 9, 15), (2, 1, 24, 10), (1, 1, 16, 16), (1, 1, 7, 64)] for seed in (0, 1, 2)]
DESIGNED = [(1, 3, 96, 80), (2, 1, 130, 70), (1, 1, 65, 129), (1, 2, 72, 200), (1, 1, 512, 512)]
BOUNDED = [("random", s, seed, "backward") for s, seed in RANDOM] + [("random", (2, 3, 12, 20), 0, "ortho"), ("random", (1, 1, 7, 64), 1, "ortho")] \
    + [("designed", s, 0, "backward") for s in DESIGNED] + [("designed", (2, 1, 130, 70), 0, "ortho")]


@functools.lru_cache(maxsize=None)
def _case(kind, shape, seed, norm):
    """inputs, reference and bounds, computed once"""
    B, C, H, W = shape
    Wh = W // 2 + 1
    pred, target = (R.random_inputs if kind == "random" else R.designed_inputs)(shape, seed)
    v64, g64 = R.fft_loss_ref(pred, target, norm)
    d = pred.double() - target.double()
    re, im = R.spectrum(d)
    tau = 2 * (W + 2 * H) * U * d.abs().sum(dim=(2, 3), keepdim=True)          # per plane
    free = ~R.structural_mask(H, W)
    near = int((re.abs() <= tau).sum()) + int(((im.abs() <= tau) & free).sum())
    margin = min(float((re.abs() / tau).min()), float((im.abs() / tau)[..., free].min()))
    _, s, n = _coef(shape, norm)
    gsum = float((torch.sign(re).abs() + torch.sign(im).abs()).sum(dim=(2, 3)).max())
    gbound = 2 * (2 * H + 2 * Wh + 2) * U * gsum * s / n + 4 * U * float(g64.abs().max())
    parts = B * C * -(-H // 64) * -(-Wh // 32)
    ks = 33 + 6 + -(-parts // 256) + 8 + 2
    vbound = s * float(tau.mean()) + 2 * ks * U * float(v64)
    return pred, target, float(v64), g64, near, margin, gbound, vbound


@pytest.mark.parametrize("kind,shape,seed,norm", BOUNDED, ids=[f"{k}-{'x'.join(map(str, s))}-{seed}-{n}" for k, s, seed, n in BOUNDED])
def test_value_and_gradient_within_the_derived_bounds(kind, shape, seed, norm):
    pred, target, v64, g64, near, margin, gbound, vbound = _case(kind, shape, seed, norm)
    assert near == 0, f"{near} components of the reference spectrum lie within tau of zero (smallest |component| / tau = {margin:.2f})"
    got, value = _run(pred, target, shape, norm)
    err, verr = float((got.double() - g64).abs().max()), abs(float(value) - v64)
    print(f"fft loss {kind} {'x'.join(map(str, shape))} seed {seed} {norm}: min |D| / tau {margin:.1f}; gradient err {err:.3e} / bound "
          f"{gbound:.3e} = {err / gbound:.4f}; value err {verr:.3e} / bound {vbound:.3e} = {verr / vbound:.4f}")
    assert err <= gbound
    assert verr <= vbound


# ---- scaling, accumulation, value only, determinism -------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,norm", [((2, 3, 12, 20), "backward"), ((2, 1, 130, 70), "ortho")], ids=["12x20", "130x70-ortho"])
def test_scaling_accumulation_value_only_determinism(shape, norm):
    kind = "random" if shape[2] == 12 else "designed"
    pred, target = _case(kind, shape, 0, norm)[:2]
    B, C, H, W = shape
    ortho, n = int(norm == "ortho"), pred.numel()
    g1, v1 = _run(pred, target, shape, norm)
    g1b, v1b = _run(pred, target, shape, norm)
    assert torch.equal(g1.view(torch.int32), g1b.view(torch.int32)) and torch.equal(v1.view(torch.int32), v1b.view(torch.int32))
    x, y = Padded(n, pred), Padded(n, target)
    # alpha = 0.25 (a power of two: the scaling is exact) added onto a known buffer; loss[0] += alpha L; value may be null
    old = torch.randn(B * C * H, W, generator=torch.Generator().manual_seed(11))
    acc = Guarded("f32", B * C * H, W, W, fill=old)
    loss = torch.full((1,), 0.5, device="cuda")
    assert _call(x, y, shape, acc, ortho, alpha=0.25, accumulate=1, loss=loss) == 0
    acc.assert_guards("accumulating fft loss")
    assert torch.equal(acc.data(), old + 0.25 * g1.view(-1, W))
    assert abs(float(loss) - (0.5 + 0.25 * float(v1))) <= 4 * U
    # overwrite with alpha = 0.25
    ow = Guarded("f32", B * C * H, W, W)
    assert _call(x, y, shape, ow, ortho, alpha=0.25) == 0
    assert torch.equal(ow.data(), 0.25 * g1.view(-1, W))
    # value only: d_x null, the same bits
    value = torch.zeros(1, device="cuda")
    assert _call(x, y, shape, None, ortho, value=value) == 0
    assert torch.equal(value.cpu().view(torch.int32), v1.view(torch.int32))
    # both scalars null: still fine
    assert _call(x, y, shape, None, ortho) == 0


def test_refusals():
    shape = (2, 3, 12, 16)
    n = 2 * 3 * 12 * 16
    x, y = torch.rand(shape, device="cuda"), torch.rand(shape, device="cuda")
    out = Guarded("f32", 2 * 3 * 12, 16, 16)
    value, loss = torch.zeros(1, device="cuda"), torch.zeros(1, device="cuda")
    ws = torch.zeros(4 * _ws_floats((2, 3, 16, 16)), dtype=torch.uint8, device="cuda")
    ok = dict(x=x, y=y, shape=shape, dptr=out, value=value, loss=loss, ws=ws)
    for change, code in ((dict(shape=(2, 3, 513, 16)), E_UNSUPPORTED), (dict(shape=(2, 3, 12, 513)), E_UNSUPPORTED),
                         (dict(shape=(0, 3, 12, 16)), E_SHAPE), (dict(shape=(2, 0, 12, 16)), E_SHAPE), (dict(shape=(2, 3, 0, 16)), E_SHAPE),
                         (dict(shape=(2, 3, 12, 0)), E_SHAPE), (dict(shape=(2, 3, -1, 16)), E_SHAPE), (dict(shape=(1024, 64, 12, 16)), E_SHAPE),
                         (dict(alpha=float("nan")), E_SHAPE), (dict(alpha=float("inf")), E_SHAPE), (dict(accumulate=2), E_SHAPE),
                         (dict(ortho=2), E_SHAPE), (dict(dptr=None, accumulate=1), E_SHAPE),
                         (dict(dptr=x.data_ptr()), E_SHAPE), (dict(dptr=y.data_ptr() + 4 * (n - 1)), E_SHAPE),
                         (dict(x=None), E_NULL), (dict(y=None), E_NULL), (dict(ws=0), E_NULL)):
        assert _call(**{**ok, **change}) == code, change
        assert _lib().srk_last_error()
    torch.cuda.synchronize()
    out.assert_untouched("d_x of refused calls")
    assert float(value) == 0.0 and float(loss) == 0.0 and int(ws.sum()) == 0
    for bad in ((2, 3, 513, 16), (2, 3, 16, 513), (0, 3, 16, 16), (1024, 64, 16, 16)):
        assert int(_lib().srk_fft_loss_workspace(*bad)) == 0
    assert int(_lib().srk_fft_loss_workspace(1, 1, 512, 512)) == 4 * _ws_floats((1, 1, 512, 512))


# ---- Python surface -------------------------------------------------------------------------------------------------------------------
def test_ops_and_make_loss_on_a_leaf():
    from tpu_superresolution_amd import ops
    from tpu_superresolution_amd.training import make_loss
    shape = (2, 3, 24, 40)
    pred, target = R.random_inputs(shape, 7)
    xd, yd = pred.cuda(), target.cuda()
    v64, g64 = R.fft_loss_ref(pred, target, "ortho")
    v, d, none = ops.fft_loss_fwd_bwd(xd, yd, norm="ortho")
    assert none is None and abs(float(v) - float(v64)) <= 1e-5 * float(v64)
    # random inputs of this size are not sign-stable: a flipped sign moves every element by 2 s / N, a few may flip
    _, s, n = _coef(shape, "ortho")
    assert float((d.cpu().double() - g64).abs().max()) <= 8 * 2 * s / n
    v2, none2, _ = ops.fft_loss_fwd_bwd(xd, yd, norm="ortho", want_grad=False)
    assert none2 is None and torch.equal(v2, v)
    with pytest.raises(RuntimeError):
        ops.fft_loss_fwd_bwd(torch.zeros(1, 1, 513, 8, device="cuda"), torch.zeros(1, 1, 513, 8, device="cuda"))
    fn = make_loss("charbonnier", ssim_weight=0.2, fft_weight=0.05)
    l_pix, d_pix, _ = ops.pixel_loss_fwd_bwd(xd, yd, "charbonnier", 1e-3)
    sm, d_ssim, _ = ops.ssim_loss_fwd_bwd(xd, yd, 1.0, alpha=0.2)
    vf, d_fft, _ = ops.fft_loss_fwd_bwd(xd, yd, alpha=0.05)
    leaf = xd.clone().requires_grad_(True)
    loss, bad = fn(leaf, yd)
    assert loss.shape == () and int(bad) == 0
    want = float(l_pix) + 0.2 * (1.0 - float(sm)) + 0.05 * float(vf)
    assert abs(float(loss.detach()) - want) <= 8 * U * want
    loss.backward()
    assert torch.equal(leaf.grad, (d_pix + d_ssim) + d_fft)          # three kernels, each adding onto the last: two fp32 additions
    # the term alone on top of L1, both norms
    for norm in R.NORMS:
        leaf = xd.clone().requires_grad_(True)
        l2, _ = make_loss("l1", fft_weight=0.1, fft_norm=norm)(leaf, yd)
        l2.backward()
        l1v, d_l1, _ = ops.pixel_loss_fwd_bwd(xd, yd, "l1")
        vn, d_n, _ = ops.fft_loss_fwd_bwd(xd, yd, norm=norm, alpha=0.1)
        assert torch.equal(leaf.grad, d_l1 + d_n)
        assert abs(float(l2.detach()) - (float(l1v) + 0.1 * float(vn))) <= 8 * U * float(l2.detach())


def test_graphed_hat_step_with_the_frequency_term():
    """GraphedTrainStep(loss_fn=make_loss(..., fft_weight=...)): replays against the same steps launched eagerly, in the manner of
    tests/test_gpu_loss.py"""
    import tpu_superresolution_amd as T
    from test_oracle_golden import hat_tiny_weights
    from tpu_superresolution_amd.optim import FusedAdamW
    from tpu_superresolution_amd.training import GraphedTrainStep, make_loss, train_step
    _, cfg, sd = hat_tiny_weights()
    gen = torch.Generator().manual_seed(9)
    batches = [(torch.rand(2, 3, 32, 32, generator=gen).cuda(), torch.rand(2, 3, 128, 128, generator=gen).cuda()) for _ in range(3)]
    fn = make_loss("l1", fft_weight=0.05)

    def model():
        m = T.HAT(drop_path_rate=0.0, **cfg.kwargs())
        m.load_state_dict(sd, strict=True)
        return m.cuda().train()
    ma, mb = model(), model()
    oa = FusedAdamW(ma, lr=1e-4, weight_decay=0.0, max_grad_norm=1.0)
    ob = FusedAdamW(mb, lr=1e-4, weight_decay=0.0, max_grad_norm=1.0)
    gs = GraphedTrainStep(mb, ob, warmup=1, loss_fn=fn)
    train_step(ma, oa, *batches[0], loss_fn=fn)          # the graphed stepper warms up with one eager step on its first batch
    la, lb = [], []
    for x, t in batches:
        la.append(float(train_step(ma, oa, x, t, loss_fn=fn)[0]))
        lg, bad = gs(x, t)
        lb.append(float(lg))
        assert int(bad) == 0
    with torch.no_grad():
        out = ma(batches[-1][0])
        l1 = float(torch.nn.functional.l1_loss(out, batches[-1][1]))
    print("eager", la, "graphed", lb, "l1 after the last step", l1)
    assert all(abs(a - b) <= 2e-3 * abs(a) for a, b in zip(la, lb))
    assert la[-1] > 1.5 * l1          # random images: the spectrum term is far larger than 0.05^-1 pixel L1s
    ga = float(torch.sqrt(sum((p.grad.float() ** 2).sum() for p in ma.parameters())))
    gb = float(torch.sqrt(sum((p.grad.float() ** 2).sum() for p in mb.parameters())))
    assert abs(ga - gb) <= 0.05 * ga, (ga, gb)
    gs.close()


def test_finetune_script_with_fft_weight_and_at_the_defaults(tmp_path, capsys, monkeypatch):
    from test_data_and_script import make_dataset
    from tpu_superresolution_amd import finetune_swinir as F
    make_dataset(str(tmp_path))
    monkeypatch.chdir(tmp_path)
    base = ["--data_root", str(tmp_path), "--scale", "X4", "--epochs", "1", "--batch_size", "2", "--workers", "0", "--lr", "1e-4"]
    F.main(base + ["--fft_weight", "0.05"])
    out = capsys.readouterr().out
    line = next(ln for ln in out.splitlines() if "epoch 001/1" in ln)
    assert "train loss[l1+0.05*fft]=" in line and "val L1=" in line and "train L1=" not in line
    value = float(line.split("train loss[l1+0.05*fft]=")[1].split()[0])
    assert math.isfinite(value) and value > 0.0
    for name in ("best_swinir_finetune_X4.pt", "bestpsnr_swinir_finetune_X4.pt"):
        ck = torch.load(tmp_path / name, map_location="cpu", weights_only=False)
        assert ck["args"]["fft_weight"] == 0.05 and "fft_norm" not in ck["args"] and "loss" not in ck["args"]
    # the defaults: the line and the files of before
    F.main(base)
    out = capsys.readouterr().out
    line = next(ln for ln in out.splitlines() if "epoch 001/1" in ln)
    assert "train L1=" in line and "loss[" not in line
    for name in ("best_swinir_finetune_X4.pt", "bestpsnr_swinir_finetune_X4.pt"):
        ck = torch.load(tmp_path / name, map_location="cpu", weights_only=False)
        assert not {"fft_weight", "fft_norm"} & set(ck["args"])
