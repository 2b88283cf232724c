"""csrc/loss.hip -- srk_pixel_loss_fwd_bwd (L1 / MSE / Charbonnier) and srk_ssim_loss_fwd_bwd (the SSIM term: value and gradient from one
fused kernel) -- and what is built on them: training.make_loss, the differentiable metrics.ssim, a graphed HAT step and the
finetune_swinir flags.  The fp64 references are those of tests/loss_ref.py, pinned to torch in tests/test_loss_ref.py.

Worst ratios error / bound measured for the SSIM gradient are printed per case (pytest -s) and recorded in DESIGN.md."""
import functools
import math

import pytest
import torch

import loss_ref as R
from guarded import Guarded

pytestmark = pytest.mark.gpu

U = R.U
E_SHAPE, E_NULL, E_UNSUPPORTED = -1, -2, -3
KIND = {"l1": 0, "mse": 1, "charbonnier": 2}
EPS = 1e-3


def _lib():
    from tpu_superresolution_amd._lib import lib
    return lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ---- pixel losses ---------------------------------------------------------------------------------------------------------------------
def _blocks(n):
    return max(1, min(2048, (n + 255) // 256))


def _chain(n):
    """K of the 2 K u sum|term| / n bound: the longest sequential chain of the loss sum of pixel_loss_kernel / pixel_loss_finish_kernel as
    built -- a thread adds ceil(n / (blocks * 256)) terms, its wave butterfly 6 levels, the four waves 3 additions, a finishing thread
    ceil(blocks / 256) partials, again 6 + 3, then the multiplication by 1/n and the addition onto loss[0] (2) -- plus 4 for the roundings
    inside one term (the subtraction, the square or fma, the square root, and 1/n itself)."""
    b = _blocks(n)
    return math.ceil(n / (b * 256)) + 9 + math.ceil(b / 256) + 9 + 2 + 4


def _pixel_call(pred, target, dptr, loss, bad, n, kind, eps=EPS, grad_scale=1.0, accumulate=0, ws=None):
    if ws is None:
        ws = torch.empty(max(4, int(_lib().srk_pixel_loss_workspace(n))), dtype=torch.uint8, device="cuda")
    ptr = lambda t: t if t is None or isinstance(t, int) else t.data_ptr()          # noqa: E731
    return _lib().srk_pixel_loss_fwd_bwd(ptr(pred), ptr(target), dptr, ptr(loss), ptr(bad), n, kind, eps, grad_scale, accumulate, ptr(ws),
                                         _stream())


@functools.lru_cache(maxsize=None)
def _pixel_inputs(n):
    g = torch.Generator().manual_seed(n)
    pred, target = torch.rand(n, generator=g), torch.rand(n, generator=g)
    pred[3::7] = target[3::7]                                 # d == 0: sign(0) = 0, Charbonnier's gradient 0, loss term eps
    refs = {k: R.pixel_loss_ref(pred, target, k, EPS) + (R.pixel_terms_abs_sum(pred, target, k, EPS),) for k in R.KINDS}
    return pred, target, refs


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("n", [1, 255, 256, 257, 2048 * 256 + 3])
def test_pixel_loss_value_gradient_determinism(n, kind):
    pred, target, refs = _pixel_inputs(n)
    loss64, grad64, abs_sum = refs[kind]
    pd, td = pred.cuda(), target.cuda()
    assert int(_lib().srk_pixel_loss_workspace(n)) == 4 * _blocks(n)
    tol_g = {"l1": 4, "mse": 4, "charbonnier": 8}[kind] * U
    tol_l = 2 * _chain(n) * U * abs_sum / n
    for scale in (1.0, 0.5):
        # accumulate == 0 onto the NaN pattern of the guarded window
        out = Guarded("f32", 1, n, n)
        loss = torch.zeros(1, device="cuda")
        bad = torch.zeros(1, dtype=torch.int32, device="cuda")
        assert _pixel_call(pd, td, out.ptr, loss, bad, n, KIND[kind], grad_scale=scale) == 0
        out.assert_guards(f"{kind} n={n}")
        want = grad64 * scale
        err = float((out.data().view(-1).double() - want).abs().max())
        lerr = abs(float(loss.double()) - float(loss64))
        print(f"{kind} n={n} scale={scale}: d_pred err {err:.3e} (tol {tol_g * float(want.abs().max()):.3e}), loss err {lerr:.3e} (tol {tol_l:.3e})")
        assert err <= tol_g * float(want.abs().max())
        assert lerr <= tol_l
        assert int(bad) == 0
        # bit-equal rerun
        out2 = Guarded("f32", 1, n, n)
        loss2 = torch.zeros(1, device="cuda")
        assert _pixel_call(pd, td, out2.ptr, loss2, bad, n, KIND[kind], grad_scale=scale) == 0
        assert torch.equal(loss.view(torch.int32), loss2.view(torch.int32))
        assert torch.equal(out.data().view(torch.int32), out2.data().view(torch.int32))
        # accumulate == 1 onto a known buffer of the gradient's sign and at least its size (no cancellation: the bound, relative to the
        # largest sum, then covers both operands of the addition); the loss is accumulated with weight 1 onto what the scalar held
        gmax = float(want.abs().max())
        old = (1.0 + torch.rand(n, generator=torch.Generator().manual_seed(3))) * gmax * torch.where(want < 0, -1.0, 1.0).float()
        acc = Guarded("f32", 1, n, n, fill=old.view(1, n))
        loss3 = torch.full((1,), 0.25, device="cuda")
        assert _pixel_call(pd, td, acc.ptr, loss3, bad, n, KIND[kind], grad_scale=scale, accumulate=1) == 0
        acc.assert_guards(f"{kind} n={n} accumulate")
        want_acc = old.double() + want
        assert float((acc.data().view(-1).double() - want_acc).abs().max()) <= tol_g * float(want_acc.abs().max())
        assert abs(float(loss3.double()) - 0.25 - float(loss64)) <= tol_l + U * (0.25 + float(loss64))
        assert int(bad) == 0
    # d_pred may be null: the value alone, same bits
    loss4 = torch.zeros(1, device="cuda")
    assert _pixel_call(pd, td, None, loss4, None, n, KIND[kind], grad_scale=0.5) == 0
    assert torch.equal(loss4.view(torch.int32), loss.view(torch.int32))


@pytest.mark.parametrize("kind", R.KINDS)
def test_pixel_loss_counts_nonfinite_predictions_exactly(kind):
    n = 2048 * 256 + 3
    pred, target, _ = _pixel_inputs(n)
    pred = pred.clone()
    where = torch.randperm(n, generator=torch.Generator().manual_seed(5))[:11].tolist() + [0, n - 1]
    for i, p in enumerate(where):
        pred[p] = (float("nan"), float("inf"), float("-inf"))[i % 3]
    tgt = target.clone()
    tgt[7] = float("nan")                                      # a non-finite TARGET is not counted
    bad = torch.full((1,), 5, dtype=torch.int32, device="cuda")          # accumulated
    loss = torch.zeros(1, device="cuda")
    out = Guarded("f32", 1, n, n)
    assert _pixel_call(pred.cuda(), tgt.cuda(), out.ptr, loss, bad, n, KIND[kind]) == 0
    out.assert_guards("non-finite run")
    assert int(bad) == 5 + len(set(where))
    assert not bool(torch.isfinite(loss))


def test_pixel_loss_refusals():
    n = 300
    x, t = torch.rand(n, device="cuda"), torch.rand(n, device="cuda")
    out = Guarded("f32", 1, n, n)
    loss = torch.zeros(1, device="cuda")
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    ws = torch.zeros(64, dtype=torch.uint8, device="cuda")
    ok = dict(pred=x, target=t, dptr=out.ptr, loss=loss, bad=bad, n=n, kind=0, ws=ws)
    for change, code in ((dict(pred=None), E_NULL), (dict(target=None), E_NULL), (dict(loss=None), E_NULL), (dict(ws=0), E_NULL),
                         (dict(n=0), E_SHAPE), (dict(n=-5), E_SHAPE), (dict(kind=3), E_SHAPE), (dict(kind=-1), E_SHAPE),
                         (dict(kind=2, eps=0.0), E_SHAPE), (dict(kind=2, eps=-1e-3), E_SHAPE), (dict(kind=2, eps=float("nan")), E_SHAPE),
                         (dict(accumulate=2), E_SHAPE)):
        assert _pixel_call(**{**ok, **change}) == code, change
        assert _lib().srk_last_error()
    torch.cuda.synchronize()
    out.assert_untouched("d_pred of refused calls")
    assert float(loss) == 0.0 and int(bad) == 0 and int(ws.sum()) == 0
    assert int(_lib().srk_pixel_loss_workspace(0)) == 0
    assert _pixel_call(**{**ok, "kind": 0, "eps": 0.0}) == 0          # eps is read by Charbonnier only


# ---- SSIM term ------------------------------------------------------------------------------------------------------------------------
def _ssim_call(x, y, shape, dptr, data_range=1.0, alpha=1.0, accumulate=0, mean=None, loss=None, ws=None):
    B, C, H, W = shape
    if ws is None:
        ws = torch.empty(max(4, int(_lib().srk_ssim_loss_workspace(B, C, H, W))), dtype=torch.uint8, device="cuda")
    ptr = lambda t: t if t is None or isinstance(t, int) else t.data_ptr()          # noqa: E731
    return _lib().srk_ssim_loss_fwd_bwd(ptr(x), ptr(y), ptr(ws), B, C, H, W, data_range, alpha, dptr, accumulate, ptr(mean), ptr(loss),
                                        _stream())


@functools.lru_cache(maxsize=None)
def _ssim_case(kind, shape, data_range=1.0):
    """inputs and the yardstick's four references, computed once: fp64 and fp32 autograd of metrics.ssim_torch on the CPU"""
    x, y = R.ssim_inputs(kind, shape)
    x, y = x * data_range, y * data_range
    v64, g64 = R.ssim_autograd(x, y, data_range, torch.float64)
    v32, g32 = R.ssim_autograd(x, y, data_range, torch.float32)
    return x, y, float(v64), g64, float(v32), g32


def _ssim_check(kind, shape, data_range=1.0):
    """run the kernel (alpha 1, overwrite) on guarded memory and hold it against the yardstick; -> (d_x, S) as the kernel left them"""
    x, y, v64, g64, v32, g32 = _ssim_case(kind, shape, data_range)
    n = x.numel()
    out = Guarded("f32", 1, n, n)
    mean = torch.full((1,), float("nan"), device="cuda")
    assert _ssim_call(x.cuda(), y.cuda(), shape, out.ptr, data_range, mean=mean) == 0
    out.assert_guards(f"ssim {kind} {shape}")
    got = out.data().view(shape)
    err = float((got.double() / -1.0 - g64).abs().max())
    bound = 4 * float((g32 - g64).abs().max()) + 64 * U * float(g64.abs().max())
    verr, vbound = abs(float(mean.double()) - v64), 4 * abs(v32 - v64) + 64 * U
    print(f"ssim {kind} {'x'.join(map(str, shape))} range {data_range:g}: gradient err {err:.3e} / bound {bound:.3e} = {err / bound:.3f}; "
          f"S err {verr:.3e} / bound {vbound:.3e} = {verr / vbound:.3f}")
    assert err <= bound
    assert verr <= vbound
    return got, mean


SSIM_CASES = [(k, s) for k in R.SSIM_INPUTS for s in R.SSIM_SHAPES]


@pytest.mark.parametrize("kind,shape", SSIM_CASES, ids=[f"{k}-{'x'.join(map(str, s))}" for k, s in SSIM_CASES])
def test_ssim_term_against_the_autograd_yardstick(kind, shape):
    _ssim_check(kind, shape)


@pytest.mark.parametrize("shape", [(2, 3, 12, 45), (2, 1, 75, 33)], ids=lambda s: "x".join(map(str, s)))
def test_ssim_term_scaling_accumulation_range_determinism(shape):
    from tpu_superresolution_amd import ops
    x, y = _ssim_case("smooth", shape)[:2]
    xd, yd = x.cuda(), y.cuda()
    n = x.numel()
    g1, s1 = _ssim_check("smooth", shape)
    # bit-equal rerun
    g1b, s1b = _ssim_check("smooth", shape)
    assert torch.equal(g1.view(torch.int32), g1b.view(torch.int32)) and torch.equal(s1.view(torch.int32), s1b.view(torch.int32))
    # the S of the metric kernel (srk_ssim: unshifted moments, another tiling), each within the yardstick's bound of the fp64 value
    v64, v32 = _ssim_case("smooth", shape)[2], _ssim_case("smooth", shape)[4]
    assert abs(float(s1) - float(ops.ssim(xd, yd, 1.0)[1])) <= 2 * (4 * abs(v32 - v64) + 64 * U)
    # alpha = 0.25 (a power of two: the scaling is exact) added onto a known buffer; loss[0] += alpha (1 - S)
    old = torch.randn(n, generator=torch.Generator().manual_seed(11))
    acc = Guarded("f32", 1, n, n, fill=old.view(1, n))
    loss = torch.full((1,), 0.5, device="cuda")
    assert _ssim_call(xd, yd, shape, acc.ptr, alpha=0.25, accumulate=1, loss=loss) == 0          # ssim_mean may be null
    acc.assert_guards("accumulating ssim")
    assert torch.equal(acc.data().view(-1), old + 0.25 * g1.view(-1))
    assert abs(float(loss) - (0.5 + 0.25 * (1.0 - float(s1)))) <= 4 * U
    # overwrite with alpha = 0.25; d_x may be null (value only)
    ow = Guarded("f32", 1, n, n)
    assert _ssim_call(xd, yd, shape, ow.ptr, alpha=0.25) == 0
    assert torch.equal(ow.data().view(-1), 0.25 * g1.view(-1))
    mean = torch.zeros(1, device="cuda")
    assert _ssim_call(xd, yd, shape, None, mean=mean) == 0
    assert torch.equal(mean.view(torch.int32), s1.view(torch.int32))
    # data_range 255 on the images scaled to it: its own yardstick
    _ssim_check("smooth", shape, 255.0)


@pytest.mark.parametrize("shape", R.SSIM_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_ssim_term_of_identical_images(shape):
    x, y = _ssim_case("smooth", shape)[:2]
    g_noise, _ = _ssim_check("smooth", shape)
    n = x.numel()
    out = Guarded("f32", 1, n, n)
    mean = torch.zeros(1, device="cuda")
    yd = y.cuda()
    assert _ssim_call(yd.clone(), yd, shape, out.ptr, mean=mean) == 0
    out.assert_guards("identical images")
    assert abs(float(mean) - 1.0) <= 1e-6
    assert float(out.data().abs().max()) <= 1e-3 * float(g_noise.abs().max())


def test_ssim_term_refusals():
    shape = (2, 3, 12, 16)
    n = 2 * 3 * 12 * 16
    x, y = torch.rand(shape, device="cuda"), torch.rand(shape, device="cuda")
    out = Guarded("f32", 1, n, n)
    mean, loss = torch.zeros(1, device="cuda"), torch.zeros(1, device="cuda")
    ws = torch.zeros(256, dtype=torch.uint8, device="cuda")
    ok = dict(x=x, y=y, shape=shape, dptr=out.ptr, mean=mean, loss=loss, ws=ws)
    for change, code in ((dict(shape=(2, 3, 10, 16)), E_UNSUPPORTED), (dict(shape=(2, 3, 12, 10)), E_UNSUPPORTED),
                         (dict(shape=(0, 3, 12, 16)), E_SHAPE), (dict(shape=(1025, 1, 12, 16)), E_SHAPE), (dict(shape=(2, 0, 12, 16)), E_SHAPE),
                         (dict(shape=(1024, 64, 12, 16)), E_SHAPE), (dict(data_range=0.0), E_SHAPE), (dict(accumulate=2), E_SHAPE),
                         (dict(dptr=x.data_ptr()), E_SHAPE), (dict(dptr=y.data_ptr() + 4 * (n - 1)), E_SHAPE),
                         (dict(dptr=x.data_ptr() - 4 * (n - 1)), E_SHAPE),
                         (dict(x=None), E_NULL), (dict(y=None), E_NULL), (dict(ws=0), E_NULL)):
        assert _ssim_call(**{**ok, **change}) == code, change
        assert _lib().srk_last_error()
    torch.cuda.synchronize()
    out.assert_untouched("d_x of refused calls")
    assert float(mean) == 0.0 and float(loss) == 0.0 and int(ws.sum()) == 0
    assert int(_lib().srk_ssim_loss_workspace(2, 3, 10, 16)) == 0
    assert int(_lib().srk_ssim_loss_workspace(2, 3, 33, 65)) == 4 * 2 * 3 * 2 * 3          # 32 x 32 tiles of INPUT pixels


# ---- Python surface -------------------------------------------------------------------------------------------------------------------
def test_make_loss_and_differentiable_ssim_on_a_leaf():
    from tpu_superresolution_amd import metrics, ops
    from tpu_superresolution_amd.training import make_loss
    shape = (2, 3, 24, 40)
    x, y = R.ssim_inputs("smooth", shape)
    xd, yd = x.cuda(), y.cuda()
    for kind in R.KINDS:
        fn = make_loss(kind, charbonnier_eps=EPS, ssim_weight=0.2)
        l_pix, d_pix, _ = ops.pixel_loss_fwd_bwd(xd, yd, kind, EPS)
        s, d_ssim, _ = ops.ssim_loss_fwd_bwd(xd, yd, 1.0, alpha=0.2)
        leaf = xd.clone().requires_grad_(True)
        loss, bad = fn(leaf, yd)
        assert loss.shape == () and int(bad) == 0 and not bad.requires_grad
        assert abs(float(loss.detach()) - (float(l_pix) + 0.2 * (1.0 - float(s)))) <= 4 * U * float(loss.detach())
        loss.backward()
        assert torch.equal(leaf.grad, d_pix + d_ssim)          # the SSIM kernel added onto the pixel kernel's d_pred: one fp32 addition
        leaf2 = xd.clone().requires_grad_(True)
        (2.0 * fn(leaf2, yd)[0]).backward()
        assert torch.equal(leaf2.grad, 2.0 * leaf.grad)
        # without the SSIM term: the pixel kernel alone
        leaf3 = xd.clone().requires_grad_(True)
        l3, _ = make_loss(kind, charbonnier_eps=EPS)(leaf3, yd)
        l3.backward()
        if kind == "l1":          # make_loss("l1") is l1_loss_checked: the L1 kernel of misc.hip (its loss sum is formed by atomics)
            assert torch.equal(leaf3.grad, d_pix) and abs(float(l3.detach()) - float(l_pix)) <= 64 * U * float(l_pix)
        else:
            assert torch.equal(leaf3.grad, d_pix) and torch.equal(l3.detach().reshape(1), l_pix)
    # the non-finite counter is the pixel kernel's
    xn = xd.clone()
    xn[1, 2, 3, 4] = float("nan")
    assert int(make_loss("mse", ssim_weight=0.1)(xn.requires_grad_(True), yd)[1]) == 1
    # metrics.ssim: differentiable in X on the device path, the value of the metric kernel, no gradient for Y
    leaf = xd.clone().requires_grad_(True)
    S = metrics.ssim(leaf, yd, data_range=1.0)
    assert S.grad_fn is not None and S.shape == ()
    S.backward()
    _, v64, g64, v32, g32 = _ssim_case("smooth", shape)[1:]
    assert float((leaf.grad.cpu().double() - g64).abs().max()) <= 4 * float((g32 - g64).abs().max()) + 64 * U * float(g64.abs().max())
    assert abs(float(S.detach()) - v64) <= 4 * abs(v32 - v64) + 64 * U
    plain = metrics.ssim(xd, yd, data_range=1.0)
    assert plain.grad_fn is None and abs(float(plain) - float(S.detach())) <= 2 * (4 * abs(v32 - v64) + 64 * U)
    with torch.no_grad():
        assert metrics.ssim(leaf, yd, data_range=1.0).grad_fn is None
    loss = 1.0 - metrics.ssim(leaf, yd.clone().requires_grad_(True), data_range=1.0)
    assert loss.requires_grad


def test_graphed_hat_step_with_charbonnier_and_ssim():
    """GraphedTrainStep(loss_fn=make_loss(...)): replays against the same steps launched eagerly (same kernels, FusedAdamW on both sides),
    as tests/test_gpu_hat.py asserts for L1; a NaN batch inside a replay leaves the weights untouched."""
    import tpu_superresolution_amd as T
    from test_oracle_golden import hat_tiny_weights
    from tpu_superresolution_amd.optim import FusedAdamW
    from tpu_superresolution_amd.training import GraphedTrainStep, make_loss, train_step
    _, cfg, sd = hat_tiny_weights()
    gen = torch.Generator().manual_seed(9)
    batches = [(torch.rand(2, 3, 32, 32, generator=gen).cuda(), torch.rand(2, 3, 128, 128, generator=gen).cuda()) for _ in range(3)]
    fn = make_loss("charbonnier", ssim_weight=0.2)

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
    # the objective is the one asked for, not L1: Charbonnier + 0.2 (1 - SSIM) of the eager model's last prediction
    with torch.no_grad():
        l1 = float(torch.nn.functional.l1_loss(ma(batches[-1][0]), batches[-1][1]))
    print("eager", la, "graphed", lb, "l1 after the last step", l1)
    assert all(abs(a - b) <= 2e-3 * abs(a) for a, b in zip(la, lb))
    assert la[-1] > l1 + 0.1          # random images: 1 - SSIM is near 1, so the SSIM term adds about 0.2
    ga = float(torch.sqrt(sum((p.grad.float() ** 2).sum() for p in ma.parameters())))
    gb = float(torch.sqrt(sum((p.grad.float() ** 2).sum() for p in mb.parameters())))
    assert abs(ga - gb) <= 0.05 * ga, (ga, gb)
    moved = torch.sqrt(sum(((pa.detach().cpu() - sd[n]).double() ** 2).sum() for n, pa in ma.named_parameters()))
    apart = torch.sqrt(sum(((pa.detach() - pb.detach()).double() ** 2).sum() for pa, pb in zip(ma.parameters(), mb.parameters())))
    print(f"weights: moved {float(moved):.4e}, eager and graphed apart {float(apart):.4e}")
    assert float(apart) <= 0.1 * float(moved)
    before = [p.detach().clone() for p in mb.parameters()]
    xbad = batches[1][0].clone()
    xbad[0, 1, 5, 7] = float("nan")
    _, bad = gs(xbad, batches[1][1])
    assert int(bad) > 0
    assert all(torch.equal(a, p.detach()) for a, p in zip(before, mb.parameters())), "a non-finite batch inside a replay changed the weights"
    lg, bad = gs(*batches[1])
    assert int(bad) == 0 and bool(torch.isfinite(lg))
    gs.close()


def test_finetune_script_with_loss_flags_and_at_the_defaults(tmp_path, capsys, monkeypatch):
    from test_data_and_script import make_dataset
    from tpu_superresolution_amd import finetune_swinir as F
    make_dataset(str(tmp_path))
    monkeypatch.chdir(tmp_path)
    base = ["--data_root", str(tmp_path), "--scale", "X4", "--epochs", "1", "--batch_size", "2", "--workers", "0", "--lr", "1e-4"]
    F.main(base + ["--loss", "charbonnier", "--ssim_weight", "0.2"])
    out = capsys.readouterr().out
    line = next(ln for ln in out.splitlines() if "epoch 001/1" in ln)
    assert "train loss[charbonnier+0.2*(1-ssim)]=" in line and "SSIM=" in line and "val L1=" in line and "train L1=" not in line
    value = float(line.split("train loss[charbonnier+0.2*(1-ssim)]=")[1].split()[0])
    assert math.isfinite(value) and value > 0.0
    for name in ("best_swinir_finetune_X4.pt", "bestpsnr_swinir_finetune_X4.pt"):
        ck = torch.load(tmp_path / name, map_location="cpu", weights_only=False)
        assert -1.0 <= ck["val_ssim"] <= 1.0
        assert ck["args"]["loss"] == "charbonnier" and ck["args"]["ssim_weight"] == 0.2 and "charbonnier_eps" not in ck["args"]
    # the defaults: the line and the files of before
    F.main(base)
    out = capsys.readouterr().out
    line = next(ln for ln in out.splitlines() if "epoch 001/1" in ln)
    assert "train L1=" in line and "SSIM" not in line and "loss[" not in line
    for name in ("best_swinir_finetune_X4.pt", "bestpsnr_swinir_finetune_X4.pt"):
        ck = torch.load(tmp_path / name, map_location="cpu", weights_only=False)
        assert "val_ssim" not in ck
        assert not {"loss", "charbonnier_eps", "ssim_weight"} & set(ck["args"])
