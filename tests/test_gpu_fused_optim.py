"""The multi-tensor clip + AdamW kernels (csrc/optim_multi.hip) and everything built on them: optim.FusedAdamW for models with separate
parameter tensors (HAT, DAT), training.GraphedTrainStep with the fused optimizer, finetune_swinir --arch / --graph.

Tolerances.  Kernel vs torch: the yardstick is clip_grad_norm_ + torch.optim.AdamW on the CPU in fp64; torch's own fp32 AdamW on the GPU
is measured against it on the same case and the fused kernel may err 8x as much, per kind (params / exp_avg / exp_avg_sq).  Why 8: a
CPU emulation of the flat kernel's formula in fp32 came out at 1.7x / 0.15x / 3.3x of torch's fp32 error (last-bit effects of folding
1 / grad_div and the clip factor into one coefficient and of the summation order), so 8 leaves a factor 2 over the worst kind and still
fails on any real mistake (a wrong bias correction or decay is orders of magnitude larger).  Training losses: relative 2e-3 per step,
the bound of the graphed-vs-eager tests of test_gpu_hat.py / test_gpu_dat.py; gradient norm 5 % (test_gpu_hat.py); eval after a step:
1.2e-2 * max|ref| against the oracle, the bound of the models' inference tests."""
import io
import os

import numpy as np
import pytest
import torch
from PIL import Image

from oracle import dat_oracle as DO
from oracle import hat_oracle as HO
from test_oracle_golden import DAT_TINY, hat_tiny_weights

pytestmark = pytest.mark.gpu

SIZES = [(1,), (3,), (63,), (64,), (65,), (180,), (180, 180), (180 * 180 * 9 + 1,)]
KINDS = ("param", "exp_avg", "exp_avg_sq")


def _case(seed=0, steps=3, many=0):
    """-> params (CPU fp32 list), grads per step (list of lists), index of the tensor that sits at a 4-byte-aligned address"""
    gen = torch.Generator().manual_seed(seed)
    shapes = list(SIZES) + [(1001,)] + [(int(torch.randint(1, 400, (1,), generator=gen)),) for _ in range(many)]
    params = [0.05 * torch.randn(*s, generator=gen) for s in shapes]
    grads = [[0.01 * torch.randn(*s, generator=gen) for s in shapes] for _ in range(steps)]
    return params, grads, len(SIZES)


def _to_gpu(tensors, odd):
    """Separate allocations; tensor `odd` is a view one float into its storage: its pointer is 4-byte aligned only."""
    out = []
    for i, t in enumerate(tensors):
        if i == odd:
            base = torch.zeros(t.numel() + 1, device="cuda")
            v = base[1:].view(t.shape)
            v.copy_(t)
            assert v.data_ptr() % 16 == 4 and v.is_contiguous()
            out.append(v)
        else:
            out.append(t.cuda())
    return out


def _torch_adamw(params, grads, dtype, device, lr, wd, max_norm, grad_div):
    ps = [torch.nn.Parameter(p.to(device=device, dtype=dtype)) for p in params]
    opt = torch.optim.AdamW(ps, lr=lr, weight_decay=wd, betas=(0.9, 0.999), eps=1e-8)
    for gs in grads:
        for p, g in zip(ps, gs):
            p.grad = g.to(device=device, dtype=dtype) / grad_div
        torch.nn.utils.clip_grad_norm_(ps, max_norm)
        opt.step()
    return {"param": [p.detach().double().cpu() for p in ps], "exp_avg": [opt.state[p]["exp_avg"].double().cpu() for p in ps],
            "exp_avg_sq": [opt.state[p]["exp_avg_sq"].double().cpu() for p in ps]}


def _max_err(got, ref):
    return {k: max(float((a.reshape(-1) - b.reshape(-1)).abs().max()) for a, b in zip(got[k], ref[k])) for k in KINDS}


def _table(ops, p, g, m, v):
    tab = ops.TensorTable(len(p))
    tab.set("params", p, first=True)
    tab.set("grads", g)
    tab.set("exp_avg", m)
    tab.set("exp_avg_sq", v)
    return tab


HYPER = dict(lr=2e-3, wd=0.01, max_norm=1.0, grad_div=2.0)


def _run_fused(params, grads, odd, flat=False):
    """3 steps of the multi-tensor kernels on separate allocations -> final {kind: [fp64 CPU tensors]}.  flat=True also feeds the same
    tensors, laid out contiguously, and the same sumsq to the single-range srk_adamw_clip_step and compares after every step."""
    from tpu_superresolution_amd import ops
    from tpu_superresolution_amd._lib import check, lib
    lr, wd, max_norm, grad_div = HYPER["lr"], HYPER["wd"], HYPER["max_norm"], HYPER["grad_div"]
    p = _to_gpu(params, odd)
    m, v = [torch.zeros_like(t) for t in p], [torch.zeros_like(t) for t in p]
    sizes = [t.numel() for t in params]
    fp = torch.cat([t.reshape(-1) for t in params]).cuda()
    fm, fv = torch.zeros_like(fp), torch.zeros_like(fp)
    sumsq = torch.zeros(1, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    for k, gs in enumerate(grads):
        g = _to_gpu(gs, odd)
        tab = _table(ops, p, g, m, v)
        sumsq.zero_()
        ops.multi_grad_sumsq(tab, sumsq)
        want = sum(float((x.double() ** 2).sum()) for x in gs)
        assert abs(float(sumsq) - want) <= 1e-5 * want, (float(sumsq), want)
        ops.multi_adamw_clip_step(tab, sumsq, max_norm, grad_div, lr, 0.9, 0.999, 1e-8, wd, k + 1)
        if not flat:
            continue
        fg = torch.cat([x.reshape(-1) for x in gs]).cuda()
        check(lib().srk_adamw_clip_step(fp.data_ptr(), fg.data_ptr(), fm.data_ptr(), fv.data_ptr(), fp.numel(), sumsq.data_ptr(), max_norm,
                                        grad_div, lr, 0.9, 0.999, 1e-8, wd, k + 1, None, st))
        for name, lst, whole in (("param", p, fp), ("exp_avg", m, fm), ("exp_avg_sq", v, fv)):
            for i, (a, b) in enumerate(zip(lst, whole.split(sizes))):
                assert torch.equal(a.reshape(-1), b), f"step {k + 1}: {name}[{i}] differs from the single-range kernel"
    return {"param": [t.double().cpu() for t in p], "exp_avg": [t.double().cpu() for t in m], "exp_avg_sq": [t.double().cpu() for t in v]}


@pytest.mark.parametrize("many", [0, 200])
def test_multi_tensor_step_equals_the_flat_kernel_bit_for_bit(many):
    """Awkward sizes (1, 3, 63, 64, 65, 180, 180 x 180, 180 x 180 x 9 + 1, one tensor at a 4-byte-aligned address) and, many=200, more
    tensors than one launch holds (chunks of 160 / 80): the multi-tensor path and srk_adamw_clip_step on the same values laid out
    contiguously, given the same sumsq, agree in every bit of params and both moments after each of 3 steps."""
    params, grads, odd = _case(seed=many, many=many)
    _run_fused(params, grads, odd, flat=True)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("many", [0, 200])
def test_multi_tensor_step_vs_torch_fp64(many, kind):
    """3 steps, max_grad_norm 1, weight_decay 0.01, grad_div 2, against clip_grad_norm_ + torch.optim.AdamW on the CPU in fp64; bound =
    8 x the error of torch's own fp32 AdamW on the same GPU against the same fp64 result (see the module docstring).

    Measured on MI355X, max abs error (fused / torch fp32 / ratio), many = 0 and many = 200; the largest of three runs, which differ
    in the last bits through the order of the atomics in the sum of squares:
      param       4.36e-08 / 4.36e-08 / 1.00      4.51e-08 / 4.51e-08 / 1.00
      exp_avg     1.70e-10 / 1.33e-10 / 1.28      2.11e-10 / 1.79e-10 / 1.18
      exp_avg_sq  1.95e-14 / 1.19e-14 / 1.64      1.54e-14 / 2.31e-14 / 0.67
    With 1 - beta and the bias corrections formed in fp32 from the fp32 betas, as srk_adamw_clip_step used to, exp_avg_sq was at
    1.06e-12 = 89x (46x): fp32(0.999) = 0.99900001287, so 1.0f - beta2 is 1.3e-5 low in relative terms on every element.  The host now
    forms these factors in fp64 from the decimal beta (csrc/adamw.h, adamw_decimal), for this kernel and the flat one alike."""
    params, grads, odd = _case(seed=many, many=many)
    h = HYPER
    ref = _torch_adamw(params, grads, torch.float64, "cpu", h["lr"], h["wd"], h["max_norm"], h["grad_div"])
    t32 = _torch_adamw(params, grads, torch.float32, "cuda", h["lr"], h["wd"], h["max_norm"], h["grad_div"])
    got = _run_fused(params, grads, odd)
    e_fused, e_torch = _max_err(got, ref), _max_err(t32, ref)
    for k in KINDS:
        print(f"[many={many}] {k}: fused {e_fused[k]:.3e}  torch fp32 {e_torch[k]:.3e}  ratio {e_fused[k] / max(e_torch[k], 1e-300):.2f}")
    assert e_fused[kind] <= 8.0 * e_torch[kind], (kind, e_fused[kind], e_torch[kind])


class _Bag(torch.nn.Module):
    def __init__(self, tensors):
        super().__init__()
        self.w = torch.nn.ParameterList([torch.nn.Parameter(t.clone()) for t in tensors])


def _bag(seed=5, steps=4):
    params, grads, _ = _case(seed=seed, steps=steps)
    params, grads = params[:7] + params[8:], [g[:7] + g[8:] for g in grads]          # without the 2.6 M element tensor
    return _Bag(params).cuda(), [[g.cuda() for g in gs] for gs in grads]


def _set_grads(net, gs):
    for p, g in zip(net.parameters(), gs):
        p.grad = g.clone()


def _snapshot(net, opt):
    ps = list(net.parameters())
    return ([p.detach().clone() for p in ps], [opt.state[p]["exp_avg"].clone() for p in ps if p in opt.state],
            [opt.state[p]["exp_avg_sq"].clone() for p in ps if p in opt.state])


def _frac_changed(a, b):
    return sum(not torch.equal(x, y) for x, y in zip(a, b)) / len(a)


def _same(a, b):
    return all(len(x) == len(y) and all(torch.equal(s, t) for s, t in zip(x, y)) for x, y in zip(a, b))


def test_gate_leaves_weights_and_moments_untouched():
    from tpu_superresolution_amd.optim import FusedAdamW
    net, grads = _bag()
    opt = FusedAdamW(net, lr=2e-3, weight_decay=0.01, max_grad_norm=1.0)
    _set_grads(net, grads[0])
    opt.step()                                         # moments are non-zero from here on
    before = _snapshot(net, opt)
    one, zero = torch.ones(1, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    _set_grads(net, grads[1])
    opt.step(nonfinite=one)                            # the loss kernel counted a non-finite prediction
    assert _same(_snapshot(net, opt), before)
    _set_grads(net, grads[1])
    list(net.parameters())[4].grad[7] = float("inf")   # one element: the norm is Inf
    opt.step(nonfinite=zero)
    assert _same(_snapshot(net, opt), before)
    _set_grads(net, grads[1])
    list(net.parameters())[6].grad[0, 3] = float("nan")
    opt.step()
    assert _same(_snapshot(net, opt), before)
    _set_grads(net, grads[1])
    opt.step(nonfinite=zero)
    after = _snapshot(net, opt)
    for kind, (a, b) in zip(KINDS, zip(after, before)):
        for i, (x, y) in enumerate(zip(a, b)):
            assert not torch.equal(x, y), f"{kind}[{i}] did not move"
    with pytest.raises(ValueError, match="int32"):
        opt.step(nonfinite=torch.zeros(1, device="cuda"))


def test_frozen_and_gradless_parameters_are_skipped_and_lr_is_read_every_step():
    from tpu_superresolution_amd.optim import FusedAdamW
    net, grads = _bag()
    ps = list(net.parameters())
    ps[2].requires_grad = False
    opt = FusedAdamW(net, lr=2e-3, weight_decay=0.0, max_grad_norm=None)
    start = [p.detach().clone() for p in ps]
    _set_grads(net, grads[0])
    ps[2].grad = None
    ps[5].grad = None                                  # trainable, but no gradient this step
    opt.step()
    moved = [not torch.equal(p.detach(), s) for p, s in zip(ps, start)]
    assert moved == [i not in (2, 5) for i in range(len(ps))]
    want = torch.sqrt(sum((g.double() ** 2).sum() for i, g in enumerate(grads[0]) if i not in (2, 5)))
    assert abs(float(opt.grad_norm()) - float(want)) <= 1e-5 * float(want)
    opt.param_groups[0]["lr"] = 0.0                    # what a scheduler does
    now = [p.detach().clone() for p in ps]
    opt.step()
    assert all(torch.equal(p.detach(), s) for p, s in zip(ps, now))
    opt.zero_grad()
    assert all(p.grad is None for p in ps)


def test_state_dict_resume_continues_bit_identically():
    from tpu_superresolution_amd.optim import FusedAdamW
    kw = dict(lr=2e-3, weight_decay=0.01, max_grad_norm=1.0, grad_div=2.0)
    na, grads = _bag()
    nb, _ = _bag()
    oa, ob = FusedAdamW(na, **kw), FusedAdamW(nb, **kw)
    for k in range(2):
        for net, opt in ((na, oa), (nb, ob)):
            _set_grads(net, grads[k])
            opt.step()
    buf = io.BytesIO()
    torch.save(ob.state_dict(), buf)
    buf.seek(0)
    oc = FusedAdamW(nb, **kw)
    oc.load_state_dict(torch.load(buf, map_location="cpu", weights_only=False))
    assert oc._step == 2
    for k in range(2, 4):
        for net, opt in ((na, oa), (nb, oc)):
            _set_grads(net, grads[k])
            opt.step()
    assert _same(_snapshot(na, oa), _snapshot(nb, oc))
    assert oa.state_dict()["fused"]["step"] == oc.state_dict()["fused"]["step"] == 4


def test_captured_step_follows_step_count_and_learning_rate_bit_for_bit():
    """The captured kernels read lr and the bias corrections from device memory: replays equal eager steps exactly, also across a
    learning-rate change, and the step count advances once per replay."""
    from tpu_superresolution_amd.optim import FusedAdamW
    kw = dict(lr=2e-3, weight_decay=0.01, max_grad_norm=1.0)
    na, grads = _bag(steps=5)
    nb, _ = _bag(steps=5)
    oa, ob = FusedAdamW(na, **kw), FusedAdamW(nb, **kw)
    static = [g.clone() for g in grads[0]]
    for p, g in zip(nb.parameters(), static):
        p.grad = g                                     # the captured launch reads these buffers
    _set_grads(na, grads[0])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        oa.step()
        ob.step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ob.step()
    assert ob._step == 1, "capturing must not count as a step"
    for k in range(1, 5):
        if k == 3:
            oa.param_groups[0]["lr"] = ob.param_groups[0]["lr"] = 5e-4
        _set_grads(na, grads[k])
        oa.step()
        for s, g in zip(static, grads[k]):
            s.copy_(g)
        ob.begin_replay()
        graph.replay()
        ob.end_replay()
        assert ob._step == k + 1
        assert _same(_snapshot(na, oa), _snapshot(nb, ob)), f"replay {k} differs from the eager step"


# ---- HAT / DAT ------------------------------------------------------------------------------------------------------------------------
def _arch(arch):
    """-> (make(): fresh training model from one seed, state_dict, batches, lr, oracle forward)"""
    import tpu_superresolution_amd as T
    gen = torch.Generator().manual_seed(9)
    if arch == "hat":
        _, cfg, sd = hat_tiny_weights()
        batches = [(torch.rand(2, 3, 32, 32, generator=gen).cuda(), torch.rand(2, 3, 128, 128, generator=gen).cuda()) for _ in range(4)]

        def make():
            m = T.HAT(drop_path_rate=0.0, **cfg.kwargs())
            m.load_state_dict(sd, strict=True)
            return m.cuda().train()
        return make, sd, batches, 1e-4, lambda s, x: HO.hat_forward(s, cfg, x)
    cfg = DO.DATConfig(**DAT_TINY)
    sd = DO.random_state_dict(cfg, seed=31, scale=1.0)
    batches = [(torch.rand(2, 3, 32, 32, generator=gen).cuda(), torch.rand(2, 3, 64, 64, generator=gen).cuda()) for _ in range(4)]

    def make():
        m = T.DAT(**cfg.kwargs(), drop_path_rate=0.0)
        m.load_state_dict(sd, strict=True)
        return m.cuda().train()
    return make, sd, batches, 1e-3, lambda s, x: DO.dat_forward(s, cfg, x)


def _torch_step(m, opt, x, t):
    from tpu_superresolution_amd.training import l1_loss_checked
    opt.zero_grad(set_to_none=True)
    loss, _ = l1_loss_checked(m(x), t)
    loss.backward()
    gn = torch.nn.utils.clip_grad_norm_(m.parameters(), 1.0)
    opt.step()
    return float(loss.detach()), float(gn)


@pytest.mark.parametrize("arch", ["hat", "dat"])
def test_eager_train_step_with_fused_optimizer_follows_torch_adamw(arch):
    from tpu_superresolution_amd.optim import FusedAdamW
    from tpu_superresolution_amd.training import train_step
    make, sd, batches, lr, _ = _arch(arch)
    ma, mb = make(), make()
    frozen = [n for n, _ in ma.named_parameters() if "conv_first" in n or ".blocks.0." in n or n.startswith("norm.")]
    assert 0 < len(frozen) < len(list(ma.parameters()))
    for m in (ma, mb):
        for n, p in m.named_parameters():
            p.requires_grad = n not in frozen
    oa = torch.optim.AdamW([p for p in ma.parameters() if p.requires_grad], lr=lr, weight_decay=0.0)
    ob = FusedAdamW(mb, lr=lr, weight_decay=0.0, max_grad_norm=1.0)
    for k, (x, t) in enumerate(batches[:3]):
        la, gna = _torch_step(ma, oa, x, t)
        lb, bad = train_step(mb, ob, x, t)
        gnb = float(ob.grad_norm())
        print(f"{arch} step {k}: loss torch {la:.6f} fused {float(lb):.6f} | grad norm torch {gna:.5f} fused {gnb:.5f}")
        assert int(bad) == 0
        assert abs(la - float(lb)) <= 2e-3 * abs(la)
        assert abs(gna - gnb) <= 0.05 * gna
    moved = []
    for n, p in mb.named_parameters():
        if n in frozen:
            assert torch.equal(p.detach().cpu(), sd[n]), n
            assert p not in ob.state
        else:
            moved.append(not torch.equal(p.detach().cpu(), sd[n]))
    assert sum(moved) >= 0.8 * len(moved)          # a parameter whose gradient is exactly zero does not move under Adam without decay


@pytest.mark.parametrize("arch", ["hat", "dat"])
def test_graphed_train_step_with_fused_optimizer(arch):
    """Replays follow the eager torch.optim.AdamW run; a NaN batch inside a replay leaves weights and moments untouched; a good batch
    steps again; a learning-rate change between replays takes effect."""
    from tpu_superresolution_amd.optim import FusedAdamW
    from tpu_superresolution_amd.training import GraphedTrainStep
    make, sd, batches, lr, _ = _arch(arch)
    ma, mb = make(), make()
    oa = torch.optim.AdamW(ma.parameters(), lr=lr, weight_decay=0.0)
    ob = FusedAdamW(mb, lr=lr, weight_decay=0.0, max_grad_norm=1.0)
    gs = GraphedTrainStep(mb, ob, warmup=1)
    _torch_step(ma, oa, *batches[0])          # the graphed stepper warms up with one eager step on its first batch
    la, lb = [], []
    for x, t in batches:
        la.append(_torch_step(ma, oa, x, t)[0])
        lg, bad = gs(x, t)
        lb.append(float(lg))
        assert int(bad) == 0
    print(arch, "eager", la, "graphed", lb)
    assert all(abs(a - b) <= 2e-3 * abs(a) for a, b in zip(la, lb))
    assert ob._step == 5
    ps = list(mb.parameters())

    def snap():
        return ([p.detach().clone() for p in ps], [ob.state[p]["exp_avg"].clone() for p in ps], [ob.state[p]["exp_avg_sq"].clone() for p in ps])
    before = snap()
    x, t = batches[1]
    xbad = x.clone()
    xbad[0, 1, 5, 7] = float("nan")
    _, bad = gs(xbad, t)
    assert int(bad) > 0
    assert _same(snap(), before), "a non-finite batch inside a replay changed weights or moments"
    lg, bad = gs(x, t)
    assert int(bad) == 0 and bool(torch.isfinite(lg))
    after = snap()

    def live():          # tensors whose gradient in the last replay is not exactly zero (Adam leaves the others where they are)
        return [i for i, p in enumerate(ps) if float(p.grad.abs().max()) > 0.0]
    idx = live()
    print(f"{arch}: {len(idx)} of {len(ps)} tensors have a non-zero gradient; weights moved: {_frac_changed(after[0], before[0]):.2f}")
    assert len(idx) >= len(ps) // 2
    assert all(not torch.equal(after[1][i], before[1][i]) and not torch.equal(after[2][i], before[2][i]) for i in idx), \
        "the good batch after the bad one did not step"
    assert _frac_changed(after[0], before[0]) >= 0.5
    # learning rate: read from param_groups before every replay
    ob.param_groups[0]["lr"] = 0.0
    gs(*batches[2])
    frozen_lr = snap()
    assert all(torch.equal(a, b) for a, b in zip(frozen_lr[0], after[0])), "lr = 0 still moved the weights"
    assert all(not torch.equal(frozen_lr[1][i], after[1][i]) for i in live())          # the moments went on
    ob.param_groups[0]["lr"] = lr
    gs(*batches[3])
    assert _frac_changed(snap()[0], frozen_lr[0]) >= 0.5
    gs.close()


@pytest.mark.parametrize("arch", ["hat", "dat"])
def test_eval_after_a_fused_step_sees_the_stepped_weights(arch):
    from tpu_superresolution_amd.optim import FusedAdamW
    from tpu_superresolution_amd.training import train_step
    make, sd, batches, lr, oracle = _arch(arch)
    m = make()
    x, t = batches[0]
    with torch.no_grad():
        y0 = m.eval()(x).cpu()                         # fills the bf16 pack cache with the initial weights
    opt = FusedAdamW(m.train(), lr=5e-3, weight_decay=0.0, max_grad_norm=1.0)
    train_step(m, opt, x, t)
    with torch.no_grad():
        y1 = m.eval()(x).cpu()
    stepped = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    with torch.no_grad():
        ref = oracle(stepped, x.cpu())
    err, moved = float((y1 - ref).abs().max()), float((y1 - y0).abs().max())
    print(f"{arch}: output moved by {moved:.3e}; max err vs oracle on the stepped weights {err:.3e} (ref max {float(ref.abs().max()):.3e})")
    assert moved > 0.0
    assert err <= 1.2e-2 * float(ref.abs().max())


# ---- script ---------------------------------------------------------------------------------------------------------------------------
def make_dataset(root, n_train=6, n_valid=2, lr=72, scale=4):
    rng = np.random.RandomState(0)
    for split, n in (("train", n_train), ("valid", n_valid)):
        hr_dir = os.path.join(root, "shuffled2D", f"shuffled2D_{split}_HR")
        lr_dir = os.path.join(root, "shuffled2D", f"shuffled2D_{split}_LR_default_X{scale}")
        os.makedirs(hr_dir)
        os.makedirs(lr_dir)
        for i in range(n):
            hr = (rng.rand(lr * scale, lr * scale) * 255).astype(np.uint8)
            Image.fromarray(hr, "L").save(os.path.join(hr_dir, f"{i:04d}.png"))
            Image.fromarray(hr, "L").resize((lr, lr), Image.BICUBIC).save(os.path.join(lr_dir, f"{i:04d}x{scale}.png"))


@pytest.mark.parametrize("arch", ["hat", "dat"])
def test_finetune_script_arch_one_epoch_reload_and_graph(arch, tmp_path, capsys, monkeypatch):
    from tpu_superresolution_amd import finetune_swinir as F
    make_dataset(str(tmp_path))
    monkeypatch.chdir(tmp_path)
    base = ["--data_root", str(tmp_path), "--scale", "X4", "--epochs", "1", "--batch_size", "2", "--workers", "0", "--lr", "1e-4", "--arch", arch]
    F.main(base)
    out = capsys.readouterr().out
    assert "[X4] epoch 001/1" in out and "[done] best_val_loss=" in out
    ck = torch.load(tmp_path / f"best_{arch}_finetune_X4.pt", map_location="cpu", weights_only=False)
    assert set(ck) >= {"model", "epoch", "best_val_loss", "val_psnr", "args"} and ck["args"]["arch"] == arch
    assert os.path.exists(tmp_path / f"bestpsnr_{arch}_finetune_X4.pt") and not os.path.exists(tmp_path / "best_swinir_finetune_X4.pt")
    fresh = F.build_sr_model(arch, 4).state_dict()
    assert list(ck["model"]) == list(fresh) and all(torch.isfinite(v).all() for v in ck["model"].values() if v.is_floating_point())
    moved = [k for k, v in ck["model"].items() if v.is_floating_point() and v.numel() > 1 and not torch.equal(v, fresh[k])]
    assert len(moved) > len(fresh) // 2
    torch.save({"params": ck["model"]}, tmp_path / "w.pth")
    F.main(base + ["--weights", str(tmp_path / "w.pth"), "--freeze_regex", "conv_first|layers\\.0"])
    out = capsys.readouterr().out
    assert "[weights] missing=0, unexpected=0" in out and "[freeze]" in out
    F.main(base + ["--weights", str(tmp_path / "w.pth"), "--graph", "--epochs", "2"])
    out = capsys.readouterr().out
    assert "[weights] missing=0, unexpected=0" in out and "[X4] epoch 002/2" in out and "[done] best_val_loss=" in out
    g = torch.load(tmp_path / f"best_{arch}_finetune_X4.pt", map_location="cpu", weights_only=False)["model"]
    assert all(torch.isfinite(v).all() for v in g.values() if v.is_floating_point())


def test_dat_batch_of_one_fails_with_torchs_own_message(tmp_path, monkeypatch):
    from tpu_superresolution_amd import finetune_swinir as F
    make_dataset(str(tmp_path), n_train=2, n_valid=1)
    monkeypatch.chdir(tmp_path)
    with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
        F.main(["--data_root", str(tmp_path), "--scale", "X4", "--epochs", "1", "--batch_size", "1", "--workers", "0", "--arch", "dat"])
