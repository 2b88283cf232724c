"""DAT fine-tuning with frozen BatchNorm statistics on the MI355X: a BatchNorm in eval mode normalises with its running buffers and
writes none of them, read per module at every forward (nn.BatchNorm2d's rule); DAT.forward builds the autograd node whenever grad is
enabled, whatever model.training says.

References: G18 (the reference's own DAT in eval mode with grad enabled, tools/make_golden_dat_frozen.py) and the eval-semantics
autograd oracle of tests/dat_frozen_ref.py, which tests/test_dat_frozen_ref.py pins against G18 on the CPU.  Tolerances are those of
test_gpu_dat.py::test_dat_train_step_vs_reference_golden: output within 2e-2 * max|ref|, loss within 5e-3 relative, per-tensor gradient
error <= 0.1 against max(|ref|, 2e-3 * the largest gradient norm).  tools/make_golden_dat_frozen.py asserts that this gradient bound
separates frozen from batch statistics (101 of 264 tensors differ by more than 0.1 between the two modes, the worst by 2.97)."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden
from dat_frozen_ref import eval_loss_and_grads, grad_errors
from guarded import Guarded
from oracle import dat_oracle as DO

pytestmark = pytest.mark.gpu

BUF = ("running_mean", "running_var", "num_batches_tracked")


def _lib():
    from tpu_superresolution_amd._lib import check, lib
    return check, lib()


def _st():
    return torch.cuda.current_stream().cuda_stream


def _model(cfg, sd, drop_path_rate=0.0):
    import tpu_superresolution_amd as T
    m = T.DAT(**cfg.kwargs(), drop_path_rate=drop_path_rate)
    m.load_state_dict(sd, strict=True)
    return m.cuda()


def _buffers(m):
    return {n: b.detach().clone() for n, b in m.named_buffers() if n.endswith(BUF)}


def _check_step(m, y, loss, yo, lo, grads, tol=0.1, floor=2e-3):
    got = {n: p.grad.detach().cpu() for n, p in m.named_parameters() if p.grad is not None}
    assert set(got) == set(grads), "a parameter got no gradient"
    errs = grad_errors(got, grads, floor)
    worst = max(errs, key=errs.get)
    eo = float((y.detach().cpu() - yo).abs().max())
    print(f"max|y - ref| {eo:.3e} (bound {2e-2 * float(yo.abs().max()):.3e}); loss {float(loss):.6f} vs {lo:.6f}; worst gradient error "
          f"{errs[worst]:.3e} at {worst}")
    assert eo <= 2e-2 * float(yo.abs().max())
    assert abs(float(loss) - lo) <= 5e-3 * lo
    assert errs[worst] <= tol, (worst, errs[worst])


def _launches():
    return int(_lib()[1].srk_dwconv3x3_bn_act_launches())


# ---- 1. the reference's own numbers ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["a", "b", "c"])
def test_dat_frozen_step_vs_reference_golden(tag):
    """G18: (a) model.eval() 24 x 40 batch 2, (b) model.eval() 32 x 32 batch 1, (c) model.train() with only the dwconv.1 BatchNorms in
    eval, 32 x 32 batch 2.  Output, loss, all 264 gradients; frozen buffers bit-unchanged, live ones as the golden's."""
    from test_dat_frozen_ref import g18_weights
    g, cfg, sd = g18_weights()
    m = _model(cfg, sd)
    if tag == "c":
        m.train()
        for n, mod in m.named_modules():
            if n.endswith("attn.dwconv.1"):
                mod.eval()
    else:
        m.eval()
    before = _buffers(m)
    x, t = torch.from_numpy(g[f"{tag}.x"]).cuda(), torch.from_numpy(g[f"{tag}.t"]).cuda()
    n0 = _launches()
    y = m(x)
    assert y.grad_fn is not None, "an eval-mode forward with grad enabled must build the autograd node"
    loss = F.l1_loss(y, t)
    loss.backward()
    assert _launches() - n0 == sum(cfg.depth)          # every block's DW-conv branch took the single-pass kernel
    _check_step(m, y, loss, torch.from_numpy(g[f"{tag}.y"]), float(g[f"{tag}.loss"]),
                {n: torch.from_numpy(g[f"{tag}.grad.{n}"]) for n, _ in m.named_parameters()})
    for n, b in _buffers(m).items():
        frozen = tag != "c" or ".dwconv.1." in n
        r = torch.from_numpy(g[f"{tag}.buf.{n}"])
        if frozen:
            assert torch.equal(b, before[n]), f"{n} was written"
            assert torch.equal(b.cpu(), r)
        elif n.endswith("num_batches_tracked"):
            assert int(b) == int(r) == int(before[n]) + 1
        else:
            assert float((b.cpu() - r).abs().max()) <= 2e-2 * max(float(r.abs().max()), 1e-2), n
            assert not torch.equal(b, before[n])


# ---- 2. DropPath follows model.training, BatchNorm its own flag ------------------------------------------------------------------------------
def test_dat_frozen_bn_with_drop_path_vs_oracle():
    from test_oracle_golden import DAT_TINY_816
    from tpu_superresolution_amd.training import freeze_batchnorm
    cfg = DO.DATConfig(**DAT_TINY_816)
    sd = DO.random_state_dict(cfg, seed=21, scale=2.0)
    m = _model(cfg, sd, drop_path_rate=0.3).train()
    assert freeze_batchnorm(m) == 3 * sum(cfg.depth)
    before = _buffers(m)
    gen = torch.Generator().manual_seed(4)
    x, t = torch.rand(3, 3, 24, 40, generator=gen), torch.rand(3, 3, 48, 80, generator=gen)
    torch.manual_seed(11)
    torch.cuda.manual_seed(11)
    y = m(x.cuda())
    loss = F.l1_loss(y, t.cuda())
    loss.backward()
    torch.manual_seed(11)
    torch.cuda.manual_seed(11)
    probs = [blk.drop_path_prob for layer in m.layers for blk in layer.blocks]
    keep = 1.0 - torch.tensor(probs, dtype=torch.float32, device="cuda").view(-1, 1, 1)
    drop = ((torch.rand(len(probs), 2, 3, device="cuda") < keep).float() / keep).cpu()
    assert float(drop.min()) == 0.0                                   # some branch is dropped for some sample
    lo, yo, grads = eval_loss_and_grads(sd, cfg, x, t, drop)          # running statistics (outside train_mode) + the same factors
    _check_step(m, y, loss, yo, lo, grads)
    assert all(torch.equal(b, before[n]) for n, b in _buffers(m).items())


# ---- 3. the width where the fused and tiled kernels run ---------------------------------------------------------------------------------------
def test_dat_width_180_frozen_step_vs_oracle():
    cfg = DO.DATConfig(**{**DO.DATConfig.sr_x4().__dict__, "depth": (2,), "num_heads": (6,), "upscale": 2})
    sd = DO.random_state_dict(cfg, seed=41, scale=1.0)
    m = _model(cfg, sd).eval()
    before = _buffers(m)
    gen = torch.Generator().manual_seed(13)
    x, t = torch.rand(2, 3, 64, 64, generator=gen), torch.rand(2, 3, 128, 128, generator=gen)
    n0 = _launches()
    y = m(x.cuda())
    loss = F.l1_loss(y, t.cuda())
    loss.backward()
    assert _launches() - n0 == 2, "the single-pass conv + BatchNorm + GELU kernel did not run once per block"
    lo, yo, grads = eval_loss_and_grads(sd, cfg, x, t)
    _check_step(m, y, loss, yo, lo, grads)
    assert all(torch.equal(b, before[n]) for n, b in _buffers(m).items())
    m.train()                                                          # live BatchNorm: the three-pass path, the counter stands still
    n1 = _launches()
    m(x.cuda())
    assert _launches() == n1


# ---- 4. kernels ---------------------------------------------------------------------------------------------------------------------------
class _Slice:
    """a bf16 operand [rows][C] as a column slice (from column `off`) of a NaN buffer [pad + rows + pad][ld]"""

    def __init__(self, t2d, ld, off, pad):
        rows, C = t2d.shape
        self.buf = torch.full((rows + 2 * pad, ld), float("nan"), dtype=torch.bfloat16, device="cuda")
        self.buf[pad:pad + rows, off:off + C] = t2d.to(torch.bfloat16).cuda()
        self.ptr, self.ld = self.buf[pad:, off:].data_ptr(), ld


@pytest.mark.parametrize("B,H,W,C", [(2, 11, 21, 40), (1, 16, 32, 192), (3, 8, 16, 64), (2, 9, 17, 72)])   # 72: C8 = 9, a second channel block
def test_dwconv_bn_act_single_pass_vs_the_three_pass_kernels(B, H, W, C):
    """srk_dwconv3x3_bn_act against srk_dwconv3x3 (scale 1, shift = bias) + srk_affine_act_bf16 (GELU) on the same inputs: c_pre bit-equal,
    conv equal up to one bf16 rounding (2^-8 relative).  Input in a NaN frame (rows around it, columns beside the slice), outputs in
    guarded buffers whose stride is wider than the slice."""
    check, L = _lib()
    g = torch.Generator().manual_seed(B * 100 + C)
    T = B * H * W
    x = torch.randn(T, C, generator=g)
    xs = _Slice(x, ld=C + 24, off=8, pad=W + 8)          # more NaN pixels than a halo row reaches
    w = (torch.randn(C, 9, generator=g) * 0.3).cuda()
    bias, ones = (torch.randn(C, generator=g) * 0.2).cuda(), torch.ones(C, device="cuda")
    s, t = (torch.rand(C, generator=g) + 0.5).cuda(), (torch.randn(C, generator=g) * 0.3).cuda()
    ldo = C + 8
    pre1, out1 = torch.zeros(T, ldo, dtype=torch.bfloat16, device="cuda"), torch.zeros(T, ldo, dtype=torch.bfloat16, device="cuda")
    check(L.srk_dwconv3x3(xs.ptr, xs.ld, w.data_ptr(), ones.data_ptr(), bias.data_ptr(), None, 0, pre1.data_ptr(), ldo, B, H, W, C // 8, 0, _st()))
    check(L.srk_affine_act_bf16(pre1.data_ptr(), ldo, s.data_ptr(), t.data_ptr(), out1.data_ptr(), ldo, T, C // 8, 0, 1, _st()))
    pre2, out2 = Guarded("bf16", T, C, ldo), Guarded("bf16", T, C, ldo)
    n0 = _launches()
    check(L.srk_dwconv3x3_bn_act(xs.ptr, xs.ld, w.data_ptr(), bias.data_ptr(), s.data_ptr(), t.data_ptr(), pre2.ptr, ldo, out2.ptr, ldo, B, H, W,
                                 C // 8, _st()))
    torch.cuda.synchronize()
    assert _launches() == n0 + 1
    pre2.assert_guards("c_pre")
    out2.assert_guards("conv")
    a, b = pre1[:, :C].cpu(), pre2.data()
    assert bool(torch.isfinite(b.float()).all()) and torch.equal(a.view(torch.int16), b.view(torch.int16)), "c_pre is not bit-equal"
    # and it is the conv: fp32 torch on the bf16-rounded input
    xi = x.to(torch.bfloat16).float().view(B, H, W, C).permute(0, 3, 1, 2)
    want = (F.conv2d(xi, w.cpu().reshape(C, 1, 3, 3), bias.cpu(), padding=1, groups=C)).permute(0, 2, 3, 1).reshape(T, C)
    assert float((b.float() - want).abs().max()) <= 2.0 ** -8 * float(want.abs().max()) + 1e-6
    c1, c2 = out1[:, :C].cpu().float(), out2.data().float()
    assert bool(torch.isfinite(c2).all())
    diff = (c1 - c2).abs()
    print(f"conv: {int((diff > 0).sum())} of {diff.numel()} elements differ, worst relative {float((diff / c1.abs().clamp_min(1e-30)).max()):.3e}")
    assert bool((diff <= 2.0 ** -8 * c1.abs()).all())


def test_dwconv_bn_act_argument_checks():
    from tpu_superresolution_amd._lib import SrkError
    check, L = _lib()
    buf = torch.zeros(64, 64, dtype=torch.bfloat16, device="cuda")
    f = torch.zeros(64, 9, device="cuda")
    ok = lambda **kw: L.srk_dwconv3x3_bn_act(*[kw.get(k, v) for k, v in dict(
        x=buf.data_ptr(), ldx=64, w=f.data_ptr(), bias=f.data_ptr(), s=f.data_ptr(), t=f.data_ptr(), pre=buf.data_ptr(), ldpre=64,
        out=buf.data_ptr() + 64 * 64, ldo=64, B=1, H=4, W=4, C8=8, st=_st()).items()])
    for kw, text in ((dict(pre=None), "null pointer"), (dict(ldo=60), "bad shape"), (dict(C8=65, ldx=1024, ldo=1024, ldpre=1024), "at most 512"),
                     (dict(out=buf.data_ptr()), "two buffers"), (dict(ldpre=32), "bad shape")):
        with pytest.raises(SrkError, match=text):
            check(ok(**kw))
    with pytest.raises(SrkError, match="bn_frozen_coeffs"):
        check(L.srk_bn_frozen_coeffs(16, 17, f.data_ptr(), f.data_ptr(), 1e-5, f.data_ptr(), f.data_ptr(), None, f.data_ptr(), _st()))
    with pytest.raises(SrkError, match="bn_frozen_bwd_coeffs"):
        check(L.srk_bn_frozen_bwd_coeffs(f.data_ptr(), 4, 16, 16, 8, f.data_ptr(), f.data_ptr(), _st()))          # row_stride < 2 ld
    with pytest.raises(SrkError, match="channel_interaction_frozen_fwd"):
        check(L.srk_channel_interaction_frozen_fwd(*([f.data_ptr(), 64, 1.0] + [f.data_ptr()] * 5 + [1e-5] + [f.data_ptr()] * 6 + [1, 48, 65, 64, _st()])))


@pytest.mark.parametrize("Cn,ld,padded,R", [(12, 16, False, 37), (192, 192, True, 64), (128, 128, True, 5)])
def test_bn_frozen_coefficient_kernels_vs_fp64(Cn, ld, padded, R):
    """srk_bn_frozen_coeffs / _bwd_coeffs against the formulas in fp64: scale = gamma rstd, shift = beta - mean scale, mean, rstd from the
    running buffers (through real_of in the head-padded layout); A = scale, B = C = 0, d gamma = rstd (S2 - mean S1), d beta = S1 from the
    partial rows.  Bounds: a handful of fp32 roundings on the forward (1e-6 relative to the magnitudes that enter), R + 4 roundings on the
    sums (eps = 6e-8 each, relative to the sum of the absolute terms).  Guard rows around both outputs; coef rows are ld wide, only the
    first Cn columns are written."""
    from tpu_superresolution_amd import packing as ha
    check, L = _lib()
    g = torch.Generator().manual_seed(Cn + R)
    dev = torch.device("cuda")
    if padded:
        nH, dh = Cn // 32, 30
        hm = ha._head_map(nH, dh, dev)
        real_of = torch.full((Cn,), -1, dtype=torch.int32, device=dev).scatter_(0, hm, torch.arange(nH * dh, dtype=torch.int32, device=dev))
        n_real = nH * dh
    else:
        real_of, n_real = None, Cn
    rm, rv = torch.randn(n_real, generator=g).double(), (torch.rand(n_real, generator=g) + 0.3).double()
    gam_r, bet_r = (torch.randn(n_real, generator=g) + 1.0).double(), torch.randn(n_real, generator=g).double()
    idx = real_of.cpu().long() if padded else torch.arange(Cn)
    live = idx >= 0

    def pad(v):          # module order -> padded layout, padding 0
        out = torch.zeros(Cn, dtype=torch.float64)
        out[live] = v[idx[live]]
        return out
    gam, bet = pad(gam_r), pad(bet_r)
    eps = 1e-5
    rstd = pad(1.0 / torch.sqrt(rv + eps))
    mean = pad(rm)
    want = torch.stack([gam * rstd, bet - mean * gam * rstd, mean, rstd])
    coef = Guarded("f32", 4, Cn, ld)
    rm_d, rv_d = rm.float().cuda(), rv.float().cuda()
    rm0, rv0 = rm_d.clone(), rv_d.clone()
    gd, bd = gam.float().cuda(), bet.float().cuda()
    check(L.srk_bn_frozen_coeffs(ld, Cn, gd.data_ptr(), bd.data_ptr(), eps, rm_d.data_ptr(), rv_d.data_ptr(),
                                 None if real_of is None else real_of.data_ptr(), coef.ptr, _st()))
    torch.cuda.synchronize()
    coef.assert_guards("coef")
    assert torch.equal(rm_d, rm0) and torch.equal(rv_d, rv0)
    got = coef.data().double()
    mag = torch.stack([(gam * rstd).abs(), bet.abs() + (mean * gam * rstd).abs(), mean.abs(), rstd])
    err = ((got - want).abs() / mag.clamp_min(1e-30))[:, live]
    print(f"forward coefficients: worst relative error {float(err.max()):.3e}")
    assert float(err.max()) <= 1e-6 and float(got[:, ~live].abs().max() if (~live).any() else 0.0) == 0.0
    # backward
    part = torch.randn(R, 2, ld, generator=g)
    part[:, :, Cn:] = float("nan")                                         # columns beyond C are not read
    S1, S2 = part[:, 0, :Cn].double().sum(0), part[:, 1, :Cn].double().sum(0)
    A1, A2 = part[:, 0, :Cn].double().abs().sum(0), part[:, 1, :Cn].double().abs().sum(0)
    fwd = coef.win.contiguous()                                                # what the forward kernel wrote (fp32), ld wide
    fs, fm, fr = fwd[0, :Cn].cpu().double(), fwd[2, :Cn].cpu().double(), fwd[3, :Cn].cpu().double()
    want_b = torch.stack([fs, torch.zeros(Cn).double(), torch.zeros(Cn).double(), fr * (S2 - fm * S1), S1])
    bc = Guarded("f32", 5, Cn, ld)
    pd = part.cuda()
    check(L.srk_bn_frozen_bwd_coeffs(pd.data_ptr(), R, 2 * ld, ld, Cn, fwd.data_ptr(), bc.ptr, _st()))
    torch.cuda.synchronize()
    bc.assert_guards("bwd coef")
    gb = bc.data().double()
    assert bool(torch.isfinite(gb).all())
    assert torch.equal(gb[0], fs) and float(gb[1].abs().max()) == 0.0 and float(gb[2].abs().max()) == 0.0
    tol = (R + 4) * 6e-8
    assert bool(((gb[4] - S1).abs() <= tol * A1).all())
    assert bool(((gb[3] - want_b[3]).abs() <= tol * fr * (A2 + fm.abs() * A1) + 1e-30).all())


@pytest.mark.parametrize("B", [1, 2, 16])
def test_channel_interaction_frozen_kernels_vs_autograd(B):
    """srk_channel_interaction_frozen_fwd / _bwd against dat_train._channel_interaction(frozen=True) under autograd: gate, all six parameter
    gradients (the bias in front of the BatchNorm has a real gradient here) and the pooled gradient, through the head-padded layout; no
    buffer written; guard rows around every output.  Bounds as test_dat_channel_interaction_kernels_vs_autograd."""
    from tpu_superresolution_amd import dat_train as DT
    from tpu_superresolution_amd import packing as ha
    check, L = _lib()
    C, S, nH = 180, 22, 6
    g = torch.Generator().manual_seed(B * 1000 + C)
    dh, CA, HW = C // nH, nH * 32, 64
    ci = torch.nn.Sequential(torch.nn.AdaptiveAvgPool2d(1), torch.nn.Conv2d(C, S, 1), torch.nn.BatchNorm2d(S), torch.nn.GELU(),
                             torch.nn.Conv2d(S, C, 1)).cuda()
    with torch.no_grad():
        for p_ in ci.parameters():
            p_.copy_(torch.randn(p_.shape, generator=g) * 0.5)
        ci[2].running_mean.copy_(torch.randn(S, generator=g))
        ci[2].running_var.copy_(torch.rand(S, generator=g) + 0.5)
    ci[2].eval()
    rm0, rv0, nb0 = ci[2].running_mean.clone(), ci[2].running_var.clone(), ci[2].num_batches_tracked.clone()
    hm = ha._head_map(nH, dh, torch.device("cuda"))
    pooled = torch.full((B, 2, CA), float("nan"), device="cuda")          # padding columns and the second partial row are not read
    pooled[:, 0, hm] = (torch.randn(B, C, generator=g) * HW).cuda()
    dcg = torch.full((B, CA), float("nan"), device="cuda")
    dcg[:, hm] = torch.randn(B, C, generator=g).cuda()
    pm_t = (pooled[:, 0] / HW)[:, hm].contiguous().requires_grad_(True)
    cg_t = DT._channel_interaction(pm_t, ci, frozen=True)
    want_eval = torch.sigmoid(ci[4](F.gelu(ci[2](ci[1](pm_t.detach()[:, :, None, None]))))).flatten(1)      # nn.BatchNorm2d itself, eval mode
    assert float((cg_t.detach() - want_eval).abs().max()) <= 1e-5
    params = [ci[1].weight, ci[1].bias, ci[2].weight, ci[2].bias, ci[4].weight, ci[4].bias]
    grads = torch.autograd.grad(cg_t, [pm_t] + params, dcg[:, hm])
    assert DT._ci_frozen_ok(B, C, S, ci) and int(L.srk_channel_interaction_frozen_covered(B, C, S)) == 1
    hm32 = hm.to(torch.int32)
    pm, cgate = Guarded("f32", B, C, C), Guarded("f32", B, CA, CA)
    view = pooled[:, 0]
    check(L.srk_channel_interaction_frozen_fwd(view.data_ptr(), view.stride(0), 1.0 / HW, hm32.data_ptr(), ci[1].weight.data_ptr(), ci[1].bias.data_ptr(),
                                               ci[2].weight.data_ptr(), ci[2].bias.data_ptr(), float(ci[2].eps), ci[4].weight.data_ptr(),
                                               ci[4].bias.data_ptr(), ci[2].running_mean.data_ptr(), ci[2].running_var.data_ptr(), pm.ptr, cgate.ptr,
                                               B, C, S, CA, _st()))
    torch.cuda.synchronize()
    pm.assert_guards("pm")
    cgate.assert_guards("cgate")
    rel = lambda a, b: float((a - b).norm()) / max(float(b.norm()), 1e-30)
    assert rel(pm.data(), pm_t.detach().cpu()) <= 1e-6
    cg = cgate.data()
    assert bool(torch.isfinite(cg).all())
    assert float((cg[:, hm.cpu()] - cg_t.detach().cpu()).abs().max()) <= 2e-5
    padm = torch.ones(CA, dtype=torch.bool); padm[hm.cpu()] = False
    assert float(cg[:, padm].abs().max()) == 0.0
    gk = [Guarded("f32", 1, p_.numel(), p_.numel()) for p_ in params]
    dpool = Guarded("f32", B, CA, CA)
    pmc = pm.win.contiguous()
    check(L.srk_channel_interaction_frozen_bwd(pmc.data_ptr(), dcg.data_ptr(), CA, 1.0 / HW, hm32.data_ptr(), ci[1].weight.data_ptr(), ci[1].bias.data_ptr(),
                                               ci[2].weight.data_ptr(), ci[2].bias.data_ptr(), float(ci[2].eps), ci[4].weight.data_ptr(),
                                               ci[4].bias.data_ptr(), ci[2].running_mean.data_ptr(), ci[2].running_var.data_ptr(), gk[0].ptr, gk[1].ptr,
                                               gk[2].ptr, gk[3].ptr, gk[4].ptr, gk[5].ptr, dpool.ptr, B, C, S, CA, _st()))
    torch.cuda.synchronize()
    for nm, got, want in zip(("W1", "b1", "gamma", "beta", "W2", "b2"), gk, grads[1:]):
        got.assert_guards(nm)
        assert bool(torch.isfinite(got.data()).all()), nm
        assert rel(got.data().reshape(-1), want.cpu().reshape(-1)) <= 2e-4, nm
    dpool.assert_guards("dpool")
    dp = dpool.data()
    assert rel(dp[:, hm.cpu()], (grads[0] / HW).cpu()) <= 2e-4 and float(dp[:, padm].abs().max()) == 0.0
    assert torch.equal(ci[2].running_mean, rm0) and torch.equal(ci[2].running_var, rv0) and torch.equal(ci[2].num_batches_tracked, nb0)


# ---- 5. equivalences ------------------------------------------------------------------------------------------------------------------------
def test_eval_with_grad_equals_train_with_all_batchnorm_frozen_and_matches_inference():
    """The same batch through (i) model.eval() with grad and (ii) model.train() + freeze_batchnorm with drop_path_rate 0: the same launch
    sequence, so torch.equal outputs, and gradients to the order of the fp32 atomics in a few reductions (1e-5 per tensor, measured like
    every gradient here against max(|ref|, 2e-3 * the largest norm): the tensors whose gradient is rounding noise have no relative error
    to speak of).  And the frozen training forward against the no_grad inference forward of the same weights (BatchNorm folded into the
    packed operands, other kernels): 2e-2 * max, the project's inference bound."""
    from test_dat_frozen_ref import g18_weights
    from tpu_superresolution_amd.training import freeze_batchnorm
    g, cfg, sd = g18_weights()
    x, t = torch.from_numpy(g["a.x"]).cuda(), torch.from_numpy(g["a.t"]).cuda()
    m1, m2 = _model(cfg, sd).eval(), _model(cfg, sd).train()
    freeze_batchnorm(m2)
    y1, y2 = m1(x), m2(x)
    assert y1.grad_fn is not None and y2.grad_fn is not None
    assert torch.equal(y1, y2)
    F.l1_loss(y1, t).backward()
    F.l1_loss(y2, t).backward()
    g1 = {n: p.grad.cpu() for n, p in m1.named_parameters()}
    g2 = {n: p.grad.cpu() for n, p in m2.named_parameters()}
    errs = grad_errors(g2, g1, 2e-3)
    worst = max(errs, key=errs.get)
    print(f"eval+grad vs train+frozen: worst gradient difference {errs[worst]:.3e} at {worst}")
    assert errs[worst] <= 1e-5
    with torch.no_grad():
        yi = m1(x)
        assert yi.grad_fn is None
        y3 = m2(x)                                                      # train mode without grad: the training forward, frozen statistics
    assert torch.equal(y3, y2.detach())
    d = float((y1.detach() - yi).abs().max())
    print(f"frozen training forward vs folded inference forward: {d:.3e} (bound {2e-2 * float(yi.abs().max()):.3e})")
    assert d <= 2e-2 * float(yi.abs().max())
    for p in m1.parameters():                                           # eval with no trainable parameter: the inference branch, as ever
        p.requires_grad_(False)
    assert torch.equal(m1(x), yi)


def test_a_frozen_submodule_is_respected_and_a_live_one_still_moves():
    """bn.eval() on ONE BatchNorm of a training model: its buffers stay, every other BatchNorm's move"""
    from test_dat_frozen_ref import g18_weights
    g, cfg, sd = g18_weights()
    m = _model(cfg, sd).train()
    name = "layers.0.blocks.1.attn.spatial_interaction.1"
    dict(m.named_modules())[name].eval()
    before = _buffers(m)
    x = torch.from_numpy(g["c.x"]).cuda()
    m(x).sum().backward()
    for n, b in _buffers(m).items():
        assert torch.equal(b, before[n]) == n.startswith(name + "."), n


# ---- 6. the graphed step --------------------------------------------------------------------------------------------------------------------
def test_graphed_frozen_steps_match_eager_and_the_state_is_checked():
    from test_oracle_golden import DAT_TINY
    from tpu_superresolution_amd.optim import FusedAdamW
    from tpu_superresolution_amd.training import GraphedTrainStep, freeze_batchnorm, train_step
    cfg = DO.DATConfig(**DAT_TINY)
    sd = DO.random_state_dict(cfg, seed=31, scale=1.0)
    gen = torch.Generator().manual_seed(9)
    batches = [(torch.rand(2, 3, 32, 32, generator=gen).cuda(), torch.rand(2, 3, 64, 64, generator=gen).cuda()) for _ in range(3)]
    ma, mb = _model(cfg, sd).train(), _model(cfg, sd).train()
    freeze_batchnorm(ma)
    freeze_batchnorm(mb)
    before = _buffers(mb)
    oa = FusedAdamW(ma, lr=1e-3, weight_decay=0.0, max_grad_norm=1.0)
    ob = FusedAdamW(mb, lr=1e-3, weight_decay=0.0, max_grad_norm=1.0)
    gs = GraphedTrainStep(mb, ob, warmup=1)
    train_step(ma, oa, *batches[0])          # the graphed stepper warms up with one eager step on its first batch
    la, lb = [], []
    for x, t in batches:
        loss, _ = train_step(ma, oa, x, t)
        la.append(float(loss))
        lg, bad = gs(x, t)
        lb.append(float(lg))
        assert int(bad) == 0
    print("eager", la, "graphed", lb)
    assert all(abs(a - b) <= 2e-3 * abs(a) for a, b in zip(la, lb))
    assert lb[-1] < lb[0]
    worst = ("", 0.0, 0.0)
    for (n, pa), (_, pb) in zip(ma.named_parameters(), mb.named_parameters()):
        if n.endswith("pos3.2.bias"):          # a softmax-invariant shift: its true gradient is zero, Adam random-walks it on rounding noise
            continue
        dmax, dmean = float((pa - pb).abs().max()), float((pa - pb).abs().mean())
        if dmax > worst[1]:
            worst = (n, dmax, dmean)
        assert dmax <= 4e-3 and dmean <= 2e-4, (n, dmax, dmean)
    print("largest weight difference", worst)
    for mm in (ma, mb):
        assert all(torch.equal(b, before[n]) for n, b in _buffers(mm).items()), "a frozen step moved a BatchNorm buffer"
    # the captured launch sequence belongs to the state it was captured in
    bn = dict(mb.named_modules())["layers.1.blocks.0.attn.dwconv.1"]
    bn.train()
    with pytest.raises(ValueError, match="BatchNorm training flags differ"):
        gs(*batches[0])
    bn.eval()
    mb.eval()
    with pytest.raises(ValueError, match="model.training True -> False"):
        gs(*batches[0])
    mb.train()
    with pytest.raises(ValueError, match="15 of 15 BatchNorm training flags differ"):
        gs(*batches[0])
    freeze_batchnorm(mb)
    lg, bad = gs(*batches[0])
    assert int(bad) == 0 and np.isfinite(float(lg))
    gs.close()


# ---- 7. the script --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", [False, True])
def test_finetune_script_freeze_bn_batch_of_one(graph, tmp_path, capsys, monkeypatch):
    from test_gpu_fused_optim import make_dataset
    from tpu_superresolution_amd import finetune_swinir as FS
    make_dataset(str(tmp_path), n_train=2, n_valid=1)
    monkeypatch.chdir(tmp_path)
    torch.manual_seed(5)
    start = FS.build_sr_model("dat", 4).state_dict()
    for k, v in start.items():                                          # a "pretrained" file: non-trivial running statistics
        if k.endswith("running_mean"):
            v.copy_(torch.randn(v.shape) * 0.2)
        elif k.endswith("running_var"):
            v.copy_(torch.rand(v.shape) * 0.6 + 0.7)
        elif k.endswith("num_batches_tracked"):
            v.fill_(1234)
    torch.save({"params": start}, tmp_path / "w.pth")
    FS.main(["--data_root", str(tmp_path), "--scale", "X4", "--epochs", "1", "--batch_size", "1", "--workers", "0", "--lr", "1e-4", "--arch", "dat",
             "--weights", str(tmp_path / "w.pth"), "--freeze_bn"] + (["--graph"] if graph else []))
    out = capsys.readouterr().out
    assert "[freeze_bn] 108 BatchNorm layers use their running statistics" in out
    assert "[X4] epoch 001/1" in out and "[done] best_val_loss=" in out
    ck = torch.load(tmp_path / "best_dat_finetune_X4.pt", map_location="cpu", weights_only=False)
    assert ck["args"]["freeze_bn"] is True
    bufs = [k for k in start if k.endswith(BUF)]
    assert len(bufs) == 3 * 108
    for k in bufs:
        assert torch.equal(ck["model"][k], start[k]), f"{k} moved"
    floats = [k for k, v in start.items() if v.is_floating_point() and v.numel() > 1 and not k.endswith(BUF) and "rpe_biases" not in k]
    moved = [k for k in floats if not torch.equal(ck["model"][k], start[k])]
    assert all(torch.isfinite(v).all() for v in ck["model"].values() if v.is_floating_point())
    print(f"{len(moved)} of {len(floats)} float tensors moved")
    assert len(moved) > len(floats) // 2


def test_freeze_bn_on_a_model_without_batchnorm_says_so(tmp_path, capsys, monkeypatch):
    from test_gpu_fused_optim import make_dataset
    from tpu_superresolution_amd import finetune_swinir as FS
    make_dataset(str(tmp_path), n_train=2, n_valid=1)
    monkeypatch.chdir(tmp_path)
    FS.main(["--data_root", str(tmp_path), "--scale", "X4", "--epochs", "1", "--batch_size", "2", "--workers", "0", "--arch", "swinir", "--freeze_bn"])
    out = capsys.readouterr().out
    assert "[freeze_bn] --arch swinir has no BatchNorm layer" in out and "[done] best_val_loss=" in out
