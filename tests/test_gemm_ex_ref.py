"""Pins tests/gemm_ex_ref.py (the fp64 restatement of srk_gemm_ex that tests/test_gpu_gemm_ex.py compares the kernels with) on the CPU:
against torch.nn.functional in float64, against torch.autograd for the gradient epilogues, and -- the negative controls -- shows that
the comparator with its derived tolerances rejects seven deliberately wrong references at every shape of the case matrix."""
import math

import pytest
import torch
import torch.nn.functional as F

import gemm_ex_ref as R

REL = 1e-12
SLOPE = float(torch.tensor(0.2, dtype=torch.float32))       # srk_gemm_args.scale is a float


def close(a, b):
    a, b = a.double(), b.double()
    assert a.shape == b.shape, (a.shape, b.shape)
    scale = max(float(b.abs().max()), 1e-30)
    assert float((a - b).abs().max()) <= REL * scale, float((a - b).abs().max()) / scale


def rnd(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def conv_weight_rows(wt):
    """torch conv weight [N][Cin][3][3] -> W [N][9*Cin] tap-major."""
    return wt.permute(0, 2, 3, 1).reshape(wt.shape[0], -1)


@pytest.mark.parametrize("B,H,Wd,Cin,N", [(1, 1, 1, 8, 4), (1, 1, 7, 8, 4), (3, 13, 9, 8, 6), (2, 5, 16, 4, 8)])
def test_conv_loader_is_conv2d(B, H, Wd, Cin, N):
    x, wt = rnd(B, H, Wd, Cin, seed=1), rnd(N, Cin, 3, 3, seed=2)
    c = R.conv_case(R.LD_CONV3, R.EP_BF16, B, H, Wd, Cin, N)
    acc, S = R.gemm_core(c, {"A": x, "W": conv_weight_rows(wt)})
    ref = F.conv2d(x.permute(0, 3, 1, 2), wt, padding=1).permute(0, 2, 3, 1).reshape(-1, N)
    close(acc, ref)
    close(S, F.conv2d(x.abs().permute(0, 3, 1, 2), wt.abs(), padding=1).permute(0, 2, 3, 1).reshape(-1, N))


def test_rows_loader_honours_lda():
    A, W = rnd(5, 24, seed=3), rnd(7, 16, seed=4)
    acc, _ = R.gemm_core(R.Case(R.LD_ROWS, R.EP_BF16, M=5, N=7, K=16, lda=24), {"A": A, "W": W})
    close(acc, A[:, :16] @ W.t())


@pytest.mark.parametrize("r,Cs", [(2, 4), (3, 2), (4, 1)])
def test_ps_store_is_pixel_shuffle(r, Cs):
    B, H, Wd = 2, 3, 5
    u = rnd(B * H * Wd, r * r * Cs, seed=5)                         # column (i*r + j)*Cs + c
    t = u.reshape(B, H, Wd, r * r, Cs).permute(0, 4, 3, 1, 2).reshape(B, Cs * r * r, H, Wd)      # torch order c*r*r + i*r + j
    close(R.ps_store(u, B, H, Wd, r, Cs), F.pixel_shuffle(t, r).permute(0, 2, 3, 1))
    # the loader of the pixel-shuffled source is its inverse
    close(R.unshuffle_source(R.ps_store(u, B, H, Wd, r, Cs), r).reshape(-1, r * r * Cs), u)


@pytest.mark.parametrize("r,Cimg", [(1, 3), (2, 3), (3, 1), (4, 1)])
def test_ps_img_store_is_pixel_shuffle_to_nchw(r, Cimg):
    B, H, Wd = 2, 3, 5
    u = rnd(B * H * Wd, 16, seed=6)                                 # column c*r*r + i*r + j: torch's own order
    t = u[:, :Cimg * r * r].reshape(B, H, Wd, -1).permute(0, 3, 1, 2)
    close(R.ps_img_store(u, B, H, Wd, r, Cimg), F.pixel_shuffle(t, r))


def test_pointwise_epilogues_are_torch_functional():
    u = 3.0 * rnd(64, 48, seed=7)
    close(R.gelu(u), F.gelu(u))
    x = u.clone().requires_grad_(True)
    (gy,) = torch.autograd.grad(F.gelu(x).sum(), x)
    close(R.dgelu(u), gy)
    assert abs(float(R.dgelu(torch.linspace(-8, 8, 160001, dtype=torch.float64)).abs().max()) - 1.1290) < 1e-3 <= R.GELU_LIP - 1.1290 + 1e-3


def _tiny_rows_case(ep, M=9, N=64, K=64, **kw):
    c = R.Case(R.LD_ROWS, ep, M=M, N=N, K=K, **kw)
    return c, R.make_inputs(c)


def test_reference_epilogues_against_torch_and_autograd():
    # BF16 / GELU / LRELU / RES / RES_BF16 (+ row scale): forward formulas
    c, inp = _tiny_rows_case(R.EP_GELU)
    acc, _ = R.gemm_core(c, inp)
    u = acc + inp["bias"].double()
    out = R.reference(c, inp)
    close(out["outb"].ref, F.linear(inp["A"].double()[:, :64], inp["W"].double(), inp["bias"].double()))
    close(out["outb2"].ref, F.gelu(u))
    c, inp = _tiny_rows_case(R.EP_LRELU, scale=0.2)
    close(R.reference(c, inp)["outb"].ref, F.leaky_relu(R.gemm_core(c, inp)[0] + inp["bias"].double(), SLOPE))
    c, inp = _tiny_rows_case(R.EP_RES, M=10, rps=4, xn_C=60)
    u = R.gemm_core(c, inp)[0] + inp["bias"].double()
    f = inp["rowscale"].double()[torch.arange(10) // 4][:, None]
    out = R.reference(c, inp)
    close(out["outf"].ref, inp["res"].double() + f * u)
    close(out["outb"].ref, out["outf"].ref)
    xn, mean, rstd = R.ln_fwd(out["outf"].ref, inp["xn_gamma"].double(), inp["xn_beta"].double(), 60)
    close(xn[:, :60], F.layer_norm(out["outf"].ref[:, :60], (60,), inp["xn_gamma"].double()[:60], inp["xn_beta"].double()[:60], 1e-5))
    assert float(xn[:, 60:].abs().max()) == 0.0
    close(mean, out["outf"].ref[:, :60].mean(1))
    close(rstd, (out["outf"].ref[:, :60].var(1, unbiased=False) + 1e-5).rsqrt())
    c, inp = _tiny_rows_case(R.EP_RES_BF16)
    close(R.reference(c, inp)["outb"].ref, inp["res"].double() + R.gemm_core(c, inp)[0] + inp["bias"].double())
    # DGELU / DLRELU: the gradient through the activation, by autograd
    c, inp = _tiny_rows_case(R.EP_DGELU)
    acc = R.gemm_core(c, inp)[0]
    z = inp["aux"].double().requires_grad_(True)
    (gz,) = torch.autograd.grad(F.gelu(z), z, acc)
    close(R.reference(c, inp)["outb"].ref, gz)
    c, inp = _tiny_rows_case(R.EP_DLRELU, scale=0.2)
    acc = R.gemm_core(c, inp)[0]
    z = rnd(9, 64, seed=8).requires_grad_(True)
    y = F.leaky_relu(z, SLOPE)
    (gz,) = torch.autograd.grad(y, z, acc)
    inp["aux"] = y.detach()                                     # aux is the activation's OUTPUT
    close(R.reference(c, inp)["outb"].ref, gz)
    aux0 = torch.tensor([[0.0, -0.0, 1.0, -1.0]], dtype=torch.float64).repeat(9, 16)
    inp["aux"] = aux0
    close(R.reference(c, inp)["outb"].ref, acc * torch.where(aux0 > 0, 1.0, SLOPE))       # both zeros take the slope


@pytest.mark.parametrize("N,C", R.LN_NC)
def test_lnbwd_reference_is_autograd_of_layer_norm(N, C):
    M = 11
    c = R.Case(R.LD_ROWS, R.EP_LNBWD, M=M, N=N, K=64, ln_C=C, rps=4)
    inp = R.make_inputs(c)
    # exact statistics for the pin (the device is handed fp32 roundings of them)
    x = inp["ln_x"].double()
    mean = x[:, :C].mean(1)
    inp["ln_mean"], inp["ln_rstd"] = mean, (x[:, :C].var(1, unbiased=False) + 1e-5).rsqrt()
    acc = R.gemm_core(c, inp)[0]
    xg = x[:, :C].clone().requires_grad_(True)
    g = inp["ln_gamma"].double()[:C].clone().requires_grad_(True)
    b = torch.zeros(C, dtype=torch.float64, requires_grad=True)
    y = F.layer_norm(xg, (C,), g, b, 1e-5)
    dx, dg, db = torch.autograd.grad(y, (xg, g, b), acc[:, :C])
    out = R.reference(c, inp)
    close(out["outf"].ref[:, :C], inp["outf0"].double()[:, :C] + dx)
    assert torch.equal(out["outf"].ref[:, C:], inp["outf0"].double()[:, C:])
    close(out["ln_dgamma"].ref[0], inp["dgamma0"].double()[:C] + dg)
    close(out["ln_dbeta"].ref[0], inp["dbeta0"].double()[:C] + db)
    f = inp["rowscale"].double()[torch.arange(M) // 4][:, None]
    close(out["outb"].ref, out["outf"].ref * f)


@pytest.mark.parametrize("r,Cs", [(2, 4), (3, 2)])
def test_pixel_shuffled_loader_is_input_gradient_of_conv_pixelshuffle(r, Cs):
    """LD_CONV3_PS + EP_BF16 with the transposed (and flipped) weights == d/dx of pixel_shuffle(conv2d(x, w))."""
    B, H, Wd, Cin = 2, 4, 5, 6
    CinP = r * r * Cs
    x = rnd(B, Cin, H, Wd, seed=9).requires_grad_(True)
    wt = rnd(CinP, Cin, 3, 3, seed=10)                              # torch output channel o = c*r*r + i*r + j
    y = F.pixel_shuffle(F.conv2d(x, wt, padding=1), r)              # [B][Cs][H*r][Wd*r]
    dy = rnd(*y.shape, seed=11)
    (dx,) = torch.autograd.grad(y, x, dy)
    # column n = (i*r + j)*Cs + c of the logical source <-> torch channel o(n)
    n = torch.arange(CinP)
    o = (n % Cs) * r * r + n // Cs
    wd = wt[o].flip(2, 3).permute(1, 2, 3, 0).reshape(Cin, 9 * CinP)          # [ci][tap][n]
    c = R.conv_case(R.LD_CONV3_PS, R.EP_BF16, B, H, Wd, CinP, Cin, r=r, Cs=Cs)
    acc, _ = R.gemm_core(c, {"A": dy.permute(0, 2, 3, 1).contiguous(), "W": wd})
    close(acc, dx.permute(0, 2, 3, 1).reshape(-1, Cin))


def test_image_heads_reference():
    c = R.conv_case(R.LD_CONV3, R.EP_PS_IMG, 2, 4, 8, 64, 16, r=2, Cimg=3, crop=(3, 5))
    inp = R.make_inputs(c)
    u = R.gemm_core(c, inp)[0] + inp["bias"].double()
    inv = float(torch.tensor(R.IMG_INV_RANGE, dtype=torch.float32))
    mean = torch.tensor(R.IMG_MEAN[:3], dtype=torch.float32).double()[None, :, None, None]
    full = F.pixel_shuffle(u[:, :12].reshape(2, 4, 8, 12).permute(0, 3, 1, 2), 2) * inv + mean
    close(R.reference(c, inp)["outf"].ref, full[:, :, :5, :11].reshape(-1, 11))
    c = R.conv_case(R.LD_CONV3, R.EP_PS_IMG, 1, 4, 8, 64, 16, r=1, Cimg=3, res4=True)
    inp = R.make_inputs(c)
    u = R.gemm_core(c, inp)[0] + inp["bias"].double()
    full = (u[:, :3] + inp["res"].double()[:, :3]).reshape(1, 4, 8, 3).permute(0, 3, 1, 2) * inv + mean
    close(R.reference(c, inp)["outf"].ref, full.reshape(-1, 8))
    c = R.conv_case(R.LD_CONV3, R.EP_IMG, 2, 6, 9, 64, 16, Cimg=1, crop=(3, 5))
    inp = R.make_inputs(c)
    u = R.gemm_core(c, inp)[0] + inp["bias"].double()
    full = u[:, :1].reshape(2, 6, 9, 1).permute(0, 3, 1, 2) * inv + mean[:, :1]
    close(R.reference(c, inp)["outf"].ref, full[:, :, :3, :4].reshape(-1, 4))


@pytest.mark.parametrize("c", R.exact_cases(), ids=lambda c: c.id)
def test_exact_gather_agrees_with_the_reference(c):
    """Two formulations of the index maps (slices vs im2col + reshape / permute) give the same integers, exactly."""
    inp = R.make_inputs(c)
    out = R.reference(c, inp)
    (name,) = out.keys()
    exp = R.exact_expected(c, inp)
    assert torch.equal(exp, out[name].ref)
    assert torch.equal(R.round_as(exp, out[name].kind), exp), "not representable: the case would not be bit-exact on the device"
    assert float(exp.abs().max()) > 0 and exp.unique().numel() > 16


def test_case_matrix_covers_every_instantiated_pair():
    vals = R.value_cases() + R.stream_cases()
    ids = [c.id for c in vals + R.exact_cases()]
    assert len(ids) == len(set(ids)), sorted(i for i in ids if ids.count(i) > 1)
    for ld, eps in R.SUPPORTED.items():
        for ep in eps:
            assert any(c.loader == ld and c.ep == ep for c in vals), (ld, ep)
    for ld, ep in R.INDEX_MAP_PAIRS:
        assert any(c.loader == ld and c.ep == ep for c in R.exact_cases()), (ld, ep)
    # every axis value of the issue's shape lists is used
    rows = [c for c in R.value_cases() if c.loader == R.LD_ROWS]
    assert {c.M for c in rows} >= set(R.TILE_M) and {c.N for c in rows} >= set(R.TILE_N) and {c.K for c in rows} >= set(R.TILE_K)
    for ep in (R.EP_BF16, R.EP_GELU, R.EP_RES, R.EP_RES_BF16, R.EP_LRELU, R.EP_DGELU, R.EP_DLRELU):
        fam = [c for c in rows if c.ep == ep]
        assert any(c.M % 128 for c in fam) and any(c.M % 128 == 0 for c in fam)
        assert any(c.LDO > c.N for c in fam) and any(c.LDA > c.K for c in fam)
    conv = [c for c in R.value_cases() if c.loader == R.LD_CONV3]
    assert {c.conv[:3] for c in conv} >= set(R.CONV_SHAPES) and {c.conv[3] for c in conv} >= set(R.CONV_CIN)
    assert {(c.r, c.Cs) for c in conv if c.ep == R.EP_PS} >= set(R.PS_RC)
    assert {(c.r, c.Cs, c.conv[2]) for c in R.value_cases() if c.loader == R.LD_CONV3_PS} >= set(
        (r, s, w) for (r, s), w in zip(R.PS_RC, (9, 40, 128, 160)))
    assert {(c.N, c.xn_C) for c in rows if c.xn_C} >= set(R.LN_NC) and {(c.N, c.ln_C) for c in rows if c.ln_C} >= set(R.LN_NC)
    st = R.stream_cases()
    assert all(R.stream_path(c, 256, False) == "tile" for c in st)
    assert sum(R.stream_path(c, 256, True) == "stream" for c in st) >= 12
    assert any(c.ep == R.EP_LNBWD and c.K == 576 and R.stream_path(c, 256, True) == "stream" for c in st)
    assert any(c.rps == 96 and R.stream_path(c, 256, True) == "tile" for c in st)


_ALL = R.value_cases() + R.stream_cases()


@pytest.mark.parametrize("c", _ALL, ids=lambda c: c.id)
def test_negative_controls_are_rejected_at_every_shape(c):
    """The comparator must be able to fail: each deliberately wrong reference, rounded to the output's format as a kernel would, is
    rejected by the derived tolerance at every shape where the control applies (no accepted control)."""
    inp = R.make_inputs(c)
    core = R.gemm_core(c, inp)
    ref = R.reference(c, inp, core)
    # the reference itself, rounded as the device rounds, is accepted (the bound is not vacuous the other way round)
    for name, o in ref.items():
        ok, ratio = R.compare(o.rounded(), o)
        assert ok, (name, ratio)
    controls = R.controls_for(c)
    accepted = []
    for label, v in controls.items():
        wrong = R.reference(c, inp, None if (v.mirror_tap is not None or (v.swap_ij and c.loader == R.LD_CONV3_PS)) else core, v)
        if all(R.compare(wrong[name].rounded(), ref[name])[0] for name in ref):
            accepted.append(label)
    if c.xn_C and c.xn_C < c.N:
        outf = ref["outf"].rounded().float()
        right = R.ln_stage2(c, inp, outf)
        for name, o in right.items():
            assert R.compare(o.rounded(), o)[0], name
        wrong = R.ln_stage2_over_N(c, inp, outf)
        if all(R.compare(R.round_as(wrong[name], right[name].kind), right[name])[0] for name in right):
            accepted.append("LayerNorm over N columns")
    assert not accepted, accepted
