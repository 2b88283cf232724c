"""CPU pins of tests/glue_ref.py: every restatement against torch in fp64, the case matrix's coverage claims, the special-value list,
and the negative controls -- each mutant of a reference must be REJECTED by the comparator of the GPU test at every case shape (or be
the reference itself by construction, which is asserted as an identity, not skipped)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gemm_ex_ref as G
import glue_ref as R


def f32(exp):
    """What a perfect fp32 kernel would return: the fp64 reference rounded once."""
    return {k: o.ref.float() for k, o in exp.items()}


# ---- LayerNorm ---------------------------------------------------------------------------------------------------------------------
def test_case_matrix_instantiates_every_layernorm_path():
    """From the case lists alone: NV = CP / 64 in {1, 2, 3, 4}, a ragged float4 (C % 4 != 0), a partial wave (rows % 4 != 0), a partial
    workgroup (rows % 16 != 0) and more than one pass of the capped grid, for both kernels; and the (C, CP) / rows the issue names."""
    for cases, cap in ((R.LN_FWD_CASES, R.LN_FWD_GRID_CAP), (R.LN_BWD_CASES, R.LN_BWD_GRID_CAP)):
        cov = R.ln_coverage(cases, cap)
        assert cov["NV"] == [1, 2, 3, 4] and cov["ragged_float4"] and cov["partial_wave"] and cov["partial_group"] and cov["grid_passes"] >= 2
        assert {(c.C, c.CP) for c in cases} == set(R.LN_C_CP)
        for C, CP in R.LN_C_CP:
            assert {c.rows for c in cases if (c.C, c.CP) == (C, CP)} >= set(R.LN_ROWS)
        assert any(c.rows == cap * 16 + 19 and c.CP == 64 for c in cases)
    # 61 = 15 float4 + 1, 181 = 45 float4 + 1, 129 = 32 float4 + 1, 250 = 62 float4 + 2: masks c + 1 < C, c + 2 < C and c + 3 < C all cut
    assert {C % 4 for C, _ in R.LN_C_CP} >= {0, 1, 2}


@pytest.mark.parametrize("C,CP", R.LN_C_CP)
def test_layernorm_references_match_torch(C, CP):
    c = R.LnCase(C, CP, 19)
    i = R.ln_inputs(c)
    x = i["x"].double().requires_grad_(True)
    gm, bt = i["gamma"].double().requires_grad_(True), i["beta"].double().requires_grad_(True)
    y = F.layer_norm(x[:, :C], (C,), gm, bt, G.LN_EPS)
    e = R.ln_fwd_ref(i["x"], i["gamma"], i["beta"], C)
    assert torch.allclose(e["y"].ref[:, :C], y.detach(), rtol=1e-12, atol=1e-12) and float(e["y"].ref[:, C:].abs().max() if C < CP else 0) == 0
    xc = i["x"][:, :C].double()
    assert torch.allclose(e["mean"].ref, xc.mean(1), rtol=1e-13, atol=1e-15)
    assert torch.allclose(e["rstd"].ref, (xc.var(1, unbiased=False) + G.LN_EPS).rsqrt(), rtol=1e-11)
    dy = i["dy"].double()
    y.backward(dy[:, :C])
    # the backward restatement on the EXACT statistics is autograd's gradient
    b = R.ln_bwd_ref(i["dy"], i["x"], e["mean"].ref, e["rstd"].ref, i["gamma"], C, 0, i["gx0"], torch.zeros(C), torch.zeros(C))
    scale = float(x.grad.abs().max())
    assert float((b["gx"].ref[:, :C] - x.grad[:, :C]).abs().max()) <= 1e-9 * max(scale, 1.0)
    assert torch.allclose(b["dgamma"].ref, gm.grad, rtol=1e-9, atol=1e-9) and torch.allclose(b["dbeta"].ref, bt.grad, rtol=1e-12, atol=1e-12)
    # accumulate and the second call
    b2 = R.ln_bwd_ref(i["dy"], i["x"], e["mean"].ref, e["rstd"].ref, i["gamma"], C, 1, i["gx0"], i["dgamma0"], i["dbeta0"], calls=2)
    assert torch.allclose(b2["gx"].ref, i["gx0"].double() + 2 * b["gx"].ref, rtol=1e-12, atol=1e-12)
    assert torch.allclose(b2["dgamma"].ref, i["dgamma0"].double() + 2 * b["dgamma"].ref, rtol=1e-12, atol=1e-12)
    assert torch.equal(b2["gx"].ref[:, C:], i["gx0"].double()[:, C:])                  # pad columns: old, unchanged


@pytest.mark.parametrize("c", R.LN_FWD_CASES, ids=lambda c: c.id)
def test_layernorm_forward_controls(c):
    i = R.ln_inputs(c)
    e = R.ln_fwd_ref(i["x"], i["gamma"], i["beta"], c.C)
    ok, ratios = R.accepts(f32(e), e)
    assert ok and max(ratios.values()) < 0.5, ratios          # the rounded reference itself sits well inside the bounds
    for mut in R.LN_FWD_MUTANTS:
        m = f32(R.ln_fwd_ref(i["x"], i["gamma"], i["beta"], c.C, mut=mut))
        if R.ln_identity(mut, c):
            assert all(torch.equal(m[k], f32(e)[k]) for k in m), mut
        else:
            assert not R.accepts(m, e)[0], (c.id, mut)


@pytest.mark.parametrize("c", R.LN_BWD_CASES, ids=lambda c: c.id)
def test_layernorm_backward_controls(c):
    i = R.ln_inputs(c)
    st = R.ln_fwd_ref(i["x"], i["gamma"], i["beta"], c.C)
    mean32, rstd32 = st["mean"].ref.float(), st["rstd"].ref.float()
    for acc in (0, 1):
        args = (i["dy"], i["x"], mean32, rstd32, i["gamma"], c.C, acc, i["gx0"], i["dgamma0"], i["dbeta0"])
        e = R.ln_bwd_ref(*args)
        ok, ratios = R.accepts(f32(e), e)
        assert ok and max(ratios.values()) < 0.5, ratios
        for mut in R.LN_BWD_MUTANTS:
            if mut == "acc_ignores_old" and not acc:
                continue                                       # the mutant is about accumulate = 1
            m = f32(R.ln_bwd_ref(*args, mut=mut))
            if R.ln_identity(mut, c):
                assert all(torch.equal(m[k], f32(e)[k]) for k in m), mut
            else:
                assert not R.accepts(m, e)[0], (c.id, acc, mut)


# ---- special values, element-wise helpers, rowscale -----------------------------------------------------------------------------------
def test_special_value_list_is_what_it_claims():
    s = R.specials()
    b = s.view(torch.int32).numpy().view(np.uint32).astype(np.uint64)
    up = (s.to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)).astype(np.uint64)      # torch's RNE conversion
    hi, lo, odd = b >> 16, b & 0xFFFF, (b >> 16) & 1
    finite = ((b >> 23) & 0xFF) != 0xFF
    assert np.any(finite & (lo == 0x8000) & (odd == 0) & (up == hi)), "a tie that rounds DOWN to the even neighbour"
    assert np.any(finite & (lo == 0x8000) & (odd == 1) & (up == hi + 1)), "a tie that rounds UP to the even neighbour"
    assert np.any(finite & ((up & 0x7FFF) == 0x7F80)), "a finite value that rounds up to bf16 infinity"
    assert np.any(b == 0) and np.any(b == 0x80000000), "+0 and -0"
    assert np.any(b == 0x7F800000) and np.any(b == 0xFF800000), "+Inf and -Inf"
    nan = ~finite & ((b & 0x7FFFFF) != 0)
    assert np.any(nan) and np.all(((up[nan] & 0x7F80) == 0x7F80) & ((up[nan] & 0x7F) != 0)), "NaN stays NaN"
    sub = (((b >> 23) & 0xFF) == 0) & ((b & 0x7FFFFF) != 0)
    assert sub.sum() >= 4 and np.any(sub & (b >> 31 == 1)) and np.any(sub & (b >> 31 == 0)), "fp32 subnormals of both signs"
    assert np.any(sub & (lo == 0x8000)), "a subnormal tie"
    # RNE restated on the bits for every finite entry: torch's conversion is the expectation the GPU test uses
    rne = (b + 0x7FFF + odd) >> 16
    assert np.array_equal(up[finite], rne[finite] & 0xFFFF)
    # the input builder really places them, singly and in pairs, and the expectations are IEEE
    a, bb = R.elem_inputs(1028)
    k = len(s)
    assert R.same_bits(a[:k], s) and bool((bb[:k] == 0).all())
    assert R.same_bits(a[k:k + k * k].view(k, k)[:, 0].contiguous(), s) and R.same_bits(bb[k:2 * k].contiguous(), s)
    e = R.elem_expected("add_f32", a, bb)["out"]
    assert R.same_bits(e, (a.double() + bb.double()).float())            # one fp32 add == the rounded exact sum
    assert bool(e[:k][s.isnan()].isnan().all()) and bool(e[k + 11 * k + 12].isnan())   # Inf + -Inf
    for name, n in R.ELEM_BIG.items():
        cap = 16384 if name == "add_f32" else 8192
        assert n % 4 == 0 and n // 4 > cap * 256, name                    # more than one pass of the launcher's capped grid


def test_same_bits_comparators():
    w = torch.tensor([1.0, float("nan"), 1e-40, -1e-40, 0.0])
    assert R.same_bits(w.clone(), w) and not R.same_bits(torch.tensor([1.0, float("nan"), 0.0, -0.0, 0.0]), w)
    assert R.same_bits_or_flushed(torch.tensor([1.0, float("nan"), 0.0, -0.0, 0.0]), w)
    assert not R.same_bits_or_flushed(torch.tensor([1.0, float("nan"), -0.0, -0.0, 0.0]), w)      # a zero of the wrong sign
    assert not R.same_bits_or_flushed(torch.tensor([0.0, float("nan"), 1e-40, -1e-40, 0.0]), w)   # a flushed NORMAL value


@pytest.mark.parametrize("c", R.ROWSCALE_CASES, ids=lambda c: c.id)
def test_rowscale_reference_and_control(c):
    src, f = R.rowscale_inputs(c)
    assert c.rows % c.rps != 0 or c.rps == 1, "the rows end in the middle of a sample"
    assert bool((f == 0).any()) and bool((f == torch.tensor(1.0 / 0.9)).any())
    want = R.rowscale_expected(src, f, c.rps)
    loop = torch.stack([(src[t].float() * f[t // c.rps]).to(torch.bfloat16) for t in range(min(c.rows, 300))])
    assert R.same_bits(want[:len(loop)], loop)
    assert not R.same_bits(R.rowscale_expected(src, f, c.rps, mut="mod_index"), want)
    if c.rows > 1000:
        assert c.rows * (c.CP // 4) > R.ROWSCALE_GRID_CAP * 256


# ---- img_prep, stem conv -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", R.IMG_CASES, ids=lambda c: c.id)
def test_img_prep_reference_and_controls(c):
    x = R.img_inputs(c)
    want = R.img_prep_expected(x, c.H, c.W)
    m = torch.tensor(R.IMG_MEAN[:c.Cimg], dtype=torch.float32).view(1, -1, 1, 1)
    ref = ((F.pad(x, (0, c.W - c.W0, 0, c.H - c.H0), mode="reflect") - m) * torch.tensor(R.IMG_RANGE)).permute(0, 2, 3, 1)
    assert torch.equal(want[..., :c.Cimg], ref) and float(want[..., c.Cimg:].abs().max()) == 0
    for mut in R.IMG_MUTANTS:
        got = R.img_prep_expected(x, c.H, c.W, mut=mut)
        assert torch.equal(got, want) == R.img_identity(mut, c), (c.id, mut)
    if c.H0 >= 1024:
        assert c.B * c.H * c.W > R.IMG_GRID_PASS


def test_img_cases_cover_the_issue():
    geo = {(c.H - c.H0, c.W - c.W0) for c in R.IMG_CASES}
    assert (0, 0) in geo and any(a == 0 and b > 0 for a, b in geo) and any(c.H - c.H0 == c.H0 - 1 for c in R.IMG_CASES)
    assert {c.Cimg for c in R.IMG_CASES} == {1, 2, 3} and all(c.B == 2 for c in R.IMG_CASES)


@pytest.mark.parametrize("c", R.STEM_CASES, ids=lambda c: c.id)
def test_stem_reference_and_controls(c):
    img, w, b = R.stem_inputs(c)
    e = R.stem_ref(img, w, b, c.CP)
    ref = F.conv2d(img[..., :c.Cin].double().permute(0, 3, 1, 2), w.double(), b.double(), padding=1).permute(0, 2, 3, 1).reshape(-1, c.C)
    assert torch.allclose(e.ref[:, :c.C], ref, rtol=1e-12, atol=1e-12)
    assert float(e.ref[:, c.C:].abs().max()) == 0 and float(e.tol[:, c.C:].abs().max()) == 0        # pad columns: exactly 0
    assert R.accepts({"y": e.ref.float()}, {"y": e})[0]
    for mut in R.STEM_MUTANTS:
        m = R.stem_ref(img, w, b, c.CP, mut=mut).ref.float()
        if R.stem_identity(mut, c):
            assert torch.equal(m, e.ref.float()), mut
        else:
            assert not R.accepts({"y": m}, {"y": e})[0], (c.id, mut)


# ---- window attention on the padded frame --------------------------------------------------------------------------------------------
def _attn_loop(qkv, bias, c):
    """The same operation the long way round: torch.roll on the zero-padded frame, one window at a time, the shift mask from region
    labels written with slices (dat_arch.py's calculate_mask)."""
    B, H, W, nH, dh = c.B, c.H, c.W, c.nH, c.dh
    Hp, Wp = c.frame
    sy, sx = c.shifts
    x = qkv.double().view(B, H, W, 3, c.layout_heads, 32)[..., :nH, :dh]
    xp = torch.roll(F.pad(x, (0, 0, 0, 0, 0, 0, 0, Wp - W, 0, Hp - H)), (-sy, -sx), (1, 2))
    lab = torch.zeros(Hp, Wp)
    if c.shift:
        n = 0
        for ys in (slice(0, -c.wh), slice(-c.wh, -sy), slice(-sy, None)):
            for xs in (slice(0, -c.ww), slice(-c.ww, -sx), slice(-sx, None)):
                lab[ys, xs] = n
                n += 1
    out = torch.zeros(B, Hp, Wp, nH, dh, dtype=torch.float64)
    for b in range(B):
        for wy in range(Hp // c.wh):
            for wx in range(Wp // c.ww):
                ys, xs = slice(wy * c.wh, (wy + 1) * c.wh), slice(wx * c.ww, (wx + 1) * c.ww)
                t = xp[b, ys, xs].reshape(-1, 3, nH, dh)
                lw = lab[ys, xs].reshape(-1)
                mask = torch.where(lw[:, None] != lw[None, :], -100.0, 0.0).double()
                for h in range(nH):
                    s = (t[:, 0, h] * dh ** -0.5) @ t[:, 1, h].t() + bias[h].double() + mask
                    out[b, ys, xs, h] = (s.softmax(-1) @ t[:, 2, h]).reshape(c.wh, c.ww, dh)
    return torch.roll(out, (sy, sx), (1, 2))[:, :H, :W]


@pytest.mark.parametrize("c", [R.AttnCase(8, 16, True, 10, 20, B=1, nH=1, dh=4), R.AttnCase(16, 8, False, 20, 9, B=2, nH=2, dh=4)],
                         ids=lambda c: c.id)
def test_attention_reference_matches_a_window_loop(c):
    qkv, bias = R.attn_inputs(c)
    assert c.frame != (c.H, c.W)
    assert torch.allclose(R.attn_fwd_ref(qkv, bias, c), _attn_loop(qkv, bias, c), rtol=1e-10, atol=1e-12)


@pytest.mark.parametrize("c", R.ATTN_CASES, ids=lambda c: c.id)
def test_attention_controls(c):
    qkv, bias = R.attn_inputs(c)
    ref = R.attn_fwd_ref(qkv, bias, c)
    assert R.attn_accepts(ref.to(torch.bfloat16), ref)[0]
    for mut in R.ATTN_MUTANTS:
        m = R.attn_fwd_ref(qkv, bias, c, mut=mut)
        if R.attn_identity(mut, c):
            assert torch.equal(m, ref), mut
        else:
            assert not R.attn_accepts(m.to(torch.bfloat16), ref)[0], (c.id, mut)


def test_attention_case_list_and_uniform_case():
    assert [(c.wh, c.ww, c.shift, c.H, c.W) for c in R.ATTN_CASES] == [(8, 32, True, 32, 64), (32, 8, False, 24, 40), (8, 16, True, 24, 40),
                                                                      (16, 8, True, 32, 32), (16, 16, True, 32, 48)]
    assert all((c.B, c.nH, c.layout_heads, c.dh) == (2, 2, 4, 12) for c in R.ATTN_CASES)
    assert any(c.frame != (c.H, c.W) and c.shift for c in R.ATTN_CASES) and any(c.wh * c.ww == 128 for c in R.ATTN_CASES)
    # q = 0, bias = 0: the general reference gives the window sum of v over N, padded tokens counted
    c = R.attn_uniform_case()
    qkv, bias, want = R.attn_uniform_inputs(c)
    assert c.frame != (c.H, c.W) and not c.shift
    ref = R.attn_fwd_ref(qkv, bias, c)
    assert torch.allclose(ref, (ref * 128).round() / 128, rtol=0, atol=1e-12)                # integers over N = 128
    assert torch.equal(ref.to(torch.bfloat16), want)
    only_real = R.attn_fwd_ref(qkv, bias, c, mut="real_keys_only")
    assert not torch.equal(only_real.to(torch.bfloat16), want)                                # the rule is visible in this case


# ---- gates -----------------------------------------------------------------------------------------------------------------------------
def test_channel_gate_reference_matches_torch():
    conv, w1, b1, w2, b2 = R.channel_gate_inputs()
    B, HW, C, CP = (R.GATE_SHAPE[k] for k in ("B", "HW", "C", "CP"))
    assert HW % 256 != 0                                                    # the last 256-row chunk is partial
    mean = conv.double().reshape(B, HW, CP)[:, :, :C].mean(1)
    for act, fn in ((0, torch.relu), (1, lambda z: F.gelu(z))):
        want = R.GATE_SHAPE["out_scale"] * torch.sigmoid(fn(mean @ w1.double().t() + b1.double()) @ w2.double().t() + b2.double())
        got = R.channel_gate_ref(conv, w1, b1, w2, b2, act)
        assert torch.allclose(got[:, :C], want, rtol=1e-12, atol=1e-15) and float(got[:, C:].abs().max()) == 0
    # the two activations differ by far more than the bound: a kernel that ignored `act` would be caught
    d = (R.channel_gate_ref(conv, w1, b1, w2, b2, 1) - R.channel_gate_ref(conv, w1, b1, w2, b2, 0)).abs().max()
    assert float(d) > 100 * R.GATE_TOL


def test_spatial_gate_inputs_replay_the_existing_test():
    a, W0, b0, w3, b3, T, CP, S = R.spatial_gate_inputs()
    assert a.shape == (T, CP) and W0.shape == (S, CP) and b0.shape == (S,) and w3.shape == (S,) and (T, CP, S, b3) == (200, 192, 11, 0.3)
