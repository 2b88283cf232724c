"""CPU pins of tests/dat_ref.py: every restatement against torch.nn.functional / autograd in fp64 (1e-12), the coverage claims of the case
lists, and the negative controls -- each mutant of a restatement must be REJECTED by the comparator of the GPU test under the derived
tolerances at every case that exercises it, or be the reference itself by construction (asserted as an identity, not skipped)."""
import pytest
import torch
import torch.nn.functional as F

import dat_ref as R
from dat_ref import BF

BF16_KEYS = {"out", "dx", "da", "db", "d_chan", "d_tok"}


def perfect(exp):
    """What a perfect kernel would store: the fp64 reference rounded once to the output's type."""
    return {k: (o.ref.to(BF) if k in BF16_KEYS else o.ref.float()) for k, o in exp.items()}


def close(a, b, tol=1e-12):
    scale = max(1.0, float(b.abs().max())) if b.numel() else 1.0
    return float((a - b).abs().max()) <= tol * scale if b.numel() else True


def controls(ref_fn, mutants, identity=lambda m: False, exercised=lambda m: True, what=""):
    e = ref_fn(None)
    good = perfect(e)
    ok, ratios = R.accepts(good, e)
    assert ok, (what, ratios)
    for mut in mutants:
        m = perfect(ref_fn(mut))
        if identity(mut):
            assert all(R.same_bits(m[k], good[k]) for k in m), (what, mut, "claimed to be the reference by construction")
        elif exercised(mut):
            assert not R.accepts(m, e)[0], (what, mut, "accepted")


# ---- row LayerNorm ---------------------------------------------------------------------------------------------------------------------
def test_rowln_case_lists_cover_what_they_claim():
    for cases in (R.ROWLN_FWD_CASES, R.ROWLN_BWD_CASES):
        cov = R.rowln_coverage(cases)
        assert cov["K"] == [1, 3, 4] and cov["LPR"] == [16, 32, 64] and cov["straddle"] and cov["dead_pieces"] and cov["partial_group"]
        assert cov["single_row"] and cov["families"]
        assert {(c.C, c.CP) for c in cases} == set(R.ROWLN_C_CP)
        for ccp in R.ROWLN_C_CP:
            assert {c.rows for c in cases if (c.C, c.CP) == ccp} >= set(R.ROWLN_ROWS)
    assert R.rowln_coverage(R.ROWLN_BWD_CASES)["capped"] and not R.rowln_coverage(R.ROWLN_FWD_CASES)["capped"]
    big = R.ROWLN_BWD_CASES[-1]
    assert big.rows == 16400 and R.rowln_bwd_blocks(big.rows) == 1024 and R.rowln_bwd_blocks(16384) == 1024 and R.rowln_bwd_blocks(17) == 2
    i = R.rowln_inputs(R.RowlnCase(180, 192, 300))
    x = i["x"].double()
    assert bool((x[1::4].std(1) == 0).all()) and float(x[0::4].mean()) > 190 and 30 < float(x[3::4].mean()) < 34 and abs(float(x[2::4].mean())) < 1e-2
    assert float(x[0::4].std(1).min()) > 0.5                       # the offset rows keep their spread after the bf16 rounding


@pytest.mark.parametrize("C,CP", R.ROWLN_C_CP)
def test_rowln_references_match_torch(C, CP):
    c = R.RowlnCase(C, CP, 17)
    i = R.rowln_inputs(c)
    x = i["x"].double().requires_grad_(True)
    gm, bt = i["gamma"].double().requires_grad_(True), i["beta"].double().requires_grad_(True)
    y = F.layer_norm(x, (C,), gm, bt, 1e-5)
    e = R.rowln_fwd_ref(i["x"], i["gamma"], i["beta"], CP)["out"]
    assert close(e.ref[:, :C], y.detach()) and float(e.ref[:, C:].abs().max()) == 0 and float(e.tol[:, C:].abs().max()) == 0
    y.backward(i["dy"].double())
    b = R.rowln_bwd_ref(i["dy"], i["x"], i["gamma"], CP)
    # every row family at 1e-12, relative to the row's largest gradient (a constant row has rstd = eps^-1/2 = 316 and gradients of that size)
    assert float(((b["dx"].ref[:, :C] - x.grad) / x.grad.abs().amax(1, keepdim=True).clamp_min(1.0)).abs().max()) <= 1e-12
    assert float(b["dx"].ref[:, C:].abs().max()) == 0
    assert close(b["partial"].ref[:, 0].sum(0), gm.grad) and close(b["partial"].ref[:, 1].sum(0), bt.grad)
    assert b["partial"].ref.shape == (2, 2, C)


@pytest.mark.parametrize("c", R.ROWLN_FWD_CASES, ids=lambda c: c.id)
def test_rowln_forward_controls(c):
    i = R.rowln_inputs(c)
    controls(lambda m: R.rowln_fwd_ref(i["x"], i["gamma"], i["beta"], c.CP, mut=m), R.ROWLN_FWD_MUTANTS,
             lambda m: R.rowln_identity(m, c), lambda m: R.rowln_exercises(m, c), c.id)


@pytest.mark.parametrize("c", R.ROWLN_BWD_CASES, ids=lambda c: c.id)
def test_rowln_backward_controls(c):
    i = R.rowln_inputs(c)
    controls(lambda m: R.rowln_bwd_ref(i["dy"], i["x"], i["gamma"], c.CP, mut=m), R.ROWLN_BWD_MUTANTS,
             lambda m: R.rowln_identity(m, c), lambda m: R.rowln_exercises(m, c), c.id)


def test_one_pass_variance_is_what_the_two_pass_bound_excludes():
    """The issue's table: relative rstd error of the fp32 one-pass form on offset rows, against the two-pass bound of the same rows."""
    c = R.RowlnCase(180, 192, 300)
    x = R.rowln_inputs(c)["x"]
    _, rstd, _, _, t_rstd = R._rowln_stats(x, c.C)
    _, r1 = R._one_pass_f32(x, c.C)
    rel, bound = ((r1 - rstd) / rstd).abs(), t_rstd / rstd
    assert float(rel[0::4].max()) > 5e-4 and float(bound[0::4].max()) < 1e-4          # mean 200 / std 1
    assert float(rel[3::4].max()) > 1e-4 and float(bound[3::4].max()) < 1e-4          # mean 32 / std 0.5
    assert float((rel[2::4] / bound[2::4]).max()) < 1.0                                # zero-mean rows: the one-pass form is fine


# ---- chan_stats, sum_rows, BatchNorm coefficients ------------------------------------------------------------------------------------------
def test_reduction_case_lists_cover_what_they_claim():
    cov = R.stats_coverage(R.STATS_CASES)
    assert cov["second_pass"] and cov["exactly_32"] and cov["ragged_second_pass"] and cov["chunks"] == [1, 2, 3] and cov["chunk_tail"]
    assert cov["partial_rowgroup"] and cov["samples"] == [1, 3]
    assert {c.C8 for c in R.STATS_CASES} == {1, 5, 32, 33, 64} and {c.rps for c in R.STATS_CASES} == {1, 7, 256, 257, 513}
    cov = R.bn_coverage(R.BN_CASES)
    assert all(cov[k] for k in ("never", "some_groups", "all_groups", "tail_after", "twice", "ragged_block")) and cov["blocks"] == [1, 2, 3]
    assert cov["outer"] == [1, 2]
    assert {c.R for c in R.BN_CASES} == set(R.BN_R) and {c.C for c in R.BN_CASES} == set(R.BN_N)
    assert all(c.row_stride > 2 * c.ld and c.ld >= c.C for c in R.BN_CASES) and len(R.BN_CASES) <= 40


@pytest.mark.parametrize("c", R.STATS_CASES, ids=lambda c: c.id)
def test_chan_stats_reference_and_controls(c):
    p, q = R.stats_inputs(c)
    e = R.chan_stats_ref(p, q, c)["partial"]
    pd, qd = p.double().view(c.samples, c.rps, -1), q.double().view(c.samples, c.rps, -1)
    assert close(e.ref[:, :, 0].sum(1), pd.sum(1)) and close(e.ref[:, :, 1].sum(1), (pd * qd).sum(1))
    assert e.ref.shape == (c.samples, -(-c.rps // 256), 2, 8 * c.C8)
    if c.rps > 256:
        assert close(e.ref[:, 0, 0], pd[:, :256].sum(1)) and close(e.ref[:, -1, 1], (pd * qd)[:, (e.ref.shape[1] - 1) * 256:].sum(1))
    controls(lambda m: R.chan_stats_ref(p, q, c, mut=m), R.STATS_MUTANTS, lambda m: R.stats_identity(m, c), what=c.id)


@pytest.mark.parametrize("c", R.BN_CASES, ids=lambda c: c.id)
def test_sum_rows_reference_and_controls(c):
    x = R.sum_rows_inputs(c)
    assert close(R.sum_rows_ref(x)["sum"].ref, x.double().sum(1))
    controls(lambda m: R.sum_rows_ref(x, mut=m), R.SUM_ROWS_MUTANTS, lambda m: R.sum_rows_identity(m, c), what=c.id)


def test_bn_coefficient_references_match_batchnorm2d_and_autograd():
    """Integer-valued data, so that the fp32 partial rows are its exact sums: nn.BatchNorm2d in train mode (fp64) gives the scale / shift, its
    running-buffer update and, through autograd, the backward coefficients."""
    c = R.BnCase(3, 5)
    g = torch.Generator().manual_seed(11)
    k = 4
    x = torch.randint(-6, 7, (c.R, k, c.C), generator=g).double()
    dz = torch.randint(-3, 4, (c.R, k, c.C), generator=g).double()
    part = torch.zeros(c.R, c.row_stride)
    part[:, :c.C], part[:, c.ld:c.ld + c.C] = x.sum(1).float(), (x * x).sum(1).float()
    bpart = torch.zeros(c.R, c.row_stride)
    bpart[:, :c.C], bpart[:, c.ld:c.ld + c.C] = dz.sum(1).float(), (dz * x).sum(1).float()
    bn = torch.nn.BatchNorm2d(c.C, eps=R.BN_EPS, momentum=R.BN_MOMENTUM).double().train()
    with torch.no_grad():
        bn.weight.copy_(torch.rand(c.C, generator=g) + 0.5)
        bn.bias.copy_(torch.randn(c.C, generator=g))
        bn.running_mean.copy_(torch.randn(c.C, generator=g))
        bn.running_var.copy_(torch.rand(c.C, generator=g) + 0.5)
    i = dict(partial=part, bwd_partial=bpart, n=float(c.R * k), gamma=bn.weight.detach().float(), beta=bn.bias.detach().float(),
             rm0=bn.running_mean.clone().float(), rv0=bn.running_var.clone().float(), real_of=torch.arange(c.ld, dtype=torch.int32))
    with torch.no_grad():
        bn.weight.copy_(i["gamma"].double()); bn.bias.copy_(i["beta"].double())
        bn.running_mean.copy_(i["rm0"].double()); bn.running_var.copy_(i["rv0"].double())
    xin = x.reshape(-1, c.C).t().reshape(1, c.C, -1, 1).clone().requires_grad_(True)
    y = bn(xin)
    e = R.bn_train_coeffs_ref(i, c)
    sc, sh = e["coef"].ref[0], e["coef"].ref[1]
    assert close(xin.detach() * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1), y.detach())
    assert close(e["running_mean"].ref, bn.running_mean) and close(e["running_var"].ref, bn.running_var)
    assert close(e["coef"].ref[2], x.reshape(-1, c.C).mean(0)) and close(e["coef"].ref[3], (x.reshape(-1, c.C).var(0, unbiased=False) + R.BN_EPS).rsqrt())
    dzin = dz.reshape(-1, c.C).t().reshape(1, c.C, -1, 1)
    y.backward(dzin)
    b = R.bn_train_bwd_coeffs_ref(i, e["coef"].ref.float().double(), c)["coef"].ref
    # the handed-over fp32 forward coefficients differ from the fp64 ones by 1e-7: pin with the exact ones
    b = R.bn_train_bwd_coeffs_ref(i, e["coef"].ref, c)["coef"].ref
    dx = b[0].view(1, -1, 1, 1) * dzin + b[1].view(1, -1, 1, 1) * xin.detach() + b[2].view(1, -1, 1, 1)
    assert close(dx, xin.grad) and close(b[3], bn.weight.grad) and close(b[4], bn.bias.grad)
    # real_of: channel c of the padded layout lands at real_of[c]; -1 leaves the buffers alone
    j = R.bn_inputs(R.BnCase(3, 65))
    er = R.bn_train_coeffs_ref(j, R.BnCase(3, 65))
    live = j["real_of"][:65] >= 0
    assert int(live.sum()) == j["n_real"] < 65
    want = (1 - R.BN_MOMENTUM) * j["rm0"].double() + R.BN_MOMENTUM * er["coef"].ref[2][live]
    assert close(er["running_mean"].ref, want)


@pytest.mark.parametrize("c", R.BN_CASES, ids=lambda c: c.id)
def test_bn_coefficient_controls(c):
    i = R.bn_inputs(c)
    if c.C > 1:
        assert float(i["partial"][:, 0].sum() / i["n"]) > 90 and float(R.bn_train_coeffs_ref(i, c)["coef"].ref[3][1]) == R.BN_EPS ** -0.5
    # real_of maps channels 0, 1 to 0, 1: ignoring it shows from channel 3 on
    controls(lambda m: R.bn_train_coeffs_ref(i, c, mut=m), R.BN_FWD_MUTANTS, lambda m: m == "real_of_ignored" and c.C <= 2, what=c.id)
    fwd = R.bn_train_coeffs_ref(i, c)["coef"].ref.float()
    controls(lambda m: R.bn_train_bwd_coeffs_ref(i, fwd, c, mut=m), R.BN_BWD_MUTANTS, what=c.id)


# ---- element-wise token passes --------------------------------------------------------------------------------------------------------
def test_elementwise_case_lists_cover_what_they_claim():
    cov = R.ew_coverage(R.EW_CASES)
    assert cov["C8"] == [1, 5, 24, 48, 64] and set(cov["rps_kinds"]) >= {"none", "row", "whole", "ragged"}
    assert cov["second_step"] and cov["short_step"] and cov["idle_lanes"] and cov["single_row"]
    for C8 in R.EW_C8:
        L4 = 4 * R.ew_lanes(C8)
        assert {c.rows for c in R.EW_CASES if c.C8 == C8} >= {1, 3, L4 - 1, L4 + 1, 1000}
    assert any(c.rps == 7 and c.rows % 7 for c in R.EW_CASES) and len(R.EW_CASES) <= 60
    cov = R.flat_coverage(R.FLAT_CASES + [R.FLAT_WRAP])
    assert set(cov["pieces"]) >= {1, 255, 257, 5 * 77, 65537 * 64} and cov["one_thread"] and cov["partial_group"] and cov["two_groups"]
    assert cov["wrap"] and cov["division"] and not R.flat_coverage(R.FLAT_CASES)["wrap"]
    v = R.flat_inputs(R.FLAT_CASES[1])
    arg = v["x"].double() * v["scale"].double() + v["shift"].double()
    assert float(arg.min()) < -6 and float(arg.max()) > 6
    x = R.flat_inputs(R.FlatCase(77, 5))["x"]
    assert int(R.bits(x[0, :1])) == 0 and int(R.bits(x[1, :1])) & 0xFFFF == 0x8000


@pytest.mark.parametrize("c", R.EW_CASES, ids=lambda c: c.id)
def test_elementwise_references_and_controls(c):
    i = R.ew_inputs(c)
    idx = R._coef_rows(c, None)
    assert int(idx.max()) == i["A"].shape[0] - 1
    x, s, t = i["p"].double(), i["A"].double()[idx], i["B"].double()[idx]
    for act in (0, 1):
        e = R.affine_act_ref(i, c, act)["out"]
        assert close(e.ref, F.gelu(x * s + t) if act else x * s + t)
        controls(lambda m: R.affine_act_ref(i, c, act, mut=m), R.AFFINE_MUTANTS, lambda m: R.ew_index_identity(m, c), what=(c.id, act))
    fused, unfused = R.affine_act_bits(i, c)
    ok, _ = R.accepts(dict(out=fused), R.affine_act_ref(i, c, 0))
    assert ok and R.accepts(dict(out=unfused), R.affine_act_ref(i, c, 0))[0]
    for pat in R.EW_PATTERNS:
        e = R.lincomb2_ref(i, c, pat)
        want = {"copy": i["p"].double(), "c_acc": i["old"].double() + i["C"].double()[idx], "ap": s * x,
                "ap_bq_c": s * x + i["B"].double()[idx] * i["q"].double() + i["C"].double()[idx], "p_acc": i["old"].double() + x}[pat]
        assert close(e["out"].ref, want)
        controls(lambda m: R.lincomb2_ref(i, c, pat, mut=m), R.LINCOMB_MUTANTS, lambda m: R.lincomb2_identity(m, c, pat), what=(c.id, pat))
        b = R.lincomb2_bits(i, c, pat)
        if b is not None:
            assert R.accepts(dict(out=b), e)[0] and R.same_bits(b, e["out"].ref.to(BF))          # one operation: the correctly rounded value
    assert int(R.bits(R.lincomb2_bits(i, c, "copy")[0, 1 % (8 * c.C8)])) == 0                    # -0 comes out +0


@pytest.mark.parametrize("c", R.FLAT_CASES, ids=lambda c: c.id)
def test_flat_references_and_controls(c):
    i = R.flat_inputs(c)
    v = (i["x"].double() * i["scale"].double() + i["shift"].double()).requires_grad_(True)
    F.gelu(v).backward(i["dy"].double())
    assert close(R.dgelu_affine_ref(i)["out"].ref, v.grad)
    controls(lambda m: R.dgelu_affine_ref(i, mut=m), R.DGELU_MUTANTS, what=c.id)
    a, b = i["a"].double().requires_grad_(True), i["b"].double().requires_grad_(True)
    (a * b).backward(i["dy"].double())
    e = R.mul_bwd_ref(i)
    assert close(e["da"].ref, a.grad) and close(e["db"].ref, b.grad)
    da, db = R.mul_bwd_bits(i)
    assert R.same_bits(da, e["da"].ref.to(BF)) and R.same_bits(db, e["db"].ref.to(BF))
    controls(lambda m: R.mul_bwd_ref(i, mut=m), ("swapped",), what=c.id)


# ---- dual gate ---------------------------------------------------------------------------------------------------------------------------
def test_gate_case_list_covers_what_it_claims():
    cov = R.gate_coverage(R.GATE_CASES)
    assert cov["CA"] == [8, 64, 192, 256] and cov["idle_pieces"] and cov["all_pieces"] and cov["chunks"] == [1, 2, 3] and cov["chunk_tail"]
    assert cov["partial_token_lanes"] and cov["B"] == [1, 3] and {c.HW for c in R.GATE_CASES} == {1, 63, 64, 65, 130}
    tg = R.gate_inputs(R.GATE_CASES[1])["tgate"]
    assert float(tg[0]) == 0.0 and float(tg[-1]) == 1.0


@pytest.mark.parametrize("c", R.GATE_CASES, ids=lambda c: c.id)
def test_dual_gate_references_and_controls(c):
    i = R.gate_inputs(c)
    a, b = i["a"].double().requires_grad_(True), i["b"].double().requires_grad_(True)
    cg = i["cgate"].double().requires_grad_(True)
    tgd = i["tgate"].double()
    smap = torch.logit(tgd.clamp(1e-6, 1 - 1e-6)).requires_grad_(True)
    smp = torch.arange(c.B).repeat_interleave(c.HW)
    interior = (tgd > 0) & (tgd < 1)
    tg = torch.where(interior, torch.sigmoid(smap), tgd)
    comb = a * cg[smp] + b * tg[:, None]                       # tok_gate_on_a = 0
    e0 = R.dual_gate_combine_ref(i, c, 0)["out"]
    ref0 = a.detach() * cg.detach()[smp] + b.detach() * tgd[:, None]
    assert close(e0.ref, ref0)
    assert close(R.dual_gate_combine_ref(i, c, 1)["out"].ref, a.detach() * tgd[:, None] + b.detach() * cg.detach()[smp])
    comb.backward(i["d"].double())
    e = R.dual_gate_bwd_ref(i, c)
    assert close(e["d_chan"].ref, a.grad) and close(e["d_tok"].ref, b.grad) and close(e["dcg_partial"].ref.sum(1), cg.grad)
    assert close(e["dsmap"].ref[interior], smap.grad[interior]) and float(e["dsmap"].ref[~interior].abs().max()) == 0
    for on_a in (0, 1):
        controls(lambda m: R.dual_gate_combine_ref(i, c, on_a, mut=m), R.GATE_COMBINE_MUTANTS, lambda m: R.gate_identity(m, c), what=(c.id, on_a))
        exp = R.dual_gate_combine_ref(i, c, on_a)
        assert all(R.accepts(dict(out=cand), exp)[0] for cand in R.dual_gate_combine_bits(i, c, on_a))
    controls(lambda m: R.dual_gate_bwd_ref(i, c, mut=m), R.GATE_BWD_MUTANTS, lambda m: R.gate_identity(m, c), what=c.id)
    dc, dt = R.dual_gate_bwd_bits(i, c)
    assert R.accepts(dict(d_chan=dc, d_tok=dt), {k: e[k] for k in ("d_chan", "d_tok")})[0]


# ---- depth-wise conv ----------------------------------------------------------------------------------------------------------------------
def test_dwconv_case_list_covers_what_it_claims():
    cov = R.dw_coverage(R.DW_CASES)
    assert cov["H"] == [1, 8, 9] and cov["W"] == [1, 16, 17, 33] and cov["C8"] == [1, 8, 9, 17] and cov["B"] == [1, 2]
    assert cov["channel_blocks"] == [1, 2, 3] and cov["ragged_block"] and cov["tiles_y"] == [1, 2] and cov["tiles_x"] == [1, 2, 3]
    assert cov["neighbour_image"] and any(c.B == 2 and c.C8 > 8 and c.H == 9 for c in R.DW_CASES)


@pytest.mark.parametrize("c", R.DW_CASES, ids=lambda c: c.id)
def test_dwconv_references_and_controls(c):
    i = R.dw_inputs(c)
    C = 8 * c.C8
    x = i["x"].double().view(c.B, c.H, c.W, C).permute(0, 3, 1, 2).clone().requires_grad_(True)
    w = i["w"].double().view(C, 1, 3, 3).clone().requires_grad_(True)
    bias = torch.zeros(C, dtype=torch.float64, requires_grad=True)
    conv = F.conv2d(x, w, bias, padding=1, groups=C)
    flat = lambda t: t.permute(0, 2, 3, 1).reshape(-1, C)
    for act, with_mul in R.DW_VARIANTS:
        v = conv.detach() * i["scale"].double().view(1, C, 1, 1) + i["shift"].double().view(1, C, 1, 1)
        want = flat(F.gelu(v) if act else v) * (i["mul"].double() if with_mul else 1.0)
        assert close(R.dwconv_ref(i, c, act, with_mul)["out"].ref, want)
        controls(lambda m: R.dwconv_ref(i, c, act, with_mul, mut=m), R.DW_MUTANTS, lambda m: R.dw_identity(m, c, with_mul), what=(c.id, act, with_mul))
    conv.backward(i["dy"].double().view(c.B, c.H, c.W, C).permute(0, 3, 1, 2))
    e = R.dwconv_wgrad_ref(i, c)["partial"]
    assert e.ref.shape == (c.B, -(-c.H // 8), 10, C)
    tot = e.ref.sum((0, 1))
    assert close(tot[:9].t(), w.grad.view(C, 9)) and close(tot[9], bias.grad)
    controls(lambda m: R.dwconv_wgrad_ref(i, c, mut=m), R.DW_WGRAD_MUTANTS, lambda m: R.dw_identity(m, c), what=c.id)


# ---- channel attention --------------------------------------------------------------------------------------------------------------------
def test_channel_attention_case_list_covers_what_it_claims():
    cov = R.chan_coverage(R.CHAN_CASES)
    assert cov["N"] == [1, 255, 256, 257, 600] and cov["nH"] == [1, 6] and cov["d"] == [1, 12, 30, 32] and cov["B"] == [1, 2]
    assert cov["chunks"] == [1, 2, 3] and cov["chunk_tail"] and cov["partial_wave"] and cov["full_heads"]
    i = R.chan_inputs(R.CHAN_CASES[1])
    c = R.CHAN_CASES[1]
    q = i["qkv"].view(c.B, c.N, 3, c.nH, 32)
    assert float(q[0, :, 0, 0, 0].abs().max()) == 0 and float(q[1, :, 0, 0, 0].abs().max()) > 0 and float(q[..., c.d:].abs().max()) == 0


@pytest.mark.parametrize("c", R.CHAN_CASES, ids=lambda c: c.id)
def test_channel_attention_references_and_controls(c):
    i = R.chan_inputs(c)
    CA = c.CA
    q, k, v = (i["qkv"][:, j * CA:(j + 1) * CA].double().view(c.B, c.N, c.nH, 32)[..., :c.d].permute(0, 2, 3, 1) for j in range(3))   # [B][h][d][N]
    # the formulation of Adaptive_Channel_Attention: normalise over the tokens, (q k^T) * temperature, softmax, @ v
    attn = (F.normalize(q, dim=-1) @ F.normalize(k, dim=-1).transpose(-2, -1)) * i["temperature"].double().view(1, -1, 1, 1)
    want = attn.softmax(-1) @ v                                                       # [B][h][d][N]
    e = R.channel_attention_ref(i, c)["out"]
    got = e.ref.view(c.B, c.N, c.nH, 32)
    assert close(got[..., :c.d].permute(0, 2, 3, 1), want) and float(got[..., c.d:].abs().max() if c.d < 32 else 0) == 0
    controls(lambda m: R.channel_attention_ref(i, c, mut=m), R.CHAN_ATTN_MUTANTS, lambda m: R.chan_identity(m, c), what=c.id)
    # the Gram partials: their chunk sums are q^T k and the squared column norms
    x, y = i["qkv"][:, :CA], i["qkv"][:, CA:2 * CA]
    p = R.chan_gram_ref(x, y, c)["partial"].ref.sum(2)
    assert close(p[..., :1024].view(c.B, c.nH, 32, 32)[..., :c.d, :c.d], q @ k.transpose(-2, -1))
    assert close(p[..., 1024:1056][..., :c.d], q.pow(2).sum(-1)) and close(p[..., 1056:][..., :c.d], k.pow(2).sum(-1))
    controls(lambda m: R.chan_gram_ref(x, y, c, mut=m), R.CHAN_GRAM_MUTANTS, lambda m: R.chan_identity(m, c), what=c.id)
    # the matrix application against einsum
    src = i["qkv"][:, 2 * CA:].double().view(c.B, c.N, c.nH, 32)
    for with_diag in (False, True):
        for acc in (0, 1):
            w = torch.einsum("bhij,bnhj->bnhi", i["M"].double(), src)
            if with_diag:
                w = w + i["diag"].double()[:, None] * i["src2"].double().view(c.B, c.N, c.nH, 32)
            if acc:
                w = w + i["old"].double().view(c.B, c.N, c.nH, 32)
            assert close(R.chan_apply_mat_ref(i, c, with_diag, acc)["out"].ref, w.reshape(c.B * c.N, CA))
            controls(lambda m: R.chan_apply_mat_ref(i, c, with_diag, acc, mut=m), R.CHAN_APPLY_MUTANTS,
                     lambda m: R.chan_identity(m, c, with_diag, acc), what=(c.id, with_diag, acc))


# ---- spatial interaction in training ---------------------------------------------------------------------------------------------------------
def test_spatial_gate_train_case_list_covers_what_it_claims():
    cov = R.sgt_coverage(R.SGT_CASES)
    assert cov["NV"] == [1, 2, 3, 4] and cov["S"] == [1, 7, 16] and cov["rows"] == [1, 255, 256, 257, 700] and cov["blocks"] == [1, 2, 3]
    assert cov["block_tail"] and cov["partial_step"] and cov["every_NV_with_tail"] == [1, 2, 3, 4]


@pytest.mark.parametrize("c", R.SGT_CASES, ids=lambda c: c.id)
def test_spatial_gate_train_references_and_controls(c):
    i = R.sgt_inputs(c)
    if c.rows > 1:
        # the chain under autograd: 1x1 conv -> BatchNorm2d (train) -> GELU -> 1x1 conv to one map; loss = sum smap * dsmap
        x = i["x"].double().requires_grad_(True)
        W0, b0, w3 = (i[k].double().requires_grad_(True) for k in ("W0", "b0", "w3"))
        bn = torch.nn.BatchNorm1d(c.S, eps=1e-5).double().train()
        with torch.no_grad():
            bn.weight.copy_(i["gamma"].double()); bn.bias.copy_(i["beta"].double())
        z = bn(x @ W0.t() + b0)
        b3 = torch.zeros(1, dtype=torch.float64, requires_grad=True)
        ((F.gelu(z) @ w3 + b3) * i["dsmap"].double()).sum().backward()
        p0 = R.spatial_gate_train_ref(i, c, 0)["partial"].ref.sum(0)
        y1 = (x @ W0.t() + b0).detach()
        assert close(p0[0, :c.S], y1.sum(0)) and close(p0[1, :c.S], (y1 * y1).sum(0)) and float(p0[:, c.S:].abs().max() if c.S < 16 else 0) == 0
        # the case's coefficients are the fp32 roundings the kernel is handed (1e-7 relative), so against autograd's exact BatchNorm they can
        # only agree to 1e-5 / 1e-4; the restatement itself is pinned at 1e-12 on the exact coefficients further down
        p1 = R.spatial_gate_train_ref(i, c, 1)["partial"].ref.sum(0)
        scale = max(1.0, float(w3.grad.abs().max()))
        assert float((p1[2, :c.S] - w3.grad).abs().max()) <= 1e-5 * scale and abs(float(p1[3, 0] - b3.grad)) <= 1e-12 * max(1.0, abs(float(b3.grad)))
        e2 = R.spatial_gate_train_ref(i, c, 2)
        gs = max(1.0, float(x.grad.abs().max()))
        assert float((e2["dx"].ref - x.grad).abs().max()) <= 1e-4 * gs
        part = e2["partial"].ref.sum(0)
        assert float((part[:16 * c.C].view(16, c.C)[:c.S] - W0.grad).abs().max()) <= 1e-4 * max(1.0, float(W0.grad.abs().max()))
        # exact coefficients: the same restatement is autograd's gradient at 1e-12
        j = dict(i)
        with torch.no_grad():
            mean, var = y1.mean(0), y1.var(0, unbiased=False)
            rstd = (var + 1e-5).rsqrt()
            sc = i["gamma"].double() * rstd
            j["bn_scale"], j["bn_shift"] = sc, i["beta"].double() - mean * sc
            dz = i["dsmap"].double()[:, None] * i["w3"].double() * R.G.dgelu(y1 * sc + j["bn_shift"])
            S1, S2 = dz.sum(0), (dz * y1).sum(0)
            dg = rstd * (S2 - mean * S1)
            j["cA"], j["cB"], j["cC"] = sc, -sc * rstd * dg / c.rows, (sc / c.rows) * (mean * rstd * dg - S1)
        e2 = R.spatial_gate_train_ref(j, c, 2)
        assert float((e2["dx"].ref - x.grad).abs().max()) <= 1e-12 * gs
        part = e2["partial"].ref.sum(0)
        assert close(part[:16 * c.C].view(16, c.C)[:c.S], W0.grad) and close(part[16 * c.C:][:c.S], b0.grad)
        assert close(R.spatial_gate_train_ref(j, c, 1)["partial"].ref.sum(0)[2, :c.S], w3.grad)
    for what in (0, 1):
        controls(lambda m: R.spatial_gate_train_ref(i, c, what, mut=m), R.SGT_MUTANTS[what], lambda m: R.sgt_identity(m, c),
                 lambda m: R.sgt_exercises(m, c), (c.id, what))
    for acc in (0, 1):
        controls(lambda m: R.spatial_gate_train_ref(i, c, 2, acc, mut=m), R.SGT_MUTANTS[2], lambda m: R.sgt_identity(m, c, acc),
                 lambda m: R.sgt_exercises(m, c), (c.id, 2, acc))
