"""CPU pins of tests/gate_ref.py: every restatement against torch (autograd, nn.BatchNorm2d, F.layer_norm, F.normalize / softmax) in fp64,
every case list against what its docstring claims, every negative control rejected on every case but its declared identities (and those
really are identities), the ReLU live / dead condition of the cab_bwd inputs and the variance floor of the channel-interaction inputs."""
import functools

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import gate_ref as R

CLOSE = dict(rtol=1e-9, atol=1e-12)


def rounded(exp, skip=()):
    """the reference itself as a device would return it at best: rounded to the output's format (fp32 here; bf16 where named)"""
    return {k: o.ref.float() for k, o in exp.items() if k not in skip}


def check_mutants(cases, mutants, identity, ref_of, skip=()):
    """ref_of(case, mut) -> Dict[str, Out].  The unmutated reference is accepted; a mutant is rejected unless declared an identity."""
    for c in cases:
        exact = ref_of(c, None)
        exact = {k: o for k, o in exact.items() if k not in skip}
        assert R.accepts(rounded(exact), exact)[0], c.id
        for m in mutants:
            got = {k: o.ref for k, o in ref_of(c, m).items() if k not in skip}
            ok, ratios = R.accepts(got, exact)
            if identity(m, c):
                assert all(torch.equal(got[k], exact[k].ref) for k in exact), f"{m} on {c.id} is declared an identity"
            else:
                assert not ok, f"mutant {m} passes on {c.id}: {ratios}"


# ---- channel_gate ----------------------------------------------------------------------------------------------------------------------
def test_gate_cases_cover_what_they_claim():
    cov = R.gate_coverage(R.GATE_CASES)
    assert cov["HW"] == sorted(R.GATE_HW) and cov["C_CP"] == sorted(R.GATE_C_CP) and cov["S"] == sorted(R.GATE_S) and cov["B"] == sorted(R.GATE_B)
    assert cov["full_chunk"] and cov["one_token_tail"] and cov["under_8_tokens"] and cov["c_not_multiple_of_4"] and cov["chunks"] == [1, 2, 3]
    assert 10 <= len(R.GATE_CASES) <= 14


@pytest.mark.parametrize("act", (0, 1))
def test_channel_gate_ref_matches_torch(act):
    for c in R.GATE_CASES:
        i = R.gate_inputs(c)
        mean = i["x"].double().reshape(c.B, c.HW, c.C).mean(1)
        h = F.linear(mean, i["w1"].double(), i["b1"].double())
        h = F.gelu(h) if act else F.relu(h)
        want = c.out_scale * torch.sigmoid(F.linear(h, i["w2"].double(), i["b2"].double()))
        o = R.channel_gate_ref(i["x"], i["w1"], i["b1"], i["w2"], i["b2"], c, act)["gate"]
        torch.testing.assert_close(o.ref[:, :c.C], want, **CLOSE)
        assert bool((o.ref[:, c.C:] == 0).all()) and bool((o.tol[:, c.C:] == 0).all())
        assert float((o.tol[:, :c.C] / o.ref[:, :c.C].abs()).max()) < 1e-2, "the bound is not vacuous"


@pytest.mark.parametrize("act", (0, 1))
def test_channel_gate_mutants(act):
    def ref_of(c, m):
        i = R.gate_inputs(c)
        return R.channel_gate_ref(i["x"], i["w1"], i["b1"], i["w2"], i["b2"], c, act, m)
    check_mutants(R.GATE_CASES, R.GATE_MUTANTS, R.gate_identity, ref_of)


# ---- cab_add_ln ------------------------------------------------------------------------------------------------------------------------
def test_addln_cases_cover_what_they_claim():
    cov = R.addln_coverage(R.ADDLN_CASES)
    assert cov["NV_full"] == [1, 2, 3, 4] and cov["NV_ragged"] == [1, 2, 3, 4]
    assert cov["rows_not_multiple_of_4"] and cov["sample_edge_in_group"] and cov["no_ln"] and cov["wrap"]


@functools.lru_cache(maxsize=None)
def addln_all(c, m):
    i = R.addln_inputs(c)
    return R.cab_add_ln_ref(i["x"], i["conv"], i["gate"], i["gamma"], i["beta"], c, m)


def test_cab_add_ln_ref_matches_torch():
    for c in R.ADDLN_CASES:
        i = R.addln_inputs(c)
        b = torch.arange(c.rows) // c.rps
        x1 = i["x"].double() + i["conv"].double() * i["gate"].double()[b]
        o = addln_all(c, None)
        torch.testing.assert_close(o["x"].ref, x1, **CLOSE)
        assert bool((o["x"].ref[:, c.C:] == 0).all()), "pad columns of x stay zero"
        assert ("xn" in o) == c.ln
        if c.ln:
            want = F.layer_norm(x1[:, :c.C], (c.C,), i["gamma"].double(), i["beta"].double(), 1e-5)
            torch.testing.assert_close(o["xn"].ref[:, :c.C], want, **CLOSE)
            assert bool((o["xn"].ref[:, c.C:] == 0).all())


def test_cab_add_ln_mutants():
    def got_of(exp):
        return {k: (o.ref.to(torch.bfloat16) if k == "xn" else o.ref.float()) for k, o in exp.items()}
    for c in R.ADDLN_CASES:
        exact = addln_all(c, None)
        assert R.accepts(got_of(exact), exact)[0], c.id
        for m in R.ADDLN_MUTANTS:
            got = {k: o.ref for k, o in addln_all(c, m).items()}
            if R.addln_identity(m, c):
                assert all(torch.equal(got[k], exact[k].ref) for k in exact), f"{m} on {c.id} is declared an identity"
            else:
                assert not R.accepts(got, exact)[0], f"mutant {m} passes on {c.id}"


# ---- cab_bwd ---------------------------------------------------------------------------------------------------------------------------
def test_cabbwd_cases_cover_what_they_claim():
    cov = R.cabbwd_coverage(R.CABBWD_CASES)
    assert set(R.GATE_HW) <= set(cov["HW"]) and cov["C_CP"] == sorted(R.GATE_C_CP) and cov["S"] == sorted(R.GATE_S) and cov["B"] == [1, 2, 3]
    assert cov["all_dead"] and cov["wrap"] and cov["one_token_tail"] and cov["under_8_tokens"]


@functools.lru_cache(maxsize=None)
def cabbwd_all(c, m):
    return R.cab_bwd_ref(R.cabbwd_inputs(c), c, m)


def test_cab_bwd_inputs_have_a_live_and_a_dead_unit_per_sample():
    for c in R.CABBWD_CASES:
        z1 = cabbwd_all(c, None)["z1"]
        assert bool((z1.ref.abs() > 4 * z1.tol).all()), f"{c.id}: a z1 within its bound of 0"
        live = z1.ref > 0
        if c.dead:
            assert c.S == 1 and not bool(live.any())
        elif c.S == 1:
            assert bool(live.all())
        else:
            assert bool(live.any(1).all()) and bool((~live).any(1).all()), c.id


def test_cab_bwd_ref_matches_autograd():
    for c in R.CABBWD_CASES:
        if c.HW > 1000:
            continue                                    # the wrap case repeats the arithmetic of the others on more rows
        i = R.cabbwd_inputs(c)
        conv = i["conv"].double().reshape(c.B, c.HW, c.C).requires_grad_(True)
        p = {k: i[k].double().requires_grad_(True) for k in ("w1", "b1", "w2", "b2")}
        h = F.relu(F.linear(conv.mean(1), p["w1"], p["b1"]))
        gate = c.out_scale * torch.sigmoid(F.linear(h, p["w2"], p["b2"]))
        g = i["g"].double().reshape(c.B, c.HW, c.CP)[:, :, :c.C]
        # d_conv of the kernel takes `gate` as a given operand in its first term: g * gate_in + (the pool term of the true gradient)
        (g * conv.detach() * gate[:, None, :]).sum().backward(retain_graph=True)
        o = cabbwd_all(c, None)
        for k in ("w1", "b1", "w2", "b2"):
            torch.testing.assert_close(o["d" + k].ref - i["fill"]["d" + k].double(), p[k].grad, rtol=1e-9, atol=1e-11)
        pool_term = conv.grad
        want = g * i["gate"].double()[:, None, :c.C] + pool_term
        torch.testing.assert_close(o["d_conv"].ref.reshape(c.B, c.HW, c.CP)[:, :, :c.C], want, rtol=1e-9, atol=1e-11)
        torch.testing.assert_close(o["dmean"].ref[:, :c.C], pool_term[:, 0, :], rtol=1e-9, atol=1e-11)
        assert bool((o["dmean"].ref[:, c.C:] == 0).all()) and bool((o["d_conv"].ref[:, c.C:] == 0).all())


def test_cab_bwd_mutants():
    def got_of(exp):
        return {k: (exp[k].ref.to(torch.bfloat16) if k == "d_conv" else exp[k].ref.float()) for k in R.CABBWD_OUTPUTS}
    for c in R.CABBWD_CASES:
        exact = {k: cabbwd_all(c, None)[k] for k in R.CABBWD_OUTPUTS}
        assert R.accepts(got_of(exact), exact)[0], c.id
        for m in R.CABBWD_MUTANTS:
            got = {k: cabbwd_all(c, m)[k].ref for k in R.CABBWD_OUTPUTS}
            if R.cabbwd_identity(m, c):
                assert all(torch.equal(got[k], exact[k].ref) for k in exact), f"{m} on {c.id} is declared an identity"
            else:
                assert not R.accepts(got, exact)[0], f"mutant {m} passes on {c.id}"
        cabbwd_all.cache_clear()


# ---- channel interaction ---------------------------------------------------------------------------------------------------------------
def test_ci_cases_cover_what_they_claim():
    cov = R.ci_coverage(R.CI_CASES)
    assert set(R.CI_SHAPES) <= set(cov["shapes"]) and cov["largest_covered"] and cov["strides_crossed"] > 2 and cov["running_null"]
    assert cov["dh_32"] and cov["dh_not_multiple_of_4"] and cov["ldp_wider"] and cov["ldg_wider"] and not cov["B1"]
    fro = R.ci_coverage(R.CI_FROZEN_CASES)
    assert set(R.CI_SHAPES) <= set(fro["shapes"]) and fro["B1"] and fro["largest_covered"]
    B = R.ci_largest_B(180, 22)
    assert R.ci_lds_floats(B, 180, 22, True) * 4 <= R.CI_MAX_LDS < R.ci_lds_floats(B + 1, 180, 22, True) * 4
    assert not R.ci_covered(1, 60, 7) and R.ci_covered(1, 60, 7, frozen=True) and not R.ci_covered(2, 60, 65)


def ci_module(i, c, train):
    net = nn.Sequential(nn.Conv2d(c.C, c.S, 1), nn.BatchNorm2d(c.S, eps=R.CI_EPS, momentum=R.CI_MOMENTUM), nn.GELU(), nn.Conv2d(c.S, c.C, 1),
                        nn.Sigmoid()).double()
    with torch.no_grad():
        net[0].weight.copy_(i["W1"].double()[:, :, None, None]); net[0].bias.copy_(i["b1"].double())
        net[1].weight.copy_(i["gamma"].double()); net[1].bias.copy_(i["beta"].double())
        net[1].running_mean.copy_(i["running_mean"].double()); net[1].running_var.copy_(i["running_var"].double())
        net[3].weight.copy_(i["W2"].double()[:, :, None, None]); net[3].bias.copy_(i["b2"].double())
    return net.train(train)


@pytest.mark.parametrize("frozen", (False, True))
def test_channel_interaction_ref_matches_batchnorm2d(frozen):
    for c in R.CI_FROZEN_CASES if frozen else R.CI_CASES:
        i = R.ci_inputs(c, frozen)
        po = R.ci_pad_of(c).long()
        net = ci_module(i, c, not frozen)
        pm32 = (i["pooled"][:, po] * R.CI_INV_HW)
        pm = pm32.double().requires_grad_(True)
        out = net(pm[:, :, None, None])[:, :, 0, 0]
        fw = R.channel_interaction_fwd_ref(i, c, frozen)
        torch.testing.assert_close(fw["pm_out"].ref, pm.detach(), **CLOSE)
        torch.testing.assert_close(fw["cgate"].ref[:, po], out.detach(), **CLOSE)
        pad = torch.ones(c.CA, dtype=torch.bool)
        pad[po] = False
        assert bool((fw["cgate"].ref[:, pad] == 0).all())
        assert ("running_mean" in fw) == (not frozen and c.running)
        if "running_mean" in fw:
            torch.testing.assert_close(fw["running_mean"].ref, net[1].running_mean, **CLOSE)
            torch.testing.assert_close(fw["running_var"].ref, net[1].running_var, **CLOSE)
        (out * i["dcg"].double()[:, po]).sum().backward()
        bw = R.channel_interaction_bwd_ref(i, pm32, c, frozen)
        want = dict(dW1=net[0].weight.grad[:, :, 0, 0], db1=net[0].bias.grad, dgamma=net[1].weight.grad, dbeta=net[1].bias.grad,
                    dW2=net[3].weight.grad[:, :, 0, 0], db2=net[3].bias.grad)
        for k, w in want.items():
            torch.testing.assert_close(bw[k].ref, w, rtol=1e-8, atol=1e-11, msg=lambda s: f"{c.id} {k}: {s}")
        torch.testing.assert_close(bw["dpool"].ref[:, po], pm.grad * R.CI_INV_HW, rtol=1e-8, atol=1e-12)
        assert bool((bw["dpool"].ref[:, pad] == 0).all())


def test_channel_interaction_inputs_keep_the_batch_variance_above_100_eps():
    for c in R.CI_CASES:
        i = R.ci_inputs(c)
        pm = (i["pooled"][:, R.ci_pad_of(c).long()] * R.CI_INV_HW).double()
        y = pm @ i["W1"].double().t() + i["b1"].double()
        assert float(y.var(0, unbiased=False).min()) > 100 * R.CI_EPS, c.id


def _pm32(i, c):
    return i["pooled"][:, R.ci_pad_of(c).long()] * R.CI_INV_HW


def test_channel_interaction_mutants():
    check_mutants(R.CI_CASES, R.CI_FWD_MUTANTS, R.ci_identity, lambda c, m: R.channel_interaction_fwd_ref(R.ci_inputs(c), c, False, m))
    check_mutants(R.CI_CASES, R.CI_BWD_MUTANTS, R.ci_identity,
                  lambda c, m: R.channel_interaction_bwd_ref(R.ci_inputs(c), _pm32(R.ci_inputs(c), c), c, False, m))
    check_mutants(R.CI_FROZEN_CASES, R.CI_FROZEN_MUTANTS, R.ci_identity,
                  lambda c, m: R.channel_interaction_fwd_ref(R.ci_inputs(c, True), c, True, m))
    check_mutants(R.CI_FROZEN_CASES, R.CI_FROZEN_BWD_MUTANTS, R.ci_identity,
                  lambda c, m: R.channel_interaction_bwd_ref(R.ci_inputs(c, True), _pm32(R.ci_inputs(c, True), c), c, True, m))


# ---- attention matrix ------------------------------------------------------------------------------------------------------------------
def test_mat_cases_cover_what_they_claim():
    cov = R.mat_coverage(R.MAT_CASES)
    assert cov["dh"] == sorted(R.MAT_DH) and cov["nchunk"] == sorted(R.MAT_NCHUNK) and cov["B_nH"] == [(1, 1), (2, 6)]
    assert cov["clamp"] and cov["saturated"] and cov["fwd_unrolled_body"] and cov["fwd_tail_after_body"] and cov["bwd_odd_tail"]
    assert cov["mask_inside_float4"]
    for c in R.MAT_CASES:
        gram = R.gram_f32(R.mat_inputs(c)["partial"])
        Gm, sq, sk = gram[:, :1024].reshape(-1, 32, 32).double(), gram[:, 1024:1056].double(), gram[:, 1056:].double()
        assert bool((Gm.abs() <= (sq[:, :, None] * sk[:, None, :]).sqrt() * (1 + 1e-5) + 1e-30).all()), "|G_ij| <= |q_i| |k_j|"
        if c.clamp:
            assert bool((sq[:, 1] == 0).all()) and bool((sk[:, 2] == 0).all()) and bool(((sq[:, 3] > 0) & (sq[:, 3] < R.CLAMP)).all())
            assert bool((Gm[:, 3, :c.dh].abs().sum(1) > 0).all())


def test_chunk_sums_are_the_plain_sum_and_order_sensitive():
    c = R.MAT_CASES[5]
    i = R.mat_inputs(c)
    torch.testing.assert_close(R.gram_f32(i["partial"]).double(), i["partial"].double().sum(1), rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(R.dA_f32(i["dpartial"]).double(), i["dpartial"].double().sum(1)[:, :1024], rtol=1e-5, atol=1e-5)
    assert not R.same_bits(R.gram_f32(i["partial"]), i["partial"].sum(1)) or not R.same_bits(R.gram_f32(i["partial"]), i["partial"].flip(1).sum(1))


def test_chan_attn_matrix_ref_matches_normalize_softmax_autograd():
    g = torch.Generator().manual_seed(5)
    for dh in (30, 12, 1):
        c = R.MatCase(dh, 1, 1, 1)
        N = 40
        q = torch.randn(N, dh, generator=g, dtype=torch.float64).requires_grad_(True)
        k = torch.randn(N, dh, generator=g, dtype=torch.float64).requires_grad_(True)
        temp = torch.tensor([1.3], dtype=torch.float64, requires_grad=True)
        dA = torch.randn(dh, dh, generator=g, dtype=torch.float64)
        A = torch.softmax(F.normalize(q.t(), dim=-1) @ F.normalize(k.t(), dim=-1).t() * temp, -1)
        (A * dA).sum().backward()
        gram = torch.zeros(1, R.GSZ, dtype=torch.float64)
        Gm = torch.zeros(32, 32, dtype=torch.float64)
        Gm[:dh, :dh] = (q.t() @ k).detach()
        gram[0, :1024], gram[0, 1024:1024 + dh], gram[0, 1056:1056 + dh] = Gm.reshape(-1), (q * q).sum(0).detach(), (k * k).sum(0).detach()
        fw = R.chan_attn_matrix_fwd_ref(gram, temp.detach(), c)["A"]
        torch.testing.assert_close(fw.ref[0, :dh, :dh], A.detach(), **CLOSE)
        assert float(fw.ref[0].sum()) == pytest.approx(dh) and bool((fw.ref[0, dh:] == 0).all()) and bool((fw.ref[0, :, dh:] == 0).all())
        dA32 = torch.zeros(1, 1024, dtype=torch.float64)
        dA32.view(32, 32)[:dh, :dh] = dA
        bw = R.chan_attn_matrix_bwd_ref(dA32, gram, fw.ref.reshape(1, 1024), temp.detach(), c)
        dG, dsq2, dsk2 = bw["dG"].ref[0, :dh, :dh], bw["dsq2"].ref[0, :dh], bw["dsk2"].ref[0, :dh]
        torch.testing.assert_close(k.detach() @ dG.t() + q.detach() * dsq2, q.grad, rtol=1e-8, atol=1e-11)
        torch.testing.assert_close(q.detach() @ dG + k.detach() * dsk2, k.grad, rtol=1e-8, atol=1e-11)
        torch.testing.assert_close(bw["dtemp"].ref, temp.grad, rtol=1e-8, atol=1e-11)
        assert torch.equal(bw["dGt"].ref, bw["dG"].ref.transpose(1, 2))


def mat_refs(c, m_f, m_b):
    i = R.mat_inputs(c)
    gram = R.gram_f32(i["partial"])
    fw = R.chan_attn_matrix_fwd_ref(gram, i["temp"], c, m_f)
    A32 = R.chan_attn_matrix_fwd_ref(gram, i["temp"], c)["A"].ref.float().reshape(-1, 1024)
    return fw, R.chan_attn_matrix_bwd_ref(R.dA_f32(i["dpartial"]), gram, A32, i["temp"], c, m_b)


def test_chan_attn_matrix_mutants_and_clamp():
    check_mutants(R.MAT_CASES, R.MAT_FWD_MUTANTS, R.mat_identity, lambda c, m: mat_refs(c, m, None)[0])
    check_mutants(R.MAT_CASES, R.MAT_BWD_MUTANTS, R.mat_identity, lambda c, m: mat_refs(c, None, m)[1])
    c = next(c for c in R.MAT_CASES if c.clamp)
    fw, bw = mat_refs(c, None, None)
    assert bool((fw["A"].ref[:, 1, :c.dh] == 1.0 / c.dh).all()), "a zero q channel: a uniform row"
    for ch in (1, 3):
        assert bool((bw["dsq2"].ref[:, ch] == 0).all()) and bool((bw["dsq2"].tol[:, ch] == 0).all())
    assert bool((bw["dsk2"].ref[:, 2] == 0).all()) and bool((bw["dsq2"].ref[:, 0] != 0).all())
