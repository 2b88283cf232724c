"""tests/attn_ref.py pinned on the CPU: every geometry front-end against autograd of the oracle's own formulation (fp64, 1e-12), the
closed-form gradient of the core against autograd of its forward, every negative control rejected by the derived tolerance at every
case that exercises the feature (and the identity asserted where the mutant equals the reference by construction), and the
tolerance itself: positive where it is not meant to be 0, and far below the 2e-2 max|ref| the older tests allow."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import attn_ref as A
from oracle import dat_oracle as DO
from oracle import hat_oracle as HO
from oracle import swinir_oracle as O

CASES = A.all_cases()
_memo = {}


def ref_of(c):
    """The reference of a case, computed once and shared (never modified)."""
    if c not in _memo:
        if len(_memo) > 6:
            _memo.clear()
        inp = A.make_inputs(c)
        _memo[c] = (inp, A.reference(c, inp))
    return _memo[c]


def oracle_autograd(c, inp):
    """o and the gradients by autograd in fp64, with the index maps, masks and dense biases of the oracle modules."""
    B, H, W, nH = c.B, c.H, c.W, c.nH
    Hp, Wp = c.frame
    x = torch.stack([inp["q"], inp["k"], inp["v"]], 1).double().view(B, H, W, 3, nH, 32)
    if c.kern == "win8":
        x[..., 0, :, :] /= c.scale                    # the buffer holds the pre-scaled q: differentiate with respect to the unscaled one
    x.requires_grad_(True)
    par = (inp["bias"] if c.kern == "rect" else inp["table"]).double().clone().requires_grad_(True)
    xp = F.pad(x, (0, 0, 0, 0, 0, 0, 0, Wp - W, 0, Hp - H)).reshape(B, Hp * Wp, 3, nH, 32)
    square_one_shift = c.wh == c.ww and c.sy == c.sx
    if square_one_shift:
        idx = torch.from_numpy(O.window_token_index(Hp, Wp, c.wh, c.sy))
        mask = torch.from_numpy(O.shift_attn_mask(Hp, Wp, c.wh, c.sy)).double() if c.sy else None
    else:
        idx = torch.from_numpy(DO.rect_window_token_index(Hp, Wp, c.wh, c.ww, c.sy, c.sx))
        mask = torch.from_numpy(DO.rect_shift_mask(Hp, Wp, c.wh, c.ww, c.sy, c.sx)).double() if (c.sy or c.sx) else None
    nW, N = idx.shape
    win = xp[:, idx.reshape(-1)].reshape(B * nW, N, 3, nH, 32).permute(2, 0, 3, 1, 4)
    q, k, v = win[0], win[1], win[2]
    if c.kern == "oca":
        kidx, valid = HO.overlap_window_index(H, W, 16, 24)
        kidx, valid = torch.from_numpy(kidx), torch.from_numpy(valid)
        kv = xp[:, kidx.reshape(-1)].reshape(B, nW, 576, 3, nH, 32) * valid[None, :, :, None, None, None]
        kv = kv.reshape(B * nW, 576, 3, nH, 32).permute(2, 0, 3, 1, 4)
        k, v = kv[1], kv[2]
        bias = HO.oca_bias(par, 16, 24)
    elif c.kern == "rect":
        bias = par
    elif c.kern == "w256":
        bias = HO.sa_bias(par, 16)
    else:
        bias = O.dense_rel_pos_bias(par, c.wh)
    attn = (q * c.scale) @ k.transpose(-2, -1) + bias[None]
    if mask is not None:
        attn = (attn.reshape(B, nW, nH, N, -1) + mask[None, :, None]).reshape(B * nW, nH, N, -1)
    o = (attn.softmax(-1) @ v).transpose(1, 2).reshape(B, nW * N, nH, 32)
    merged = torch.zeros(B, Hp * Wp, nH, 32, dtype=torch.float64).index_copy(1, idx.reshape(-1), o).reshape(B, Hp, Wp, nH, 32)[:, :H, :W]
    merged.backward(inp["do"].double().view(B, H, W, nH, 32))
    g = x.grad.reshape(c.T, 3, nH, 32)
    return dict(o=merged.detach().reshape(c.T, nH, 32), dq=g[:, 0], dk=g[:, 1], dv=g[:, 2], par=par.grad)


@pytest.mark.parametrize("c", [c for c in CASES if c.ops == "rand" and not c.fwd and c.scratch], ids=lambda c: c.id)
def test_front_end_agrees_with_autograd_of_the_oracle_formulation(c):
    inp, ref = ref_of(c)
    want = oracle_autograd(c, inp)
    for name, w in want.items():
        key = ("dbias" if c.kern == "rect" else "dtab") if name == "par" else name
        got = ref.out[key].ref
        err = float((got - w).abs().max())
        assert err <= 1e-12 * float(w.abs().max()), f"{c.id} {key}: {err:.3e} vs max {float(w.abs().max()):.3e}"


def test_closed_form_gradient_of_the_core_against_autograd():
    g = torch.Generator().manual_seed(3)
    for N, NK, a, cq in ((5, 9, 1.0, 0.3), (8, 8, 0.25, 0.25), (16, 36, 0.18, 0.18)):
        q, do = torch.randn(3, 2, N, 6, generator=g).double(), torch.randn(3, 2, N, 6, generator=g).double()
        k, v = torch.randn(3, 2, NK, 6, generator=g).double(), torch.randn(3, 2, NK, 6, generator=g).double()
        bias = torch.randn(3, 2, N, NK, generator=g).double()
        bias[torch.rand(3, 2, N, NK, generator=g) < 0.2] -= 100.0
        kvalid = torch.rand(3, 1, 1, NK, generator=g) < 0.8
        kvalid[..., 0] = True
        qu = (q / (cq / a)).requires_grad_(True)              # the core's dq is the gradient of q_buffer * (a / cq)... of the unscaled q
        kr, vr, br = k.clone().requires_grad_(True), v.clone().requires_grad_(True), bias.clone().requires_grad_(True)
        _, o = A.forward_only(qu * (cq / a), kr, vr, br, a, kvalid)
        o.backward(do)
        c = A.core(q, k, v, do, bias, a, cq, kvalid)
        assert torch.allclose(c["O"], o.detach(), rtol=0, atol=1e-13)
        for got, want in ((c["dq"], qu.grad), (c["dk"], kr.grad), (c["dv"], vr.grad), (c["dS"], br.grad)):
            assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())
        assert float(c["dk"][~kvalid.expand(3, 2, 1, NK).squeeze(2)].abs().max()) == 0.0      # an excluded key gets nothing


def _differs(mut, ref):
    """Whether the mutant lies outside the tolerance of the true reference in at least one element of one output."""
    return any(bool(((mut.out[k].ref - o.ref).abs() > o.tol).any()) for k, o in ref.out.items())


def _same(mut, ref):
    return all(float((mut.out[k].ref - o.ref).abs().max()) <= 1e-13 * max(1.0, float(o.ref.abs().max())) for k, o in ref.out.items())


@pytest.mark.parametrize("c", [c for c in CASES if not c.fwd and c.scratch], ids=lambda c: c.id)
def test_every_negative_control_is_rejected_or_is_the_identity(c):
    inp, ref = ref_of(c)
    for name, (var, applies) in A.controls_for(c).items():
        mut = A.reference(c, inp, var)
        if applies:
            assert _differs(mut, ref), f"{c.id}: '{name}' stays within the tolerance"
        else:
            assert _same(mut, ref), f"{c.id}: '{name}' should equal the reference by construction"
    # d table overwritten instead of accumulated: the fill of the GPU test is lost
    key = "dbias" if c.kern == "rect" else "dtab"
    o = ref.out[key]
    tol = A.fill_tol(o.tol, ref.dS_abs_sum, ref.n_terms, 0.75)
    assert bool(((o.ref - (o.ref + 0.75)).abs() > tol).all()), f"{c.id}: an overwritten {key} stays within the tolerance"


@pytest.mark.parametrize("c", [c for c in CASES if c.fwd], ids=lambda c: c.id)
def test_forward_controls(c):
    """The forward-only cases (the forward's own multi-window walk): the controls that change o."""
    inp, ref = ref_of(c)
    for name, (var, applies) in A.controls_for(c).items():
        if applies and var.no_rowsum + var.dk_no_scale + var.dq_scale_twice + var.drop_slice == 0:
            o, m = ref.out["o"], A.reference(c, inp, var).out["o"]
            assert bool(((m.ref - o.ref).abs() > o.tol).any()), f"{c.id}: '{name}' stays within the tolerance of o"


def test_tolerance_is_positive_and_small(capsys):
    """Positive wherever it is not meant to be 0 (the pad channels); the median of tol / max|ref| per output over the whole matrix is far
    below the 2e-2 of the max-norm tests."""
    ratios = {}
    for c in CASES:
        inp, ref = ref_of(c)
        for k, o in ref.out.items():
            t = o.tol
            if o.kind == "bf16":
                assert float(t[..., c.d:].abs().max()) == 0.0 if c.d < 32 else True
                t = t[..., :c.d]
            assert bool((t > 0).all()) and bool(torch.isfinite(t).all()), f"{c.id} {k}"
            ratios.setdefault(k, []).append(float(t.median()) / float(o.ref.abs().max()))
    with capsys.disabled():
        for k, r in ratios.items():
            print(f"\n[attn_ref] {k}: median tol / max|ref| over {len(r)} cases: median {np.median(r):.2e}, largest {max(r):.2e}", end="")
        print()
    for k, r in ratios.items():
        assert np.median(r) < 2e-2 / 4, k


def test_peaked_cases_are_peaked_and_scores_stay_in_range():
    for c in CASES:
        if c.ops == "peaked":
            assert ref_of(c)[1].maxP > 0.99, c.id
    kerns = {c.kern for c in CASES if c.ops == "peaked"}
    assert kerns == {"win8", "small", "w256", "oca", "rect"}


@pytest.mark.parametrize("c", A.uniform_cases(), ids=lambda c: c.id)
def test_uniform_softmax_expectation_is_the_core_on_zero_scores(c):
    """uniform_dv (an explicit loop over windows and regions) against the core at q = 0, bias = 0; the expected values are bf16 numbers
    wherever the region size is a power of two."""
    inp = A.uniform_inputs(c)
    dv, exact = A.uniform_dv(c, inp)
    ref = A.reference(c, inp).out["dv"].ref
    assert float((dv - ref).abs().max()) <= 1e-12 * float(ref.abs().max())
    assert bool(exact.all()) and torch.equal(dv.to(torch.bfloat16).double(), dv)


def test_case_matrix_reaches_the_paths():
    """What a reviewer would otherwise confirm from the case ids."""
    win8 = [c for c in CASES if c.kern == "win8"]
    assert any(A.win8_wpw(c.windows, c.nH, False) == 2 and c.windows % 2 and not c.fwd for c in win8)
    assert any(A.win8_wpw(c.windows, c.nH, True) == 2 and c.windows % 2 and c.fwd for c in win8)
    assert any(c.B > 1 and c.sy for c in win8)                                        # b_ % nW matters
    for kern in ("small", "w256", "oca", "rect"):
        assert any(c.windows > 32 and c.windows % 32 and c.windows % 8 for c in CASES if c.kern == kern), kern      # second slice, ragged
    small = [c for c in CASES if c.kern == "small"]
    for ws in range(2, 8):
        shifts = {c.sy for c in small if c.wh == ws}
        assert {0, ws // 2} <= shifts and (ws == 2 or len(shifts) >= 3)
    assert {1, 6, 9} <= {c.nH for c in small} and any(c.spare for c in small)
    assert any(c.sy != c.sx and 8 not in (c.sy, c.sx) for c in CASES if c.kern == "w256")
    rect = [c for c in CASES if c.kern == "rect"]
    assert {(8, 32), (32, 8), (8, 16), (16, 8), (16, 16)} <= {(c.wh, c.ww) for c in rect}
    assert any(not c.scratch for c in rect) and any(c.spare for c in rect)
    assert any(c.sy not in (0, c.wh // 2) and c.sx not in (0, c.ww // 2) for c in rect)
    assert any(bool((A.frame_tokens(c) < 0).all(1).any()) for c in rect) and any(bool(((A.frame_tokens(c) < 0).any(1) & ~(A.frame_tokens(c) < 0).all(1)).any()) for c in rect)
    assert max(c.T for c in CASES) <= 25000


@pytest.mark.parametrize("n", [16, 64, 104, 256, 304])
def test_fused_cases_reach_every_window_list_length_on_any_cu_count(n):
    """B_ == n, lists of unequal length, and a case where every list walks at least 3 windows and some 4 (the steady state of the two
    alternating row slots), whatever the CU count; the kernel refuses B_ < n, so every case has B_ >= n."""
    cs = A.fused_cases(n)
    lens = [A.fused_lists(c.windows, n) for c in cs]
    assert all(c.windows >= n and c.windows % c.nW == 0 and c.nH == 6 and c.d == 30 for c in cs)
    assert any(lo >= 3 and hi > lo for lo, hi in lens) and any(hi > lo for lo, hi in lens[:3])
    assert {c.sy for c in cs} == {0, 4} and any(c.H != c.W for c in cs) and any(c.ops == "peaked" for c in cs)


def test_fused_projection_marks_uncertain_operands_only_near_rounding_boundaries():
    c = A.ACase("win8", 1, 16, 24, 6, 30, sy=4, sx=4)
    f = A.fused_inputs(c)
    inp, unc = A.fused_project(c, f)
    y = (f["xn"].double() @ f["wqkv"].double().t() + f["bqkv"].double()).view(c.T, 3, 6, 32)
    assert torch.equal(inp["k"].double(), y[:, 1].to(torch.bfloat16).double()) and torch.equal(inp["q"].double(), (y[:, 0] * c.scale).to(torch.bfloat16).double())
    for k in "qkv":
        assert float(inp[k][..., 30:].float().abs().max()) == 0.0 and float(unc[k][..., 30:].max()) == 0.0
        frac = float((unc[k][..., :30] > 0).double().mean())
        assert 0.0 < frac < 0.5, (k, frac)
        # one bf16 step (two across a binade boundary); next to zero the interval is 2 delta itself, delta = 2 * 192 u S < 5e-4 here
        assert bool((unc[k] <= 2.0 ** -6 * inp[k].double().abs() + 1e-3).all())
    ref, ref0 = A.reference(c, inp, unc=unc), A.reference(c, inp)
    for k, o in ref.out.items():
        assert bool((o.tol >= ref0.out[k].tol).all()) and torch.equal(o.ref, ref0.out[k].ref)
