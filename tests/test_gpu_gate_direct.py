"""Direct parity, through the C ABI, of HAT's CAB tail (srk_channel_gate / srk_channel_gate_act, srk_cab_add_ln, srk_cab_bwd; csrc/hat.hip,
csrc/hat_train.hip) and DAT's small functions (srk_channel_interaction_fwd / _bwd, their _frozen_ forms, srk_chan_attn_matrix_fwd / _bwd;
csrc/dat_small.hip) against the fp64 restatements of tests/gate_ref.py.

Every case checks
  1. values per element within the DERIVED bound of gate_ref (the log line `[gate] <entry> <case> out:max(err / tol) ...` carries the
     share of each bound that is used; a failure names the first offending index), every row of the two grid-wrap cases included;
  2. that nothing else is written: every output is a guarded.Guarded buffer; outputs the header promises to write fully start as the NaN
     pattern (pad columns included where it says +0), the accumulated gradients of srk_cab_bwd and the overwritten ones of the channel
     interaction from a non-zero fill, workspaces 0xFF-filled;
  3. that nothing else is read: operands sit between NaN rows; pad columns the kernels mask hold NaN (the x pads of channel_gate, the conv
     pads of cab_bwd, the positions of pooled / dcgate that pad_of does not name), pad columns the contract wants zero hold zero;
  4. exact identities, bit for bit (listed at each test).

The comparators' ability to fail is pinned on the CPU (tests/test_gate_ref.py); the argument refusals in tests/test_abi_and_host.py."""
import pytest
import torch

import gate_ref as R
from dat_ref import embed
from gate_ref import BF
from test_gpu_dat_direct import Operand, Out, assert_bits, ok, st, zero_bits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    from tpu_superresolution_amd import _lib
    _lib.claim_device(0)
    torch.cuda.set_device(0)
    return _lib.lib()


def check(entry, case, got, exp, outs=()):
    for g in outs:
        g.assert_guards(f"{entry} {case}")
    good, ratios = R.accepts(got, exp)
    print(f"[gate] {entry} {case} " + " ".join(f"{k}:{v:.3f}" for k, v in ratios.items()))
    if not good:
        msg = []
        for k, o in exp.items():
            err = (got[k].double() - o.ref).abs()
            bad = ~(err <= o.tol.expand_as(o.ref))
            if bool(bad.any()):
                idx = tuple(int(v) for v in bad.nonzero()[0])
                msg.append(f"{k}: max err/tol {ratios[k]:.3g}, {int(bad.sum())} of {bad.numel()} outside, first at {idx}: got "
                           f"{float(got[k][idx]):.9g} want {float(o.ref[idx]):.9g} tol {float(o.tol.expand_as(o.ref)[idx]):.3g}")
        raise AssertionError(f"{entry} {case}: " + "; ".join(msg))


def nan_pad(t, CP):
    """[rows][C] -> [rows][CP] with NaN in the pad columns"""
    return embed(t, CP, 0)


def f32(rows, width, **kw):
    return Out("f32", rows, width, **kw)


def vec(t):
    return Operand(t.contiguous())


# ---- srk_channel_gate / srk_channel_gate_act ----------------------------------------------------------------------------------------------
def run_gate(L, c, i, act, plain=False):
    x = Operand(nan_pad(i["x"], c.CP))                                    # the pad columns of x are read and never used: NaN
    nws = int(L.srk_channel_gate_workspace(c.B, c.HW, c.CP))
    assert nws == c.B * c.nchunk * c.CP * 4
    ws, gate = f32(1, nws // 4, ff=True), f32(c.B, c.CP)
    w1, b1, w2, b2 = vec(i["w1"]), vec(i["b1"]), vec(i["w2"]), vec(i["b2"])
    if plain:
        ok(L, L.srk_channel_gate(x.ptr, ws.ptr, w1.ptr, b1.ptr, w2.ptr, b2.ptr, c.out_scale, gate.ptr, c.B, c.HW, c.C, c.CP, c.S, st()))
    else:
        ok(L, L.srk_channel_gate_act(x.ptr, ws.ptr, w1.ptr, b1.ptr, w2.ptr, b2.ptr, c.out_scale, gate.ptr, c.B, c.HW, c.C, c.CP, c.S, act, st()))
    torch.cuda.synchronize()
    ws.assert_guards(f"channel_gate workspace {c.id}")
    return gate


@pytest.mark.parametrize("act", (0, 1), ids=("relu", "gelu"))
@pytest.mark.parametrize("c", R.GATE_CASES, ids=lambda c: c.id)
def test_channel_gate(L, c, act):
    i = R.gate_inputs(c)
    gate = run_gate(L, c, i, act)
    check("channel_gate_act" if act else "channel_gate", c.id, dict(gate=gate.data()),
          R.channel_gate_ref(i["x"], i["w1"], i["b1"], i["w2"], i["b2"], c, act), (gate,))
    assert zero_bits(gate.data()[:, c.C:]), "pad columns C .. CP - 1 are +0"
    assert_bits(run_gate(L, c, i, act).data(), gate.data(), "two runs (fixed-order sums, no atomics)")
    if act == 0:
        assert_bits(run_gate(L, c, i, 0, plain=True).data(), gate.data(), "srk_channel_gate == srk_channel_gate_act(act = 0)")
    z = dict(i, w2=torch.zeros_like(i["w2"]), b2=torch.zeros_like(i["b2"]))
    half = run_gate(L, c, z, act).data()
    want = torch.zeros(c.B, c.CP)
    want[:, :c.C] = torch.tensor(c.out_scale, dtype=torch.float32) / 2
    assert_bits(half, want, "w2 = 0, b2 = 0: out_scale / 2 on the real columns, +0 on the pads")


# ---- srk_cab_add_ln -----------------------------------------------------------------------------------------------------------------------
def run_add_ln(L, c, i):
    x = f32(c.rows, c.CP, fill=i["x"])
    conv, gate = Operand(i["conv"]), Operand(i["gate"])
    gm, bt, xn = (vec(i["gamma"]), vec(i["beta"]), Out("bf16", c.rows, c.CP)) if c.ln else (None, None, None)
    ok(L, L.srk_cab_add_ln(x.ptr, conv.ptr, gate.ptr, gm.ptr if gm else None, bt.ptr if bt else None, xn.ptr if xn else None, c.rows, c.rps,
                           c.C, c.CP, st()))
    torch.cuda.synchronize()
    return x, xn


@pytest.mark.parametrize("c", R.ADDLN_CASES, ids=lambda c: c.id)
def test_cab_add_ln(L, c):
    i = R.addln_inputs(c)
    x, xn = run_add_ln(L, c, i)
    got = dict(x=x.data())
    if c.ln:
        got["xn"] = xn.data()
    check("cab_add_ln", c.id, got, R.cab_add_ln_ref(i["x"], i["conv"], i["gate"], i["gamma"], i["beta"], c), (x, xn) if c.ln else (x,))
    assert zero_bits(x.data()[:, c.C:]), "pad columns of x stay +0"
    if c.ln:
        assert zero_bits(xn.data()[:, c.C:]), "pad columns of xn are +0"
    if c.rows <= 1000:
        x0, _ = run_add_ln(L, c, dict(i, gate=torch.zeros_like(i["gate"])))
        assert_bits(x0.data(), i["x"], "gate = 0 leaves x bit-identical")


# ---- srk_cab_bwd --------------------------------------------------------------------------------------------------------------------------
def run_cab_bwd(L, c, i):
    conv = Operand(nan_pad(i["conv"], c.CP))                              # the pad columns of conv are read and never used: NaN
    g, gate = Operand(i["g"]), Operand(i["gate"])
    nws = int(L.srk_cab_bwd_workspace(c.B, c.HW, c.CP))
    assert nws == c.B * c.nchunk * 2 * c.CP * 4
    ws = f32(1, nws // 4, ff=True)
    w1, b1, w2, b2 = vec(i["w1"]), vec(i["b1"]), vec(i["w2"]), vec(i["b2"])
    o = dict(dw1=f32(c.S, c.C, fill=i["fill"]["dw1"]), db1=f32(1, c.S, fill=i["fill"]["db1"][None]), dw2=f32(c.C, c.S, fill=i["fill"]["dw2"]),
             db2=f32(1, c.C, fill=i["fill"]["db2"][None]), dmean=f32(c.B, c.CP), d_conv=Out("bf16", c.B * c.HW, c.CP))
    ok(L, L.srk_cab_bwd(conv.ptr, g.ptr, gate.ptr, ws.ptr, w1.ptr, b1.ptr, w2.ptr, b2.ptr, c.out_scale, o["dw1"].ptr, o["db1"].ptr, o["dw2"].ptr,
                        o["db2"].ptr, o["dmean"].ptr, o["d_conv"].ptr, c.B, c.HW, c.C, c.CP, c.S, st()))
    torch.cuda.synchronize()
    ws.assert_guards(f"cab_bwd workspace {c.id}")
    for k, b in o.items():
        b.assert_guards(f"cab_bwd {k} {c.id}")
    return {k: b.data().reshape(i["fill"][k].shape) if k in i["fill"] else b.data() for k, b in o.items()}


@pytest.mark.parametrize("c", R.CABBWD_CASES, ids=lambda c: c.id)
def test_cab_bwd(L, c):
    i = R.cabbwd_inputs(c)
    got = run_cab_bwd(L, c, i)
    exp = R.cab_bwd_ref(i, c)
    check("cab_bwd", c.id, got, {k: exp[k] for k in R.CABBWD_OUTPUTS})
    assert zero_bits(got["dmean"][:, c.C:]) and zero_bits(got["d_conv"][:, c.C:]), "pad columns of dmean and d_conv are +0"
    if c.dead:                                                            # nothing flows through the hidden layer
        assert_bits(got["dw1"], i["fill"]["dw1"], "all units dead: dw1 keeps its fill")
        assert_bits(got["db1"], i["fill"]["db1"], "all units dead: db1 keeps its fill")
        assert zero_bits(got["dmean"]), "all units dead: dmean is +0"
        b = torch.arange(c.B * c.HW) // c.HW
        assert_bits(got["d_conv"], (i["g"] * i["gate"][b] + 0.0).to(BF), "all units dead: d_conv == bf16(g * gate + 0)")      # -0 + +0 = +0
    if c.HW <= 700:                                                       # g = 0: no gradient at all
        z = run_cab_bwd(L, c, dict(i, g=torch.zeros_like(i["g"])))
        for k in i["fill"]:
            assert_bits(z[k], i["fill"][k], f"g = 0: {k} keeps its fill")
        assert bool((z["dmean"] == 0).all()) and bool((z["d_conv"].float() == 0).all()), "g = 0: dmean and d_conv are zero"


# ---- srk_channel_interaction_fwd / _bwd and the frozen forms -----------------------------------------------------------------------------------
def ci_common(i, c):
    return dict(pad_of=Operand(R.ci_pad_of(c)), W1=vec(i["W1"]), b1=vec(i["b1"]), gamma=vec(i["gamma"]), beta=vec(i["beta"]), W2=vec(i["W2"]),
                b2=vec(i["b2"]))


@pytest.mark.parametrize("c", R.CI_CASES, ids=lambda c: c.id)
def test_channel_interaction_fwd(L, c):
    assert L.srk_channel_interaction_covered(c.B, c.C, c.S) == 1 == int(R.ci_covered(c.B, c.C, c.S))
    for B in (c.B, c.B + 1):
        assert L.srk_channel_interaction_covered(B, c.C, c.S) == int(R.ci_covered(B, c.C, c.S)), "the edge of the covered shapes"
    i = R.ci_inputs(c)
    p, pooled = ci_common(i, c), Operand(i["pooled"])                     # NaN wherever pad_of does not point, and in columns CA .. ldp - 1
    pm_out, cgate = f32(c.B, c.C), f32(c.B, c.CA)
    rm, rv = (f32(1, c.S, fill=i["running_mean"][None]), f32(1, c.S, fill=i["running_var"][None])) if c.running else (None, None)
    ok(L, L.srk_channel_interaction_fwd(pooled.ptr, c.ldp, R.CI_INV_HW, p["pad_of"].ptr, p["W1"].ptr, p["b1"].ptr, p["gamma"].ptr, p["beta"].ptr,
                                        R.CI_EPS, p["W2"].ptr, p["b2"].ptr, rm.ptr if rm else None, rv.ptr if rv else None, R.CI_MOMENTUM,
                                        pm_out.ptr, cgate.ptr, c.B, c.C, c.S, c.CA, st()))
    torch.cuda.synchronize()
    got = dict(pm_out=pm_out.data(), cgate=cgate.data())
    if c.running:
        got.update(running_mean=rm.data()[0], running_var=rv.data()[0])
    check("channel_interaction_fwd", c.id, got, R.channel_interaction_fwd_ref(i, c), (pm_out, cgate) + ((rm, rv) if c.running else ()))
    pad = torch.ones(c.CA, dtype=torch.bool)
    pad[R.ci_pad_of(c).long()] = False
    assert zero_bits(cgate.data()[:, pad]), "the padding channels of cgate are +0"
    assert_bits(pm_out.data(), i["pooled"][:, R.ci_pad_of(c).long()] * R.CI_INV_HW, "pm_out is one IEEE product")


@pytest.mark.parametrize("c", R.CI_FROZEN_CASES, ids=lambda c: c.id)
def test_channel_interaction_frozen_fwd(L, c):
    assert L.srk_channel_interaction_frozen_covered(c.B, c.C, c.S) == 1
    i = R.ci_inputs(c, True)
    p, pooled = ci_common(i, c), Operand(i["pooled"])
    rm, rv = vec(i["running_mean"]), vec(i["running_var"])
    pm_out, cgate = f32(c.B, c.C), f32(c.B, c.CA)
    ok(L, L.srk_channel_interaction_frozen_fwd(pooled.ptr, c.ldp, R.CI_INV_HW, p["pad_of"].ptr, p["W1"].ptr, p["b1"].ptr, p["gamma"].ptr,
                                               p["beta"].ptr, R.CI_EPS, p["W2"].ptr, p["b2"].ptr, rm.ptr, rv.ptr, pm_out.ptr, cgate.ptr, c.B, c.C,
                                               c.S, c.CA, st()))
    torch.cuda.synchronize()
    check("channel_interaction_frozen_fwd", c.id, dict(pm_out=pm_out.data(), cgate=cgate.data()), R.channel_interaction_fwd_ref(i, c, True),
          (pm_out, cgate))
    pad = torch.ones(c.CA, dtype=torch.bool)
    pad[R.ci_pad_of(c).long()] = False
    assert zero_bits(cgate.data()[:, pad]), "the padding channels of cgate are +0"


CI_GRADS = (("dW1", lambda c: (c.S, c.C)), ("db1", lambda c: (1, c.S)), ("dgamma", lambda c: (1, c.S)), ("dbeta", lambda c: (1, c.S)),
            ("dW2", lambda c: (c.C, c.S)), ("db2", lambda c: (1, c.C)))


def run_ci_bwd(L, c, i, frozen):
    p = ci_common(i, c)
    pm32 = i["pooled"][:, R.ci_pad_of(c).long()] * R.CI_INV_HW
    pm, dcg = Operand(pm32), Operand(i["dcg"])                            # dcg: NaN wherever pad_of does not point, columns CA .. ldg - 1 too
    o = {k: f32(*shape(c), fill=torch.full(shape(c), 7.0)) for k, shape in CI_GRADS}      # overwritten: the fill must be gone
    o["dpool"] = f32(c.B, c.CA)
    head = (pm.ptr, dcg.ptr, c.ldg, R.CI_INV_HW, p["pad_of"].ptr, p["W1"].ptr, p["b1"].ptr, p["gamma"].ptr, p["beta"].ptr, R.CI_EPS, p["W2"].ptr,
            p["b2"].ptr)
    tail = tuple(o[k].ptr for k, _ in CI_GRADS) + (o["dpool"].ptr, c.B, c.C, c.S, c.CA, st())
    if frozen:
        rm, rv = vec(i["running_mean"]), vec(i["running_var"])
        ok(L, L.srk_channel_interaction_frozen_bwd(*head, rm.ptr, rv.ptr, *tail))
    else:
        ok(L, L.srk_channel_interaction_bwd(*head, *tail))
    torch.cuda.synchronize()
    exp = R.channel_interaction_bwd_ref(i, pm32, c, frozen)
    got = {k: b.data().reshape(exp[k].ref.shape) for k, b in o.items()}
    check("channel_interaction_frozen_bwd" if frozen else "channel_interaction_bwd", c.id, got, exp, tuple(o.values()))
    pad = torch.ones(c.CA, dtype=torch.bool)
    pad[R.ci_pad_of(c).long()] = False
    assert zero_bits(got["dpool"][:, pad]), "the padding channels of dpool are +0"


@pytest.mark.parametrize("c", R.CI_CASES, ids=lambda c: c.id)
def test_channel_interaction_bwd(L, c):
    run_ci_bwd(L, c, R.ci_inputs(c), False)


@pytest.mark.parametrize("c", R.CI_FROZEN_CASES, ids=lambda c: c.id)
def test_channel_interaction_frozen_bwd(L, c):
    run_ci_bwd(L, c, R.ci_inputs(c, True), True)


# ---- srk_chan_attn_matrix_fwd / _bwd ----------------------------------------------------------------------------------------------------------
def run_mat_bwd(L, c, dpartial, gram, A32, temp):
    BH = c.B * c.nH
    dp, gr, Ao, tp = Operand(dpartial.reshape(BH * c.nchunk, R.GSZ)), Operand(gram), Operand(A32.reshape(BH * 32, 32)), vec(temp)
    o = dict(dG=f32(BH * 32, 32), dGt=f32(BH * 32, 32), dsq2=f32(BH, 32), dsk2=f32(BH, 32), dtemp=f32(1, BH))
    ok(L, L.srk_chan_attn_matrix_bwd(dp.ptr, c.nchunk, gr.ptr, Ao.ptr, tp.ptr, o["dG"].ptr, o["dGt"].ptr, o["dsq2"].ptr, o["dsk2"].ptr,
                                     o["dtemp"].ptr, c.B, c.nH, c.dh, st()))
    torch.cuda.synchronize()
    for k, b in o.items():
        b.assert_guards(f"chan_attn_matrix_bwd {k} {c.id}")
    return dict(dG=o["dG"].data().reshape(BH, 32, 32), dGt=o["dGt"].data().reshape(BH, 32, 32), dsq2=o["dsq2"].data(), dsk2=o["dsk2"].data(),
                dtemp=o["dtemp"].data()[0])


@pytest.mark.parametrize("c", R.MAT_CASES, ids=lambda c: c.id)
def test_chan_attn_matrix(L, c):
    i = R.mat_inputs(c)
    BH = c.B * c.nH
    part, tp = Operand(i["partial"].reshape(BH * c.nchunk, R.GSZ)), vec(i["temp"])
    gram, A = f32(BH, R.GSZ), f32(BH * 32, 32)
    ok(L, L.srk_chan_attn_matrix_fwd(part.ptr, c.nchunk, tp.ptr, gram.ptr, A.ptr, c.B, c.nH, c.dh, st()))
    torch.cuda.synchronize()
    want_gram = R.gram_f32(i["partial"])
    gram.assert_guards(f"gram {c.id}")
    assert_bits(gram.data(), want_gram, "gram: (a0 + a1) + (a2 + a3) over chunks strided by 4, the tail onto a0")
    fw = R.chan_attn_matrix_fwd_ref(want_gram, i["temp"], c)
    gotA = A.data().reshape(BH, 32, 32)
    check("chan_attn_matrix_fwd", c.id, dict(A=gotA), fw, (A,))
    assert zero_bits(gotA[:, c.dh:]) and zero_bits(gotA[:, :, c.dh:]), "padding rows / columns of A are +0"
    if c.clamp:
        assert_bits(gotA[:, 1, :c.dh], torch.full((BH, c.dh), 1.0) / c.dh, "a zero-norm q channel: its row of A is exactly 1 / dh")

    A32 = fw["A"].ref.float()
    got = run_mat_bwd(L, c, i["dpartial"], want_gram, A32, i["temp"])
    check("chan_attn_matrix_bwd", c.id, got, R.chan_attn_matrix_bwd_ref(R.dA_f32(i["dpartial"]), want_gram, A32, i["temp"], c))
    assert_bits(got["dGt"], got["dG"].transpose(1, 2).contiguous(), "dGt == dG transposed")
    for k in ("dG", "dGt"):
        assert zero_bits(got[k][:, c.dh:]) and zero_bits(got[k][:, :, c.dh:]), f"padding of {k} is +0"
    assert zero_bits(got["dsq2"][:, c.dh:]) and zero_bits(got["dsk2"][:, c.dh:])
    if c.clamp:
        assert bool((got["dsq2"][:, [1, 3]] == 0).all()) and bool((got["dsk2"][:, 2] == 0).all()), "clamped channels get no gradient"
    zero = run_mat_bwd(L, c, torch.zeros_like(i["dpartial"]), want_gram, A32, i["temp"])
    assert all(bool((v == 0).all()) for v in zero.values()), "dpartial = 0 gives zero outputs"
