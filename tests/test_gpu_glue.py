"""Direct parity, through the C ABI, of the kernels between the GEMMs of the host-orchestrated models (include/srk.h: srk_layernorm_fwd,
srk_layernorm_bwd, srk_rowscale_bf16, srk_add_f32_bf16, srk_add_bf16_into_f32, srk_add_f32, srk_cast_f32_bf16, srk_img_prep, srk_stem_conv,
srk_win_attention_fwd_padded, srk_channel_gate_act with act = 1, srk_spatial_gate_dev) against the fp64 restatements of tests/glue_ref.py.

Every case checks
  1. values: within the DERIVED bound of glue_ref (the log line carries max(err / tol) per output), or bit for bit where the arithmetic is a
     fixed sequence of IEEE operations (img_prep, rowscale, the adds, the cast, bf16 copies of an fp32 output);
  2. that nothing else is written: outputs live in guarded.Guarded buffers, 256 rows of a NaN pattern before and after stay bit-identical;
  3. that nothing else is read: operands sit between NaN rows (a masked over-read would surface as NaN or as a non-zero pad column);
  4. pad columns (exactly +0, or unchanged under accumulate = 1), the accumulate contracts, and the return code.

The comparators' ability to fail is pinned on the CPU (tests/test_glue_ref.py).  srk_channel_gate_act runs here at the one shape of
tests/test_gpu_hat.py; its direct coverage with a derived bound, and that of srk_channel_gate / srk_cab_add_ln / srk_cab_bwd, is
tests/test_gpu_gate_direct.py."""
import ctypes as C

import pytest
import torch

import glue_ref as R
from guarded import Guarded
from oracle import swinir_oracle as O

pytestmark = pytest.mark.gpu

NAN_ROWS = 72            # NaN rows in front of and after every operand (a multiple of 8: the operand itself stays 16-byte aligned)


@pytest.fixture(scope="module")
def L():
    from tpu_superresolution_amd import _lib
    _lib.claim_device(0)
    torch.cuda.set_device(0)
    return _lib


def st():
    return torch.cuda.current_stream().cuda_stream


class Operand:
    """A device operand [rows][cols] (a vector is one row) between NAN_ROWS rows of NaN."""

    def __init__(self, t):
        t2 = t.reshape(t.shape[0], -1) if t.dim() > 1 else t.reshape(1, -1)
        pad = torch.full((NAN_ROWS, t2.shape[1]), float("nan"), dtype=t2.dtype)
        self.buf = torch.cat([pad, t2, pad]).cuda()
        self.ptr = self.buf.data_ptr() + NAN_ROWS * t2.shape[1] * t2.element_size()


def ok(L, rc):
    assert rc == 0, (rc, L.lib().srk_last_error().decode())


def is_zero_bits(t):
    return bool((R.bits(t) == 0).all())


def assert_same_bits(got, want, what, src=None, flush_ok=False):
    """Bit patterns equal (NaN as NaN-ness); the message names the first mismatches with their inputs."""
    if (R.same_bits_or_flushed if flush_ok else R.same_bits)(got, want):
        return
    bad = ((R.bits(got) != R.bits(want)) & ~(got.isnan() & want.isnan())).reshape(-1).nonzero().reshape(-1)
    rows = [f"[{int(i)}] got {int(R.bits(got).reshape(-1)[i]) & 0xFFFFFFFF:#x} want {int(R.bits(want).reshape(-1)[i]) & 0xFFFFFFFF:#x}"
            + ("" if src is None else " from " + " ".join(f"{int(R.bits(s).reshape(-1)[i]) & 0xFFFFFFFF:#x}" for s in src)) for i in bad[:8]]
    raise AssertionError(f"{what}: {len(bad)} of {got.numel()} elements differ: " + "; ".join(rows))


def log(entry, case, ratios=None, note=""):
    print(f"[glue] {entry} {case} " + " ".join(f"{k}:{v:.3f}" for k, v in (ratios or {}).items()) + note)


# ---- srk_layernorm_fwd ---------------------------------------------------------------------------------------------------------------
def ln_fwd_call(L, x, gm, bt, rows, C, CP, yb=None, yf=None, mean=None, rstd=None, geom=None):
    p = lambda g: g.ptr if g is not None else None
    ok(L, L.lib().srk_layernorm_fwd(x.ptr, gm.ptr, bt.ptr, p(yb), p(yf), p(mean), p(rstd), rows, C, CP, geom, st()))


@pytest.mark.parametrize("c", R.LN_FWD_CASES, ids=lambda c: c.id)
def test_layernorm_fwd(L, c):
    i = R.ln_inputs(c)
    e = R.ln_fwd_ref(i["x"], i["gamma"], i["beta"], c.C)
    x, gm, bt = Operand(i["x"]), Operand(i["gamma"]), Operand(i["beta"])
    new = lambda kind, cols: Guarded(kind, c.rows, cols, cols)
    # both outputs with mean / rstd
    yb, yf, mean, rstd = new("bf16", c.CP), new("f32", c.CP), new("f32", 1), new("f32", 1)
    ln_fwd_call(L, x, gm, bt, c.rows, c.C, c.CP, yb, yf, mean, rstd)
    torch.cuda.synchronize()
    for g, what in ((yb, "y_bf16"), (yf, "y_f32"), (mean, "mean"), (rstd, "rstd")):
        g.assert_guards(f"{c.id} {what}")
    got = dict(y=yf.data(), mean=mean.data()[:, 0], rstd=rstd.data()[:, 0])
    good, ratios = R.accepts(got, e)
    log("layernorm_fwd", c.id, ratios)
    assert good, ratios
    assert is_zero_bits(yf.data()[:, c.C:]) and is_zero_bits(yb.data()[:, c.C:]), "pad columns"
    assert torch.equal(R.bits(yb.data()), R.bits(yf.data().to(torch.bfloat16))), "y_bf16 is the RNE rounding of the device's y_f32"
    # bf16 only / fp32 only / both without statistics: the same bits, nothing else touched
    for want_b, want_f in ((True, False), (False, True), (True, True)):
        b2, f2 = new("bf16", c.CP) if want_b else None, new("f32", c.CP) if want_f else None
        ln_fwd_call(L, x, gm, bt, c.rows, c.C, c.CP, b2, f2)
        torch.cuda.synchronize()
        if want_b:
            b2.assert_guards(f"{c.id} y_bf16 alone")
            assert torch.equal(R.bits(b2.data()), R.bits(yb.data()))
        if want_f:
            f2.assert_guards(f"{c.id} y_f32 alone")
            assert torch.equal(R.bits(f2.data()), R.bits(yf.data()))


@pytest.mark.parametrize("shift", R.LN_GATHER["shifts"])
def test_layernorm_fwd_gather_is_in_window_order(L, shift):
    """geom != null: output row m, mean[m] and rstd[m] belong to token roll + partition(m)."""
    H, W, B, Cc, CP = (R.LN_GATHER[k] for k in ("H", "W", "B", "C", "CP"))
    c = R.LnCase(Cc, CP, B * H * W)
    i = R.ln_inputs(c, seed_salt=shift)
    idx = torch.from_numpy(O.window_token_index(H, W, 8, shift)).reshape(-1)
    tok = torch.cat([b * H * W + idx for b in range(B)])
    e = R.ln_fwd_ref(i["x"][tok], i["gamma"], i["beta"], Cc)
    x, gm, bt = Operand(i["x"]), Operand(i["gamma"]), Operand(i["beta"])
    yb, yf = Guarded("bf16", c.rows, CP, CP), Guarded("f32", c.rows, CP, CP)
    mean, rstd = Guarded("f32", c.rows, 1, 1), Guarded("f32", c.rows, 1, 1)
    geom = L.WinGeom(H, W, shift)
    ln_fwd_call(L, x, gm, bt, c.rows, Cc, CP, yb, yf, mean, rstd, C.byref(geom))
    torch.cuda.synchronize()
    for g in (yb, yf, mean, rstd):
        g.assert_guards(f"gather shift {shift}")
    good, ratios = R.accepts(dict(y=yf.data(), mean=mean.data()[:, 0], rstd=rstd.data()[:, 0]), e)
    log("layernorm_fwd", f"gather-shift{shift}", ratios)
    assert good, ratios
    assert torch.equal(R.bits(yb.data()), R.bits(yf.data().to(torch.bfloat16))) and is_zero_bits(yf.data()[:, Cc:])
    if shift:                                           # the map is not the identity: raster-order statistics would be rejected
        raster = R.ln_fwd_ref(i["x"], i["gamma"], i["beta"], Cc)
        assert not R.accepts(dict(y=raster["y"].ref, mean=raster["mean"].ref, rstd=raster["rstd"].ref), e)[0]


# ---- srk_layernorm_bwd ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", R.LN_BWD_CASES, ids=lambda c: c.id)
def test_layernorm_bwd(L, c):
    """accumulate 0 / 1, gx_bf16 given / null, dgamma / dbeta from non-zero values, and a second call.  Pad columns C..CP-1 of gx: +0 with
    accumulate = 0; with accumulate = 1 the old value stays (the kernel adds dx = 0 to it) and gx_bf16 carries bf16 of it."""
    i = R.ln_inputs(c)
    stats = R.ln_fwd_ref(i["x"], i["gamma"], i["beta"], c.C)
    mean32, rstd32 = stats["mean"].ref.float(), stats["rstd"].ref.float()          # the fp64 statistics rounded once
    dy, x, mean, rstd, gm = Operand(i["dy"]), Operand(i["x"]), Operand(mean32), Operand(rstd32), Operand(i["gamma"])
    worst = {}
    for acc in (0, 1):
        for with_bf16 in (True, False):
            gx = Guarded("f32", c.rows, c.CP, c.CP, i["gx0"] if acc else None)
            gxb = Guarded("bf16", c.rows, c.CP, c.CP) if with_bf16 else None
            dg, db = Guarded("f32", 1, c.C, c.C, i["dgamma0"][None]), Guarded("f32", 1, c.C, c.C, i["dbeta0"][None])
            for calls in (1, 2):
                ok(L, L.lib().srk_layernorm_bwd(dy.ptr, x.ptr, mean.ptr, rstd.ptr, gm.ptr, gx.ptr, gxb.ptr if gxb else None, dg.ptr, db.ptr,
                                                c.rows, c.C, c.CP, acc, st()))
                torch.cuda.synchronize()
                what = f"{c.id} acc={acc} bf16={with_bf16} call {calls}"
                for g in (gx, dg, db) + ((gxb,) if gxb else ()):
                    g.assert_guards(what)                          # dgamma / dbeta: the guard starts right after element C
                e = R.ln_bwd_ref(i["dy"], i["x"], mean32, rstd32, i["gamma"], c.C, acc, i["gx0"], i["dgamma0"], i["dbeta0"], calls=calls)
                good, ratios = R.accepts(dict(gx=gx.data(), dgamma=dg.data()[0], dbeta=db.data()[0]), e)
                assert good, (what, ratios)
                worst = {k: max(worst.get(k, 0.0), v) for k, v in ratios.items()}
                pads = gx.data()[:, c.C:]
                if acc:
                    assert torch.equal(R.bits(pads), R.bits(i["gx0"][:, c.C:])), f"{what}: pad columns changed"
                else:
                    assert is_zero_bits(pads), f"{what}: pad columns"
                if gxb:
                    assert torch.equal(R.bits(gxb.data()), R.bits(gx.data().to(torch.bfloat16))), f"{what}: gx_bf16 != RNE(gx)"
    log("layernorm_bwd", c.id, worst)


# ---- srk_rowscale_bf16 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", R.ROWSCALE_CASES, ids=lambda c: c.id)
def test_rowscale_bf16(L, c):
    src, f = R.rowscale_inputs(c)
    want = R.rowscale_expected(src, f, c.rps)
    s, fd = Operand(src), Operand(f)                      # f: one factor per sample, NaN right after the last (partial) sample's
    dst = Guarded("bf16", c.rows, c.CP, c.CP)
    ok(L, L.lib().srk_rowscale_bf16(s.ptr, dst.ptr, fd.ptr, c.rows, c.rps, c.CP, st()))
    alias = Guarded("bf16", c.rows, c.CP, c.CP, src)
    ok(L, L.lib().srk_rowscale_bf16(alias.ptr, alias.ptr, fd.ptr, c.rows, c.rps, c.CP, st()))
    torch.cuda.synchronize()
    for g, what in ((dst, "separate dst"), (alias, "dst == src")):
        g.assert_guards(f"{c.id} {what}")
        assert_same_bits(g.data(), want, f"{c.id} {what}", src=(src,))
    log("rowscale_bf16", c.id, note="bit-equal")


# ---- the adds and the cast -------------------------------------------------------------------------------------------------------------
ELEM = [(name, n) for name in R.ELEM_BIG for n in R.ELEM_N + (R.ELEM_BIG[name],)]


@pytest.mark.parametrize("name,n", ELEM, ids=[f"{a}-n{n}" for a, n in ELEM])
def test_elementwise_bits(L, name, n):
    """Expected bits: the same fp32 expression on the CPU, torch's round-to-nearest-even conversion to bf16.  The inputs carry every pair
    of glue_ref.SPECIAL_BITS (ties, overflow to Inf, signed zeros, Inf, NaN, fp32 subnormals) in front of the random values."""
    a, b = R.elem_inputs(n)
    want = R.elem_expected(name, a, b)
    h = L.lib()
    rows = n // 4
    g4 = lambda kind, fill=None: Guarded(kind, rows, 4, 4, fill)
    if name == "add_f32_bf16":
        A, Bo, AB = g4("f32", a.view(-1, 4)), Operand(b.view(-1, 4)), g4("bf16")
        ok(L, h.srk_add_f32_bf16(A.ptr, Bo.ptr, AB.ptr, n, st()))
        outs = dict(a=A, ab=AB)
    elif name == "add_bf16_into_f32":
        A, Bo = g4("f32", a.view(-1, 4)), Operand(b.to(torch.bfloat16).view(-1, 4))
        ok(L, h.srk_add_bf16_into_f32(A.ptr, Bo.ptr, n, st()))
        outs = dict(a=A)
    elif name == "add_f32":
        Ao, Bo, Out_ = Operand(a.view(-1, 4)), Operand(b.view(-1, 4)), g4("f32")
        ok(L, h.srk_add_f32(Out_.ptr, Ao.ptr, Bo.ptr, n, st()))
        outs = dict(out=Out_)
    else:
        Ao, Y = Operand(a.view(-1, 4)), g4("bf16")
        ok(L, h.srk_cast_f32_bf16(Ao.ptr, Y.ptr, n, st()))
        outs = dict(y=Y)
    torch.cuda.synchronize()
    for k, g in outs.items():
        g.assert_guards(f"{name} n={n} {k}")
        assert_same_bits(g.data().reshape(-1), want[k], f"{name} n={n} {k}", src=(a, b))
    log(name, f"n={n}", note="bit-equal")


# ---- srk_img_prep ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", R.IMG_CASES, ids=lambda c: c.id)
def test_img_prep(L, c):
    x = R.img_inputs(c)
    want = R.img_prep_expected(x, c.H, c.W)
    xo = Operand(x.reshape(-1, c.W0))                     # NaN rows right before the first and after the last image row
    out = Guarded("f32", c.B * c.H * c.W, 4, 4)
    mean3 = (C.c_float * 3)(*R.IMG_MEAN)
    ok(L, L.lib().srk_img_prep(xo.ptr, out.ptr, c.B, c.Cimg, c.H0, c.W0, c.H, c.W, R.IMG_RANGE, C.byref(mean3), st()))
    torch.cuda.synchronize()
    out.assert_guards(c.id)
    got = out.data().view(c.B, c.H, c.W, 4)
    assert torch.equal(R.bits(got), R.bits(want)), f"{c.id}: {int((R.bits(got) != R.bits(want)).sum())} values differ"
    assert is_zero_bits(got[..., c.Cimg:])                # channel 3 and the channels >= Cimg
    log("img_prep", c.id, note="bit-equal")


# ---- srk_stem_conv ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", R.STEM_CASES, ids=lambda c: c.id)
def test_stem_conv(L, c):
    img, w, b = R.stem_inputs(c)
    e = R.stem_ref(img, w, b, c.CP)
    io, wo, bo = Operand(img.reshape(-1, 4)), Operand(w.reshape(-1)), Operand(b)       # 72 NaN pixels around the image: more than a halo row
    out = Guarded("f32", c.B * c.H * c.W, c.CP, c.CP)
    ok(L, L.lib().srk_stem_conv(io.ptr, wo.ptr, bo.ptr, out.ptr, c.B, c.H, c.W, c.Cin, c.C, c.CP, st()))
    torch.cuda.synchronize()
    out.assert_guards(c.id)
    good, ratios = R.accepts(dict(y=out.data()), dict(y=e))
    log("stem_conv", c.id, ratios)
    assert good, ratios
    assert is_zero_bits(out.data()[:, c.C:]), "columns C..CP-1"


# ---- srk_win_attention_fwd_padded ------------------------------------------------------------------------------------------------------
def attn_call(L, c, q_ptr, bias_dev, out_ptr, nH, padded=True):
    Hp, Wp = c.frame
    sy, sx = c.shifts
    CA = c.layout_heads * 32
    h = L.lib()
    if padded:
        ok(L, h.srk_win_attention_fwd_padded(q_ptr, 3 * CA, CA, bias_dev.data_ptr(), 0, out_ptr, CA, c.B, c.H, c.W, Hp, Wp, c.wh, c.ww, sy, sx, nH,
                                             c.dh ** -0.5, 0, st()))
    else:
        ok(L, h.srk_win256_attention_fwd(q_ptr, 3 * CA, CA, bias_dev.data_ptr(), 0, out_ptr, CA, c.B, c.H, c.W, c.wh, c.ww, sy, sx, nH,
                                         c.dh ** -0.5, 0, st()))


@pytest.mark.parametrize("c", R.ATTN_CASES, ids=lambda c: c.id)
def test_win_attention_fwd_padded(L, c):
    T, CA = c.B * c.H * c.W, c.layout_heads * 32
    qkv, bias = R.attn_inputs(c)
    ref = R.attn_fwd_ref(qkv, bias, c)
    q, bd = Operand(qkv), bias.cuda()
    out = Guarded("bf16", T, c.nH * 32, CA)               # the launch owns columns 0 .. 63 of the 128-column rows
    attn_call(L, c, q.ptr, bd, out.ptr, c.nH)
    torch.cuda.synchronize()
    out.assert_guards(f"{c.id}: the other branch's head columns and the guard rows")
    got = out.data().view(c.B, c.H, c.W, c.nH, 32)
    good, ratio = R.attn_accepts(got[..., :c.dh], ref)
    log("win_attention_fwd_padded", c.id, dict(out=ratio))
    assert good, ratio
    assert is_zero_bits(got[..., c.dh:]), "pad channels dh..31"
    # a 4-head launch == two 2-head launches, the second at + 64 columns
    qkv4, bias4 = R.attn_inputs(c, heads=4)
    q4, b4, b_lo, b_hi = Operand(qkv4), bias4.cuda(), bias4[:2].contiguous().cuda(), bias4[2:].contiguous().cuda()
    one, two = Guarded("bf16", T, CA, CA), Guarded("bf16", T, CA, CA)
    attn_call(L, c, q4.ptr, b4, one.ptr, 4)
    attn_call(L, c, q4.ptr, b_lo, two.ptr, 2)
    attn_call(L, c, q4.ptr + 64 * 2, b_hi, two.ptr + 64 * 2, 2)
    torch.cuda.synchronize()
    one.assert_guards(c.id)
    two.assert_guards(c.id)
    assert torch.equal(R.bits(one.data()), R.bits(two.data()))
    good4, _ = R.attn_accepts(one.data().view(c.B, c.H, c.W, 4, 32)[..., :c.dh], R.attn_fwd_ref(qkv4, bias4, c, heads=4))
    assert good4
    if c.frame == (c.H, c.W) and (c.wh, c.ww) == (16, 16):
        same = Guarded("bf16", T, c.nH * 32, CA)
        attn_call(L, c, q.ptr, bd, same.ptr, c.nH, padded=False)
        torch.cuda.synchronize()
        assert torch.equal(same.raw, out.raw), "Hp = H, Wp = W: srk_win256_attention_fwd"


def test_win_attention_fwd_padded_counts_padded_tokens(L):
    """q = 0, bias = 0, no shift, integer v: every weight is exactly 1 / N, so an output is the window's sum of v over N = 128 with the
    padded tokens counted in N; the expectation is the RNE bf16 of that exact value."""
    c = R.attn_uniform_case()
    qkv, bias, want = R.attn_uniform_inputs(c)
    q, bd = Operand(qkv), bias.cuda()
    out = Guarded("bf16", c.B * c.H * c.W, c.nH * 32, c.layout_heads * 32)
    attn_call(L, c, q.ptr, bd, out.ptr, c.nH)
    torch.cuda.synchronize()
    out.assert_guards("uniform")
    got = out.data().view(c.B, c.H, c.W, c.nH, 32)
    assert_same_bits(got[..., :c.dh].contiguous(), want, "window mean with padded tokens counted")
    assert is_zero_bits(got[..., c.dh:])
    log("win_attention_fwd_padded", "uniform", note="bit-equal")


# ---- srk_channel_gate_act (GELU), srk_spatial_gate_dev ---------------------------------------------------------------------------------
def test_channel_gate_act_gelu(L):
    B, HW, Cc, CP, S = (R.GATE_SHAPE[k] for k in ("B", "HW", "C", "CP", "S"))
    conv, w1, b1, w2, b2 = R.channel_gate_inputs()
    ref = R.channel_gate_ref(conv, w1, b1, w2, b2, 1)
    h = L.lib()
    ops = [Operand(t) for t in (conv, w1, b1, w2, b2)]
    ws = torch.empty(int(h.srk_channel_gate_workspace(B, HW, CP)), dtype=torch.uint8, device="cuda")
    gate = Guarded("f32", B, CP, CP)
    ok(L, h.srk_channel_gate_act(ops[0].ptr, ws.data_ptr(), ops[1].ptr, ops[2].ptr, ops[3].ptr, ops[4].ptr, R.GATE_SHAPE["out_scale"], gate.ptr,
                                 B, HW, Cc, CP, S, 1, st()))
    torch.cuda.synchronize()
    gate.assert_guards("channel gate")
    err = float((gate.data().double() - ref).abs().max())
    log("channel_gate_act", "gelu", dict(gate=err / R.GATE_TOL))
    assert err <= R.GATE_TOL, err
    assert is_zero_bits(gate.data()[:, Cc:])


def test_spatial_gate_dev_equals_spatial_gate(L):
    a, W0, b0, w3, b3, T, CP, S = R.spatial_gate_inputs()
    h = L.lib()
    ao, Wo, bo, wo, b3o = Operand(a), Operand(W0), Operand(b0), Operand(w3), Operand(torch.tensor([b3]))
    host, dev = Guarded("f32", T, 1, 1), Guarded("f32", T, 1, 1)
    ok(L, h.srk_spatial_gate(ao.ptr, CP, Wo.ptr, bo.ptr, wo.ptr, b3, S, host.ptr, T, CP, st()))
    ok(L, h.srk_spatial_gate_dev(ao.ptr, CP, Wo.ptr, bo.ptr, wo.ptr, b3o.ptr, S, dev.ptr, T, CP, st()))
    torch.cuda.synchronize()
    host.assert_guards("spatial_gate")
    dev.assert_guards("spatial_gate_dev")
    assert torch.equal(dev.raw, host.raw)
    ref = torch.sigmoid(torch.nn.functional.gelu(a.double() @ W0.double().t() + b0.double()) @ w3.double() + b3)
    assert float((dev.data()[:, 0].double() - ref).abs().max()) <= 2e-5          # the bound of test_dwconv_rowln_gates_vs_torch
    log("spatial_gate_dev", "dat-test-inputs", note="bit-equal to srk_spatial_gate")
