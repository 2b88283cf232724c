"""The window-attention kernels through the C ABI against the fp64 restatement and the derived per-element bound of tests/attn_ref.py
(pinned on the CPU in tests/test_attn_ref.py): srk_window_attention_fwd / _bwd, srk_win_small_attention_fwd / _bwd,
srk_win256_attention_fwd / _bwd (self-attention and the overlapping form), srk_win_attention_bwd_padded and
srk_window_attention_bwd_fused.

Per case: operands in buffers whose unused parts are NaN (leading-dimension padding, rows beyond T, the scratch), outputs in guarded
buffers that start as NaN; the guards are intact, every element the header says is written is written, err <= tol element-wise, pad
channels are exactly 0, d_table / d_bias is accumulated onto a non-zero fill.  max(err / tol) per output is printed.  Exact identities
(bit for bit): d_out = 0, v = 0, the uniform softmax, scratch against atomics, table mode against the dense bias.  No tolerance here is
a fraction of max|ref|: each comes from attn_ref.bound or is 0."""
import ctypes as C

import pytest
import torch

import attn_ref as A
from gemm_ex_ref import Out, compare
from guarded import Guarded

pytestmark = pytest.mark.gpu

FILL = 0.75
CASES = A.all_cases()


def _lib():
    from tpu_superresolution_amd import _lib as M
    return M.check, M.lib(), M.WinGeom


def _st():
    return torch.cuda.current_stream().cuda_stream


def _nan(shape, dtype):
    return torch.full(shape, float("nan"), dtype=dtype, device="cuda")


def _scratch(nbytes):
    """A scratch whose every byte is 0xFF (NaN as fp32 and as bf16): nothing in it may be taken for a zero."""
    return torch.full((max(16, int(nbytes)),), 0xFF, dtype=torch.uint8, device="cuda")


# ---- layouts ---------------------------------------------------------------------------------------------------------------------------------
def raster_operands(c, inp):
    """qkv [T + 3][3 CA + 8] and d_out [T + 3][nH 32 + 8] on the device: NaN beyond the data window and in the rows beyond T; the spare
    column blocks of a wider CA hold 1.0 (they are another launch's heads: what sits there must not matter)."""
    CA, T = c.CA, c.T
    qkv = _nan((T + 3, 3 * CA + 8), torch.bfloat16)
    for i, name in enumerate("qkv"):
        qkv[:T, i * CA:i * CA + c.nH * 32] = inp[name].reshape(T, c.nH * 32).cuda()
        if c.spare:
            qkv[:T, i * CA + c.nH * 32:(i + 1) * CA] = 1.0
    do = _nan((T + 3, c.nH * 32 + 8), torch.bfloat16)
    do[:T, :c.nH * 32] = inp["do"].reshape(T, c.nH * 32).cuda()
    return qkv, do


def from_raster(c, dq: Guarded):
    """d_qkv [T][3 CA] -> dq, dk, dv [T][nH][32] (and the spare blocks)."""
    g = dq.data().view(c.T, 3, c.CA)
    heads = g[:, :, :c.nH * 32].reshape(c.T, 3, c.nH, 32)
    return dict(dq=heads[:, 0], dk=heads[:, 1], dv=heads[:, 2]), g[:, :, c.nH * 32:]


def win8_operands(c, inp):
    """[3][B_][nH][64][32] window-ordered q / k / v and d_out [B_ 64][nH 32]: row m holds token tok[m]."""
    tok = A.geometry(c)[0].reshape(-1)
    x = torch.stack([inp["q"], inp["k"], inp["v"]])[:, tok].view(3, c.windows, 64, c.nH, 32).permute(0, 1, 3, 2, 4).contiguous()
    return tok, x.cuda(), inp["do"][tok].reshape(-1, c.nH * 32).contiguous().cuda()


def to_tokens(rows: torch.Tensor, tok: torch.Tensor) -> torch.Tensor:
    out = torch.empty_like(rows)
    out[tok] = rows
    return out


# ---- one call of every entry point -------------------------------------------------------------------------------------------------------------
def n_atomic(c, ref):
    """fp32 atomic additions that land on one d_table / d_bias entry: attn.hip's reduce adds once per (i, j) pair of the entry, the
    table / bias reduce kernels once per 32-window slice, the rectangular kernel without scratch once per window."""
    if c.kern == "win8":
        return ref.n_terms / c.windows
    if c.kern == "rect" and not c.scratch:
        return torch.full_like(ref.n_terms, float(c.windows))
    return torch.full_like(ref.n_terms, float(-(-c.windows // 32)))


def run_bwd(c, inp, fill=FILL):
    """-> (dq / dk / dv [T][nH][32] bf16 on the host in token order, d_table or d_bias with the fill still in it, the Guarded d_qkv, the
    spare column blocks or None)."""
    check, L, WinGeom = _lib()
    rows = c.table_rows
    if c.kern == "win8":
        tok, qkv, do = win8_operands(c, inp)
        bias = A.dense_bias(c, inp).float().contiguous().cuda()
        dq = Guarded("bf16", c.windows * 64, 3 * c.CA, 3 * c.CA)
        dtab = torch.full((225, c.nH), fill, device="cuda")
        slab = _scratch(L.srk_window_attention_bwd_scratch(c.windows, c.nH))
        check(L.srk_window_attention_bwd(qkv.data_ptr(), bias.data_ptr(), do.data_ptr(), dq.ptr, dtab.data_ptr(), slab.data_ptr(), c.windows, c.nH,
                                         c.scale, C.byref(WinGeom(c.H, c.W, c.sy)), _st()))
        torch.cuda.synchronize()
        g = to_tokens(dq.data(), tok).view(c.T, 3, c.nH, 32)
        return dict(dq=g[:, 0], dk=g[:, 1], dv=g[:, 2]), dtab.cpu(), dq, None
    qkv, do = raster_operands(c, inp)
    ldq, ldo = qkv.shape[1], do.shape[1]
    dq = Guarded("bf16", c.T, 3 * c.CA, ldq)
    par = (inp["bias"] if c.kern == "rect" else inp["table"]).contiguous().cuda()       # held until the synchronize below
    if c.kern == "small":
        dtab = torch.full((rows, c.nH), fill, device="cuda")
        scr = _scratch(L.srk_win_small_attention_bwd_scratch(c.B, c.H, c.W, c.wh, c.nH))
        check(L.srk_win_small_attention_bwd(qkv.data_ptr(), ldq, c.CA, par.data_ptr(), do.data_ptr(), ldo, dq.ptr, dtab.data_ptr(),
                                            scr.data_ptr(), c.B, c.H, c.W, c.wh, c.sy, c.nH, c.scale, _st()))
    elif c.kern in ("w256", "oca"):
        ov = 8 if c.kern == "oca" else 0
        dtab = torch.full((rows, c.nH), fill, device="cuda")
        scr = _scratch(L.srk_win256_attention_bwd_scratch(c.B, c.H, c.W, c.nH, c.CA, rows, ov))
        check(L.srk_win256_attention_bwd(qkv.data_ptr(), ldq, c.CA, par.data_ptr(), rows, do.data_ptr(), ldo, dq.ptr, dtab.data_ptr(),
                                         scr.data_ptr(), c.B, c.H, c.W, c.sy, c.sx, c.nH, c.scale, ov, _st()))
    else:
        Hp, Wp = c.frame
        dtab = torch.full((c.nH, c.N, c.N), fill, device="cuda")
        scr = _scratch(L.srk_win_attention_bwd_padded_scratch(c.B, Hp, Wp, c.wh, c.ww, c.nH)) if c.scratch else None
        check(L.srk_win_attention_bwd_padded(qkv.data_ptr(), ldq, c.CA, par.data_ptr(), do.data_ptr(), ldo, dq.ptr, dtab.data_ptr(),
                                             scr.data_ptr() if c.scratch else None, c.B, c.H, c.W, Hp, Wp, c.wh, c.ww, c.sy, c.sx, c.nH, c.scale, _st()))
    torch.cuda.synchronize()
    got, spare = from_raster(c, dq)
    return got, dtab.cpu(), dq, spare


def run_fwd(c, inp, dense=False):
    """-> o [T][nH][32] bf16 on the host and its Guarded buffer."""
    check, L, WinGeom = _lib()
    if c.kern == "win8":
        tok, qkv, _ = win8_operands(c, inp)
        bias = A.dense_bias(c, inp).float().contiguous().cuda()
        o = Guarded("bf16", c.windows * 64, c.CA, c.CA)
        check(L.srk_window_attention_fwd(qkv.data_ptr(), bias.data_ptr(), o.ptr, c.windows, c.nH, C.byref(WinGeom(c.H, c.W, c.sy)), _st()))
        torch.cuda.synchronize()
        return to_tokens(o.data(), tok).view(c.T, c.nH, 32), o
    qkv, _ = raster_operands(c, inp)
    ldq = qkv.shape[1]
    o = Guarded("bf16", c.T, c.nH * 32, c.nH * 32 + 8)
    if c.kern == "small":
        b = inp["table"].cuda()
        check(L.srk_win_small_attention_fwd(qkv.data_ptr(), ldq, c.CA, b.data_ptr(), o.ptr, o.ld, c.B, c.H, c.W, c.wh, c.sy, c.nH,
                                            c.scale, _st()))
    else:
        ov = 8 if c.kern == "oca" else 0
        b = (A.dense_bias(c, inp).float().contiguous() if dense else inp["table"]).cuda()
        check(L.srk_win256_attention_fwd(qkv.data_ptr(), ldq, c.CA, b.data_ptr(), 0 if dense else c.table_rows, o.ptr, o.ld, c.B, c.H, c.W, 16, 16,
                                         c.sy, c.sx, c.nH, c.scale, ov, _st()))
    torch.cuda.synchronize()
    return o.data().view(c.T, c.nH, 32), o


def _written(t, what):
    assert not bool(torch.isnan(t.float()).any()), f"{what}: {int(torch.isnan(t.float()).sum())} elements were not written (or are NaN)"


def _check(what, got, out: Out, d):
    ok, ratio = compare(got, out)
    print(f"[attn] {what}: max err / tol {ratio:.3f}")
    assert ok, f"{what}: max err / tol {ratio:.3f}"
    if out.kind == "bf16" and d < 32:
        assert float(got[..., d:].float().abs().max()) == 0.0, f"{what}: pad channels are not exactly 0"


def _check_spare(c, spare, dq):
    if c.spare and c.kern == "small":          # the header: every column 0 .. 3 CA - 1 is written, the block without a head as zeros
        assert float(spare.float().abs().max()) == 0.0
    elif c.spare:                              # rect: the q | k | v slices of the heads of this launch, nothing else
        assert bool(torch.isnan(spare.float()).all()), "columns of the other launch's heads were written"


_refs = {}


def ref_of(c):
    """Reference of the operands of a case (shared by the backward and the forward test of the case; never modified)."""
    key = A.with_(c, fwd=False, scratch=True)
    if key not in _refs:
        if len(_refs) > 4:
            _refs.clear()
        inp = A.make_inputs(key)
        _refs[key] = (inp, A.reference(key, inp))
    return _refs[key]


# ---- values -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [c for c in CASES if not c.fwd], ids=lambda c: c.id)
def test_attention_backward_within_the_derived_bound(c):
    inp, ref = ref_of(c)
    got, dtab, dq, spare = run_bwd(c, inp)
    dq.assert_guards(c.id)
    for k in ("dq", "dk", "dv"):
        _written(got[k], f"{c.id} {k}")
        _check(f"{c.id} {k}", got[k], ref.out[k], c.d)
    _check_spare(c, spare, dq)
    key = "dbias" if c.kern == "rect" else "dtab"
    o = ref.out[key]
    _written(dtab, f"{c.id} {key}")
    _check(f"{c.id} {key}", dtab.double() - FILL, Out(o.ref, A.fill_tol(o.tol, ref.dS_abs_sum, n_atomic(c, ref), FILL), "f32"), 32)


@pytest.mark.parametrize("c", [c for c in CASES if c.kern != "rect" and c.scratch], ids=lambda c: c.id)
def test_attention_forward_within_the_derived_bound(c):
    inp, ref = ref_of(c)
    got, o = run_fwd(c, inp)
    o.assert_guards(c.id)
    _written(got, f"{c.id} o")
    _check(f"{c.id} o", got, ref.out["o"], c.d)
    if c.kern in ("w256", "oca"):          # table mode is bit-equal to dense mode on the expanded table
        dense, od = run_fwd(c, inp, dense=True)
        od.assert_guards(c.id + " dense")
        assert torch.equal(dense.view(torch.int16), got.view(torch.int16)), f"{c.id}: table mode differs from the dense bias"


# ---- exact identities ----------------------------------------------------------------------------------------------------------------------------
IDENT = [A.ACase("win8", 9, 24, 40, 6, 30, sy=4, sx=4), A.ACase("small", 1, 12, 12, 6, 30, 2, 2, 1, 1), A.ACase("small", 2, 21, 14, 2, 16, 7, 7, 3, 3),
         A.ACase("w256", 3, 48, 64, 2, 30, 16, 16, 5, 11), A.ACase("oca", 2, 32, 48, 3, 30, 16, 16),
         A.ACase("rect", 2, 40, 48, 2, 12, wh=8, ww=16, sy=5, sx=3, Hp=48, Wp=48), A.ACase("rect", 2, 40, 48, 2, 12, wh=8, ww=16, sy=5, sx=3, Hp=48, Wp=48, scratch=False)]


@pytest.mark.parametrize("c", IDENT, ids=lambda c: c.id)
def test_zero_gradient_and_zero_v_are_exact(c):
    """d_out = 0: d_qkv = 0 and d_table bit-unchanged.  v = 0: dP = 0, so dS = P (0 - 0) = 0: dq = dk = 0 exactly and d_table
    bit-unchanged, while dv = P^T dO stays within its bound."""
    inp = A.make_inputs(c)
    zero = dict(inp, do=torch.zeros_like(inp["do"]))
    got, dtab, dq, _ = run_bwd(c, zero)
    dq.assert_guards(c.id)
    for k in ("dq", "dk", "dv"):
        assert float(got[k].float().abs().max()) == 0.0, f"{c.id}: d_out = 0 must give {k} = 0 exactly"
    assert torch.equal(dtab.view(torch.int32), torch.full_like(dtab, FILL).view(torch.int32)), f"{c.id}: d_out = 0 must leave d_table bit-unchanged"
    zv = dict(inp, v=torch.zeros_like(inp["v"]))
    got, dtab, dq, _ = run_bwd(c, zv)
    for k in ("dq", "dk"):
        assert float(got[k].float().abs().max()) == 0.0, f"{c.id}: v = 0 must give {k} = 0 exactly"
    assert torch.equal(dtab.view(torch.int32), torch.full_like(dtab, FILL).view(torch.int32)), f"{c.id}: v = 0 must leave d_table bit-unchanged"
    _check(f"{c.id} dv at v = 0", got["dv"], A.reference(c, zv).out["dv"], c.d)


@pytest.mark.parametrize("c", A.uniform_cases(), ids=lambda c: c.id)
def test_uniform_softmax_gives_the_region_mean_exactly(c):
    """q = 0 and table / bias = 0: P = 1 / n over the n keys of the query's mask region (a masked score is -100: its exponential is
    below 2^-133 against 1 and vanishes from the fp32 row sum and from the bf16 copy of P).  With d_out in {-256, 0, 256} every region
    sum is a multiple of 256 of at most 2^16 and the mean over a power-of-two region is a bf16 number, so dv[token] == mean of d_out over
    the token's region, bit for bit: an exact check of the row maps, the transposing reads and the store permutation.  Unshifted, every
    region is the window (64, 16 / 4, 256, 128 tokens).  With the half-window shift the regions of the last window row / column are the
    halves and quarters of the window (32 + 32 or 4 x 16 of 64; 128 + 128 or 4 x 64 of 256; 64 + 64 or 4 x 32 of 128): all powers of two,
    so the equality holds at every token of these cases (attn_ref.uniform_dv reports where it would not)."""
    inp = A.uniform_inputs(c)
    want, exact = A.uniform_dv(c, inp)
    assert bool(exact.all())
    got, _, dq, _ = run_bwd(c, inp)
    dq.assert_guards(c.id)
    assert torch.equal(got["dv"].double(), want), f"{c.id}: {int((got['dv'].double() != want).sum())} elements of dv differ from the region mean"


def test_rect_scratch_and_atomics_agree():
    """The two d-bias paths of srk_win_attention_bwd_padded: d_qkv bit-equal, d_bias within the any-order summation term of each."""
    c = A.ACase("rect", 2, 40, 48, 2, 12, wh=8, ww=16, sy=5, sx=3, Hp=48, Wp=48)
    inp, ref = ref_of(c)
    g1, b1, _, _ = run_bwd(c, inp)
    g2, b2, _, _ = run_bwd(A.with_(c, scratch=False), inp)
    for k in ("dq", "dk", "dv"):
        assert torch.equal(g1[k].view(torch.int16), g2[k].view(torch.int16)), k
    n = ref.n_terms
    tol = 2 * (n * A.U * ref.dS_abs_sum + n_atomic(A.with_(c, scratch=False), ref) * A.U * (FILL + ref.dS_abs_sum)) + A.F32_TINY
    err = (b1.double() - b2.double()).abs()
    print(f"[attn] rect scratch vs atomics: d_bias max err / tol {float((err / tol).max()):.3f}")
    assert bool((err <= tol).all())


# ---- the re-projecting backward -----------------------------------------------------------------------------------------------------------------
FUSED = A.fused_cases(256)          # the ids are those of the 256-CU matrix; the shapes follow the device


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def run_fused(c, f, lda, ldg, fill=FILL):
    check, L, WinGeom = _lib()
    tok = A.geometry(c)[0].reshape(-1)
    M = c.windows * 64
    xn, g = _nan((M + 3, lda), torch.bfloat16), _nan((M + 3, ldg), torch.bfloat16)
    xn[:M, :192], g[:M, :192] = f["xn"][tok].cuda(), f["g"][tok].cuda()
    w, b, wp = f["wqkv"].cuda(), f["bqkv"].cuda(), f["wproj_t"].cuda()
    bias = A.dense_bias(c, f).float().contiguous().cuda()
    dq = Guarded("bf16", M, 576, 576)
    dtab = torch.full((225, 6), fill, device="cuda")
    slab = _scratch(L.srk_window_attention_bwd_fused_scratch(c.windows, 6))
    rc = L.srk_window_attention_bwd_fused(xn.data_ptr(), lda, w.data_ptr(), b.data_ptr(), c.scale, g.data_ptr(), ldg, wp.data_ptr(), bias.data_ptr(), dq.ptr,
                                          dtab.data_ptr(), slab.data_ptr(), c.windows, 6, C.byref(WinGeom(c.H, c.W, c.sy)), _st())
    torch.cuda.synchronize()
    return rc, tok, dq, dtab.cpu()


@pytest.mark.parametrize("i", range(len(FUSED)), ids=[c.id for c in FUSED])
def test_fused_backward_within_the_derived_bound_and_the_composition_it_replaces(i):
    """srk_window_attention_bwd_fused against the 8 x 8 restatement on the operands of attn_ref.fused_project, with one bf16 step of
    operand uncertainty exactly where the fp64 projection lies within its accumulation bound of a rounding boundary.  Then the
    composition it replaces, srk_window_attention_bwd on the same operands materialised on the host, within ITS bound (no operand
    uncertainty: it reads them).  Bit-equality of the two is not asserted: nothing in the code guarantees it -- the fused kernel's q / k /
    v / dO can differ by a bf16 step at the uncertain elements, it takes dQ from the dS accumulators where attn.hip reads the bf16 copy
    back from LDS in another k order, and its d(bias) slabs hold other window lists, so d_table is summed in another order."""
    n = _cus()
    c = A.fused_cases(n)[i]
    lists = A.fused_lists(c.windows, n)
    f = A.fused_inputs(c)
    inp, unc = A.fused_project(c, f)
    ref = A.reference(c, inp, unc=unc)
    rc, tok, dq, dtab = run_fused(c, f, *((192, 192) if i % 2 == 0 else (200, 208)))
    assert rc == 0
    dq.assert_guards(c.id)
    g = to_tokens(dq.data(), tok).view(c.T, 3, 6, 32)
    tag = f"fused {c.id} ({c.windows} windows, lists of {lists[0]}..{lists[1]})"
    for j, k in enumerate(("dq", "dk", "dv")):
        _written(g[:, j], f"{tag} {k}")
        _check(f"{tag} {k}", g[:, j], ref.out[k], c.d)
    o = ref.out["dtab"]
    _check(f"{tag} dtab", dtab.double() - FILL, Out(o.ref, A.fill_tol(o.tol, ref.dS_abs_sum, n_atomic(c, ref), FILL), "f32"), 32)
    ref0 = A.reference(c, inp)
    got, dtab0, dq0, _ = run_bwd(c, inp)
    dq0.assert_guards(c.id)
    for k in ("dq", "dk", "dv"):
        _check(f"composition {c.id} {k}", got[k], ref0.out[k], c.d)
    o = ref0.out["dtab"]
    _check(f"composition {c.id} dtab", dtab0.double() - FILL, Out(o.ref, A.fill_tol(o.tol, ref0.dS_abs_sum, n_atomic(c, ref0), FILL), "f32"), 32)


def test_fused_backward_zero_gradient_zero_v_and_refusal():
    """g = 0 gives dO = 0: d_qkv = 0 exactly, d_table bit-unchanged.  v = 0 (the v rows of w_qkv and b_qkv zero): dq = dk = 0 exactly,
    d_table bit-unchanged.  Fewer windows than CUs, or a leading dimension that is no multiple of 8: SRK_E_UNSUPPORTED, nothing written."""
    n = _cus()
    c = A.fused_cases(n)[1]
    f = A.fused_inputs(c)
    for what, ff in (("g = 0", dict(f, g=torch.zeros_like(f["g"]))),
                     ("v = 0", dict(f, wqkv=torch.cat([f["wqkv"][:384], torch.zeros_like(f["wqkv"][384:])]), bqkv=torch.cat([f["bqkv"][:384], torch.zeros(192)])))):
        rc, tok, dq, dtab = run_fused(c, ff, 200, 192)
        assert rc == 0
        dq.assert_guards(what)
        g = dq.data().float().view(-1, 3, 6, 32)
        for j, k in enumerate(("dq", "dk", "dv")):
            if what == "g = 0" or k != "dv":
                assert float(g[:, j].abs().max()) == 0.0, f"{what} must give {k} = 0 exactly"
        assert torch.equal(dtab.view(torch.int32), torch.full_like(dtab, FILL).view(torch.int32)), f"{what} must leave d_table bit-unchanged"
    small = A.ACase("win8", n - 1, 8, 8, 6, 30)
    fs = A.fused_inputs(small)
    for lda, ldg, cc in ((192, 192, small), (196, 192, c), (192, 204, c)):
        rc, _, dq, dtab = run_fused(cc, fs if cc is small else f, lda, ldg)
        assert rc == -3, (lda, ldg, cc.id)
        dq.assert_untouched("d_qkv of a refused call")
        assert torch.equal(dtab, torch.full_like(dtab, FILL))


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------------
def test_illegal_shifts_and_misaligned_leading_dimensions_are_refused():
    check, L, WinGeom = _lib()
    SHAPE = -1
    z = torch.zeros(1 << 20, dtype=torch.bfloat16, device="cuda")
    f = torch.zeros(1 << 20, dtype=torch.float32, device="cuda")
    out = Guarded("bf16", 1024, 192, 640)
    p, fp = z.data_ptr(), f.data_ptr()
    # 8 x 8: the shift is 0 or 4, the map a multiple of 8, B_ a multiple of the windows of a map
    for geom in (WinGeom(16, 16, 3), WinGeom(16, 16, 8), WinGeom(16, 12, 0)):
        assert L.srk_window_attention_bwd(p, fp, p, out.ptr, fp, fp, 4, 2, 0.25, C.byref(geom), _st()) == SHAPE
        assert L.srk_window_attention_fwd(p, fp, out.ptr, 4, 2, C.byref(geom), _st()) == SHAPE
    assert L.srk_window_attention_bwd(p, fp, p, out.ptr, fp, fp, 5, 2, 0.25, C.byref(WinGeom(16, 16, 0)), _st()) == SHAPE
    # ws 2 .. 7: 0 <= shift < ws; ldq % 8, ldo % 8 (backward) / % 4 (forward)
    small_b = lambda shift=3, ldq=200, ldo=64: L.srk_win_small_attention_bwd(p, ldq, 64, fp, p, ldo, out.ptr, fp, fp, 1, 14, 14, 7, shift, 2, 0.25, _st())
    small_f = lambda shift=3, ldq=200, ldo=64: L.srk_win_small_attention_fwd(p, ldq, 64, fp, out.ptr, ldo, 1, 14, 14, 7, shift, 2, 0.25, _st())
    for fn in (small_b, small_f):
        assert fn(shift=7) == SHAPE and fn(shift=-1) == SHAPE and fn(ldq=196) == SHAPE and fn(ldq=184) == SHAPE and fn(ldo=66) == SHAPE
    assert small_b(ldo=68) == SHAPE
    # 16 x 16
    w_b = lambda sy=8, sx=8, ldq=296, ldo=96, ov=0: L.srk_win256_attention_bwd(p, ldq, 96, fp, 1521 if ov else 961, p, ldo, out.ptr, fp, fp, 1, 32, 32, sy,
                                                                               sx, 3, 0.25, ov, _st())
    w_f = lambda sy=8, sx=8, ldq=296, ldo=96, ov=0: L.srk_win256_attention_fwd(p, ldq, 96, fp, 1521 if ov else 961, out.ptr, ldo, 1, 32, 32, 16, 16, sy,
                                                                               sx, 3, 0.25, ov, _st())
    for fn in (w_b, w_f):
        assert fn(sy=16) == SHAPE and fn(sx=16) == SHAPE and fn(sy=-1) == SHAPE and fn(ldq=292) == SHAPE and fn(ldq=280) == SHAPE and fn(ldo=98) == SHAPE
        assert fn(sy=8, sx=8, ov=8) == -3          # SRK_E_UNSUPPORTED: the overlapping form takes no shift
    assert w_b(ldo=100) == SHAPE
    # rectangular
    r_b = lambda sy=4, sx=8, ldq=200, ldo=64, wh=8, ww=16: L.srk_win_attention_bwd_padded(p, ldq, 64, fp, p, ldo, out.ptr, fp, None, 1, 24, 40, 32, 48, wh, ww,
                                                                                          sy, sx, 2, 0.25, _st())
    assert r_b(sy=8) == SHAPE and r_b(sx=16) == SHAPE and r_b(sx=-1) == SHAPE and r_b(ldq=196) == SHAPE and r_b(ldq=184) == SHAPE and r_b(ldo=68) == SHAPE
    assert r_b(wh=8, ww=8) == -3
    torch.cuda.synchronize()
    out.assert_untouched("the output of a refused call")
    assert float(f.abs().max()) == 0.0
