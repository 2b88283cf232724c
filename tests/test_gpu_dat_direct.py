"""Direct parity, through the C ABI, of DAT's token passes and token reductions (csrc/dat_train.hip, the non-attention half of csrc/dat.hip)
against the fp64 restatements of tests/dat_ref.py: srk_rowln_bf16, srk_rowln_bwd_bf16, srk_chan_stats, srk_sum_rows_f32, srk_bn_train_coeffs,
srk_bn_train_bwd_coeffs, srk_affine_act_bf16, srk_lincomb2_bf16, srk_dgelu_affine_bf16, srk_mul_bwd_bf16, srk_dual_gate_combine,
srk_dual_gate_bwd, srk_dwconv3x3, srk_dwconv3x3_wgrad, srk_chan_gram, srk_chan_apply_mat, srk_channel_attention_fwd, srk_spatial_gate_train.

Every case checks
  1. values per element: within the DERIVED bound of dat_ref (the log line carries max(err / tol) per output; a failure names the first
     offending index), and bit for bit where the kernel is a fixed sequence of IEEE operations;
  2. that nothing else is written: outputs are slices (column offset 8, stride wider than the slice) of guarded.Guarded buffers -- the
     guard rows, the columns beside the slice and the pad columns the kernel does not promise to write stay bit-identical; partial
     buffers start 0xFF-filled (no kernel may rely on zeroed partials), accumulated outputs from a non-zero fill;
  3. that nothing else is read: every operand is a slice of a NaN buffer between NaN rows; pad columns the kernels promise to mask hold NaN;
  4. exact identities (dy = 0, unit / zero gates, integer-valued operands of the reductions) and the argument refusals of the launchers.

The comparators' ability to fail is pinned on the CPU (tests/test_dat_ref.py)."""
import pytest
import torch

import dat_ref as R
from dat_ref import BF
from guarded import Guarded

pytestmark = pytest.mark.gpu

NAN_ROWS = 72
OFF = 8                   # column offset of every slice
E_SHAPE, E_NULL = -1, -2


@pytest.fixture(scope="module")
def L():
    from tpu_superresolution_amd import _lib
    _lib.claim_device(0)
    torch.cuda.set_device(0)
    return _lib.lib()


def st():
    return torch.cuda.current_stream().cuda_stream


def ok(L, rc):
    assert rc == 0, (rc, L.srk_last_error().decode())


class Operand:
    """A device operand [rows][width] (a vector is one row) as a column slice (from column `off`) of a NaN buffer with row stride ld,
    between NAN_ROWS rows of NaN.  Integer operands (real_of) are framed with -1."""

    def __init__(self, t, ld=None, off=0, nan_rows=NAN_ROWS):
        t2 = t.reshape(t.shape[0], -1) if t.dim() > 1 else t.reshape(1, -1)
        rows, width = t2.shape
        self.ld = ld or width
        assert off + width <= self.ld
        fill = float("nan") if t2.dtype.is_floating_point else -1
        self.buf = torch.full((rows + 2 * nan_rows, self.ld), fill, dtype=t2.dtype)
        self.buf[nan_rows:nan_rows + rows, off:off + width] = t2
        self.buf = self.buf.cuda()
        self.ptr = self.buf.data_ptr() + (nan_rows * self.ld + off) * t2.element_size()


def sl(t, extra=24, **kw):
    """a bf16 slice at column OFF of rows `extra` elements wider than it"""
    return Operand(t, ld=t.shape[1] + extra, off=OFF, **kw)


class Out(Guarded):
    """A Guarded buffer whose data window is the slice [rows][off : off + width] of rows with stride ld; the columns in front of the slice
    belong to the guard.  ff: the slice starts 0xFF-filled (partials); fill: it starts from these values (accumulated outputs)."""

    def __init__(self, kind, rows, width, ld=None, off=0, fill=None, ff=False):
        ld = ld or width + off
        super().__init__(kind, rows, off + width, ld)
        self.off, self.width = off, width
        if fill is not None:
            self.win[:, off:off + width] = fill.to(self.win.dtype).cuda()
        if ff:
            self.win[:, off:off + width].view(torch.int32 if kind == "f32" else torch.int16).fill_(-1)
        self.before = self.raw.clone()

    @property
    def ptr(self):
        return self.win.data_ptr() + self.off * self.win.element_size()

    def data(self):
        return self.win[:, self.off:self.off + self.width].cpu()

    def assert_guards(self, what):
        super().assert_guards(what)
        if self.off:
            front = slice(0, self.off)
            now = self.raw.view(-1, self.ld)[:, front]
            assert torch.equal(now, self.before.view(-1, self.ld)[:, front]), f"{what}: columns in front of the slice were written"


def oslice(rows, width, extra=16, **kw):
    return Out("bf16", rows, width, ld=width + OFF + extra, off=OFF, **kw)


def check(family, case, got, exp, outs=()):
    """per-element acceptance; the failure message carries max(err / tol) per output and the first offending index"""
    for g in outs:
        g.assert_guards(f"{family} {case}")
    good, ratios = R.accepts(got, exp)
    print(f"[dat] {family} {case} " + " ".join(f"{k}:{v:.3f}" for k, v in ratios.items()))
    if not good:
        msg = []
        for k, o in exp.items():
            err = (got[k].double() - o.ref).abs()
            bad = ~(err <= o.tol.expand_as(o.ref))
            if bool(bad.any()):
                idx = tuple(int(v) for v in bad.nonzero()[0])
                msg.append(f"{k}: max err/tol {ratios[k]:.3g}, {int(bad.sum())} of {bad.numel()} outside, first at {idx}: got "
                           f"{float(got[k][idx]):.9g} want {float(o.ref[idx]):.9g} tol {float(o.tol.expand_as(o.ref)[idx]):.3g}")
        raise AssertionError(f"{family} {case}: " + "; ".join(msg))
    return ratios


def assert_bits(got, want, what):
    if R.same_bits(got, want):
        return
    bad = ((R.bits(got) != R.bits(want)) & ~(got.isnan() & want.isnan())).nonzero()
    i = tuple(int(v) for v in bad[0])
    raise AssertionError(f"{what}: {len(bad)} of {got.numel()} elements differ in their bits, first at {i}: got {float(got[i]):.9g} want {float(want[i]):.9g}")


def zero_bits(t):
    return bool((R.bits(t.contiguous()) == 0).all())


# ---- srk_rowln_bf16 / srk_rowln_bwd_bf16 --------------------------------------------------------------------------------------------------
def nan_pad(t, CP):
    """[rows][C] -> [rows][CP] with NaN in the pad columns the kernels promise to mask"""
    return R.embed(t, CP, 0)


@pytest.mark.parametrize("c", R.ROWLN_FWD_CASES, ids=lambda c: c.id)
def test_rowln_bf16(L, c):
    i = R.rowln_inputs(c)
    x, gm, bt = sl(nan_pad(i["x"], c.CP)), Operand(i["gamma"]), Operand(i["beta"])
    out = oslice(c.rows, c.CP)
    ok(L, L.srk_rowln_bf16(x.ptr, x.ld, gm.ptr, bt.ptr, out.ptr, out.ld, c.rows, c.C, c.CP, st()))
    torch.cuda.synchronize()
    check("rowln_bf16", c.id, dict(out=out.data()), R.rowln_fwd_ref(i["x"], i["gamma"], i["beta"], c.CP), (out,))
    assert zero_bits(out.data()[:, c.C:]), "pad columns C .. CP_out - 1 are +0"


@pytest.mark.parametrize("c", R.ROWLN_BWD_CASES, ids=lambda c: c.id)
def test_rowln_bwd_bf16(L, c):
    i = R.rowln_inputs(c)
    nb = R.rowln_bwd_blocks(c.rows)
    assert int(L.srk_rowln_bwd_blocks(c.rows)) == nb
    x, dy, gm = sl(nan_pad(i["x"], c.CP)), sl(nan_pad(i["dy"], c.CP), extra=40), Operand(i["gamma"])
    dx, part = oslice(c.rows, c.CP), Out("f32", nb, 2 * c.C, ff=True)
    ok(L, L.srk_rowln_bwd_bf16(dy.ptr, dy.ld, x.ptr, x.ld, gm.ptr, dx.ptr, dx.ld, part.ptr, c.rows, c.C, c.CP, st()))
    torch.cuda.synchronize()
    check("rowln_bwd_bf16", c.id, dict(dx=dx.data(), partial=part.data().view(nb, 2, c.C)), R.rowln_bwd_ref(i["dy"], i["x"], i["gamma"], c.CP),
          (dx, part))
    assert zero_bits(dx.data()[:, c.C:]), "pad columns C .. CP_out - 1 are +0"
    if c.rows <= 300:                                   # dy = 0: dx and the partials are exactly zero
        z = sl(nan_pad(torch.zeros_like(i["dy"]), c.CP))
        dx0, p0 = oslice(c.rows, c.CP), Out("f32", nb, 2 * c.C, ff=True)
        ok(L, L.srk_rowln_bwd_bf16(z.ptr, z.ld, x.ptr, x.ld, gm.ptr, dx0.ptr, dx0.ld, p0.ptr, c.rows, c.C, c.CP, st()))
        torch.cuda.synchronize()
        assert bool((dx0.data().float() == 0).all()) and bool((p0.data() == 0).all()), "dy = 0"


def test_rowln_argument_refusals(L):
    b = torch.zeros(64, 1024, dtype=BF, device="cuda")
    f = torch.zeros(4096, device="cuda")
    p, q = b.data_ptr(), f.data_ptr()
    assert L.srk_rowln_bf16(None, 64, q, q, p, 64, 4, 60, 64, st()) == E_NULL
    assert L.srk_rowln_bf16(p, 64, q, q, p, 64, 4, 60, 520, st()) == E_SHAPE           # CP_out > 512
    assert L.srk_rowln_bf16(p, 60, q, q, p, 64, 4, 60, 64, st()) == E_SHAPE            # stride not a multiple of 8
    assert L.srk_rowln_bf16(p, 64, q, q, p, 64, 4, 65, 64, st()) == E_SHAPE            # C > CP_out
    assert L.srk_rowln_bwd_bf16(p, 64, p, 64, q, None, 64, q, 4, 60, 64, st()) == E_NULL
    assert L.srk_rowln_bwd_bf16(p, 64, p, 64, q, p, 64, q, 4, 60, 520, st()) == E_SHAPE
    assert L.srk_rowln_bwd_bf16(p, 64, p, 60, q, p, 64, q, 4, 60, 64, st()) == E_SHAPE
    assert L.srk_rowln_bwd_bf16(p, 64, p, 64, q, p, 56, q, 4, 60, 64, st()) == E_SHAPE  # stride below CP_out


# ---- srk_chan_stats ------------------------------------------------------------------------------------------------------------------------
def run_chan_stats(L, p, q, c):
    nck = -(-c.rps // R.ST_ROWS)
    assert int(L.srk_chan_stats_chunks(c.rps)) == nck
    ps, qs = sl(p), sl(q, extra=56)                       # ldp != ldq
    part = Out("f32", c.samples * nck, 2 * 8 * c.C8, ff=True)
    ok(L, L.srk_chan_stats(ps.ptr, ps.ld, qs.ptr, qs.ld, part.ptr, c.samples, c.rps, c.C8, st()))
    torch.cuda.synchronize()
    return part, part.data().view(c.samples, nck, 2, 8 * c.C8)


@pytest.mark.parametrize("c", R.STATS_CASES, ids=lambda c: c.id)
def test_chan_stats(L, c):
    p, q = R.stats_inputs(c)
    part, got = run_chan_stats(L, p, q, c)
    check("chan_stats", c.id, dict(partial=got), R.chan_stats_ref(p, q, c), (part,))
    p, q = R.stats_inputs(c, integers=True)                # integer operands: the sums are exact in fp32 in any order
    part, got = run_chan_stats(L, p, q, c)
    part.assert_guards(c.id)
    assert torch.equal(got.double(), R.chan_stats_ref(p, q, c)["partial"].ref), "integer-valued operands: exact sums"
    _, pp = run_chan_stats(L, p, p, c)                      # chan_stats(p, p) row 1 = the squared column norms
    assert torch.equal(pp[:, :, 1].sum(1).double(), (p.double() ** 2).view(c.samples, c.rps, -1).sum(1))


def test_chan_stats_argument_refusals(L):
    b = torch.zeros(64, 1024, dtype=BF, device="cuda")
    f = torch.zeros(4096, device="cuda")
    p, q = b.data_ptr(), f.data_ptr()
    assert L.srk_chan_stats(None, 64, p, 64, q, 1, 4, 8, st()) == E_NULL
    assert L.srk_chan_stats(p, 64, p, 64, None, 1, 4, 8, st()) == E_NULL
    assert L.srk_chan_stats(p, 1024, p, 1024, q, 1, 4, 65, st()) == E_SHAPE            # C8 > 64
    assert L.srk_chan_stats(p, 60, p, 64, q, 1, 4, 4, st()) == E_SHAPE                 # stride not a multiple of 8
    assert L.srk_chan_stats(p, 64, p, 64, q, 1, 0, 8, st()) == E_SHAPE


# ---- srk_sum_rows_f32, srk_bn_train_coeffs, srk_bn_train_bwd_coeffs ---------------------------------------------------------------------------
@pytest.mark.parametrize("c", R.BN_CASES, ids=lambda c: c.id)
def test_sum_rows_f32(L, c):
    x = R.sum_rows_inputs(c)
    for integers in (False, True):
        if integers:
            x = torch.randint(-1000, 1001, x.shape, generator=torch.Generator().manual_seed(c.R)).float()
        xin, out = Operand(x.reshape(c.outer * c.R, c.C)), Out("f32", c.outer, c.C)
        ok(L, L.srk_sum_rows_f32(xin.ptr, c.outer, c.R, c.C, out.ptr, st()))
        torch.cuda.synchronize()
        if integers:
            out.assert_guards(c.id)
            assert torch.equal(out.data().double(), x.double().sum(1)), "integer-valued rows: exact sums"
        else:
            check("sum_rows_f32", c.id, dict(sum=out.data()), R.sum_rows_ref(x), (out,))


@pytest.mark.parametrize("c", R.BN_CASES, ids=lambda c: c.id)
def test_bn_train_coeffs(L, c):
    i = R.bn_inputs(c)
    part, gm, bt = Operand(i["partial"]), Operand(i["gamma"]), Operand(i["beta"])
    real_of = Operand(i["real_of"])
    coef = Out("f32", 4, c.C, ld=c.ld)                       # columns C .. ld - 1 of every coefficient row are not written
    rm, rv = Out("f32", 1, i["n_real"], fill=i["rm0"][None]), Out("f32", 1, i["n_real"], fill=i["rv0"][None])
    ok(L, L.srk_bn_train_coeffs(part.ptr, c.R, c.row_stride, c.ld, c.C, i["n"], gm.ptr, bt.ptr, R.BN_EPS, coef.ptr, rm.ptr, rv.ptr, R.BN_MOMENTUM,
                                real_of.ptr, st()))
    torch.cuda.synchronize()
    e = R.bn_train_coeffs_ref(i, c)
    check("bn_train_coeffs", c.id, dict(coef=coef.data(), running_mean=rm.data()[0], running_var=rv.data()[0]), e, (coef, rm, rv))
    # without running buffers: the same coefficients, bit for bit
    coef2 = Out("f32", 4, c.C, ld=c.ld)
    ok(L, L.srk_bn_train_coeffs(part.ptr, c.R, c.row_stride, c.ld, c.C, i["n"], gm.ptr, bt.ptr, R.BN_EPS, coef2.ptr, None, None, R.BN_MOMENTUM, None, st()))
    # the backward, from the fp64 forward coefficients rounded once to fp32
    fwd32 = R.embed(e["coef"].ref.float(), c.ld, 0)
    bpart, fwd = Operand(i["bwd_partial"]), Operand(fwd32)
    bc = Out("f32", 5, c.C, ld=c.ld)
    ok(L, L.srk_bn_train_bwd_coeffs(bpart.ptr, c.R, c.row_stride, c.ld, c.C, i["n"], fwd.ptr, bc.ptr, st()))
    torch.cuda.synchronize()
    coef2.assert_guards(c.id)
    assert_bits(coef2.data(), coef.data(), "coefficients without running buffers")
    check("bn_train_bwd_coeffs", c.id, dict(coef=bc.data()), R.bn_train_bwd_coeffs_ref(i, fwd32[:, :c.C], c), (bc,))


def test_bn_coeffs_argument_refusals(L):
    f = torch.zeros(4096, device="cuda")
    q = f.data_ptr()
    assert L.srk_sum_rows_f32(None, 1, 4, 8, q, st()) == E_NULL and L.srk_sum_rows_f32(q, 1, 0, 8, q, st()) == E_SHAPE
    assert L.srk_bn_train_coeffs(q, 4, 32, 16, 8, 64.0, q, q, 1e-5, None, None, None, 0.1, None, st()) == E_NULL
    assert L.srk_bn_train_coeffs(q, 4, 24, 16, 8, 64.0, q, q, 1e-5, q, None, None, 0.1, None, st()) == E_SHAPE     # row_stride < 2 ld
    assert L.srk_bn_train_coeffs(q, 4, 32, 16, 17, 64.0, q, q, 1e-5, q, None, None, 0.1, None, st()) == E_SHAPE    # C > ld
    assert L.srk_bn_train_coeffs(q, 4, 32, 16, 8, 64.0, q, q, 1e-5, q, q, None, 0.1, None, st()) == E_SHAPE        # one running buffer only
    assert L.srk_bn_train_bwd_coeffs(q, 4, 32, 16, 8, 64.0, None, q, st()) == E_NULL
    assert L.srk_bn_train_bwd_coeffs(q, 4, 24, 16, 8, 64.0, q, q, st()) == E_SHAPE


# ---- srk_affine_act_bf16, srk_lincomb2_bf16 --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", R.EW_CASES, ids=lambda c: c.id)
def test_affine_act_bf16(L, c):
    i = R.ew_inputs(c)
    C = 8 * c.C8
    x, s, t = sl(i["p"]), Operand(i["A"]), Operand(i["B"])           # NaN right after the last sample's coefficients
    for act in (0, 1):
        out = oslice(c.rows, C)
        ok(L, L.srk_affine_act_bf16(x.ptr, x.ld, s.ptr, t.ptr, out.ptr, out.ld, c.rows, c.C8, c.rps, act, st()))
        torch.cuda.synchronize()
        check("affine_act_bf16", f"{c.id}-act{act}", dict(out=out.data()), R.affine_act_ref(i, c, act), (out,))
        if act == 0:
            assert_bits(out.data(), R.affine_act_bits(i, c)[0], "x * s + t is one fused multiply-add, rounded once")


@pytest.mark.parametrize("c", R.EW_CASES, ids=lambda c: c.id)
def test_lincomb2_bf16(L, c):
    i = R.ew_inputs(c)
    C = 8 * c.C8
    p, q = sl(i["p"]), sl(i["q"], extra=40)
    A, Bc, Cc = Operand(i["A"]), Operand(i["B"]), Operand(i["C"])
    args = {"copy": (p, None, None, None, None, 0), "c_acc": (None, None, None, None, Cc, 1), "ap": (p, None, A, None, None, 0),
            "ap_bq_c": (p, q, A, Bc, Cc, 0), "p_acc": (p, None, None, None, None, 1)}
    for pat in R.EW_PATTERNS:
        pp, qq, a, b, cc, acc = args[pat]
        out = oslice(c.rows, C, fill=i["old"] if acc else None)
        ptr = lambda o: o.ptr if o is not None else None
        ok(L, L.srk_lincomb2_bf16(ptr(pp), pp.ld if pp else 0, ptr(qq), qq.ld if qq else 0, ptr(a), ptr(b), ptr(cc), out.ptr, out.ld, c.rows, c.C8,
                                  c.rps, acc, st()))
        torch.cuda.synchronize()
        check("lincomb2_bf16", f"{c.id}-{pat}", dict(out=out.data()), R.lincomb2_ref(i, c, pat), (out,))
        want = R.lincomb2_bits(i, c, pat)
        if want is not None:
            assert_bits(out.data(), want, f"lincomb2 {pat}: one IEEE operation, one rounding")


def test_elementwise_argument_refusals(L):
    b = torch.zeros(64, 1024, dtype=BF, device="cuda")
    f = torch.zeros(4096, device="cuda")
    p, q = b.data_ptr(), f.data_ptr()
    assert L.srk_affine_act_bf16(None, 64, q, q, p, 64, 4, 8, 0, 0, st()) == E_NULL
    assert L.srk_affine_act_bf16(p, 60, q, q, p, 64, 4, 4, 0, 0, st()) == E_SHAPE
    assert L.srk_affine_act_bf16(p, 64, q, q, p, 64, 0, 8, 0, 0, st()) == E_SHAPE
    assert L.srk_lincomb2_bf16(p, 64, None, 0, None, None, None, None, 64, 4, 8, 0, 0, st()) == E_NULL
    assert L.srk_lincomb2_bf16(p, 60, None, 0, None, None, None, p, 64, 4, 4, 0, 0, st()) == E_SHAPE
    assert L.srk_lincomb2_bf16(None, 0, None, 0, q, None, None, p, 64, 4, 8, 0, 0, st()) == E_SHAPE          # a coefficient without its operand
    assert L.srk_dgelu_affine_bf16(p, 64, None, 64, q, q, p, 64, 4, 8, st()) == E_NULL
    assert L.srk_dgelu_affine_bf16(p, 64, p, 64, q, q, p, 60, 4, 4, st()) == E_SHAPE
    assert L.srk_dgelu_affine_bf16(p, 64, p, 64, q, q, p, 64, 1 << 26, 64, st()) == E_SHAPE                   # rows * C8 >= 2^31
    assert L.srk_mul_bwd_bf16(p, 64, p, 64, p, 64, None, 64, p, 64, 4, 8, st()) == E_NULL
    assert L.srk_mul_bwd_bf16(p, 64, p, 60, p, 64, p, 64, p, 64, 4, 4, st()) == E_SHAPE


# ---- srk_dgelu_affine_bf16, srk_mul_bwd_bf16 (flat kernels) -----------------------------------------------------------------------------------
@pytest.mark.parametrize("c", R.FLAT_CASES + [R.FLAT_WRAP], ids=lambda c: c.id)
def test_dgelu_affine_and_mul_bwd(L, c):
    i = R.flat_inputs(c)
    C = 8 * c.C8
    dy, x, a, b = sl(i["dy"]), sl(i["x"], extra=8), sl(i["a"], extra=40), sl(i["b"], extra=16)
    s, t = Operand(i["scale"]), Operand(i["shift"])
    out = oslice(c.rows, C)
    ok(L, L.srk_dgelu_affine_bf16(dy.ptr, dy.ld, x.ptr, x.ld, s.ptr, t.ptr, out.ptr, out.ld, c.rows, c.C8, st()))
    da, db = oslice(c.rows, C), oslice(c.rows, C, extra=32)
    ok(L, L.srk_mul_bwd_bf16(dy.ptr, dy.ld, a.ptr, a.ld, b.ptr, b.ld, da.ptr, da.ld, db.ptr, db.ld, c.rows, c.C8, st()))
    torch.cuda.synchronize()
    check("dgelu_affine_bf16", c.id, dict(out=out.data()), R.dgelu_affine_ref(i), (out,))
    da.assert_guards(c.id)
    db.assert_guards(c.id)
    wa, wb = R.mul_bwd_bits(i)
    assert_bits(da.data(), wa, "mul_bwd da = bf16(dy b)")
    assert_bits(db.data(), wb, "mul_bwd db = bf16(dy a)")
    print(f"[dat] mul_bwd_bf16 {c.id} bit-equal")


# ---- srk_dual_gate_combine, srk_dual_gate_bwd ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", R.GATE_CASES, ids=lambda c: c.id)
def test_dual_gate_combine_and_bwd(L, c):
    i = R.gate_inputs(c)
    T = c.B * c.HW
    a, b, d = Operand(i["a"]), Operand(i["b"]), Operand(i["d"])                     # contiguous [T][CA]: the entry points take no stride
    cg, tg = Operand(i["cgate"]), Operand(i["tgate"])
    for on_a in (0, 1):
        out = Out("bf16", T, c.CA)
        ok(L, L.srk_dual_gate_combine(a.ptr, b.ptr, cg.ptr, tg.ptr, out.ptr, T, c.HW, c.CA, on_a, st()))
        torch.cuda.synchronize()
        check("dual_gate_combine", f"{c.id}-tok_on_a{on_a}", dict(out=out.data()), R.dual_gate_combine_ref(i, c, on_a), (out,))
        assert any(R.same_bits(out.data(), cand) for cand in R.dual_gate_combine_bits(i, c, on_a)), \
            "a g1 + b g2 is none of: two products and a sum, a multiply-add around the first product, one around the second"
    # unit / zero gates: the token-gated operand passes unchanged, the other vanishes
    one, zero = Operand(torch.ones(T)), Operand(torch.zeros(c.B, c.CA))
    out = Out("bf16", T, c.CA)
    ok(L, L.srk_dual_gate_combine(a.ptr, b.ptr, zero.ptr, one.ptr, out.ptr, T, c.HW, c.CA, 1, st()))
    nck = -(-c.HW // 64)
    d_chan, d_tok = Out("bf16", T, c.CA), Out("bf16", T, c.CA)
    dcg, dsmap = Out("f32", c.B * nck, c.CA, ff=True), Out("f32", T, 1, ff=True)
    ok(L, L.srk_dual_gate_bwd(d.ptr, a.ptr, b.ptr, cg.ptr, tg.ptr, d_chan.ptr, d_tok.ptr, dcg.ptr, dsmap.ptr, c.B, c.HW, c.CA, st()))
    torch.cuda.synchronize()
    out.assert_guards(c.id)
    assert bool((out.data().float() == i["a"].float()).all()), "token gate 1 on a, channel gate 0 on b: out == a"
    e = R.dual_gate_bwd_ref(i, c)
    got = dict(d_chan=d_chan.data(), d_tok=d_tok.data(), dcg_partial=dcg.data().view(c.B, nck, c.CA), dsmap=dsmap.data()[:, 0])
    check("dual_gate_bwd", c.id, got, e, (d_chan, d_tok, dcg, dsmap))
    wc, wt = R.dual_gate_bwd_bits(i, c)
    assert_bits(d_chan.data(), wc, "d_chan = bf16(d cgate)")
    assert_bits(d_tok.data(), wt, "d_tok = bf16(d tgate)")
    assert float(got["dsmap"][0]) == 0.0 and float(got["dsmap"][T - 1]) == 0.0, "token gates exactly 0 and exactly 1: no gradient through the sigmoid"


def test_dual_gate_argument_refusals(L):
    b = torch.zeros(64, 1024, dtype=BF, device="cuda")
    f = torch.zeros(4096, device="cuda")
    p, q = b.data_ptr(), f.data_ptr()
    assert L.srk_dual_gate_combine(p, None, q, q, p, 4, 4, 64, 0, st()) == E_NULL
    assert L.srk_dual_gate_combine(p, p, q, q, p, 4, 4, 60, 0, st()) == E_SHAPE
    assert L.srk_dual_gate_combine(p, p, q, q, p, 6, 4, 64, 0, st()) == E_SHAPE          # rows not a multiple of rows_per_sample
    assert L.srk_dual_gate_bwd(p, p, p, q, q, p, p, None, q, 1, 4, 64, st()) == E_NULL
    assert L.srk_dual_gate_bwd(p, p, p, q, q, p, p, q, q, 1, 4, 264, st()) == E_SHAPE     # CA > 256
    assert L.srk_dual_gate_bwd(p, p, p, q, q, p, p, q, q, 1, 4, 60, st()) == E_SHAPE      # CA % 8


# ---- srk_dwconv3x3, srk_dwconv3x3_wgrad -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", R.DW_CASES, ids=lambda c: c.id)
def test_dwconv3x3_and_wgrad(L, c):
    i = R.dw_inputs(c)
    C, T = 8 * c.C8, c.B * c.H * c.W
    halo = c.W + 8                                           # more NaN pixels around the images than a halo row reaches
    x, mul, dy = sl(i["x"], nan_rows=halo), sl(i["mul"], extra=40), sl(i["dy"], extra=8, nan_rows=halo)
    w, sc, sh = Operand(i["w"]), Operand(i["scale"]), Operand(i["shift"])
    for act, with_mul in R.DW_VARIANTS:
        out = oslice(T, C)                                   # ldo != ldm
        ok(L, L.srk_dwconv3x3(x.ptr, x.ld, w.ptr, sc.ptr, sh.ptr, mul.ptr if with_mul else None, mul.ld if with_mul else 0, out.ptr, out.ld,
                              c.B, c.H, c.W, c.C8, act, st()))
        torch.cuda.synchronize()
        check("dwconv3x3", f"{c.id}-act{act}-mul{int(with_mul)}", dict(out=out.data()), R.dwconv_ref(i, c, act, with_mul), (out,))
    nb = -(-c.H // 8)
    assert int(L.srk_dwconv3x3_wgrad_chunks(c.H)) == nb
    part = Out("f32", c.B * nb, 10 * C, ff=True)
    ok(L, L.srk_dwconv3x3_wgrad(dy.ptr, dy.ld, x.ptr, x.ld, part.ptr, c.B, c.H, c.W, c.C8, st()))
    torch.cuda.synchronize()
    check("dwconv3x3_wgrad", c.id, dict(partial=part.data().view(c.B, nb, 10, C)), R.dwconv_wgrad_ref(i, c), (part,))
    g = torch.Generator().manual_seed(c.H * 100 + c.W)        # integer operands: exact sums
    j = dict(x=torch.randint(-8, 9, (T, C), generator=g).float().to(BF), dy=torch.randint(-8, 9, (T, C), generator=g).float().to(BF))
    xi, dyi = sl(j["x"], nan_rows=halo), sl(j["dy"], nan_rows=halo)
    part = Out("f32", c.B * nb, 10 * C, ff=True)
    ok(L, L.srk_dwconv3x3_wgrad(dyi.ptr, dyi.ld, xi.ptr, xi.ld, part.ptr, c.B, c.H, c.W, c.C8, st()))
    torch.cuda.synchronize()
    part.assert_guards(c.id)
    assert torch.equal(part.data().view(c.B, nb, 10, C).double(), R.dwconv_wgrad_ref(j, c)["partial"].ref), "integer-valued operands: exact sums"


def test_dwconv_argument_refusals(L):
    b = torch.zeros(64, 1024, dtype=BF, device="cuda")
    f = torch.zeros(8192, device="cuda")
    p, q = b.data_ptr(), f.data_ptr()
    assert L.srk_dwconv3x3(None, 64, q, q, q, None, 0, p, 64, 1, 2, 2, 8, 0, st()) == E_NULL
    assert L.srk_dwconv3x3(p, 1024, q, q, q, None, 0, p, 1024, 1, 2, 2, 65, 0, st()) == E_SHAPE      # C8 > 64
    assert L.srk_dwconv3x3(p, 60, q, q, q, None, 0, p, 64, 1, 2, 2, 4, 0, st()) == E_SHAPE          # stride not a multiple of 8
    assert L.srk_dwconv3x3(p, 56, q, q, q, None, 0, p, 64, 1, 2, 2, 8, 0, st()) == E_SHAPE          # stride below the slice
    assert L.srk_dwconv3x3(p, 64, q, q, q, p, 60, p, 64, 1, 2, 2, 8, 0, st()) == E_SHAPE
    assert L.srk_dwconv3x3_wgrad(p, 64, None, 64, q, 1, 2, 2, 8, st()) == E_NULL
    assert L.srk_dwconv3x3_wgrad(p, 1024, p, 1024, q, 1, 2, 2, 65, st()) == E_SHAPE
    assert L.srk_dwconv3x3_wgrad(p, 60, p, 64, q, 1, 2, 2, 4, st()) == E_SHAPE


# ---- srk_chan_gram, srk_chan_apply_mat, srk_channel_attention_fwd ----------------------------------------------------------------------------
@pytest.mark.parametrize("c", R.CHAN_CASES, ids=lambda c: c.id)
def test_chan_gram_and_apply_mat(L, c):
    i = R.chan_inputs(c)
    CA, T, nck = c.CA, c.B * c.N, -(-c.N // R.GRAM_CH)
    xq, yk = i["qkv"][:, :CA].contiguous(), i["qkv"][:, CA:2 * CA].contiguous()
    x, y = sl(xq), sl(yk, extra=40)
    assert int(L.srk_chan_gram_floats(c.B, c.N, c.nH)) == c.B * c.nH * nck * R.GRAM_SZ
    part = Out("f32", c.B * c.nH * nck, R.GRAM_SZ, ff=True)
    ok(L, L.srk_chan_gram(x.ptr, x.ld, y.ptr, y.ld, part.ptr, c.B, c.N, c.nH, st()))
    torch.cuda.synchronize()
    check("chan_gram", c.id, dict(partial=part.data().view(c.B, c.nH, nck, R.GRAM_SZ)), R.chan_gram_ref(xq, yk, c), (part,))
    # integer operands: exact Gram sums, and the squared norms are what chan_stats(p, p) returns in its second row
    g = torch.Generator().manual_seed(c.N + c.d)
    xi = torch.zeros(T, c.nH, 32)
    xi[..., :c.d] = torch.randint(-8, 9, (T, c.nH, c.d), generator=g).float()
    xi = xi.reshape(T, CA).to(BF)
    xs = sl(xi)
    part = Out("f32", c.B * c.nH * nck, R.GRAM_SZ, ff=True)
    ok(L, L.srk_chan_gram(xs.ptr, xs.ld, xs.ptr, xs.ld, part.ptr, c.B, c.N, c.nH, st()))
    sc = R.StatsCase(CA // 8, c.N, c.B)
    stats = Out("f32", c.B * nck, 2 * CA, ff=True)
    ok(L, L.srk_chan_stats(xs.ptr, xs.ld, xs.ptr, xs.ld, stats.ptr, c.B, c.N, sc.C8, st()))
    torch.cuda.synchronize()
    part.assert_guards(c.id)
    got = part.data().view(c.B, c.nH, nck, R.GRAM_SZ)
    assert torch.equal(got.double(), R.chan_gram_ref(xi, xi, c)["partial"].ref), "integer-valued operands: exact sums"
    norms = got[..., 1024:1056].sum(2).reshape(c.B, CA)                          # [B][nH][32] -> [B][CA]
    assert torch.equal(norms, stats.data().view(c.B, nck, 2, CA)[:, :, 1].sum(1)), "chan_gram's squared norms == chan_stats(p, p) row 1"
    # the matrix application
    src, src2 = sl(i["qkv"][:, 2 * CA:].contiguous()), sl(i["src2"], extra=40)
    M, dg = Operand(i["M"].reshape(-1, 1024)), Operand(i["diag"].reshape(-1, 32))
    for with_diag in (False, True):
        for acc in (0, 1):
            out = oslice(T, CA, fill=i["old"] if acc else None)
            ok(L, L.srk_chan_apply_mat(M.ptr, src.ptr, src.ld, dg.ptr if with_diag else None, src2.ptr if with_diag else None,
                                       src2.ld if with_diag else 0, out.ptr, out.ld, c.B, c.N, c.nH, acc, st()))
            torch.cuda.synchronize()
            check("chan_apply_mat", f"{c.id}-diag{int(with_diag)}-acc{acc}", dict(out=out.data()), R.chan_apply_mat_ref(i, c, with_diag, acc), (out,))
    eye = Operand(torch.eye(32).repeat(c.B * c.nH, 1, 1).reshape(-1, 1024))
    out = oslice(T, CA)
    ok(L, L.srk_chan_apply_mat(eye.ptr, src.ptr, src.ld, None, None, 0, out.ptr, out.ld, c.B, c.N, c.nH, 0, st()))
    torch.cuda.synchronize()
    out.assert_guards(c.id)
    assert bool((out.data().float() == i["qkv"][:, 2 * CA:].float()).all()), "an identity matrix copies src"


@pytest.mark.parametrize("c", R.CHAN_CASES, ids=lambda c: c.id)
def test_channel_attention_fwd(L, c):
    i = R.chan_inputs(c)
    T = c.B * c.N
    qkv = sl(i["qkv"])
    temp = Operand(i["temperature"])
    nbytes = int(L.srk_channel_attention_workspace(c.B, c.N, c.nH))
    assert nbytes == 4 * (c.B * c.nH * (-(-c.N // R.GRAM_CH)) * R.GRAM_SZ + c.B * c.nH * 1024)
    ws = Out("f32", 1, nbytes // 4, ff=True)
    out = oslice(T, c.CA)
    ok(L, L.srk_channel_attention_fwd(qkv.ptr, qkv.ld, c.CA, temp.ptr, ws.ptr, out.ptr, out.ld, c.B, c.N, c.nH, c.d, st()))
    torch.cuda.synchronize()
    check("channel_attention_fwd", c.id, dict(out=out.data()), R.channel_attention_ref(i, c), (out, ws))
    pads = out.data().view(T, c.nH, 32)[..., c.d:]
    assert bool((pads.float() == 0).all()), "channels head_dim .. 31 of every head are zero"


def test_channel_attention_argument_refusals(L):
    b = torch.zeros(64, 1024, dtype=BF, device="cuda")
    f = torch.zeros(65536, device="cuda")
    p, q = b.data_ptr(), f.data_ptr()
    assert L.srk_chan_gram(None, 64, p, 64, q, 1, 4, 1, st()) == E_NULL
    assert L.srk_chan_gram(p, 60, p, 64, q, 1, 4, 1, st()) == E_SHAPE
    assert L.srk_chan_apply_mat(None, p, 64, None, None, 0, p, 64, 1, 4, 1, 0, st()) == E_NULL
    assert L.srk_chan_apply_mat(q, p, 64, q, None, 0, p, 64, 1, 4, 1, 0, st()) == E_NULL            # diag without src2
    assert L.srk_chan_apply_mat(q, p, 60, None, None, 0, p, 64, 1, 4, 1, 0, st()) == E_SHAPE
    assert L.srk_channel_attention_fwd(p, 96, 32, q, None, p, 32, 1, 4, 1, 30, st()) == E_NULL
    assert L.srk_channel_attention_fwd(p, 96, 32, q, q, p, 32, 1, 4, 1, 33, st()) == E_SHAPE          # head_dim > 32
    assert L.srk_channel_attention_fwd(p, 96, 64, q, q, p, 64, 1, 4, 1, 30, st()) == E_SHAPE          # CA != 32 heads
    assert L.srk_channel_attention_fwd(p, 88, 32, q, q, p, 32, 1, 4, 1, 30, st()) == E_SHAPE          # ldq < 3 CA


# ---- srk_spatial_gate_train -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", R.SGT_CASES, ids=lambda c: c.id)
def test_spatial_gate_train(L, c):
    i = R.sgt_inputs(c)
    nb = -(-c.rows // R.SGT_BLOCK)
    x = sl(i["x"])                                            # ldx > C
    W0, b0, sc, sh, w3 = (Operand(i[k]) for k in ("W0", "b0", "bn_scale", "bn_shift", "w3"))
    ds, cA, cB, cC = (Operand(i[k]) for k in ("dsmap", "cA", "cB", "cC"))
    call = lambda what, dx, lddx, acc, part: ok(L, L.srk_spatial_gate_train(
        what, x.ptr, x.ld, W0.ptr, b0.ptr, sc.ptr if what else None, sh.ptr if what else None, w3.ptr if what else None, ds.ptr if what else None,
        cA.ptr if what == 2 else None, cB.ptr if what == 2 else None, cC.ptr if what == 2 else None, dx, lddx, acc, part.ptr, c.rows, c.C, c.S, st()))
    p0, p1 = Out("f32", nb, 32, ff=True), Out("f32", nb, 64, ff=True)
    call(0, None, 0, 0, p0)
    call(1, None, 0, 0, p1)
    torch.cuda.synchronize()
    check("spatial_gate_train", f"{c.id}-what0", dict(partial=p0.data().view(nb, 2, 16)), R.spatial_gate_train_ref(i, c, 0), (p0,))
    check("spatial_gate_train", f"{c.id}-what1", dict(partial=p1.data().view(nb, 4, 16)), R.spatial_gate_train_ref(i, c, 1), (p1,))
    assert bool((p0.data().view(nb, 2, 16)[..., c.S:] == 0).all()) and bool((p1.data().view(nb, 4, 16)[:, 3, 1:] == 0).all()), "unused slots are 0"
    for acc in (0, 1):
        dx, p2 = oslice(c.rows, c.C, fill=i["old"] if acc else None), Out("f32", nb, 16 * (c.C + 1), ff=True)
        call(2, dx.ptr, dx.ld, acc, p2)
        torch.cuda.synchronize()
        check("spatial_gate_train", f"{c.id}-what2-acc{acc}", dict(dx=dx.data(), partial=p2.data()), R.spatial_gate_train_ref(i, c, 2, acc), (dx, p2))
    # dsmap = 0: no gradient reaches dz; with cB = cC = 0 as well dx, d W0 and d b0 are exactly zero
    zrow, zS = Operand(torch.zeros(c.rows)), Operand(torch.zeros(c.S))
    dx, p2 = oslice(c.rows, c.C), Out("f32", nb, 16 * (c.C + 1), ff=True)
    ok(L, L.srk_spatial_gate_train(2, x.ptr, x.ld, W0.ptr, b0.ptr, sc.ptr, sh.ptr, w3.ptr, zrow.ptr, cA.ptr, zS.ptr, zS.ptr, dx.ptr, dx.ld, 0, p2.ptr,
                                   c.rows, c.C, c.S, st()))
    torch.cuda.synchronize()
    dx.assert_guards(c.id)
    assert bool((dx.data().float() == 0).all()) and bool((p2.data() == 0).all()), "dsmap = 0, cB = cC = 0"


def test_spatial_gate_train_argument_refusals(L):
    b = torch.zeros(64, 1024, dtype=BF, device="cuda")
    f = torch.zeros(65536, device="cuda")
    p, q = b.data_ptr(), f.data_ptr()
    base = lambda **kw: L.srk_spatial_gate_train(*[kw.get(k, v) for k, v in dict(
        what=0, x=p, ldx=256, W0=q, b0=q, sc=q, sh=q, w3=q, ds=q, cA=q, cB=q, cC=q, dx=p, lddx=256, acc=0, part=q, rows=4, C=128, S=7, st=st()).items()])
    assert base() == 0
    assert base(x=None) == E_NULL and base(part=None) == E_NULL
    assert base(what=1, w3=None) == E_NULL and base(what=2, dx=None) == E_NULL and base(what=2, cB=None) == E_NULL
    assert base(S=17) == E_SHAPE and base(C=72) == E_SHAPE and base(C=320) == E_SHAPE and base(ldx=252) == E_SHAPE and base(what=3) == E_SHAPE
    torch.cuda.synchronize()
