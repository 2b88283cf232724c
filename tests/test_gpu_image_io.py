"""srk_image_unpack / srk_image_pack (csrc/image_io.hip) through the C ABI, against the numpy restatement tests/image_io_ref.py (pinned
on the host by tests/test_image_io_ref.py).  Every operand and output sits between guards (NaN pattern for fp32, 0xFF bytes for samples,
0x55555555 for the counters); every comparison is bit equality.

Shapes: B in {1, 2} x H in {1, 2, 17} x W in {1, 3, 63, 64, 65, 130} -- one pixel, less than one group of four, one short of / exactly
/ one past a wave's 64 columns, more than one workgroup's first stride, P = H * W both a multiple of 4 (the float4 path) and not; with
B = 2 the second image starts at every dword phase the 1- .. 8-byte pixels produce.  The largest case is under 0.2 MB."""
import itertools

import numpy as np
import pytest
import torch

import image_io_ref as R
from guarded import Guarded

pytestmark = pytest.mark.gpu

E_SHAPE, E_NULL, E_ALIGN = -1, -2, -5
GUARD = 256          # bytes on either side of a sample buffer (the allocation is 256-byte aligned, so the window keeps its phase)
SHAPES = list(itertools.product((1, 2), (1, 2, 17), (1, 3, 63, 64, 65, 130)))
DT = {8: np.uint8, 16: np.uint16}
_TIES = {}


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return t if (t is None or isinstance(t, int)) else t.ptr


def _unpack(src, dst, alpha, B, H, W, ic, bits, oc):
    from tpu_superresolution_amd._lib import lib
    return lib().srk_image_unpack(_ptr(src), _ptr(dst), _ptr(alpha), B, H, W, ic, bits, oc, _stream())


def _pack(y, alpha, dst, counters, B, H, W, C, oc, bits):
    from tpu_superresolution_amd._lib import lib
    return lib().srk_image_pack(_ptr(y), _ptr(alpha), _ptr(dst), _ptr(counters), B, H, W, C, oc, bits, _stream())


class Bytes:
    """A byte window at `offset` past a 256-byte boundary, with GUARD bytes of 0xFF before and after it."""

    def __init__(self, nbytes, offset=0, fill=None):
        self.n, self.lo = nbytes, GUARD + offset
        self.raw = torch.full((self.lo + nbytes + GUARD,), 0xFF, dtype=torch.uint8, device="cuda")
        assert self.raw.data_ptr() % 256 == 0
        if fill is not None:
            self.raw[self.lo:self.lo + nbytes] = torch.from_numpy(np.ascontiguousarray(fill).view(np.uint8).reshape(-1)).cuda()
        self.before = self.raw.clone()

    @property
    def ptr(self):
        return self.raw.data_ptr() + self.lo

    def data(self, dtype, shape):
        return self.raw[self.lo:self.lo + self.n].cpu().numpy().view(dtype).reshape(shape)

    def assert_guards(self, what):
        same = self.raw == self.before
        same[self.lo:self.lo + self.n] = True
        assert bool(same.all()), f"{what}: {int((~same).sum())} bytes outside the window were written, first at {int((~same).nonzero()[0])} " \
                                 f"(window {self.lo}..{self.lo + self.n})"

    def assert_untouched(self, what):
        assert torch.equal(self.raw, self.before), f"{what} was written"


class Counters:
    def __init__(self, start=(5, 7)):
        self.raw = torch.full((64 + 2 + 64,), 0x55555555, dtype=torch.int32, device="cuda")
        self.raw[64:66] = torch.tensor(start, dtype=torch.int32)
        self.before = self.raw.clone()

    @property
    def ptr(self):
        return self.raw.data_ptr() + 64 * 4

    def values(self):
        return self.raw[64:66].tolist()

    def assert_guards(self, what):
        assert torch.equal(self.raw[:64], self.before[:64]) and torch.equal(self.raw[66:], self.before[66:]), f"{what}: counter guards written"

    def assert_untouched(self, what):
        assert torch.equal(self.raw, self.before), f"{what} was written"


def _f32(t):
    """fp32 operand [1][n] between NaN guards."""
    t = torch.as_tensor(np.ascontiguousarray(t)).reshape(1, -1)
    return Guarded("f32", 1, t.shape[1], t.shape[1], fill=t)


def _out_f32(n):
    return Guarded("f32", 1, n, n)


def _bits32(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.uint32)


def _samples(bits, shape, seed):
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256 if bits == 8 else 65536, size=shape, dtype=np.uint32).astype(DT[bits])
    ends = np.array([np.iinfo(DT[bits]).max, 0], dtype=DT[bits])[:a.size]          # both ends of the range, where they fit
    a.reshape(-1)[:len(ends)] = ends
    return a


def _values(shape, bits, seed):
    """fp32 in about [-0.1, 1.1] with the specials and the searched ties planted where they fit."""
    rng = np.random.default_rng(seed)
    y = (rng.random(shape, dtype=np.float32) * np.float32(1.2) - np.float32(0.1)).astype(np.float32)
    if bits not in _TIES:
        _TIES[bits] = R.ties(bits, limit=16)[0]
        assert len(_TIES[bits]) > 0
    plant = np.concatenate([R.specials(), _TIES[bits]])
    flat = y.reshape(-1)
    n = min(len(plant), flat.size)
    flat[flat.size - n:] = plant[:n]          # at the end: the last, possibly partial, group of four sees them
    return y


# ---- unpack ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [8, 16])
@pytest.mark.parametrize("ic", [1, 2, 3, 4])
def test_unpack_every_shape(ic, bits):
    for (B, H, W), oc, with_alpha in itertools.product(SHAPES, (1, 3), (False, True)):
        what = f"unpack B{B} {H}x{W} ic{ic} {bits}b oc{oc} alpha={with_alpha}"
        a = _samples(bits, (B, H, W, ic), seed=H * 131 + W + ic)
        src, dst = Bytes(a.nbytes, fill=a), _out_f32(B * oc * H * W)
        al = _out_f32(B * H * W) if with_alpha else None
        assert _unpack(src, dst, al, B, H, W, ic, bits, oc) == 0, what
        rx, ra = R.unpack_ref(a, oc, want_alpha=True)
        dst.assert_guards(what)
        src.assert_untouched(what + ": src")
        assert np.array_equal(_bits32(dst.data().numpy().reshape(rx.shape)), _bits32(rx)), what
        if al is not None:
            al.assert_guards(what + ": alpha")
            if ra is None:          # no alpha sample in the source: the plane is left alone
                al.assert_untouched(what + ": alpha of a source without one")
            else:
                assert np.array_equal(_bits32(al.data().numpy().reshape(ra.shape)), _bits32(ra)), what + ": alpha"


@pytest.mark.parametrize("ic", [1, 2, 3, 4])
def test_unpack_src_at_every_byte_phase(ic):
    B, H, W = 2, 17, 65
    a = _samples(8, (B, H, W, ic), seed=ic)
    rx, ra = R.unpack_ref(a, 3, want_alpha=True)
    for off in (0, 1, 2, 3):
        src, dst, al = Bytes(a.nbytes, offset=off, fill=a), _out_f32(B * 3 * H * W), _out_f32(B * H * W)
        assert src.ptr % 4 == off
        assert _unpack(src, dst, al, B, H, W, ic, 8, 3) == 0
        dst.assert_guards(f"src + {off}")
        assert np.array_equal(_bits32(dst.data().numpy().reshape(rx.shape)), _bits32(rx)), f"ic{ic} src + {off}"
        if ra is not None:
            assert np.array_equal(_bits32(al.data().numpy().reshape(ra.shape)), _bits32(ra))
    a16 = _samples(16, (B, H, W, ic), seed=ic + 9)
    r16, _ = R.unpack_ref(a16, 1)
    src, dst = Bytes(a16.nbytes, offset=2, fill=a16), _out_f32(B * H * W)
    assert _unpack(src, dst, None, B, H, W, ic, 16, 1) == 0
    dst.assert_guards("16-bit src + 2")
    assert np.array_equal(_bits32(dst.data().numpy().reshape(r16.shape)), _bits32(r16))


def test_unpack_planes_off_16_bytes():
    """P % 4 == 0 but the planes start 4 bytes past a 16-byte boundary: the one-float-per-pixel path."""
    B, H, W = 2, 2, 64
    a = _samples(8, (B, H, W, 4), seed=3)
    rx, ra = R.unpack_ref(a, 3, want_alpha=True)
    src, dst, al = Bytes(a.nbytes, fill=a), _out_f32(B * 3 * H * W + 1), _out_f32(B * H * W + 1)
    assert _unpack(src, dst.ptr + 4, al.ptr + 4, B, H, W, 4, 8, 3) == 0
    dst.assert_guards("dst + 4")
    al.assert_guards("alpha + 4")
    d, q = dst.data().numpy().reshape(-1), al.data().numpy().reshape(-1)
    assert np.isnan(d[0]) and np.isnan(q[0])
    assert np.array_equal(_bits32(d[1:]), _bits32(rx).reshape(-1)) and np.array_equal(_bits32(q[1:]), _bits32(ra).reshape(-1))


def test_unpack_two_runs_equal_bits():
    a = _samples(16, (2, 17, 130, 4), seed=1)
    outs = []
    for _ in range(2):
        src, dst = Bytes(a.nbytes, fill=a), _out_f32(2 * 3 * 17 * 130)
        assert _unpack(src, dst, None, 2, 17, 130, 4, 16, 3) == 0
        outs.append(dst.data().view(torch.int32))
    assert torch.equal(outs[0], outs[1])


def test_unpack_refusals_leave_buffers_untouched():
    a = _samples(16, (1, 4, 6, 2), seed=1)
    src, dst, al = Bytes(a.nbytes + 8, fill=np.concatenate([a.reshape(-1), np.zeros(4, np.uint16)])), _out_f32(3 * 24 + 2), _out_f32(24 + 2)
    ok = dict(B=1, H=4, W=6, ic=2, bits=16, oc=3)
    cases = [(E_SHAPE, dict(B=0)), (E_SHAPE, dict(H=0)), (E_SHAPE, dict(W=-1)), (E_SHAPE, dict(B=65536)), (E_SHAPE, dict(ic=0)), (E_SHAPE, dict(ic=5)),
             (E_SHAPE, dict(bits=12)), (E_SHAPE, dict(oc=2)), (E_SHAPE, dict(oc=4))]
    for code, kw in cases:
        p = {**ok, **kw}
        assert _unpack(src, dst, al, p["B"], p["H"], p["W"], p["ic"], p["bits"], p["oc"]) == code, kw
    assert _unpack(None, dst, al, 1, 4, 6, 2, 16, 3) == E_NULL and _unpack(src, None, al, 1, 4, 6, 2, 16, 3) == E_NULL
    assert _unpack(src.ptr + 1, dst, al, 1, 4, 6, 2, 16, 3) == E_ALIGN          # odd src at 16 bits
    assert _unpack(src, dst.ptr + 2, al, 1, 4, 6, 2, 16, 3) == E_ALIGN and _unpack(src, dst, al.ptr + 1, 1, 4, 6, 2, 16, 3) == E_ALIGN
    assert _unpack(None, dst, al, 0, 4, 6, 2, 16, 3) == E_SHAPE                # the order of the checks: shape before null
    for b, name in ((src, "src"), (dst, "dst"), (al, "alpha")):
        b.assert_untouched(f"refused unpack: {name}")
    from tpu_superresolution_amd._lib import lib
    assert b"image_unpack" in lib().srk_last_error()


# ---- pack ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [8, 16])
@pytest.mark.parametrize("C", [1, 3])
def test_pack_every_shape(C, bits):
    for (B, H, W), oc in itertools.product(SHAPES, (1, 2, 3, 4)):
        what = f"pack B{B} {H}x{W} C{C} oc{oc} {bits}b"
        y = _values((B, C, H, W), bits, seed=H * 977 + W + C)
        a = _values((B, 1, H, W), bits, seed=H * 31 + W + 5)
        yb, ab = _f32(y), _f32(a)
        with_alpha = oc in (2, 4) or (H + W) % 2 == 0          # an alpha pointer that must be ignored at out_chans 1 | 3, every other shape
        dst, cnt = Bytes(B * H * W * oc * (bits // 8)), Counters()
        assert _pack(yb, ab if with_alpha else None, dst, cnt, B, H, W, C, oc, bits) == 0, what
        ref, (nf, cl) = R.pack_ref(y, a if oc in (2, 4) else None, out_chans=oc, bits=bits)
        dst.assert_guards(what)
        cnt.assert_guards(what)
        yb.assert_untouched(what + ": y")
        ab.assert_untouched(what + ": alpha")
        assert np.array_equal(dst.data(DT[bits], ref.shape), ref), what
        assert cnt.values() == [5 + nf, 7 + cl], what
        if (H, W) == (17, 130):          # a second call accumulates; without counters nothing else changes
            assert _pack(yb, ab if with_alpha else None, dst, cnt, B, H, W, C, oc, bits) == 0
            assert cnt.values() == [5 + 2 * nf, 7 + 2 * cl] and nf >= 3 and cl > 0, what
            dst2 = Bytes(dst.n)
            assert _pack(yb, ab if with_alpha else None, dst2, None, B, H, W, C, oc, bits) == 0
            assert torch.equal(dst2.raw, dst.raw), what + ": two runs"
            cnt.assert_guards(what)


@pytest.mark.parametrize("oc", [1, 2, 3, 4])
def test_pack_dst_at_every_byte_phase(oc):
    B, H, W = 2, 17, 65
    y, a = _values((B, 3, H, W), 8, seed=oc), _values((B, 1, H, W), 8, seed=oc + 4)
    ref, counts = R.pack_ref(y, a, out_chans=oc, bits=8)
    yb, ab = _f32(y), _f32(a)
    for off in (0, 1, 2, 3):
        dst, cnt = Bytes(ref.nbytes, offset=off), Counters((0, 0))
        assert dst.ptr % 4 == off
        assert _pack(yb, ab, dst, cnt, B, H, W, 3, oc, 8) == 0
        dst.assert_guards(f"dst + {off}")
        assert np.array_equal(dst.data(np.uint8, ref.shape), ref), f"oc{oc} dst + {off}"
        assert cnt.values() == list(counts)
    y16 = _values((B, 1, H, W), 16, seed=oc + 8)
    r16, _ = R.pack_ref(y16, a, out_chans=oc, bits=16)
    dst = Bytes(r16.nbytes, offset=2)
    assert _pack(_f32(y16), ab, dst, None, B, H, W, 1, oc, 16) == 0
    dst.assert_guards("16-bit dst + 2")
    assert np.array_equal(dst.data(np.uint16, r16.shape), r16)


def test_pack_planes_off_16_bytes():
    B, H, W = 2, 2, 64
    y, a = _values((B, 3, H, W), 8, seed=1), _values((B, 1, H, W), 8, seed=2)
    ref, counts = R.pack_ref(y, a, out_chans=4, bits=8)
    yb = _f32(np.concatenate([[np.float32(np.nan)], y.reshape(-1)]))
    ab = _f32(np.concatenate([[np.float32(np.inf)], a.reshape(-1)]))
    dst, cnt = Bytes(ref.nbytes), Counters((0, 0))
    assert _pack(yb.ptr + 4, ab.ptr + 4, dst, cnt, B, H, W, 3, 4, 8) == 0
    dst.assert_guards("y + 4")
    assert np.array_equal(dst.data(np.uint8, ref.shape), ref) and cnt.values() == list(counts)          # the NaN / Inf in front are not read


def test_pack_specials_and_ties_alone():
    for bits in (8, 16):
        mx = 255 if bits == 8 else 65535
        v, k = R.ties(bits)
        assert len(v) > 0 and (k % 2 == 0).any()
        row = np.concatenate([R.specials(), v]).astype(np.float32)
        dst, cnt = Bytes(row.size * (bits // 8)), Counters((0, 0))
        assert _pack(_f32(row), None, dst, cnt, 1, 1, row.size, 1, 1, bits) == 0
        got = dst.data(DT[bits], (row.size,)).astype(np.int64)
        assert got[:8].tolist() == [0, mx, 0, 0, mx, 0, 0, mx]
        assert np.array_equal(got[8:], np.where(k % 2 == 0, k, k + 1)), f"{bits}-bit ties do not round to even"
        assert cnt.values() == [3, 2]


def test_pack_refusals_leave_buffers_untouched():
    y, a = _values((1, 3, 4, 6), 8, seed=1), _values((1, 1, 4, 6), 8, seed=2)
    yb, ab, dst, cnt = _f32(np.append(y.reshape(-1), 0)), _f32(np.append(a.reshape(-1), 0)), Bytes(4 * 6 * 4 * 2 + 8), Counters()
    ok = dict(B=1, H=4, W=6, C=3, oc=4, bits=16)
    for kw in (dict(B=0), dict(H=0), dict(W=0), dict(B=65536), dict(C=2), dict(C=4), dict(oc=0), dict(oc=5), dict(bits=32)):
        p = {**ok, **kw}
        assert _pack(yb, ab, dst, cnt, p["B"], p["H"], p["W"], p["C"], p["oc"], p["bits"]) == E_SHAPE, kw
    assert _pack(None, ab, dst, cnt, 1, 4, 6, 3, 4, 16) == E_NULL and _pack(yb, ab, None, cnt, 1, 4, 6, 3, 4, 16) == E_NULL
    assert _pack(yb, None, dst, cnt, 1, 4, 6, 3, 4, 16) == E_NULL and _pack(yb, None, dst, cnt, 1, 4, 6, 3, 2, 16) == E_NULL
    assert _pack(yb, ab, dst.ptr + 1, cnt, 1, 4, 6, 3, 4, 16) == E_ALIGN        # odd dst at 16 bits
    assert _pack(yb.ptr + 2, ab, dst, cnt, 1, 4, 6, 3, 4, 16) == E_ALIGN and _pack(yb, ab.ptr + 1, dst, cnt, 1, 4, 6, 3, 4, 16) == E_ALIGN
    assert _pack(yb, ab, dst, cnt.ptr + 2, 1, 4, 6, 3, 4, 16) == E_ALIGN
    assert _pack(None, ab, dst, cnt, 1, 4, 6, 2, 4, 16) == E_SHAPE
    for b, name in ((yb, "y"), (ab, "alpha"), (dst, "dst"), (cnt, "counters")):
        b.assert_untouched(f"refused pack: {name}")


# ---- the ops on the device -------------------------------------------------------------------------------------------------------------
def test_ops_on_the_device_equal_their_cpu_branches():
    from tpu_superresolution_amd import ops
    a = torch.from_numpy(_samples(8, (2, 17, 65, 4), seed=4))
    x, al = ops.image_unpack(a.cuda(), 3, want_alpha=True)
    hx, hal = ops.image_unpack(a, 3, want_alpha=True)
    assert torch.equal(x.cpu().view(torch.int32), hx.view(torch.int32)) and torch.equal(al.cpu().view(torch.int32), hal.view(torch.int32))
    y = torch.from_numpy(_values((2, 3, 17, 65), 16, seed=5))
    for bits in (8, 16):
        c_dev, c_host = torch.zeros(2, dtype=torch.int32, device="cuda"), torch.zeros(2, dtype=torch.int32)
        got = ops.image_pack(y.cuda(), hal.cuda(), bits=bits, counters=c_dev)
        want = ops.image_pack(y, hal, bits=bits, counters=c_host)
        assert got.dtype == want.dtype and torch.equal(got.cpu().view(torch.uint8), want.view(torch.uint8))
        assert c_dev.tolist() == c_host.tolist() and c_host[0] >= 3


def test_both_launches_are_capturable():
    from tpu_superresolution_amd import ops
    a = torch.from_numpy(_samples(8, (1, 17, 65, 3), seed=6)).cuda()
    cnt = torch.zeros(2, dtype=torch.int32, device="cuda")
    want = ops.image_pack(ops.image_unpack(a, 3)[0], counters=cnt)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        got = ops.image_pack(ops.image_unpack(a, 3)[0], counters=cnt)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(got, want) and torch.equal(got, a)          # k / 255 quantises back to k
