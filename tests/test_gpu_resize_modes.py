"""srk_resize_ragged_mode_f32 (csrc/resize_modes.hip) through the C ABI on guarded buffers: the ragged family of DESIGN 7p
(B 4, padded 40 x 72, NaN input padding, a NaN pattern in the output padding that must keep its bits) with a resize rule per sample.

Exact (torch.equal): a mode-0 sample and mode == NULL against srk_resize_aa_ragged_f32; dyadic factors on integer levels against the
reference; the bilinear identity; a mode word of 7 against mode 2; each sample against the dense call on it alone.
Bounded: 2 (n_x + n_y + 2) u S (tests/resize_modes_ref.py); quantised levels equal the reference's where it decides them."""
import numpy as np
import pytest
import torch

import filter2d_ref as Fr
import resize_modes_ref as Mr
from guarded import Guarded

pytestmark = pytest.mark.gpu

E_SHAPE, E_NULL, E_UNSUPPORTED = -1, -2, -3
PAT = 0x7FC0BEEF
EXT = Fr.RAGGED_EXT
HP, WP = Fr.RAGGED_PAD
TARGETS = {
    "up": [(60, 108), (50, 75), (24, 22), (23, 96)],
    "down": [(20, 36), (11, 17), (4, 5), (12, 8)],
    "identity": list(EXT),
    "noninteger": [(29, 47), (40, 41), (7, 13), (31, 50)],
}
MODES = ([0, 1, 2, 1], [2, 2, 0, 1])


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _lib():
    from tpu_superresolution_amd._lib import lib
    return lib()


def _ptr(t):
    return t if isinstance(t, int) or t is None else t.data_ptr()


def _i32(v):
    return None if v is None else torch.tensor(v, dtype=torch.int32).cuda()


def _mode(x, ei, out, eo, mode, B, C, Hp, Wp, Hop, Wop, q=0):
    return _lib().srk_resize_ragged_mode_f32(_ptr(x), _ptr(ei), _ptr(out), _ptr(eo), _ptr(mode), B, C, Hp, Wp, Hop, Wop, q, _stream())


def _aa(x, ei, out, eo, B, C, Hp, Wp, Hop, Wop, q=0):
    return _lib().srk_resize_aa_ragged_f32(_ptr(x), _ptr(ei), _ptr(out), _ptr(eo), B, C, Hp, Wp, Hop, Wop, q, _stream())


def _bits(t):
    return t.contiguous().view(torch.int32)


class Out:
    """A guarded padded output [B][C][Hp][Wp] prefilled with a NaN pattern."""

    def __init__(self, B, C, Hp, Wp):
        self.g = Guarded("f32", 1, B * C * Hp * Wp, B * C * Hp * Wp)
        self.t = self.g.win.view(B, C, Hp, Wp)
        self.ptr = self.g.ptr

    def check(self, ext, what):
        torch.cuda.synchronize()
        self.g.assert_guards(what)
        B, _, Hp, Wp = self.t.shape
        outs = []
        for b in range(B):
            h, w = (Hp, Wp) if ext is None else ext[b]
            pad = torch.ones(Hp, Wp, dtype=torch.bool, device="cuda")
            pad[:h, :w] = False
            assert bool((_bits(self.t[b])[:, pad] == PAT).all()), f"{what}: the output padding of sample {b} was written"
            assert bool(torch.isfinite(self.t[b, :, :h, :w]).all()), f"{what}: sample {b} read the NaN padding of the input"
            outs.append(self.t[b, :, :h, :w].clone())
        return outs


def ragged(x, ei, eo, modes, C, q=0, pad=None):
    Hop, Wop = pad or (max(h for h, _ in eo), max(w for _, w in eo))
    out = Out(len(eo), C, Hop, Wop)
    assert _mode(x, _i32(ei), out.ptr, _i32(eo), _i32(modes), len(eo), C, x.shape[2], x.shape[3], Hop, Wop, q) == 0
    return out.check(eo, f"resize_ragged_mode {modes}")


@pytest.mark.parametrize("C", [3, 1])
@pytest.mark.parametrize("case", list(TARGETS))
def test_modes_on_the_ragged_family(case, C):
    buf, samples = Fr.ragged_batch(31 + C, C, lo=0.0, hi=1.0)
    x = torch.from_numpy(buf).cuda()
    eo = TARGETS[case]
    Hop, Wop = max(h for h, _ in eo), max(w for _, w in eo)
    B = len(EXT)
    aa = Out(B, C, Hop, Wop)
    assert _aa(x, _i32(EXT), aa.ptr, _i32(eo), B, C, HP, WP, Hop, Wop) == 0
    cubic = aa.check(eo, "resize_aa_ragged")
    for modes in MODES:
        got = ragged(x, EXT, eo, modes, C)
        got8 = ragged(x, EXT, eo, modes, C, q=8)
        for b, s in enumerate(samples):
            m, (ho, wo) = modes[b], eo[b]
            if m == 0:
                assert torch.equal(got[b], cubic[b]), f"{case}: the mode-0 sample {b} differs from srk_resize_aa_ragged_f32"
                continue
            # the sample against the dense call on it alone
            alone = Out(1, C, ho, wo)
            assert _mode(torch.from_numpy(s[None]).cuda(), None, alone.ptr, None, _i32([m]), 1, C, s.shape[1], s.shape[2], ho, wo) == 0
            assert torch.equal(alone.check(None, "dense")[0], got[b]), f"{case}: sample {b} differs from the dense call on it alone"
            want, bnd = Mr.resize(s, ho, wo, m), Mr.bound(s, ho, wo, m)
            err = np.abs(got[b].cpu().numpy().astype(np.float64) - want)
            print(f"{case} C={C} sample {b} mode {m}: max err / bound = {np.max(err / np.maximum(bnd, 1e-300)):.3f}")
            assert (err <= bnd).all(), f"{case}: sample {b} mode {m} misses 2 (nx + ny + 2) u S by {np.max(err - bnd):.3e}"
            if case == "identity" and m == 1:
                assert torch.equal(got[b].cpu(), torch.from_numpy(s)), "the bilinear identity must copy finite inputs"
            lv, und = Fr.quant8(want)[1], Fr.near_half(want, bnd)
            got_lv = np.rint(got8[b].cpu().numpy().astype(np.float64) * 255.0)
            assert (got_lv[~und] == lv[~und]).all(), f"{case}: sample {b} mode {m}: a decided level differs"
            assert np.array_equal(got8[b].cpu().numpy(), (got_lv.astype(np.float32) / np.float32(255)))


def test_null_mode_and_clamped_words():
    buf, _ = Fr.ragged_batch(9, 3, lo=0.0, hi=1.0)
    x = torch.from_numpy(buf).cuda()
    eo = TARGETS["noninteger"]
    Hop, Wop = 40, 50
    aa = Out(4, 3, Hop, Wop)
    assert _aa(x, _i32(EXT), aa.ptr, _i32(eo), 4, 3, HP, WP, Hop, Wop, 8) == 0
    cubic = aa.check(eo, "aa")
    for got in (ragged(x, EXT, eo, None, 3, q=8), ragged(x, EXT, eo, [0, 0, 0, 0], 3, q=8), ragged(x, EXT, eo, [-5, 0, -2 ** 31, 0], 3, q=8)):
        for a, b in zip(got, cubic):
            assert torch.equal(a, b)
    for a, b in zip(ragged(x, EXT, eo, [7, 2 ** 31 - 1, 3, 2], 3), ragged(x, EXT, eo, [2, 2, 2, 2], 3)):
        assert torch.equal(a, b), "a mode word above 2 must count as 2"
    again = ragged(x, EXT, eo, [1, 2, 1, 2], 3)
    for a, b in zip(again, ragged(x, EXT, eo, [1, 2, 1, 2], 3)):
        assert torch.equal(_bits(a), _bits(b)), "a second launch differs"


@pytest.mark.parametrize("C", [3, 1])
def test_dyadic_factors_are_exact(C):
    x = Mr.levels(4 + C, (2, C, 40, 72))
    xc = torch.from_numpy(x).cuda()
    for mode, (ho, wo) in ((Mr.AREA, (20, 36)), (Mr.AREA, (10, 18)), (Mr.BILINEAR, (80, 144))):
        out = Out(2, C, ho, wo)
        assert _mode(xc, None, out.ptr, None, _i32([mode, mode]), 2, C, 40, 72, ho, wo) == 0
        got = torch.stack(out.check(None, "dyadic")).cpu()
        want = torch.from_numpy(Mr.resize(x, ho, wo, mode).astype(np.float32))
        assert torch.equal(got, want), f"mode {mode} to {(ho, wo)}: dyadic weights on integer levels must be exact"


def test_through_ops_and_refusals():
    from tpu_superresolution_amd import _lib as L
    from tpu_superresolution_amd import ops
    buf, _ = Fr.ragged_batch(13, 3, lo=0.0, hi=1.0)
    x = torch.from_numpy(buf).cuda()
    eo = TARGETS["down"]
    got = ragged(x, EXT, eo, [0, 1, 2, 1], 3, q=8)
    for pad in (None, (25, 40)):
        via = ops.resize_ragged(x, EXT, eo, [0, 1, 2, 1], pad, 8)
        for b, (ho, wo) in enumerate(eo):
            assert torch.equal(via[b, :, :ho, :wo], got[b])
    for modes in (None, [0, 0, 0, 0]):
        assert torch.equal(_bits(ops.resize_ragged(x, EXT, eo, modes, (20, 36), 8, out=torch.zeros(4, 3, 20, 36, device="cuda"))),
                           _bits(ops.resize_aa_ragged(x, EXT, eo, (20, 36), 8, out=torch.zeros(4, 3, 20, 36, device="cuda"))))
    with pytest.raises(ValueError):
        ops.resize_ragged(x, EXT, eo, [0, 1, 3, 0])
    with pytest.raises(ValueError):
        ops.resize_ragged(x, EXT, eo, [0, 1])
    with pytest.raises(L.SrkUnsupported):
        ops.resize_ragged(x, EXT, [(4, 9), (11, 17), (4, 5), (12, 8)], [2, 2, 2, 2])          # 40 rows -> 4
    d = torch.rand(2, 3, 37, 70, device="cuda")
    out = torch.empty(2, 3, 19, 35, device="cuda")
    m = _i32([1, 2])
    assert _mode(None, None, out, None, m, 2, 3, 37, 70, 19, 35) == E_NULL
    assert _mode(d, None, None, None, m, 2, 3, 37, 70, 19, 35) == E_NULL
    for shp in ((0, 3, 37, 70, 19, 35), (2, 0, 37, 70, 19, 35), (2, 3, 0, 70, 19, 35), (2, 3, 37, 0, 19, 35), (2, 3, 37, 70, 0, 35),
                (2, 3, 37, 70, 19, -1)):
        assert _mode(d, None, out, None, m, *shp) == E_SHAPE
    assert _mode(d, None, out, None, m, 2, 3, 37, 70, 19, 35, 4) == E_SHAPE
    assert _mode(d, None, d, None, m, 2, 3, 37, 70, 19, 35) == E_SHAPE
    big = torch.zeros(4096, dtype=torch.int32, device="cuda")
    assert _mode(d, None, big.view(torch.float32), None, big, 2, 1, 37, 70, 19, 35) == E_SHAPE          # out overlaps mode
    assert _mode(d, None, out, None, m, 2, 3, 37, 70, 4, 35) == E_UNSUPPORTED
    assert _mode(d, None, out, None, m, 2, 3, 37, 70, 19, 8) == E_UNSUPPORTED
    torch.cuda.synchronize()
