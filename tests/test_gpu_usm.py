"""srk_usm_sharpen_f32 (csrc/usm.hip) through the C ABI on guarded buffers: NaN guard rows around the input, a NaN pattern
around out and work that must keep its bits.

Exact (torch.equal): ks 1, a constant image and threshold 1e9 give x; a second launch gives the same bits; a sample alone is the sample
in the batch; the interior of usm(img[window grown by 2R]) is the same window of usm(img).
Bounded: out lies in the hull that tests/usm_ref.py derives from the fp64 reference (decided mask pixels are the reference's, the
undecided ones widen soft's interval); nothing here is tuned.  The largest measured |out - ref| / E_out is printed."""
import numpy as np
import pytest
import torch

import usm_ref as Ur
from guarded import Guarded

pytestmark = pytest.mark.gpu

E_SHAPE, E_NULL, E_UNSUPPORTED = -1, -2, -3


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _lib():
    from tpu_superresolution_amd._lib import lib
    return lib()


def _ptr(t):
    return t if isinstance(t, int) or t is None else t.data_ptr()


def _usm_raw(x, taps, out, work, B, C, H, W, ks, weight=0.5, threshold=10.0):
    return _lib().srk_usm_sharpen_f32(_ptr(x), _ptr(taps), _ptr(out), _ptr(work), B, C, H, W, ks, weight, threshold, _stream())


def run(x_np, taps_np, weight=0.5, threshold=10.0):
    """x [B][C][H][W] numpy -> out as a CPU tensor; every guard checked."""
    B, C, H, W = x_np.shape
    n = B * C * H * W
    xin = Guarded("f32", 1, n, n, fill=torch.from_numpy(x_np).reshape(1, n))
    tp = Guarded("f32", 1, len(taps_np), len(taps_np), fill=torch.from_numpy(taps_np).reshape(1, -1))
    out, work = Guarded("f32", 1, n, n), Guarded("f32", 1, n, n)
    assert _usm_raw(xin.ptr, tp.ptr, out.ptr, work.ptr, B, C, H, W, len(taps_np), weight, threshold) == 0
    torch.cuda.synchronize()
    out.assert_guards("usm out")
    work.assert_guards("usm work")
    xin.assert_untouched("usm x")
    tp.assert_untouched("usm taps")
    got = out.data().view(B, C, H, W)
    assert bool(torch.isfinite(got).all()), "a NaN guard was read"
    return got


_REF = {}


def ref(seed, C, shape, ks, weight=0.5, threshold=10.0):
    key = (seed, C, shape, ks, weight, threshold)
    if key not in _REF:
        x = Ur.image(seed, shape, channels=C, batch=2)
        taps = Ur.gaussian1d(ks)
        _REF[key] = (x, taps, Ur.intervals(x, taps, weight, threshold))
    return _REF[key]


@pytest.mark.parametrize("C", [3, 1])
@pytest.mark.parametrize("shape", Ur.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("ks", [51, 3])
def test_usm_within_derived_hull(ks, shape, C):
    for thr in (10.0, -1.0):          # -1: the mask is all 1, an ordinary bounded case
        x, taps, iv = ref(7 + C, C, shape, ks, 0.5, thr)
        got = run(x, taps, 0.5, thr).numpy().astype(np.float64)
        if thr < 0:
            assert iv["ref"]["mask"].min() == 1.0
        lo, hi = iv["lo"], iv["hi"]
        bad = (got < lo) | (got > hi)
        dec = ~iv["undecided"]
        frac = np.max(np.abs(got - iv["ref"]["out"])[dec] / np.maximum(iv["e_out"], 1e-300)[dec])
        print(f"usm ks={ks} {shape} C={C} thr={thr}: undecided {int(iv['undecided'].sum())} of {got.size}, max |out - ref| / E_out = {frac:.3f}")
        assert not bad.any(), f"{int(bad.sum())} pixels outside the derived hull, worst by {np.max(np.maximum(lo - got, got - hi)):.3e}"
        assert dec.any()


@pytest.mark.parametrize("C", [3, 1])
def test_usm_exact_cases(C):
    shape = (33, 50)
    x = Ur.image(21 + C, shape, channels=C, batch=2)
    xt = torch.from_numpy(x)
    assert torch.equal(run(x, np.ones(1, dtype=np.float32)), xt), "ks 1 must give x"
    for ks in (51, 3):
        taps = Ur.gaussian1d(ks)
        assert torch.equal(run(x, taps, 0.5, 1e9), xt), "threshold 1e9 must give x"
        const = np.full_like(x, np.float32(77.0 / 255.0))
        assert torch.equal(run(const, taps), torch.from_numpy(const)), "a constant image must give x"
        a, b = run(x, taps), run(x, taps)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "a second launch differs"
        for s in range(2):
            assert torch.equal(run(x[s:s + 1], taps)[0], a[s]), f"sample {s} alone differs from the sample in the batch"


@pytest.mark.parametrize("ks,grow", [(51, 50), (3, 2)])
def test_usm_window_interior_is_the_whole_image(ks, grow):
    """The data-path rule: a patch is a window of the whole-window sharpening, whatever the tile position."""
    taps = Ur.gaussian1d(ks)
    img = Ur.image(5, (150, 180), channels=3, batch=1)
    whole = run(img, taps)
    for (y, x, h, w) in ((53, 61, 40, 37), (50, 64, 33, 66)):
        win = np.ascontiguousarray(img[:, :, y - grow:y + h + grow, x - grow:x + w + grow])
        got = run(win, taps)[:, :, grow:grow + h, grow:grow + w]
        assert torch.equal(got, whole[:, :, y:y + h, x:x + w])


def test_usm_through_ops_and_refusals():
    from tpu_superresolution_amd import _lib as L
    from tpu_superresolution_amd import ops
    x = Ur.image(3, (40, 72), channels=3, batch=2)
    xc = torch.from_numpy(x).cuda()
    assert torch.equal(ops.usm_sharpen(xc).cpu(), run(x, Ur.gaussian1d(51)))
    assert torch.equal(ops.usm_sharpen(xc, radius=3, weight=0.8, threshold=4.0).cpu(), run(x, Ur.gaussian1d(3), 0.8, 4.0))
    assert ops.usm_taps(51, 8.0, xc.device) is ops.usm_taps(51, 8.0, xc.device)
    with pytest.raises(L.SrkUnsupported):
        ops.usm_sharpen(xc[:, :, :25])
    with pytest.raises(ValueError):
        ops.usm_sharpen(xc[:, :2])
    taps = torch.from_numpy(Ur.gaussian1d(51)).cuda()
    out, work = torch.empty_like(xc), torch.empty_like(xc)
    B, C, H, W = xc.shape
    for args in ((None, taps, out, work), (xc, None, out, work), (xc, taps, None, work), (xc, taps, out, None)):
        assert _usm_raw(*args, B, C, H, W, 51) == E_NULL
    for (b, c, h, w, ks) in ((0, C, H, W, 51), (B, 2, H, W, 51), (B, C, 0, W, 51), (B, C, H, 0, 51), (B, C, H, W, 50), (B, C, H, W, 53),
                             (B, C, H, W, 0), (B, C, H, W, -1)):
        assert _usm_raw(xc, taps, out, work, b, c, h, w, ks) == E_SHAPE
    assert _usm_raw(xc, taps, xc, work, B, C, H, W, 51) == E_SHAPE
    assert _usm_raw(xc, taps, out, out, B, C, H, W, 51) == E_SHAPE
    assert _usm_raw(xc, taps, out, xc, B, C, H, W, 51) == E_SHAPE
    assert _usm_raw(xc, taps, out, work, B, C, 25, W, 51) == E_UNSUPPORTED
    assert _usm_raw(xc, taps, out, work, B, C, H, 25, 51) == E_UNSUPPORTED
    assert _usm_raw(xc, taps, out, work, B, C, 26, 26, 51) == 0
    torch.cuda.synchronize()
