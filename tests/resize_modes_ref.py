"""fp64 restatement of the resize rules of srk_resize_ragged_mode_f32 (include/srk.h; csrc/resize_modes.hip): mode 0 is
tests/resize_ref.py, modes 1 (bilinear, not antialiased) and 2 (area) are the tables below.  The table arithmetic is fp64 and the
weights are rounded once to fp32, as the kernel rounds them; the passes (horizontal first, then vertical) are fp64.

The bound, derived as tests/resize_ref.py derives its own: an n-term fmaf chain errs by n u sum |w| |x|, the vertical pass runs over
the results of the horizontal one, each weight carries one rounding of its own (here it is IN the reference), and the 2 of the project's
2 n u S covers the higher orders: 2 (n_x + n_y + 2) u S, S = sum |w_y| |w_x| |x| over the output's footprint."""
import numpy as np

import resize_ref as Rr

U = 2.0 ** -24
BILINEAR, AREA = 1, 2


def tables(mode, n_in, n_out, align_corners=False, antialias=False, rounded_area=False):
    """-> (lo, hi, [fp64 arrays of the fp32 weights]).  The keyword arguments are the NEGATIVE CONTROLS of tests/test_resize_modes_ref.py."""
    if mode == 0:
        lo, hi, ws = Rr.tables(n_in, n_out)
        return lo, hi, [w.astype(np.float32).astype(np.float64) for w in ws]
    los, his, ws = [], [], []
    for i in range(n_out):
        if mode == BILINEAR and antialias:          # the triangle widened by the scale (F.interpolate(antialias=True))
            scale = n_in / n_out
            m = max(scale, 1.0)
            c = scale * (i + 0.5)
            lo, hi = max(int(c - m + 0.5), 0), min(int(c + m + 0.5), n_in)
            w = np.maximum(0.0, 1.0 - np.abs((np.arange(hi - lo) + lo - c + 0.5) / m))
            w = w / w.sum()
        elif mode == BILINEAR:
            if align_corners:
                src = i * ((n_in - 1) / (n_out - 1)) if n_out > 1 else 0.0
            else:
                src = max((n_in / n_out) * (i + 0.5) - 0.5, 0.0)
            i0 = min(int(np.floor(src)), n_in - 1)
            l = src - i0
            lo, hi = i0, min(i0 + 1, n_in - 1) + 1
            w = np.array([1.0]) if hi - lo == 1 else np.array([1.0 - l, l])
        else:
            if rounded_area:
                lo, hi = int(round(i * n_in / n_out)), max(int(round((i + 1) * n_in / n_out)), int(round(i * n_in / n_out)) + 1)
                hi = min(hi, n_in)
                lo = min(lo, hi - 1)
            else:
                lo, hi = (i * n_in) // n_out, ((i + 1) * n_in + n_out - 1) // n_out
            w = np.full(hi - lo, 1.0 / (hi - lo))
        los.append(lo)
        his.append(hi)
        ws.append(w.astype(np.float32).astype(np.float64))
    return np.array(los), np.array(his), ws


def resize(x, Ho, Wo, mode, vertical_first=False, **kw):
    """x [..., H, W] -> fp64 [..., Ho, Wo]."""
    x = np.asarray(x, dtype=np.float64)
    tx, ty = tables(mode, x.shape[-1], Wo, **kw), tables(mode, x.shape[-2], Ho, **kw)
    if vertical_first:
        mid = np.swapaxes(Rr._pass(np.swapaxes(x, -1, -2), *ty), -1, -2)
        return Rr._pass(mid, *tx)
    mid = Rr._pass(x, *tx)
    return np.swapaxes(Rr._pass(np.swapaxes(mid, -1, -2), *ty), -1, -2)


def _pass32(x, lo, hi, ws):
    """One pass along the last axis as the kernel's chain: acc = fmaf(w_j, x_j, acc) from 0 in fp32, emulated in fp64 (the product of
    two fp32 numbers is exact there; the sum is rounded to fp64 and then to fp32, which can differ from one rounding only in a tie)."""
    out = []
    for i in range(len(ws)):
        acc = np.zeros(x.shape[:-1], dtype=np.float32)
        for j, w in enumerate(ws[i]):
            acc = (w * x[..., lo[i] + j].astype(np.float64) + acc.astype(np.float64)).astype(np.float32)
        out.append(acc)
    return np.stack(out, axis=-1)


def resize_f32(x, Ho, Wo, mode, vertical_first=False):
    """The kernel's own arithmetic, emulated: what shows that the ORDER of the passes is part of the contract (in exact arithmetic the
    two orders agree)."""
    x = np.asarray(x, dtype=np.float32)
    tx, ty = tables(mode, x.shape[-1], Wo), tables(mode, x.shape[-2], Ho)
    if vertical_first:
        return _pass32(np.swapaxes(_pass32(np.swapaxes(x, -1, -2), *ty), -1, -2), *tx)
    return np.swapaxes(_pass32(np.swapaxes(_pass32(x, *tx), -1, -2), *ty), -1, -2)


def bound(x, Ho, Wo, mode):
    """2 (n_x + n_y + 2) u S per output pixel."""
    x = np.abs(np.asarray(x, dtype=np.float64))
    lox, hix, wx = tables(mode, x.shape[-1], Wo)
    loy, hiy, wy = tables(mode, x.shape[-2], Ho)
    nx, ny = max(len(w) for w in wx), max(len(w) for w in wy)
    mid = Rr._pass(x, lox, hix, [np.abs(w) for w in wx])
    S = np.swapaxes(Rr._pass(np.swapaxes(mid, -1, -2), loy, hiy, [np.abs(w) for w in wy]), -1, -2)
    return 2.0 * (nx + ny + 2) * U * S


def levels(seed, shape, top=32):
    """Integer levels 0..top-1 as fp32 (NOT divided by 255): with dyadic weights every summation order gives the same bits."""
    return np.random.RandomState(seed).randint(0, top, size=shape).astype(np.float32)
