"""fp64 restatement of srk_filter2d_f32 (include/srk.h "Ragged batches"; csrc/filter2d.hip), pinned in tests/test_filter2d_ref.py:

    out(p, q) = sum_a sum_b K[a][b] x(rho(p + a - R, h), rho(q + b - R, w)),   rho = reflect-101, R = (ks - 1) / 2

a correlation (no flip), `a` the row index of the table, no mass and no division.

Tolerance of the fp32 kernel against this (derived, not tuned): the kernel runs ONE chain of n = ks^2 fused multiply-adds from 0, each
rounding once, so by the standard bound for recursive summation |err| <= gamma_n S with S = sum |K| |x| over the window and
gamma_n = n u / (1 - n u), u = 2^-24.  n u <= 441 * 2^-24 < 3e-5, so gamma_n < 2 n u with room for the reference's own fp64 rounding:
`bound` returns 2 n u S, n counted BEFORE any zero-padding of the table (a zero tap adds no rounding: fmaf(0, x, acc) == acc).

Quantised outputs (quant_bits 8): level = rint(clamp(v, 0, 1) * 255).  The kernel's level is the reference's wherever the reference is
further than the bound from a half-integer (`near_half` marks the rest, which may differ by one level).  How many pixels of an image
are undecided is a property of the inputs; the dim images below (levels 0..31) keep it under 1 % for sinc tables."""
import numpy as np

U = 2.0 ** -24


def rho(i, n):
    i = np.asarray(i)
    r = np.where(i < 0, -i, np.where(i >= n, 2 * (n - 1) - i, i))
    return np.clip(r, 0, n - 1)


def _window_sum(x, K, border, absolute=False):
    """sum_a sum_b K[a][b] x(p + a - R, q + b - R) for a plane x [H][W] in fp64 with the given border; with `absolute` the sum of
    magnitudes.  Also returns the in-image mass of each pixel (the sum of the taps that fall inside the plane)."""
    x = np.asarray(x, dtype=np.float64)
    K = np.asarray(K, dtype=np.float64)
    ks = K.shape[0]
    R = ks // 2
    H, W = x.shape
    yy = np.arange(-R, H + R)
    xx = np.arange(-R, W + R)
    inside = ((yy >= 0) & (yy < H))[:, None] & ((xx >= 0) & (xx < W))[None, :]
    if border == "reflect":
        xp = x[rho(yy, H)][:, rho(xx, W)]
    elif border == "replicate":
        xp = x[np.clip(yy, 0, H - 1)][:, np.clip(xx, 0, W - 1)]
    elif border in ("zero", "mass"):
        xp = np.where(inside, x[np.clip(yy, 0, H - 1)][:, np.clip(xx, 0, W - 1)], 0.0)
    else:
        raise ValueError(border)
    if absolute:
        xp, K = np.abs(xp), np.abs(K)
    acc = np.zeros((H, W))
    mass = np.zeros((H, W))
    for a in range(ks):
        for b in range(ks):
            acc += K[a, b] * xp[a:a + H, b:b + W]
            mass += K[a, b] * inside[a:a + H, b:b + W]
    return acc, mass


def filter2d(x, K, border="reflect", flip=False, transpose=False):
    """The reference: x [H][W] or [C][H][W] -> fp64 of the same shape.  The other arguments are the NEGATIVE CONTROLS of
    tests/test_filter2d_ref.py -- what the kernel must not compute: border 'zero' / 'replicate' / 'mass' (srk_blur2d_f32's rule: taps
    outside dropped, the rest divided by their mass), flip = a convolution, transpose = `b` as the row index of the table."""
    x = np.asarray(x, dtype=np.float64)
    if x.ndim == 3:
        return np.stack([filter2d(p, K, border, flip, transpose) for p in x])
    K = np.asarray(K, dtype=np.float64)
    if flip:
        K = K[::-1, ::-1]
    if transpose:
        K = K.T
    acc, mass = _window_sum(x, K, border)
    return acc / mass if border == "mass" else acc


def bound(x, K, n=None):
    """2 n u S per pixel (the docstring above); n defaults to the table's own ks^2."""
    x = np.asarray(x, dtype=np.float64)
    if x.ndim == 3:
        return np.stack([bound(p, K, n) for p in x])
    K = np.asarray(K, dtype=np.float64)
    n = K.size if n is None else n
    S, _ = _window_sum(x, K, "reflect", absolute=True)
    return 2.0 * n * U * S + 1e-300


def quant8(v):
    """-> (k / 255.0f as fp32, k) of rint(clamp(v, 0, 1) * 255)."""
    lv = np.rint(np.clip(np.asarray(v, dtype=np.float64), 0.0, 1.0) * 255.0)
    return (lv.astype(np.float32) / np.float32(255)).astype(np.float32), lv


def near_half(ref, bnd):
    """Pixels whose level the reference alone does not decide: within the bound (in levels, plus the kernel's own rounding of the
    product by 255) of a half-integer, inside or at the ends of [0, 255]."""
    t = np.asarray(ref, dtype=np.float64) * 255.0
    tol = np.asarray(bnd, dtype=np.float64) * 255.0 + 4.0 * U * np.maximum(np.abs(t), 1.0)
    d = np.abs(t - np.floor(t) - 0.5)
    return (d <= tol) & (t > -1.0) & (t < 256.0)


def pad_to(K, ks):
    K = np.asarray(K, dtype=np.float32)
    return np.pad(K, (ks - K.shape[0]) // 2)


def delta(ks):
    K = np.zeros((ks, ks), dtype=np.float32)
    K[ks // 2, ks // 2] = 1.0
    return K


def int_table(rng, ks):
    """Integer taps in -3..3 (asymmetric with probability ~1): exact in fp32 on integer images."""
    return rng.randint(-3, 4, size=(ks, ks)).astype(np.float32)


def dim_image(seed, shape=(45, 61), channels=None):
    """Levels 0..31 (the dim images of the PSF tests): integers / 255 as fp32."""
    rng = np.random.RandomState(seed)
    shp = shape if channels is None else (channels,) + tuple(shape)
    return (rng.randint(0, 32, size=shp).astype(np.float32) / np.float32(255)).astype(np.float32)


# ---- the ragged batch of the GPU tests -------------------------------------------------------------------------------------------------
RAGGED_PAD = (40, 72)
RAGGED_EXT = [(40, 72), (33, 50), (12, 11), (23, 64)]


def ragged_batch(seed, C, pad=RAGGED_PAD, ext=RAGGED_EXT, lo=-0.25, hi=1.25):
    """(padded fp32 [B][C][Hp][Wp] with NaN outside every sample's extents, the list of the samples [C][h][w])."""
    rng = np.random.RandomState(seed)
    buf = np.full((len(ext), C) + tuple(pad), np.nan, dtype=np.float32)
    samples = []
    for b, (h, w) in enumerate(ext):
        s = (rng.rand(C, h, w) * (hi - lo) + lo).astype(np.float32)
        buf[b, :, :h, :w] = s
        samples.append(s)
    return buf, samples


# ---- the clamped window of DeviceHR2Pool -----------------------------------------------------------------------------------------------
def window_origin(top, left, Hr, Wr, s, P, m):
    """The E x E window, E = s (P + 2 m), of an HR patch at (top, left) (multiples of s) in a region Hr x Wr: cut at the patch origin
    minus s m and clamped into the region.  -> (wtop, wleft, oy, ox): the window's origin and the LR offset of the patch inside it."""
    E = s * (P + 2 * m)
    wt = min(max(top - s * m, 0), Hr - E)
    wl = min(max(left - s * m, 0), Wr - E)
    return wt, wl, (top - wt) // s, (left - wl) // s
