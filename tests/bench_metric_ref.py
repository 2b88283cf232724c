"""fp64 restatement of the benchmark-protocol PSNR / SSIM (include/srk.h "Benchmark-protocol PSNR / SSIM"), written
independently of the device path, and the error bounds the fp32 forms are held to.

The definition: both images clamped to [0, 1] and rounded to 8 bits (one fp32 multiply by 255, round-half-to-even), `border`
pixels cropped on every side, mode 'y': the BT.601 luma 16 + (65.481 R + 128.553 G + 24.966 B) / 255 of RGB levels (a single-channel
image is its own luma), mode 'rgb': every channel; PSNR = 10 log10(255^2 / mse) per image (+inf for mse 0); SSIM = Wang et al. 2004,
11-tap Gaussian sigma 1.5, VALID, K = (0.01, 0.03), data_range 255, mean over channels.  The SSIM is restated from the published
algorithm; parity with the third-party test scripts is unpinned.

What is taken exactly: the quantised integers.  q = rint(fp32(c * 255)) is formed from the fp32 product, as the definition says --
the product is part of the definition, not an error of it -- and everything after it is fp64 from the decimal constants.

Bounds (u = 2^-24, the unit round-off of fp32; nothing here was tuned against the code under test):
  plane, mode y   |Y32 - Y64| <= PLANE_ROUNDINGS * u * 256.  Every intermediate, brought to the scale of Y, is below 256: the three
                  partial sums t are at most 219 * 255 and enter Y divided by 255.  Roundings that can each move Y by u * 256 at the
                  most: the product 65.481 qR (1), the two fmaf (2), the division (1), the add of 16 (1) = 5, and the roundings of
                  the three constants to fp32 (3; each is relative u on a term of at most 128.553 * 255 / 255) = 8.
  plane, mode rgb 0: small integers, exact in fp32.
  sums            |S32 - S64| <= 2 M u S for a sum of M non-negative terms in ANY order (each term d * d + acc is one rounding in
                  the fmaf form; M - 1 further additions; 2 M u covers both with room for the second-order terms), plus, in mode y,
                  what the plane error e does to the terms: |(d + 2e)^2 - d^2| summed is at most 4 e sqrt(M S) + 4 e^2 M (Cauchy-Schwarz).
  PSNR            d/dS of 10 log10(255^2 M / S) is (10 / ln 10) / S, so the sum's bound delta moves it by (10 / ln 10) delta / S; the
                  divisions by M and into 255^2 and the conversion of M to fp32 add 3 u to delta / S; log10f is taken at 2 ulp of its
                  result (the accuracy the device math library documents for it) and the product with 10 adds one rounding:
                  5 u |PSNR|.
  SSIM            tests/test_gpu_metrics.py holds srk_ssim to 2e-5 absolute against the torch-operator form, at data_range 1 and
                  at data_range 255 alike (the index has no unit), on noise-like images; the same figure is used here for such images.
"""
import numpy as np

U = 2.0 ** -24
PLANE_ROUNDINGS = 8
PLANE_BOUND_Y = PLANE_ROUNDINGS * U * 256.0
SSIM_BOUND = 2e-5
BT601 = (65.481, 128.553, 24.966)
LOG10_ULPS = 2


def quantise(x):
    """fp32 array -> the 8-bit levels as fp64 integers; a NaN stays a NaN."""
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        c = np.where(x < 0, np.float32(0), np.where(x > 1, np.float32(1), x)).astype(np.float32)
    return np.rint(c * np.float32(255.0)).astype(np.float64)


def planes(x, border, mode, coef=BT601, offset=16.0):
    """fp32 [B, C, H, W] -> fp64 [B, Cm, Hc, Wc]."""
    q = quantise(x)
    B, C, H, W = q.shape
    assert mode in ("y", "rgb") and 0 <= 2 * border < min(H, W)
    q = q[:, :, border:H - border, border:W - border]
    if mode == "rgb" or C == 1:
        return q
    assert C == 3
    return (offset + (coef[0] * q[:, 0] + coef[1] * q[:, 1] + coef[2] * q[:, 2]) / 255.0)[:, None]


def sqsum(pp, pt):
    return ((pp - pt) ** 2).reshape(pp.shape[0], -1).sum(1)


def psnr_from_sqsum(s, count, max_val=255.0):
    with np.errstate(divide="ignore"):
        return np.where(s == 0, np.inf, 10.0 * np.log10(max_val * max_val * count / np.where(s == 0, 1.0, s)))


def gaussian(size=11, sigma=1.5):
    g = np.exp(-((np.arange(size, dtype=np.float64) - size // 2) ** 2) / (2.0 * sigma * sigma))
    return g / g.sum()


def _valid_blur(a, g):
    k = g.size
    H, W = a.shape[-2:]
    v = sum(g[i] * a[..., i:H - k + 1 + i, :] for i in range(k))
    return sum(g[i] * v[..., :, i:W - k + 1 + i] for i in range(k))


def ssim(pp, pt, data_range=255.0):
    """fp64 [B, Cm, Hc, Wc] planes -> per-image SSIM [B]."""
    g = gaussian()
    C1, C2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    m1, m2 = _valid_blur(pp, g), _valid_blur(pt, g)
    s11, s22, s12 = _valid_blur(pp * pp, g) - m1 * m1, _valid_blur(pt * pt, g) - m2 * m2, _valid_blur(pp * pt, g) - m1 * m2
    smap = ((2 * m1 * m2 + C1) / (m1 * m1 + m2 * m2 + C1)) * ((2 * s12 + C2) / (s11 + s22 + C2))
    return smap.reshape(smap.shape[0], smap.shape[1], -1).mean(-1).mean(-1)


def bench_ref(pred, target, border, mode, with_ssim=True):
    """-> dict(pp, pt: fp64 planes, sqsum [B], psnr [B], ssim [B] or None)."""
    pp, pt = planes(pred, border, mode), planes(target, border, mode)
    s = sqsum(pp, pt)
    return {"pp": pp, "pt": pt, "sqsum": s, "psnr": psnr_from_sqsum(s, pp[0].size),
            "ssim": ssim(pp, pt) if with_ssim and min(pp.shape[2:]) >= 11 else None}


def plane_bound(mode, channels):
    return PLANE_BOUND_Y if mode == "y" and channels == 3 else 0.0


def sqsum_bound(s, count, mode, channels):
    s = np.asarray(s, dtype=np.float64)
    e = plane_bound(mode, channels)
    return 2.0 * count * U * s + 4.0 * e * np.sqrt(count * s) + 4.0 * e * e * count


def psnr_bound(s, count, mode, channels):
    """Bound on |PSNR32 - PSNR64| for images whose exact sum of squares is s > 0."""
    s = np.asarray(s, dtype=np.float64)
    p = np.abs(psnr_from_sqsum(s, count))
    return 10.0 / np.log(10.0) * (sqsum_bound(s, count, mode, channels) / s + 3.0 * U) + (2 * LOG10_ULPS + 1) * U * np.maximum(p, 1.0)


def tie_inputs():
    """For every k in 0..254 an fp32 x whose fp32 product with 255 is exactly k + 0.5, searched among the fp32 neighbours (three steps
    either side) of (k + .5) / 255 -> (x fp32 [n], k int [n]); one x per k that has one."""
    xs, ks = [], []
    for k in range(255):
        x = np.float32((k + 0.5) / 255.0)
        cand = [x]
        lo = hi = x
        for _ in range(3):
            lo, hi = np.nextafter(lo, np.float32(-1)), np.nextafter(hi, np.float32(2))
            cand += [lo, hi]
        hit = [c for c in cand if np.float32(c) * np.float32(255.0) == np.float32(k + 0.5)]
        if hit:
            xs.append(hit[0])
            ks.append(k)
    return np.array(xs, dtype=np.float32), np.array(ks, dtype=np.int64)
