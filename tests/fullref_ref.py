"""An independent fp64 restatement of the two full-reference scores of include/srk.h "Full-reference scores: PSNR-B, MS-SSIM" (DESIGN 7y),
in numpy slicing and loops; nothing of the package is used.  tests/test_fullref_ref.py pins it (known answers, torch's avg_pool2d, negative
controls); the kernel and CLI tests compare with it.  The keyword switches exist for the negative controls only: each default is the
definition."""
import math

import numpy as np

WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
U = 2.0 ** -24


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
def pink_image(seed, H, W):
    """1/f noise scaled to 0..255 and rounded: float64 [H, W] holding integers."""
    rng = np.random.RandomState(seed)
    fy, fx = np.fft.fftfreq(H)[:, None], np.fft.fftfreq(W)[None, :]
    f = np.sqrt(fy * fy + fx * fx)
    f[0, 0] = 1.0
    img = np.real(np.fft.ifft2(np.fft.fft2(rng.standard_normal((H, W))) / f))
    img = (img - img.min()) / (img.max() - img.min())
    return np.round(img * 255.0)


def noised(img, sigma, seed=0):
    """Gaussian noise of `sigma`, clamped and rounded."""
    rng = np.random.RandomState(1000 + seed + int(sigma))
    return np.round(np.clip(img + sigma * rng.standard_normal(img.shape), 0.0, 255.0))


# ---- PSNR-B ---------------------------------------------------------------------------------------------------------------------------
def psnrb_sums(p, t, phase=7):
    """One plane pair -> (sums [5] = squared error, Dh_b, Dh_n, Dv_b, Dv_n; the sums of the absolute terms [5], which are the same
    numbers: every term is a square).  Plain loops over the pairs."""
    p, t = np.asarray(p, np.float64), np.asarray(t, np.float64)
    H, W = p.shape
    s = np.zeros(5)
    s[0] = ((p - t) ** 2).sum()
    for x in range(W - 1):
        d = ((p[:, x] - p[:, x + 1]) ** 2).sum()
        s[1 if x % 8 == phase else 2] += d
    for y in range(H - 1):
        d = ((p[y, :] - p[y + 1, :]) ** 2).sum()
        s[3 if y % 8 == phase else 4] += d
    return s


def psnrb_counts(H, W):
    """(n_b, n_n): the published counts."""
    n_bh, n_bv = H * (W // 8 - 1), W * (H // 8 - 1)
    return n_bh + n_bv, H * (W - 1) - n_bh + W * (H - 1) - n_bv


def psnrb_parts(s, H, W):
    """sums [5] -> (mse, bef, D_b, D_n)."""
    n_b, n_n = psnrb_counts(H, W)
    d_b, d_n = (s[1] + s[3]) / n_b, (s[2] + s[4]) / n_n
    bef = 3.0 / math.log2(min(H, W)) * (d_b - d_n) if d_b > d_n else 0.0
    return s[0] / (H * W), bef, d_b, d_n


def psnr_of(den):
    if den != den:
        return float("nan")
    return float("inf") if den == 0 else 10.0 * math.log10(65025.0 / den)


def psnrb_plane(p, t, phase=7, bef_from="pred"):
    H, W = np.asarray(p).shape
    mse, bef, _, _ = psnrb_parts(psnrb_sums(p, t, phase), H, W)
    if bef_from == "target":
        bef = psnrb_parts(psnrb_sums(t, p, phase), H, W)[1]
    return psnr_of(mse + bef)


def psnrb(pp, pt, **kw):
    """planes [B, Cm, Hc, Wc] -> float64 [B]: the mean over the planes of an image."""
    pp, pt = np.asarray(pp, np.float64), np.asarray(pt, np.float64)
    return np.array([np.mean([psnrb_plane(pp[b, c], pt[b, c], **kw) for c in range(pp.shape[1])]) for b in range(pp.shape[0])])


def psnrb_bound(pp, pt):
    """What fp32 sums of n terms in any order, each term one fused multiply-add, may differ from the exact sums by, and what that does to the
    score.  Returns (sum bounds [B, Cm, 5], score bounds [B]).  A sum of n non-negative terms: |err| <= 2 n u S (S the exact sum: n - 1
    additions and one rounding per term, first order, doubled).  The score: den = mse + bef is Lipschitz in the sums (bef = scale
    max(D_b - D_n, 0)), so d(den) <= e0 / N + scale (e_b / n_b + e_n / n_n), plus 8 u of every intermediate for the handful of fp32
    operations of the finishing step; 10 log10 has slope 10 / (ln 10 den), and log10f, the division and the mean add 8 u |psnrb|."""
    pp, pt = np.asarray(pp, np.float64), np.asarray(pt, np.float64)
    B, C, H, W = pp.shape
    eb, es = np.zeros((B, C, 5)), np.zeros(B)
    n_b, n_n = psnrb_counts(H, W)
    scale = 3.0 / math.log2(min(H, W))
    for b in range(B):
        for c in range(C):
            s = psnrb_sums(pp[b, c], pt[b, c])
            eb[b, c] = 2.0 * H * W * U * s
            mse, bef, d_b, d_n = psnrb_parts(s, H, W)
            dden = eb[b, c, 0] / (H * W) + scale * ((eb[b, c, 1] + eb[b, c, 3]) / n_b + (eb[b, c, 2] + eb[b, c, 4]) / n_n)
            dden += 8.0 * U * (mse + scale * (d_b + d_n))
            den = mse + bef
            v = psnr_of(den)
            es[b] += ((10.0 / math.log(10.0)) * dden / den + 8.0 * U * abs(v)) / C if den > 0 and np.isfinite(v) else 0.0
    return eb, es


# ---- MS-SSIM --------------------------------------------------------------------------------------------------------------------------
def window():
    c = np.arange(11, dtype=np.float64) - 5.0
    g = np.exp(-(c * c) / (2.0 * 1.5 * 1.5))
    return g / g.sum()


def _blur(a, w):
    H, W = a.shape
    v = np.zeros((H - 10, W))
    for k in range(11):
        v += w[k] * a[k:k + H - 10, :]
    o = np.zeros((H - 10, W - 10))
    for k in range(11):
        o += w[k] * v[:, k:k + W - 10]
    return o


def ssim_means(x, y, data_range=255.0):
    """One plane pair -> (S, CS): the mean of the SSIM map and of its contrast-structure factor."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    w = window()
    C1, C2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    m1, m2 = _blur(x, w), _blur(y, w)
    s11, s22, s12 = _blur(x * x, w) - m1 * m1, _blur(y * y, w) - m2 * m2, _blur(x * y, w) - m1 * m2
    cs = (2.0 * s12 + C2) / (s11 + s22 + C2)
    s = (2.0 * m1 * m2 + C1) / (m1 * m1 + m2 * m2 + C1) * cs
    return s.mean(), cs.mean()


def pool(a, include_pad=True):
    """avg_pool2d(kernel 2, stride 2, padding = extent % 2, count_include_pad): an odd extent gains a line of zeros in front."""
    a = np.asarray(a, np.float64)
    H, W = a.shape
    ph, pw = H % 2, W % 2
    Ho, Wo = (H + ph) // 2, (W + pw) // 2
    o = np.zeros((Ho, Wo))
    for j in range(Ho):
        for i in range(Wo):
            ys = [r for r in (2 * j - ph, 2 * j - ph + 1) if r >= 0]
            xs = [c for c in (2 * i - pw, 2 * i - pw + 1) if c >= 0]
            o[j, i] = sum(a[r, c] for r in ys for c in xs) / (4.0 if include_pad else len(ys) * len(xs))
    return o


def msssim_levels(x, y, levels=5, data_range=255.0, include_pad=True):
    """One plane pair -> (means [levels, 2] = (S, CS), the pooled pairs [(x_s, y_s) for s = 1 .. levels - 1])."""
    means, pyr = np.zeros((levels, 2)), []
    for s in range(levels):
        means[s] = ssim_means(x, y, data_range)
        if s < levels - 1:
            x, y = pool(x, include_pad), pool(y, include_pad)
            pyr.append((x, y))
    return means, pyr


def msssim_from_means(means, weights=WEIGHTS, cs_fine=True):
    """means [levels, 2] of one channel -> its score."""
    L = len(means)
    v = [max(means[s][1 if (cs_fine and s < L - 1) else 0], 0.0) for s in range(L)]
    return float(np.prod([v[s] ** weights[s] for s in range(L)]))


def msssim(X, Y, weights=WEIGHTS, data_range=255.0, include_pad=True, cs_fine=True):
    """images [B, C, H, W] -> float64 [B]: the mean over channels."""
    X, Y = np.asarray(X, np.float64), np.asarray(Y, np.float64)
    return np.array([np.mean([msssim_from_means(msssim_levels(X[b, c], Y[b, c], len(weights), data_range, include_pad)[0], weights, cs_fine)
                              for c in range(X.shape[1])]) for b in range(X.shape[0])])
