"""fp64 restatement of NIQE as BasicSR's calculate_niqe computes it (Mittal et al.), independent of the package: scipy.ndimage.convolve
(mode='nearest') in the NAIVE form (v - mu) / (sqrt|E[v^2] - mu^2| + 1), np.roll, the grid argmin of estimate_aggd_param with
scipy.special.gamma, np.cov, pinv.  Also the fp32 restatement of the plane, the exact half-size filter, the centred MSCN form in fp64
with its error bound, and the test images.  The switches of `Opt` are the negative controls of tests/test_niqe_ref.py."""
from dataclasses import dataclass, replace      # noqa: F401

import numpy as np
from scipy import ndimage
from scipy.special import gamma

U = 2.0 ** -24          # fp32 unit roundoff
TAPS = np.array([-3, -9, 29, 111, 111, 29, -9, -3], dtype=np.float64) / 256.0
SHIFTS = ((0, 1), (1, 0), (1, 1), (1, -1))


@dataclass(frozen=True)
class Opt:
    roll_wraps: bool = True           # False: the roll does not wrap (the vacated row / column is zero)
    last_shift: tuple = (1, -1)       # (1, 1): the fourth shift taken as the third
    round_luma: bool = True           # False: the luma is not rounded
    crop: bool = True                 # False: the border crop is skipped
    border_mode: str = "nearest"      # 'reflect': another border rule for the 7 x 7 window
    nan_rows_in_mean: bool = False    # True: a NaN row is counted into the mean (nan -> mean instead of nanmean)


def window():
    r = np.arange(-3, 4, dtype=np.float64)
    g = np.exp(-(r[:, None] ** 2 + r[None, :] ** 2) / (2.0 * (7.0 / 6.0) ** 2))
    return g / g.sum()


# ---- plane ---------------------------------------------------------------------------------------------------------------------------
def quant_f32(x):
    x = np.asarray(x, dtype=np.float32)
    c = np.where(x < 0, np.float32(0), np.where(x > 1, np.float32(1), x)).astype(np.float32)
    return np.rint(c * np.float32(255.0)).astype(np.float32)


def plane_f32(x, border, bs, opt=Opt()):
    """fp32 [B, C, H, W] -> fp32 [B, Hk, Wk]: the operation chain of the benchmark-protocol planes plus one rint of the luma.  Each fma is
    an fp64 multiply-add of fp32 operands (exact there: integers <= 255 times 24-bit constants), rounded once to fp32."""
    q = quant_f32(x)
    if q.shape[1] == 3:
        k = [np.float64(np.float32(v)) for v in (65.481, 128.553, 24.966)]
        t = (q[:, 0] * np.float32(65.481)).astype(np.float32)
        t = (k[1] * q[:, 1].astype(np.float64) + t.astype(np.float64)).astype(np.float32)
        t = (k[2] * q[:, 2].astype(np.float64) + t.astype(np.float64)).astype(np.float32)
        y = (np.float32(16.0) + (t / np.float32(255.0)).astype(np.float32)).astype(np.float32)
        p = np.rint(y).astype(np.float32) if opt.round_luma else y
    else:
        p = q[:, 0]
    H, W = p.shape[-2:]
    b = border if opt.crop else 0
    p = p[:, b:H - b, b:W - b]
    Hk, Wk = (H - 2 * border) // bs * bs, (W - 2 * border) // bs * bs          # the block grid is that of the cropped image either way
    return np.ascontiguousarray(p[:, :Hk, :Wk])


# ---- half size -------------------------------------------------------------------------------------------------------------------------
def half_ref(plane):
    """[..., H, W] (H, W even) -> fp64 [..., H/2, W/2]: out[i] = sum_k TAPS[k] in[2 i - 3 + k], symmetric border, rows then columns.
    Exact in fp64 for an integer-valued plane (every term is an integer times 2^-16)."""
    s = np.asarray(plane, dtype=np.float64)
    for axis in (-1, -2):
        n = s.shape[axis]
        idx = np.arange(-3, n + 3)
        idx = np.where(idx < 0, -1 - idx, np.where(idx >= n, 2 * n - 1 - idx, idx))
        p = np.take(s, idx, axis=axis)
        out = 0.0
        for k in range(8):
            out = out + TAPS[k] * np.take(p, np.arange(k, k + n, 2), axis=axis)
        s = out
    return s


# ---- MSCN ------------------------------------------------------------------------------------------------------------------------------
def mscn_naive(v, w, mode="nearest"):
    """BasicSR's form in fp64 on one [H, W] plane -> (m, sigma)."""
    v = np.asarray(v, dtype=np.float64)
    mu = ndimage.convolve(v, w, mode=mode)
    sigma = np.sqrt(np.abs(ndimage.convolve(v * v, w, mode=mode) - mu * mu))
    return (v - mu) / (sigma + 1.0), sigma


def mscn_centred(v, w):
    """The centred form in fp64 on one [H, W] plane with the taps w (replicate border) -> (m, sigma, a, Sa, Sb): Sa = sum |w d|,
    Sb = sum |w d^2| are the sums of the absolute terms the error bound is formed from."""
    v = np.asarray(v, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64).reshape(7, 7)
    H, W = v.shape
    p = np.pad(v, 3, mode="edge")
    a, b, Sa, Sb = (np.zeros_like(v) for _ in range(4))
    for dy in range(7):
        for dx in range(7):
            d = p[dy:dy + H, dx:dx + W] - v
            a += w[dy, dx] * d
            b += w[dy, dx] * d * d
            Sa += np.abs(w[dy, dx] * d)
            Sb += np.abs(w[dy, dx] * d * d)
    sigma = np.sqrt(np.abs(b - a * a))
    return -a / (sigma + 1.0), sigma, a, Sa, Sb


def mscn_bounds(sigma, a, Sa, Sb, da_extra=0.0, db_extra=0.0):
    """Per-element bounds on |sigma32 - sigma| and |m32 - m| of the fp32 centred form (49 fmaf per sum; d and d^2 are exact).
    Sums: |da| <= 2 K u Sa, |db| <= 2 K u Sb with K = 49.  t = b - a^2: |dt| <= db + 2 |a| da + da^2 + 2 u (|b| + a^2) (the product and
    the subtraction round once each; |b| <= Sb, a^2 <= Sa^2).  sqrt|.|: |sqrt|t'| - sqrt|t|| <= min(sqrt(dt), dt / sigma), plus one
    rounding u sigma'.  m = -a / (sigma + 1): |dm| <= da / (sigma + 1) + |a| dsigma / (sigma + 1)^2 + 2 u |m| (the add and the division)."""
    K = 49.0
    da, db = 2 * K * U * Sa + da_extra, 2 * K * U * Sb + db_extra          # *_extra: what the reference's own sums may be off by
    dt = db + 2 * np.abs(a) * da + da * da + 2 * U * (Sb + Sa * Sa)
    with np.errstate(divide="ignore", invalid="ignore"):
        ds = np.minimum(np.sqrt(dt), np.where(sigma > 0, dt / np.maximum(sigma, 1e-300), np.inf))
    ds = ds + U * (sigma + ds)
    m = np.abs(a) / (sigma + 1.0)
    dm = da / (sigma + 1.0) + np.abs(a) * ds / (sigma + 1.0) ** 2 + 2 * U * (m + da) + 1e-45
    return ds, dm


# ---- features --------------------------------------------------------------------------------------------------------------------------
_GAM = np.arange(0.2, 10.001, 0.001)
_R_GAM = np.square(gamma(2.0 / _GAM)) / (gamma(1.0 / _GAM) * gamma(3.0 / _GAM))


def estimate_aggd(block):
    block = np.asarray(block, dtype=np.float64).ravel()
    with np.errstate(divide="ignore", invalid="ignore"):
        neg, pos = block[block < 0], block[block > 0]
        left = np.sqrt(np.sum(neg ** 2) / neg.size) if neg.size else np.nan
        right = np.sqrt(np.sum(pos ** 2) / pos.size) if pos.size else np.nan
        gh = left / right
        rhat = np.mean(np.abs(block)) ** 2 / np.mean(block ** 2)
        rnorm = rhat * (gh ** 3 + 1) * (gh + 1) / (gh ** 2 + 1) ** 2
        alpha = _GAM[np.argmin((_R_GAM - rnorm) ** 2)]
        bl = left * np.sqrt(gamma(1 / alpha) / gamma(3 / alpha))
        br = right * np.sqrt(gamma(1 / alpha) / gamma(3 / alpha))
    return alpha, bl, br


def roll(block, shift, wraps=True):
    out = np.roll(block, shift, axis=(0, 1))
    if not wraps:
        if shift[0] > 0:
            out[:shift[0], :] = 0
        if shift[1] > 0:
            out[:, :shift[1]] = 0
        if shift[1] < 0:
            out[:, shift[1]:] = 0
    return out


def block_features(block, opt=Opt()):
    a, bl, br = estimate_aggd(block)
    feat = [a, (bl + br) / 2]
    for s in (*SHIFTS[:3], opt.last_shift):
        a, bl, br = estimate_aggd(block * roll(block, s, opt.roll_wraps))
        feat += [a, (br - bl) * (gamma(2 / a) / gamma(1 / a)), bl, br]
    return feat


def features_from_moments(mom, npix):
    """Block moments [n, 5, 5] (count and square sum of both signs, sum of magnitudes per map) of blocks of npix pixels -> [n, 18]:
    estimate_aggd and block_features restated on the moments, in fp64."""
    mom = np.asarray(mom, dtype=np.float64)
    out = np.empty((mom.shape[0], 18))
    with np.errstate(divide="ignore", invalid="ignore"):
        for i in range(mom.shape[0]):
            est = []
            for cn, sn, cp, sp, sa in mom[i]:
                left, right = np.sqrt(sn / cn), np.sqrt(sp / cp)
                gh = left / right
                rnorm = (sa / npix) ** 2 / ((sn + sp) / npix) * (gh ** 3 + 1) * (gh + 1) / (gh ** 2 + 1) ** 2
                alpha = _GAM[np.argmin((_R_GAM - rnorm) ** 2)]
                k = np.sqrt(gamma(1 / alpha) / gamma(3 / alpha))
                est.append((alpha, left * k, right * k))
            feat = [est[0][0], (est[0][1] + est[0][2]) / 2]
            for a, bl, br in est[1:]:
                feat += [a, (br - bl) * (gamma(2 / a) / gamma(1 / a)), bl, br]
            out[i] = feat
    return out


def plane_rows(plane, w, bs, opt=Opt()):
    """One integer-valued plane [Hk, Wk] -> (rows [nb, 36], sharp [nb]): both scales side by side, the block means of sigma at scale 1."""
    plane = np.asarray(plane, dtype=np.float64)
    nbh, nbw = plane.shape[0] // bs, plane.shape[1] // bs
    feats, sharp = [], None
    for scale, img in ((1, plane), (2, half_ref(plane))):
        m, sigma = mscn_naive(img, w, opt.border_mode)
        b = bs // scale
        rows = [block_features(m[i * b:(i + 1) * b, j * b:(j + 1) * b], opt) for i in range(nbh) for j in range(nbw)]
        feats.append(np.array(rows))
        if scale == 1:
            sharp = np.array([sigma[i * b:(i + 1) * b, j * b:(j + 1) * b].mean() for i in range(nbh) for j in range(nbw)])
    return np.concatenate(feats, axis=1), sharp


def distance(rows, mu_p, cov_p, opt=Opt()):
    rows = np.asarray(rows, dtype=np.float64)
    mu_d = np.mean(rows, axis=0) if opt.nan_rows_in_mean else np.nanmean(rows, axis=0)
    clean = rows[~np.isnan(rows).any(axis=1)]
    cov_d = np.cov(clean, rowvar=False)
    d = (np.reshape(mu_p, (1, 36)) - mu_d.reshape(1, 36))
    return float(np.sqrt(d @ np.linalg.pinv((np.asarray(cov_p) + cov_d) / 2) @ d.T).reshape(()))


def score(x, mu_p, cov_p, w=None, border=0, bs=96, opt=Opt()):
    """fp32 [B, C, H, W] in [0, 1] -> list of scores."""
    w = window() if w is None else w
    return [distance(plane_rows(p, w, bs, opt)[0], mu_p, cov_p, opt) for p in plane_f32(x, border, bs, opt)]


def fit(xs, sharpness=0.75, w=None, border=0, bs=96):
    """Images (each fp32 [B, C, H, W]) -> (mu [36], cov [36, 36])."""
    w = window() if w is None else w
    kept = []
    for x in xs:
        for p in plane_f32(x, border, bs):
            rows, sharp = plane_rows(p, w, bs)
            kept.append(rows[sharp > sharpness * sharp.max()])
    rows = np.concatenate(kept)
    return np.nanmean(rows, axis=0), np.cov(rows[~np.isnan(rows).any(axis=1)], rowvar=False)


# ---- images ----------------------------------------------------------------------------------------------------------------------------
def pink_image(seed, n=288):
    """uint8-valued 1/f-noise image [n, n]: clip(round(128 + 45 pink)), pink of unit standard deviation."""
    rng = np.random.RandomState(seed)
    f = np.fft.fft2(rng.standard_normal((n, n)))
    fy, fx = np.meshgrid(np.fft.fftfreq(n), np.fft.fftfreq(n), indexing="ij")
    r = np.sqrt(fy * fy + fx * fx)
    r[0, 0] = 1.0
    p = np.real(np.fft.ifft2(f / r))
    p = (p - p.mean()) / p.std()
    return np.clip(np.rint(128.0 + 45.0 * p), 0, 255)


def as_batch(img8):
    """An integer-valued [H, W] image -> fp32 [1, 1, H, W] in [0, 1]."""
    return (np.asarray(img8, dtype=np.float32) / np.float32(255.0))[None, None]


def noised(img8, sigma, seed=100):
    return np.clip(np.rint(img8 + np.random.RandomState(seed).standard_normal(img8.shape) * sigma), 0, 255)


def blurred(img8, sigma):
    return np.clip(np.rint(ndimage.gaussian_filter(np.asarray(img8, dtype=np.float64), sigma, mode="nearest")), 0, 255)


_SUITE = None


def suite():
    """Computed once, shared, left unchanged: the pristine fit on pink_image(0..5) and the seventh image clean, noised and blurred ->
    dict(mu, cov, images {name: fp32 [1, 1, 288, 288]}, scores {name: fp64 reference score})."""
    global _SUITE
    if _SUITE is None:
        mu, cov = fit([as_batch(pink_image(s)) for s in range(6)])
        base = pink_image(6)
        images = {"clean": as_batch(base)}
        for s in (10, 25, 50):
            images[f"noise{s}"] = as_batch(noised(base, s))
        for s in (0.8, 1.5, 3):
            images[f"blur{s}"] = as_batch(blurred(base, s))
        scores = {k: score(v, mu, cov)[0] for k, v in images.items()}
        _SUITE = {"mu": mu, "cov": cov, "images": images, "scores": scores}
    return _SUITE
