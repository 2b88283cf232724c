"""fp64 restatement of srk_usm_sharpen_f32 (include/srk.h; csrc/usm.hip), evaluated from the fp32 taps, the fp32 x and the fp32 scalars
weight / threshold taken as exact numbers, and the interval logic of tests/test_gpu_usm.py.

    G(v)(p, q) = sum_i taps[i] h(rho(p + i - R, H), q),  h(p, q) = sum_j taps[j] v(p, rho(q + j - R, W))       rho = reflect-101
    blur = G(x); res = x - blur; mask = |res| 255 > threshold; soft = G(mask)
    sharp = clip(x + weight res, 0, 1); out = soft sharp + (1 - soft) x

The bound, u = 2^-24, derived and not tuned.  A chain acc = fmaf(t_j, v_j, acc) of n terms from 0 makes n roundings, each at most u of a
partial sum that is at most sum |t_j| |v_j|: n u sum |t| |v|.  G is two such chains of ks terms, the second over the results of the first:
2 ks u S with S = sum_i sum_j |t_i| |t_j| |v| to first order; doubled, as DESIGN 7p doubles its n u S, for the higher orders:
    E_G(v)  = 2 (2 ks) u S(v)
    E_res   = E_G(x) + u (|res| + E_G(x))                                   one subtraction
A mask pixel is UNDECIDED when | |res| 255 - threshold | <= 255 E_res + 255 u |res| (the error of res, and the rounding of the product).
Every other pixel has the reference's mask.  soft therefore lies in [G(mask, undecided = 0) - E_G, G(mask, undecided = 1) + E_G] with
E_G = E_G(mask, undecided = 1).  With A = |w| (|res| + E_res):
    E_sharp = |w| E_res + u A + u (|x| + A (1 + u))                         one product, one sum; the clamp is exact and 1-Lipschitz
The blend is linear in soft, so over the interval it lies in the hull of its two ends; the kernel's soft * sharp, 1 - soft, (1 - soft) * x
and the final sum add one u each:
    E_out   = (smax E_sharp + u (2 smax (|sharp| + E_sharp) + 3 omax |x|)) (1 + 4 u)      smax = max |soft|, omax = max |1 - soft|
"""
import numpy as np

U = 2.0 ** -24
SHAPES = [(26, 27), (40, 72), (33, 50), (70, 130)]


def gaussian1d(ks, sigma=0.0, rule="opencv"):
    """fp32 taps, normalised in fp64; sigma <= 0 -> OpenCV's rule (or, as a negative control, ks / 6)."""
    r = (ks - 1) // 2
    if sigma <= 0:
        sigma = 0.3 * (r - 1) + 0.8 if rule == "opencv" else ks / 6.0
    d = np.arange(-r, r + 1, dtype=np.float64)
    k = np.exp(-(d * d) / (2.0 * sigma * sigma))
    return (k / k.sum()).astype(np.float32)


def _pad(v, R, axis, border):
    pw = [(0, 0)] * v.ndim
    pw[axis] = (R, R)
    if R == 0:
        return v
    if border == "reflect":
        return np.pad(v, pw, mode="reflect")
    if border == "replicate":
        return np.pad(v, pw, mode="edge")
    return np.pad(v, pw, mode="constant")


def gauss(v, taps, border="reflect", vertical_first=False):
    """G(v) over the last two axes in fp64."""
    v = np.asarray(v, dtype=np.float64)
    t = np.asarray(taps, dtype=np.float64)
    R = (len(t) - 1) // 2
    for axis in ((-2, -1) if vertical_first else (-1, -2)):
        p = _pad(v, R, axis, border)
        n = v.shape[axis]
        acc = np.zeros_like(v)
        for j in range(len(t)):
            acc = acc + t[j] * np.take(p, np.arange(j, j + n), axis=axis)
        v = acc
    return v


def usm(x, taps, weight=0.5, threshold=10.0, border="reflect", use_abs=True, thr_scale=255.0, clip=True, hard=False, swapped=False):
    """-> dict(blur, res, mask, soft, sharp, out) in fp64.  The keyword arguments are the NEGATIVE CONTROLS of tests/test_usm_ref.py."""
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    w, thr = float(np.float32(weight)), float(np.float32(threshold))
    blur = gauss(x, taps, border)
    res = x - blur
    mask = ((np.abs(res) if use_abs else res) * thr_scale > thr).astype(np.float64)
    soft = mask if hard else gauss(mask, taps, border)
    sharp = x + w * res
    if clip:
        sharp = np.clip(sharp, 0.0, 1.0)
    out = (soft * x + (1.0 - soft) * sharp) if swapped else (soft * sharp + (1.0 - soft) * x)
    return dict(blur=blur, res=res, mask=mask, soft=soft, sharp=sharp, out=out)


def intervals(x, taps, weight=0.5, threshold=10.0):
    """-> dict(lo, hi, undecided, ref): the kernel's out must lie in [lo, hi] (the docstring above); undecided is the boolean map."""
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    t = np.asarray(taps, dtype=np.float64)
    ks = len(t)
    w, thr = float(np.float32(weight)), float(np.float32(threshold))
    r = usm(x, taps, weight, threshold)
    res = r["res"]
    eg = lambda v: 2.0 * (2 * ks) * U * gauss(np.abs(v), np.abs(t))          # noqa: E731
    e_blur = eg(x)
    e_res = e_blur + U * (np.abs(res) + e_blur)
    und = np.abs(np.abs(res) * 255.0 - thr) <= 255.0 * e_res + 255.0 * U * np.abs(res)
    m_lo, m_hi = np.where(und, 0.0, r["mask"]), np.where(und, 1.0, r["mask"])
    e_soft = eg(m_hi)
    s_lo, s_hi = gauss(m_lo, taps) - e_soft, gauss(m_hi, taps) + e_soft
    a = abs(w) * (np.abs(res) + e_res)
    e_sharp = abs(w) * e_res + U * a + U * (np.abs(x) + a * (1.0 + U))
    sharp = r["sharp"]
    smax = np.maximum(np.abs(s_lo), np.abs(s_hi))
    omax = np.maximum(np.abs(1.0 - s_lo), np.abs(1.0 - s_hi))
    e_out = (smax * e_sharp + U * (2.0 * smax * (np.abs(sharp) + e_sharp) + 3.0 * omax * np.abs(x))) * (1.0 + 4.0 * U)
    f_lo, f_hi = s_lo * sharp + (1.0 - s_lo) * x, s_hi * sharp + (1.0 - s_hi) * x
    return dict(lo=np.minimum(f_lo, f_hi) - e_out, hi=np.maximum(f_lo, f_hi) + e_out, undecided=und, ref=r, e_out=e_out)


def image(seed, shape, channels=None, batch=None):
    """Seeded 8-bit levels / 255 as fp32: a smooth field plus step edges (rectangles), so that the mask has both values and few pixels
    sit at the threshold.  [H][W], [C][H][W] or [B][C][H][W]."""
    rng = np.random.RandomState(seed)
    lead = tuple(n for n in (batch, channels) if n is not None)
    H, W = shape
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    out = np.empty(lead + (H, W), dtype=np.float32)
    for idx in np.ndindex(*lead) if lead else [()]:
        fx, fy, ph = rng.uniform(0.02, 0.09), rng.uniform(0.02, 0.09), rng.uniform(0, 6.28)
        v = 128.0 + 60.0 * np.sin(fx * xx + ph) * np.cos(fy * yy + 0.5 * ph)
        for _ in range(3):
            y0, x0 = rng.randint(0, H - 3), rng.randint(0, W - 3)
            y1, x1 = rng.randint(y0 + 2, H + 1), rng.randint(x0 + 2, W + 1)
            v[y0:y1, x0:x1] += rng.choice([-70.0, -45.0, 45.0, 70.0])
        out[idx] = (np.rint(np.clip(v, 0, 255)) / 255.0).astype(np.float32)
    return out
