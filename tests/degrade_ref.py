"""fp64 numpy restatement of the blind degradation (include/srk.h: srk_degrade_blind_f32, srk_crop_degrade_blind_u8): the antialiased
bicubic downscale of tests/resize_ref.py behind an axis-aligned Gaussian blur, composed into one table per output, plus Philox4x32-10 /
Box-Muller noise keyed by the coordinates in the whole downscaled image.  Pinned in tests/test_degrade_ref.py (known-answer vectors,
statistics, F.conv2d + F.interpolate(antialias=True) on fp64 tensors); the reference of tests/test_gpu_degrade.py.

`tables` / `degrade` / `patch` take the blur as (sigma_y, sigma_x) in HR pixels; sigmas and noise amplitudes are used as the fp32 values
the parameter table carries (`f32`).  The negative controls of the CPU tests are built from these pieces (`blur` alone, `degrade(patch_keyed=True)`, `add_noise` after `quant8`)."""
import functools

import numpy as np

import resize_ref as R

U = R.U
RMAX = 8
M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF
# The device z against `normal` below, measured over the draws of tests/test_gpu_degrade.py::test_device_normal (MI355X): the largest
# |z_dev - z| / (u (r + |z|)) over its 92 160 draws was 1.547; C_NOISE is 4 x that (a finite sample underestimates the maximum).  DESIGN 7k records both.
C_NOISE_MEASURED = 1.547
C_NOISE = 4.0 * C_NOISE_MEASURED


def f32(v):
    return float(np.float32(v))


def radius(sigma):
    sigma = f32(sigma)
    return min(int(np.ceil(3.0 * sigma)), RMAX) if sigma > 0.0 else 0


def gauss(sigma):
    """g[d], d = -R..R, normalised in fp64."""
    sigma, r = f32(sigma), radius(sigma)
    d = np.arange(-r, r + 1, dtype=np.float64)
    g = np.exp(-(d * d) / (2.0 * sigma * sigma))
    return g / g.sum()


def tables(n_in, n_out, sigma):
    """-> (lo, hi, weights) like resize_ref.tables: W[m] = sum_j w_c[j] g[m - lo_c - j] on [max(lo_c - R, 0), min(hi_c + R, n_in)),
    divided by its sum.  sigma == 0: the cubic tables themselves."""
    lo_c, hi_c, wc = R.tables(n_in, n_out)
    r = radius(sigma)
    if r == 0:
        return lo_c, hi_c, wc
    g = gauss(sigma)
    los, his, ws = [], [], []
    for i in range(n_out):
        full = np.convolve(wc[i], g)                      # index k <-> input lo_c - R + k
        lo, hi = max(lo_c[i] - r, 0), min(hi_c[i] + r, n_in)
        w = full[lo - (lo_c[i] - r):hi - (lo_c[i] - r)]
        los.append(lo)
        his.append(hi)
        ws.append(w / w.sum())
    return np.array(los), np.array(his), ws


def blur(x, sigma_y, sigma_x):
    """The Gaussian alone on [..., H, W] with the same border rule (taps outside dropped, the rest renormalised): a negative control."""
    x = np.asarray(x, dtype=np.float64)
    for axis, sigma in ((-1, sigma_x), (-2, sigma_y)):
        r = radius(sigma)
        if r == 0:
            continue
        g, n = gauss(sigma), x.shape[axis]
        xm = np.moveaxis(x, axis, -1)
        out = np.empty_like(xm)
        for i in range(n):
            lo, hi = max(i - r, 0), min(i + r + 1, n)
            w = g[lo - (i - r):hi - (i - r)]
            out[..., i] = (xm[..., lo:hi] * (w / w.sum())).sum(axis=-1)
        x = np.moveaxis(out, -1, axis)
    return x


def filtered(img, s, sigma_y, sigma_x, top=0, left=0, P=None):
    """img [..., H, W] in [0, 1] -> fp64: rows top / s .. and columns left / s .. (P of each; everything when P is None) of the blurred
    (H // s, W // s) downscale of the top-left (H - H % s, W - W % s) region; only those outputs are computed."""
    img = np.asarray(img, dtype=np.float64)
    H, W = img.shape[-2:]
    reg = img[..., :H - H % s, :W - W % s]
    rows = range(top // s, top // s + P) if P else range(H // s)
    cols = range(left // s, left // s + P) if P else range(W // s)
    mid = R._pass(reg, *tables(W - W % s, W // s, sigma_x), rows=cols)
    return np.swapaxes(R._pass(np.swapaxes(mid, -1, -2), *tables(H - H % s, H // s, sigma_y), rows=rows), -1, -2)


# ---- Philox4x32-10 and the normal draw ---------------------------------------------------------------------------------------------------
def philox_int(ctr, key):
    """Philox4x32-10 in Python integers: ctr = 4 words, key = 2 words -> 4 words."""
    c0, c1, c2, c3 = (int(v) & MASK for v in ctr)
    k0, k1 = (int(v) & MASK for v in key)
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & MASK, (p0 >> 32) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


def philox(c0, c1, c2, c3, k0, k1):
    """The same on uint64 numpy arrays holding 32-bit words (broadcast against each other) -> 4 arrays."""
    c0, c1, c2, c3, k0, k1 = np.broadcast_arrays(*(np.asarray(v, dtype=np.uint64) & np.uint64(MASK) for v in (c0, c1, c2, c3, k0, k1)))
    m, sh = np.uint64(MASK), np.uint64(32)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2
        c0, c1, c2, c3 = (p1 >> sh) ^ c1 ^ k0, p1 & m, (p0 >> sh) ^ c3 ^ k1, p0 & m
        k0, k1 = (k0 + np.uint64(W0)) & m, (k1 + np.uint64(W1)) & m
    return c0, c1, c2, c3


def normal(x, y, ch, noise_id):
    """-> (z, r): the standard normal of output (x, y) of the whole downscaled image, channel ch, and r = sqrt(-2 ln u1).
    u1 = ((r0 >> 8) + 1) 2^-24, u2 = (r1 >> 8) 2^-24 from the first two words of counter (x, y, ch, 0) under key = noise_id."""
    noise_id = int(noise_id) & 0xFFFFFFFFFFFFFFFF
    r0, r1, _, _ = philox(x, y, ch, 0, noise_id & MASK, noise_id >> 32)
    u1 = ((r0 >> np.uint64(8)) + np.uint64(1)).astype(np.float64) * 2.0 ** -24
    u2 = (r1 >> np.uint64(8)).astype(np.float64) * 2.0 ** -24
    r = np.sqrt(-2.0 * np.log(u1))
    return r * np.cos(2.0 * np.pi * u2), r


def normal_field(C, y0, x0, Ph, Pw, noise_id, gray):
    """z, r [C, Ph, Pw] of the window at (y0, x0) of the downscaled image; gray: one draw (channel 0) for every channel."""
    yy, xx = np.meshgrid(np.arange(y0, y0 + Ph), np.arange(x0, x0 + Pw), indexing="ij")
    zr = [normal(xx, yy, 0 if gray else c, noise_id) for c in range(1 if gray else C)]
    z, r = np.stack([a for a, _ in zr]), np.stack([b for _, b in zr])
    return (np.repeat(z, C, axis=0), np.repeat(r, C, axis=0)) if gray else (z, r)


def noise_std(v, sigma_n, gain):
    return np.sqrt(f32(sigma_n) ** 2 + f32(gain) * np.maximum(v, 0.0))


def add_noise(v, z, sigma_n, gain):
    """v + sqrt(sigma_n^2 + gain max(v, 0)) z; nothing at all when both amplitudes are 0."""
    return v if (f32(sigma_n) == 0.0 and f32(gain) == 0.0) else v + noise_std(v, sigma_n, gain) * z


def degrade(img, s, sigma, noise=(0.0, 0.0), noise_id=0, gray=False, top=0, left=0, P=None, patch_keyed=False):
    """The unquantised fp64 LR of img [C, H, W] -> (lr, noise bound term per element): the whole image (P None) or the patch at (top,
    left) in HR pixels.  patch_keyed (a negative control): the counter takes the coordinates inside the patch."""
    v = filtered(img, s, sigma[0], sigma[1], top, left, P)
    C, Ph, Pw = v.shape
    y0, x0 = (0, 0) if patch_keyed else (top // s, left // s)
    if f32(noise[0]) == 0.0 and f32(noise[1]) == 0.0:
        return v, np.zeros_like(v)
    z, r = normal_field(C, y0, x0, Ph, Pw, noise_id, gray or C == 1)
    return add_noise(v, z, *noise), C_NOISE * U * (r + np.abs(z)) * noise_std(v, *noise)


def bound(H, W, s, sigma, max_abs, u=U):
    """resize_ref.bound on the composed tables: 2 (Ky + Kx + 4) u Ly Lx max|x|, K the largest tap count and L the largest sum |w| of
    each axis.  H, W: the filtered region (multiples of s)."""
    _, _, wy = tables(H, H // s, sigma[0])
    _, _, wx = tables(W, W // s, sigma[1])
    ky, kx = max(len(w) for w in wy), max(len(w) for w in wx)
    ly, lx = max(np.abs(w).sum() for w in wy), max(np.abs(w).sum() for w in wx)
    return 2.0 * (ky + kx + 4) * u * ly * lx * max_abs


def nan_footprint(H, W, s, sigma, y, x):
    """Boolean [H // s, W // s]: the outputs whose composed footprint contains input (y, x) on both axes."""
    loy, hiy, _ = tables(H, H // s, sigma[0])
    lox, hix, _ = tables(W, W // s, sigma[1])
    return np.outer((loy <= y) & (y < hiy), (lox <= x) & (x < hix))


near_half = R.near_half
quant8 = R.quant8
to_unit3 = R.to_unit3


# ---- parameter packing, restated ---------------------------------------------------------------------------------------------------------
def bits(v):
    return int(np.float32(v).view(np.uint32))


def signed64(v):
    v &= 0xFFFFFFFFFFFFFFFF
    return v - (1 << 64) if v >> 63 else v


def pack(sigma, noise, noise_id, gray):
    """Slots 6..9 of a descriptor as signed 64-bit integers."""
    return [signed64(bits(sigma[0]) | bits(sigma[1]) << 32), signed64(bits(noise[0]) | bits(noise[1]) << 32), signed64(int(noise_id)),
            int(bool(gray))]


# ---- the cases tests/test_degrade_ref.py (CPU: the skip cap) and tests/test_gpu_degrade.py (device) share -----------------------------------
SCALES = (2, 3, 4)
PATCH = 72                               # two column tiles (64 + 8) and nine row tiles
SIGMAS = [(0.0, 0.0), (0.0, 1.7), (1.7, 0.0), (0.3, 2.5), (2.5, 2.5)]
NOISES = [(0.04, 0.0), (0.03, 0.01), (0.02, 0.0), (0.05, 0.005), (0.01, 0.002)]          # sigma_n > 0 keeps d std / d v <= gain / (2 sigma_n)
GRAYS = [True, False, True, False, False]
SOURCES = ("gray8", "rgb8", "gray16")
NOISE_ID0 = 0x9E3779B97F4A7C15          # bit 63 set: the id travels as a signed 64-bit integer


def case_image(s, k):
    """HR image k of factor s: LR extents PATCH + 9 and PATCH + 14 -- a patch on each border and one inside -- plus a remainder row."""
    rng = np.random.RandomState(300 + 10 * s + k)
    h, w = (PATCH + 9) * s + (s - 1), (PATCH + 14) * s
    if SOURCES[k] == "gray8":
        return rng.randint(0, 256, (h, w)).astype(np.uint8)
    if SOURCES[k] == "rgb8":
        return rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
    return rng.randint(0, 65536, (h, w)).astype(np.uint16)


def case_samples(s, k):
    """[(top, left, sigma, noise, noise_id, gray)] x 5: the four corners and an interior position, the sigma pairs rotated by k + s."""
    a = case_image(s, k)
    mt, ml = a.shape[0] // s - PATCH, a.shape[1] // s - PATCH
    pos = [(0, 0), (0, ml * s), (mt * s, 0), (mt * s, ml * s), ((mt // 2) * s, ((ml + 1) // 2) * s)]
    return [(top, left, SIGMAS[(b + k + s) % 5], NOISES[(b + k) % 5], NOISE_ID0 + 7 * b + k, GRAYS[b] or a.ndim == 2)
            for b, (top, left) in enumerate(pos)]


@functools.lru_cache(maxsize=None)
def case_reference(s, k, noisy):
    """(ref [5, 3, P, P] fp64 unquantised, bnd [5, 3, P, P]) of case (s, k), computed once and shared."""
    a = case_image(s, k)
    img = to_unit3(a)
    H, W = a.shape[0] // s * s, a.shape[1] // s * s
    refs, bnds = [], []
    for top, left, sigma, noise, nid, gray in case_samples(s, k):
        v, nb = degrade(img, s, sigma, noise if noisy else (0.0, 0.0), nid, gray, top, left, PATCH)
        refs.append(v)
        bnds.append(bound(H, W, s, sigma, 1.0) + nb)
    ref, bnd = np.stack(refs), np.stack(bnds)
    ref.setflags(write=False)
    bnd.setflags(write=False)
    return ref, bnd
