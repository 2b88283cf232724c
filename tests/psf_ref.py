"""fp64 numpy restatement of the general 2-D blur (include/srk.h: srk_blur2d_f32, srk_crop_degrade_psf_u8): a ks x ks table applied as a
CORRELATION with taps outside the image dropped and the rest renormalised per blurred pixel, then the antialiased bicubic downscale of
tests/resize_ref.py on the blurred region and the noise of tests/degrade_ref.py.  Pinned in tests/test_psf_ref.py (F.conv2d on fp64
tensors, closed forms, the separable operator of degrade_ref in the interior); the reference of tests/test_gpu_psf.py.

Bit rule of a delta table.  With K zero except K[R][R] = k, the device's chains are num = fmaf(k, x, 0) = fl(k x) (every other tap adds
k' x' = 0 exactly) and mass = fl(k): the output is fl(fl(k x) / k).  For k == 1 that is x bit for bit -- at any ks, so a delta padded to 21
is the same copy -- and srk_crop_degrade_psf_u8 without noise then has the bits of srk_crop_degrade_u8.  For k != 1 it is x up to the two
roundings of x * k / k, not a copy.

Error bounds (derived; u = 2^-24, n = ks^2 of the table before any zero padding -- a zero tap adds nothing, exactly):
  blur:    |err| <= 2 (2 n + 2) u S / m,  S = sum K |x| over the in-image taps, m = the mass.  An n-term fmaf chain errs by at most
           n u S (n u m for the mass), the division adds one rounding; the project's rule keeps a factor 2.
  resize:  Ly Lx max(blur bound) + 2 (Ky + Kx + 4) u Ly Lx max|blurred|, K / L the largest tap count / sum |w| of the cubic tables:
           the two passes carry the blur's error through at most Ly Lx, and add resize_ref.bound on the blurred values.
  noise:   degrade_ref's term C_NOISE u (r + |z|) std per element."""
import functools

import numpy as np

import degrade_ref as D
import resize_ref as R

U = R.U
KS_MAX = 21


# ---- tables ------------------------------------------------------------------------------------------------------------------------------
def quad_form(ks, s1, s2, theta):
    """q^T Sigma^-1 q on the integer grid, q = (x, y) with x along columns and y along rows, Sigma = Rot(theta) diag(s1^2, s2^2) Rot(theta)^T,
    written out element by element (no matrix inverse): u = cos x + sin y, v = -sin x + cos y, (u / s1)^2 + (v / s2)^2."""
    r = (ks - 1) // 2
    out = np.empty((ks, ks), dtype=np.float64)
    c, s = np.cos(theta), np.sin(theta)
    for a in range(ks):
        for b in range(ks):
            x, y = float(b - r), float(a - r)
            u, v = c * x + s * y, -s * x + c * y
            out[a, b] = (u / s1) ** 2 + (v / s2) ** 2
    return out


def kernel(kind, ks, s1, s2, theta, beta=1.0):
    """'gaussian' exp(-q/2), 'generalized' exp(-q^beta / 2), 'plateau' 1 / (q^beta + 1): normalised in fp64, rounded once to fp32."""
    q = quad_form(ks, s1, s2, theta)
    k = {"gaussian": lambda: np.exp(-0.5 * q), "generalized": lambda: np.exp(-0.5 * q ** beta), "plateau": lambda: 1.0 / (q ** beta + 1.0)}[kind]()
    return (k / k.sum()).astype(np.float32)


def pad_to(K, ks):
    """K zero-padded, centred, to ks x ks."""
    K = np.asarray(K)
    p = (ks - K.shape[0]) // 2
    assert K.shape[0] == K.shape[1] and K.shape[0] % 2 == 1 and ks % 2 == 1 and p >= 0
    return np.pad(K, p)


def delta(ks, k=1.0):
    K = np.zeros((ks, ks), dtype=np.float32)
    K[ks // 2, ks // 2] = k
    return K


# ---- the blur ----------------------------------------------------------------------------------------------------------------------------
def _sums(x, K, rows, cols):
    """(num, mass) for the pixels rows x cols of x [..., H, W]: correlation on the zero-padded image, and the same with x == 1."""
    K = np.asarray(K, dtype=np.float64)
    ks = K.shape[0]
    r = (ks - 1) // 2
    H, W = x.shape[-2:]
    xp = np.zeros(x.shape[:-2] + (H + 2 * r, W + 2 * r), dtype=np.float64)
    xp[..., r:r + H, r:r + W] = x
    op = np.zeros((H + 2 * r, W + 2 * r), dtype=np.float64)
    op[r:r + H, r:r + W] = 1.0
    (ra, rb), (ca, cb) = rows, cols
    num = np.zeros(x.shape[:-2] + (rb - ra, cb - ca), dtype=np.float64)
    mass = np.zeros((rb - ra, cb - ca), dtype=np.float64)
    finite = bool(np.isfinite(x).all())          # a zero tap of a NaN still gives NaN, on the device too
    for a in range(ks):
        for b in range(ks):
            if K[a, b] == 0.0 and finite:
                continue
            num += K[a, b] * xp[..., ra + a:rb + a, ca + b:cb + b]          # xp index (p + a) <-> image row p + a - R
            mass += K[a, b] * op[ra + a:rb + a, ca + b:cb + b]
    return num, mass


def blur2d(x, K, rows=None, cols=None, flip=False, renorm=True):
    """x [..., H, W] -> fp64 blurred = num / mass, for all pixels or for the half-open ranges rows = (ra, rb), cols = (ca, cb) alone.
    Negative controls: flip -- a convolution (the table turned by 180 degrees); renorm False -- zero padding without the division."""
    x = np.asarray(x, dtype=np.float64)
    K = np.asarray(K, dtype=np.float64)
    H, W = x.shape[-2:]
    num, mass = _sums(x, K[::-1, ::-1] if flip else K, rows or (0, H), cols or (0, W))
    return num / mass if renorm else num


def blur_bound(x, K, rows=None, cols=None):
    """2 (2 n + 2) u S / m per pixel (module docstring); n counts the table before zero padding: the smallest centred square holding its
    non-zero taps."""
    K = np.asarray(K, dtype=np.float64)
    r = (K.shape[0] - 1) // 2
    nz = np.argwhere(K != 0.0)
    rr = int(np.abs(nz - r).max()) if len(nz) else 0
    n = (2 * rr + 1) ** 2
    x = np.asarray(x, dtype=np.float64)
    H, W = x.shape[-2:]
    num, mass = _sums(np.abs(x), np.abs(K), rows or (0, H), cols or (0, W))
    return 2.0 * (2 * n + 2) * U * num / mass


# ---- the degradation ---------------------------------------------------------------------------------------------------------------------
def _spans(n_in, n_out, outs):
    """The input range [lo, hi) under the outputs `outs` (a range) of the cubic tables."""
    lo, hi, _ = R.tables(n_in, n_out)
    return int(lo[outs[0]]), int(hi[outs[-1]])


def filtered(img, s, K, top=0, left=0, P=None, region=True):
    """img [..., H, W] -> (v, bnd): the unquantised, noise-free fp64 LR -- rows top / s .. and columns left / s .. (P of each; everything
    when P is None) of the (H // s, W // s) cubic downscale of the blurred top-left (H - H % s, W - W % s) region -- and the bound of the
    device against it (one number: module docstring).  Only the blurred pixels under those outputs are computed.
    region False (a negative control): the blur is bounded by the whole image instead of the region."""
    img = np.asarray(img, dtype=np.float64)
    H, W = img.shape[-2:]
    Hr, Wr = H - H % s, W - W % s
    rows = range(top // s, top // s + P) if P else range(H // s)
    cols = range(left // s, left // s + P) if P else range(W // s)
    (ra, rb), (ca, cb) = _spans(Hr, H // s, rows), _spans(Wr, W // s, cols)
    src = img[..., :Hr, :Wr] if region else img
    bl = np.zeros(img.shape[:-2] + (Hr, Wr), dtype=np.float64)
    bl[..., ra:rb, ca:cb] = blur2d(src, K, (ra, rb), (ca, cb))
    bb = blur_bound(src, K, (ra, rb), (ca, cb)).max()
    mid = R._pass(bl, *R.tables(Wr, W // s), rows=cols)
    v = np.swapaxes(R._pass(np.swapaxes(mid, -1, -2), *R.tables(Hr, H // s), rows=rows), -1, -2)
    _, _, wy = R.tables(Hr, H // s)
    _, _, wx = R.tables(Wr, W // s)
    ky, kx = max(len(wy[i]) for i in rows), max(len(wx[i]) for i in cols)
    ly, lx = max(np.abs(wy[i]).sum() for i in rows), max(np.abs(wx[i]).sum() for i in cols)
    bnd = ly * lx * bb + 2.0 * (ky + kx + 4) * U * ly * lx * np.abs(bl[..., ra:rb, ca:cb]).max()
    return v, bnd


def degrade(img, s, K, noise=(0.0, 0.0), noise_id=0, gray=False, top=0, left=0, P=None):
    """-> (lr, bound per element): filtered() plus degrade_ref's noise on whole-image LR coordinates and its bound term."""
    v, bnd = filtered(img, s, K, top, left, P)
    return add_noise(v, bnd, s, noise, noise_id, gray, top, left)


def add_noise(v, bnd, s, noise, noise_id, gray, top=0, left=0):
    C, Ph, Pw = v.shape
    if D.f32(noise[0]) == 0.0 and D.f32(noise[1]) == 0.0:
        return v, np.full_like(v, bnd)
    z, r = D.normal_field(C, top // s, left // s, Ph, Pw, noise_id, gray or C == 1)
    return D.add_noise(v, z, *noise), bnd + D.C_NOISE * U * (r + np.abs(z)) * D.noise_std(v, *noise)


def nan_footprint(H, W, s, ks, y, x):
    """Boolean [H // s, W // s]: the outputs whose cubic footprint, dilated by the ks x ks window, contains input (y, x)."""
    r = (ks - 1) // 2
    loy, hiy, _ = R.tables(H, H // s)
    lox, hix, _ = R.tables(W, W // s)
    return np.outer((loy - r <= y) & (y < hiy + r), (lox - r <= x) & (x < hix + r))


near_half = R.near_half
quant8 = R.quant8
to_unit3 = R.to_unit3


def pack(noise, noise_id, gray):
    """Slots 6..9 of a descriptor: slot 6 (the sigma pair of the separable entry) is reserved and left 0."""
    return D.pack((0.0, 0.0), noise, noise_id, gray)


# ---- the cases tests/test_psf_ref.py (CPU: the cap on undecided levels) and tests/test_gpu_psf.py (device) share -------------------------
SCALES = D.SCALES
PATCH = D.PATCH                          # 72: two column tiles (64 + 8, one ragged) and nine row tiles
SOURCES = D.SOURCES
NOISES = D.NOISES                        # sigma_n > 0 in every one
GRAYS = D.GRAYS
NOISE_ID0 = D.NOISE_ID0
# The images are dim: levels 0..31 of 255 (0..8191 of 65535).  The blur bound is RELATIVE, 2 (2 n + 2) u S / m with n = 441 at ks 21, i.e.
# 1.05e-4 of the local mean; a quantised output is undecided within 255 x bound of a half-integer on either side, so a full-range image
# (mean 0.5) would leave 510 x 1.05e-4 x 0.5 x Ly Lx = 3.5 % of a ks-21 sample undecided, above the 1 % cap.  At a mean of 1 / 16 it is
# 0.45 %.  The relative accuracy asked of the kernel is the same.
LEVELS8, LEVELS16 = 32, 8192


def case_image(s, k):
    """HR image k of factor s: LR extents PATCH + 9 and PATCH + 14 -- a patch on each border and one inside -- plus s - 1 remainder rows
    (H % s != 0) that hold the LARGEST level: a blur bounded by the image instead of the region shows at the bottom border."""
    rng = np.random.RandomState(700 + 10 * s + k)
    h, w = (PATCH + 9) * s + (s - 1), (PATCH + 14) * s
    if SOURCES[k] == "gray8":
        a = rng.randint(0, LEVELS8, (h, w)).astype(np.uint8)
    elif SOURCES[k] == "rgb8":
        a = rng.randint(0, LEVELS8, (h, w, 3)).astype(np.uint8)
    else:
        a = rng.randint(0, LEVELS16, (h, w)).astype(np.uint16)
    a[h - (s - 1):] = 255 if a.dtype == np.uint8 else 65535
    return a


def case_tables(s, k):
    """Five tables, ks 3 / 7 / 21 / 7 / 3 before padding: a random one, a rotated Gaussian, a rotated plateau, a rotated generalized
    Gaussian, a random one again.  The generated ones are multiplied tap by tap with a random factor in [0.5, 1.5): a rotated kernel alone is
    symmetric under a half turn, and a convolution in place of the correlation would pass on it."""
    rng = np.random.RandomState(900 + 10 * s + k)

    def rand(ks):
        t = rng.rand(ks, ks) + 0.05
        return (t / t.sum()).astype(np.float32)

    def skewed(t):
        t = t.astype(np.float64) * (0.5 + rng.rand(*t.shape))
        return (t / t.sum()).astype(np.float32)

    return [rand(3), skewed(kernel("gaussian", 7, 2.0, 0.7, 0.5 + 0.1 * k)), skewed(kernel("plateau", 21, 3.0, 1.5, -1.0 + 0.2 * s, 1.5)),
            skewed(kernel("generalized", 7, 1.1, 2.3, -0.6, 1.7)), rand(3)]


def case_samples(s, k):
    """[(top, left, table, noise, noise_id, gray)] x 5: the four corners and an interior position."""
    a = case_image(s, k)
    mt, ml = a.shape[0] // s - PATCH, a.shape[1] // s - PATCH
    pos = [(0, 0), (0, ml * s), (mt * s, 0), (mt * s, ml * s), ((mt // 2) * s, ((ml + 1) // 2) * s)]
    tabs = case_tables(s, k)
    return [(top, left, tabs[(b + k) % 5], NOISES[(b + k) % 5], NOISE_ID0 + 7 * b + k, GRAYS[b] or a.ndim == 2) for b, (top, left) in enumerate(pos)]


@functools.lru_cache(maxsize=None)
def case_filtered(s, k):
    """[(v [C', P, P], bnd)] per sample, noise-free, computed once; a gray source is computed on one channel."""
    a = case_image(s, k)
    img = to_unit3(a)[:1] if a.ndim == 2 else to_unit3(a)
    return [filtered(img, s, K, top, left, PATCH) for top, left, K, *_ in case_samples(s, k)]


@functools.lru_cache(maxsize=None)
def case_reference(s, k, noisy):
    """(ref [5, 3, P, P] fp64 unquantised, bnd [5, 3, P, P]) of case (s, k), computed once and shared."""
    refs, bnds = [], []
    for (v, bnd), (top, left, _, noise, nid, gray) in zip(case_filtered(s, k), case_samples(s, k)):
        v = np.repeat(v, 3, axis=0) if v.shape[0] == 1 else v
        v, b = add_noise(v, bnd, s, noise if noisy else (0.0, 0.0), nid, gray or case_image(s, k).ndim == 2, top, left)
        refs.append(v)
        bnds.append(b)
    ref, bnd = np.stack(refs), np.stack(bnds)
    ref.setflags(write=False)
    bnd.setflags(write=False)
    return ref, bnd
