"""fp64 numpy restatement of the antialiased bicubic resampler (include/srk.h: srk_resize_aa_f32, srk_crop_degrade_u8): the Keys cubic
with a = -0.5 in the convention of PIL's Image.BICUBIC and F.interpolate(mode='bicubic', antialias=True, align_corners=False).
Pinned against both in tests/test_resize_ref.py; the reference of tests/test_gpu_resize.py.

`tables` takes the three choices that define the convention as arguments (a, whether the support widens with the scale, what happens to
taps outside the image) so that the CPU tests can show each of them matters; the defaults are the convention."""
import numpy as np

U = 2.0 ** -24          # unit roundoff of fp32


def cubic(x, a=-0.5):
    x = np.abs(np.asarray(x, dtype=np.float64))
    return np.where(x < 1.0, ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0,
                    np.where(x < 2.0, (((x - 5.0) * x + 8.0) * x - 4.0) * a, 0.0))


def tables(n_in, n_out, a=-0.5, widen=True, border="renorm"):
    """-> (lo [n_out] int, hi [n_out] int, weights: list of fp64 arrays).  border 'renorm': taps outside the image are dropped and the
    rest renormalised; 'clamp' (a negative control): they keep their weight and read the border pixel."""
    scale = n_in / n_out
    m = max(scale, 1.0) if widen else 1.0
    support, inv = 2.0 * m, 1.0 / m
    los, his, ws = [], [], []
    for i in range(n_out):
        c = scale * (i + 0.5)
        lo_raw, hi_raw = int(c - support + 0.5), int(c + support + 0.5)
        lo, hi = max(lo_raw, 0), min(hi_raw, n_in)
        if border == "renorm":
            w = cubic((np.arange(hi - lo) + lo - c + 0.5) * inv, a)
        else:
            lo_raw = int(np.floor(c - support + 0.5))
            full = cubic((np.arange(hi_raw - lo_raw) + lo_raw - c + 0.5) * inv, a)
            w = np.zeros(hi - lo)
            for j, v in zip(range(lo_raw, hi_raw), full):
                w[min(max(j, lo), hi - 1) - lo] += v
        los.append(lo)
        his.append(hi)
        ws.append(w / w.sum())
    return np.array(los), np.array(his), ws


def _pass(x, lo, hi, ws, rows=None):
    """One axis pass along the LAST axis: out[..., k] = sum_j w_j x[..., lo + j] for the outputs `rows` (all by default).  Every output is
    its own short sum, so a window of outputs has the bits of the same outputs of the whole axis."""
    rows = range(len(ws)) if rows is None else rows
    return np.stack([(x[..., lo[i]:hi[i]] * ws[i]).sum(axis=-1) for i in rows], axis=-1)


def resize(x, Ho, Wo, **kw):
    """x [..., H, W] (any float dtype) -> fp64 [..., Ho, Wo]: horizontal pass first, then the vertical pass."""
    x = np.asarray(x, dtype=np.float64)
    mid = _pass(x, *tables(x.shape[-1], Wo, **kw))
    return np.swapaxes(_pass(np.swapaxes(mid, -1, -2), *tables(x.shape[-2], Ho, **kw)), -1, -2)


def patch(img, top, left, P, s):
    """The LR patch of srk_crop_degrade_u8: img [..., H, W] (already in [0, 1]), (top, left) in HR pixels and multiples of s -> fp64
    [..., P, P], output rows top / s .. and columns left / s .. of the (H // s, W // s) downscale of the top-left (H - H % s, W - W % s)
    region, computed for the patch's outputs alone (no whole-image result is formed)."""
    img = np.asarray(img, dtype=np.float64)
    H, W = img.shape[-2:]
    reg = img[..., :H - H % s, :W - W % s]
    mid = _pass(reg, *tables(W - W % s, W // s), rows=range(left // s, left // s + P))
    return np.swapaxes(_pass(np.swapaxes(mid, -1, -2), *tables(H - H % s, H // s), rows=range(top // s, top // s + P)), -1, -2)


def quant8(v):
    """(float)rint(clamp(v, 0, 1) * 255) / 255.0f in fp32 arithmetic -> (fp32 values, integer levels)."""
    k = np.rint(np.clip(np.asarray(v, dtype=np.float32), np.float32(0), np.float32(1)) * np.float32(255))
    return (k / np.float32(255)).astype(np.float32), k.astype(np.int64)


def bound(H, W, Ho, Wo, max_abs):
    """The derived fp32 bound of the device result against this reference: 2 (Ky + Kx + 4) u Ly Lx max|x|.  K = the largest tap count
    and L = max sum |w| of each axis, from the tables; a K-term fp32 dot product errs by at most ~K u sum|w||x| (the project's 2 K u S
    rule keeps a factor 2), each weight carries one more rounding (fp64 -> fp32), the vertical pass amplifies the horizontal error by Ly."""
    _, _, wy = tables(H, Ho)
    _, _, wx = tables(W, Wo)
    ky, kx = max(len(w) for w in wy), max(len(w) for w in wx)
    ly, lx = max(np.abs(w).sum() for w in wy), max(np.abs(w).sum() for w in wx)
    return 2.0 * (ky + kx + 4) * U * ly * lx * max_abs


def nan_footprint(H, W, Ho, Wo, y, x):
    """Boolean [Ho, Wo]: the outputs whose footprint [lo, hi) contains input (y, x) on both axes."""
    loy, hiy, _ = tables(H, Ho)
    lox, hix, _ = tables(W, Wo)
    return np.outer((loy <= y) & (y < hiy), (lox <= x) & (x < hix))


def near_half(ref_unquantised, bnd):
    """Where 255 x the reference's unquantised value lies within 255 x bnd of a half-integer: there either neighbouring level passes."""
    v = 255.0 * np.clip(np.asarray(ref_unquantised, dtype=np.float64), 0.0, 1.0)
    return np.abs(v - np.floor(v) - 0.5) <= 255.0 * bnd


# ---- the cases tests/test_resize_ref.py (CPU) and tests/test_gpu_resize.py (device) share ------------------------------------------
# (B, C, H, W, Ho, Wo)
CASES = [(1, 1, 1, 1, 1, 1),
         (1, 1, 4, 4, 1, 1),
         (1, 1, 8, 8, 2, 2),            # every output is a border output
         (2, 3, 13, 18, 6, 9),
         (1, 3, 33, 47, 16, 23),
         (1, 1, 64, 72, 16, 18),
         (1, 3, 20, 20, 7, 3),
         (2, 1, 7, 5, 14, 10),
         (1, 1, 13, 9, 52, 36),
         (1, 1, 3, 700, 3, 175),        # crosses block edges in x
         (1, 1, 260, 5, 65, 5),         # crosses block edges in y
         (1, 3, 11, 11, 11, 11)]        # identity
CASE_IDS = ["x".join(map(str, c[:4])) + "-to-" + "x".join(map(str, c[4:])) for c in CASES]
QUANT_CASES = [3, 4, 5, 9]              # indices into CASES run with quant_bits = 8
SCALES = (2, 3, 4)
PATCH = 8                               # LR patch of the srk_crop_degrade_u8 cases


def case_input(idx, lo=0.0, hi=1.0):
    """The fp32 input of CASES[idx], uniform in [lo, hi): one seed per case."""
    B, C, H, W = CASES[idx][:4]
    return (np.random.RandomState(100 + idx).rand(B, C, H, W) * (hi - lo) + lo).astype(np.float32)


def pool_images(s):
    """The four images of the srk_crop_degrade_u8 cases at factor s: gray u8 37 x 45 (not a multiple of the factor), RGB u8 64 x 48, gray
    u16 40 x 40, and an RGB u8 image that is exactly one patch (every tap truncated)."""
    rng = np.random.RandomState(200 + s)
    return [rng.randint(0, 256, (37, 45)).astype(np.uint8), rng.randint(0, 256, (64, 48, 3)).astype(np.uint8),
            rng.randint(0, 65536, (40, 40)).astype(np.uint16), rng.randint(0, 256, (PATCH * s, PATCH * s, 3)).astype(np.uint8)]


def pool_positions(imgs, s, P=PATCH):
    """[(image, top, left)] in HR pixels: the four corners and one interior position of the first three images, the whole fourth image."""
    pos = []
    for k, a in enumerate(imgs[:3]):
        mt, ml = a.shape[0] // s - P, a.shape[1] // s - P
        pos += [(k, 0, 0), (k, 0, ml * s), (k, mt * s, 0), (k, mt * s, ml * s), (k, (mt // 2) * s, ((ml + 1) // 2) * s)]
    return pos + [(3, 0, 0)]


def to_unit3(a):
    """uint8 / uint16 [H,W] or [H,W,3] -> fp32 [3,H,W] in [0, 1] as the device converts it (u8 / 255, u16 / 65535 in fp32; gray repeated)."""
    v = a.astype(np.float32) / np.float32(65535.0 if a.dtype == np.uint16 else 255.0)
    return np.repeat(v[None], 3, axis=0) if v.ndim == 2 else np.ascontiguousarray(v.transpose(2, 0, 1))
