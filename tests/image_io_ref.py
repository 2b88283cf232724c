"""A numpy restatement of srk_image_unpack / srk_image_pack (include/srk.h, csrc/image_io.hip) that imports nothing from the package.

unpack_ref: interleaved uint8 / uint16 [B][H][W][ch] -> planar fp32 [B][out_chans][H][W] (+ alpha [B][1][H][W]).
pack_ref:   planar fp32 [B][C][H][W] (+ alpha) -> interleaved samples [B][H][W][out_chans] and the two counts.
The `variant` arguments are the negative controls of tests/test_image_io_ref.py: each is a plausible wrong convention.
"""
import numpy as np

LUMA = (4899, 9617, 1868)          # / 16384, + 8192 >> 14: ops.to_gray


def luma(r, g, b):
    r, g, b = (np.asarray(v).astype(np.uint64) for v in (r, g, b))
    return ((LUMA[0] * r + LUMA[1] * g + LUMA[2] * b + 8192) >> 14).astype(np.uint32)


def unpack_ref(a, out_chans, want_alpha=False, variant=None):
    """variant: None | 'swap_rb' | 'alpha_slot0' (alpha of a 2-sample pixel taken from sample 0, gray from sample 1)."""
    a = np.asarray(a)
    assert a.dtype in (np.uint8, np.uint16) and a.ndim == 4 and 1 <= a.shape[3] <= 4 and out_chans in (1, 3)
    ch = a.shape[3]
    mx = np.float32(255.0 if a.dtype == np.uint8 else 65535.0)
    s = a.astype(np.uint32)
    gray_slot, alpha_slot = (1, 0) if (variant == "alpha_slot0" and ch == 2) else (0, ch - 1)
    if ch <= 2:
        planes = [s[..., gray_slot]] * out_chans
    else:
        r, g, b = (s[..., 2], s[..., 1], s[..., 0]) if variant == "swap_rb" else (s[..., 0], s[..., 1], s[..., 2])
        planes = [r, g, b] if out_chans == 3 else [luma(r, g, b)]
    x = np.stack(planes, 1).astype(np.float32) / mx                        # one IEEE fp32 division
    alpha = None
    if want_alpha and ch in (2, 4):
        alpha = (s[..., alpha_slot].astype(np.float32) / mx)[:, None]
    return np.ascontiguousarray(x), alpha


def quantise(v, mx, variant=None):
    """q(v): NaN -> 0, v <= 0 -> 0, v >= 1 -> max, else rint(fp32(v) * fp32(max)).  variant 'trunc' | 'half_up' replace the rint."""
    v = np.asarray(v, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        p = v * np.float32(mx)                                                # the fp32 product
        if variant == "trunc":
            r = np.trunc(p)
        elif variant == "half_up":
            r = np.floor(p.astype(np.float64) + 0.5)
        else:
            r = np.rint(p)                                                    # round-half-to-even
        r = np.where(v >= 1, np.float32(mx), r)
        r = np.where(v > 0, r, 0)                                             # NaN, -0.0, negatives and -Inf fail `v > 0`
    return r.astype(np.uint32)


def count_ref(*arrays):
    """(non-finite values, finite values outside [0, 1]) over the arrays."""
    nf = cl = 0
    for v in arrays:
        v = np.asarray(v, dtype=np.float32)
        fin = np.isfinite(v)
        nf += int((~fin).sum())
        with np.errstate(invalid="ignore"):
            cl += int((fin & ((v < 0) | (v > 1))).sum())
    return nf, cl


def pack_ref(y, alpha=None, out_chans=None, bits=8, variant=None):
    """-> (samples [B][H][W][out_chans], (non-finite, clipped)).  variant: None | 'trunc' | 'half_up' | 'luma_first' (the luma of the
    fp32 values, quantised afterwards) | 'swap_rb' | 'no_alpha' (alpha written as opaque)."""
    y = np.asarray(y, dtype=np.float32)
    assert y.ndim == 4 and y.shape[1] in (1, 3) and bits in (8, 16)
    C = y.shape[1]
    if out_chans is None:
        out_chans = C + (alpha is not None)
    assert out_chans in (1, 2, 3, 4) and (out_chans % 2 == 1 or alpha is not None)
    mx = 255 if bits == 8 else 65535
    rv = variant if variant in ("trunc", "half_up") else None
    q = quantise(y, mx, rv)
    if out_chans <= 2:
        if C == 3 and variant == "luma_first":
            yl = (np.float32(LUMA[0]) * y[:, 0] + np.float32(LUMA[1]) * y[:, 1] + np.float32(LUMA[2]) * y[:, 2]) / np.float32(16384.0)
            chans = [quantise(yl, mx)]
        else:
            chans = [luma(q[:, 0], q[:, 1], q[:, 2]) if C == 3 else q[:, 0]]
    else:
        order = (2, 1, 0) if variant == "swap_rb" else (0, 1, 2)
        chans = [q[:, c if C == 3 else 0] for c in order]
    counted = [y]
    if out_chans % 2 == 0:
        a = np.asarray(alpha, dtype=np.float32)
        counted.append(a)
        chans.append(np.full_like(chans[0], mx) if variant == "no_alpha" else quantise(a, mx, rv)[:, 0])
    out = np.stack(chans, -1).astype(np.uint8 if bits == 8 else np.uint16)
    return np.ascontiguousarray(out), count_ref(*counted)


def specials():
    """The planted pack inputs: NaN, +-Inf, -0.0, 1 + ulp, -ulp (the smallest negative), and exact 0 / 1."""
    one_up = np.nextafter(np.float32(1.0), np.float32(2.0))
    neg_tiny = -np.nextafter(np.float32(0.0), np.float32(1.0))
    return np.array([np.nan, np.inf, -np.inf, -0.0, one_up, neg_tiny, 0.0, 1.0], dtype=np.float32)


def ties(bits, limit=64):
    """fp32 v in (0, 1) whose fp32 product v * max is exactly k + 0.5, found by search: for each k the fp32 neighbours of (k + 0.5) / max
    are tried.  -> (v array, k array), at most `limit` of them, even and odd k alternating where both exist."""
    mx = np.float32(255.0 if bits == 8 else 65535.0)
    found = {0: [], 1: []}
    kmax = 255 if bits == 8 else 65535
    for k in range(kmax):
        target = np.float32(k + 0.5)
        c = np.float32(np.float64(k + 0.5) / np.float64(mx))
        for v in (c, np.nextafter(c, np.float32(0)), np.nextafter(c, np.float32(1))):
            if np.float32(v * mx) == target and 0 < v < 1:
                found[k & 1].append((v, k))
                break
        if min(len(found[0]), len(found[1])) >= limit // 2:
            break
    both = [p for pair in zip(found[0], found[1]) for p in pair] or found[0] + found[1]
    both = both[:limit]
    return np.array([p[0] for p in both], dtype=np.float32), np.array([p[1] for p in both], dtype=np.int64)
