"""fp64 restatement of srk_jpeg_roundtrip_f32 (include/srk.h, csrc/jpeg.hip) and the bounds its device test uses.

What is restated EXACTLY (same bits as the device, so no bound is needed):
  * the level step and both colour matrices.  Every operand there is an 8-bit level or an fp32 constant, every value a multiple of
    2^-27 below 2^10, so `fp64(a) * fp64(b) + fp64(c)` is exact and its one rounding to fp32 IS fmaf(a, b, c); numpy's fp32 multiply,
    divide and rint are IEEE like the device's.  The colour chain's bound is therefore 0: a pixel's three channels are decided as
    soon as its component values are.
  * the quantisation tables (integers) and c' = k Q.
What is bounded: the two 8-tap fp32 fmaf passes of the DCT against fp64 sums with the SAME fp32-rounded matrix D.  A chain of K
fused multiply-adds is off by at most K u sum|d||x| (u = 2^-24) to first order; two passes give (8 + 8) u S with S = |D| |x| |D|^T,
4 more units cover the level shift, the division / final add and the second-order terms, and the factor 2 is the margin of
tests/test_gpu_resize.py: bound = 2 (8 + 8 + 4) u S.
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

U = 2.0 ** -24
K_UNITS = 8 + 8 + 4

# ITU-T T.81 Annex K, tables K.1 and K.2, natural (row = vertical frequency) order
LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101,
                 72, 92, 95, 98, 112, 100, 103, 99], dtype=np.int64).reshape(8, 8)
CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99]
                  + [99] * 32, dtype=np.int64).reshape(8, 8)
ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])

VARIANTS = ("transposed_table", "chroma_table_on_y", "zigzag_table", "no_level_shift", "swap_cbcr", "anchor_1_0", "zero_pad")


def quant_table(base: np.ndarray, q: int, variant: str = "") -> np.ndarray:
    """libjpeg's jpeg_quality_scaling + jpeg_add_quant_table (baseline): int64 [8][8], natural order."""
    q = int(q)
    s = 5000 // q if q < 50 else 200 - 2 * q
    t = np.clip((base * s + 50) // 100, 1, 255)
    if variant == "transposed_table":
        t = t.T.copy()
    if variant == "zigzag_table":          # the file order of a DQT segment read as if it were natural order
        t = t.reshape(64)[ZIGZAG].reshape(8, 8)
    return t


def tables(q: int, variant: str = ""):
    luma = quant_table(CHROMA if variant == "chroma_table_on_y" else LUMA, q, variant)
    return luma, quant_table(CHROMA, q, variant)


def dct_matrix64() -> np.ndarray:
    u, k = np.arange(8)[:, None], np.arange(8)[None, :]
    d = 0.5 * np.cos((2 * k + 1) * u * np.pi / 16.0)
    d[0] *= 1.0 / np.sqrt(2.0)
    return d


D32 = dct_matrix64().astype(np.float32)          # the device's matrix
D = D32.astype(np.float64)


def fma32(a, b, c) -> np.ndarray:
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def _c(v: float) -> np.float32:
    return np.float32(v)


def level(x: np.ndarray) -> np.ndarray:
    """step 1, fp32: NaN -> 0"""
    x = np.asarray(x, np.float32)
    return np.rint(np.fmin(np.fmax(x, _c(0)), _c(1)) * _c(255)).astype(np.float32)


def _round8(v: np.ndarray) -> np.ndarray:
    return np.fmin(np.fmax(np.rint(np.asarray(v, np.float32)), _c(0)), _c(255))


def rgb_to_ycc(r, g, b, variant: str = ""):
    y = fma32(_c(0.114), b, fma32(_c(0.587), g, _c(0.299) * np.asarray(r, np.float32)))
    cb = fma32(_c(0.5), b, fma32(_c(-0.331264108), g, fma32(_c(-0.168735892), r, _c(128))))
    cr = fma32(_c(-0.081312411), b, fma32(_c(-0.418687589), g, fma32(_c(0.5), r, _c(128))))
    if variant == "swap_cbcr":
        cb, cr = cr, cb
    return _round8(y), _round8(cb), _round8(cr)


def ycc_to_rgb(y, cb, cr):
    cb, cr = np.asarray(cb, np.float32) - _c(128), np.asarray(cr, np.float32) - _c(128)
    r = fma32(_c(1.402), cr, y)
    g = fma32(_c(-0.714136286), cr, fma32(_c(-0.344136286), cb, y))
    b = fma32(_c(1.772), cb, y)
    return _round8(r), _round8(g), _round8(b)


def mcu_extent(n: int, mcu: int) -> int:
    return -(-n // mcu) * mcu


def _extend(p: np.ndarray, hm: int, wm: int, variant: str) -> np.ndarray:
    h, w = p.shape
    mode = "constant" if variant == "zero_pad" else "edge"
    return np.pad(p, ((0, hm - h), (0, wm - w)), mode=mode)


def _blocks(p: np.ndarray) -> np.ndarray:
    h, w = p.shape
    return p.reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3)


def _unblocks(b: np.ndarray) -> np.ndarray:
    nb, mb = b.shape[:2]
    return b.transpose(0, 2, 1, 3).reshape(nb * 8, mb * 8)


def half_distance(r: np.ndarray) -> np.ndarray:
    """distance of r from the nearest half-integer"""
    return np.abs(r - np.floor(r) - 0.5)


def forward(plane: np.ndarray, table: np.ndarray, variant: str = ""):
    """plane fp64 [8n][8m] of component values -> (k int64, decided bool), same layout (coefficient (u, v) of block (by, bx) at
    row 8 by + u, column 8 bx + v)."""
    x = _blocks(np.asarray(plane, np.float64)) - (0.0 if variant == "no_level_shift" else 128.0)
    c = np.einsum("uk,abkl,vl->abuv", D, x, D)
    s = np.einsum("uk,abkl,vl->abuv", np.abs(D), np.abs(x), np.abs(D))
    r = c / table
    decided = half_distance(r) > 2 * K_UNITS * U * s / table
    return _unblocks(np.rint(r).astype(np.int64)), _unblocks(decided)


def inverse(k: np.ndarray, table: np.ndarray):
    """k [8n][8m] -> (component values fp32 in 0..255, decided bool)"""
    c = _blocks(np.asarray(k, np.float64)) * table
    v = np.einsum("uy,abuv,vx->abyx", D, c, D) + 128.0
    s = np.einsum("uy,abuv,vx->abyx", np.abs(D), np.abs(c), np.abs(D)) + 128.0
    bound = 2 * K_UNITS * U * s
    decided = (half_distance(v) > bound) | (v - bound > 254.5) | (v + bound < 0.5)          # past the clamp either rounding gives 255 / 0
    # A block that keeps only its DC term decodes to 128 + k Q / 8 in real arithmetic: x.5 EXACTLY whenever k Q = 4 (mod 8) (q = 50:
    # 17 * 4 / 8 = 8.5; q = 5: 170 * 2 / 8 = 42.5), in every pixel of the block, and smooth images are full of such blocks.  No bound
    # decides them, but the device's arithmetic on them is restated bit for bit: every tap but the first multiplies a zero and
    # fmaf(d, 0, acc) = acc, so both passes are one fp32 product each: v = fl(fl(D00 fl(D00 c')) + 128).
    dc_only = (np.abs(c).reshape(c.shape[0], c.shape[1], 64)[:, :, 1:] == 0).all(axis=2)
    d00 = D32[0, 0]
    v_dc = (d00 * (d00 * c[:, :, 0, 0].astype(np.float32)) + _c(128)).astype(np.float32)
    assert v_dc.dtype == np.float32
    v = np.where(dc_only[:, :, None, None], v_dc.astype(np.float64)[:, :, None, None], v)
    decided = decided | dc_only[:, :, None, None]
    return _unblocks(np.clip(np.rint(v), 0, 255)).astype(np.float32), _unblocks(decided)


def roundtrip(x: np.ndarray, q: int, subsample: bool = False, coef: np.ndarray = None, variant: str = ""):
    """One sample x fp32 [C][H][W] at quality q (1..100; 0 = pass-through).  `coef` int [C][Hm][Wm]: decode these instead of the
    reference's own.  -> out fp32 [C][H][W], coef int16 [C][Hm][Wm], coef_valid / coef_decided bool [C][Hm][Wm], pix_decided [H][W]."""
    x = np.asarray(x, np.float32)
    C, H, W = x.shape
    sub = bool(subsample) and C == 3
    mcu = 16 if sub else 8
    if variant == "anchor_1_0":          # the grid one row lower: a replicated row on top, removed afterwards
        r = roundtrip(np.concatenate([x[:, :1], x], axis=1), q, subsample, None, "")
        return SimpleNamespace(out=r.out[:, 1:], pix_decided=r.pix_decided[1:], coef=None, coef_valid=None, coef_decided=None)
    hm, wm = mcu_extent(H, mcu), mcu_extent(W, mcu)
    valid = np.zeros((C, hm, wm), bool)
    if int(q) == 0:
        return SimpleNamespace(out=x.copy(), coef=np.zeros((C, hm, wm), np.int16), coef_valid=valid, coef_decided=valid.copy(),
                               pix_decided=np.ones((H, W), bool))
    q = min(max(int(q), 1), 100)
    tl, tc = tables(q, variant)
    p = level(x)
    comps = list(rgb_to_ycc(p[0], p[1], p[2], variant)) if C == 3 else [p[0]]
    ks = np.zeros((C, hm, wm), np.int64)
    decided = np.zeros((C, hm, wm), bool)
    for i, comp in enumerate(comps):
        e = _extend(comp.astype(np.float64), hm, wm, variant)
        if sub and i:
            e = (e[0::2, 0::2] + e[0::2, 1::2] + e[1::2, 0::2] + e[1::2, 1::2]) * 0.25
        k, d = forward(e, tc if i else tl, variant)
        hh, ww = k.shape
        ks[i, :hh, :ww], decided[i, :hh, :ww], valid[i, :hh, :ww] = k, d, True
    if coef is not None:
        ks = np.where(valid, np.asarray(coef, np.int64), 0)
    vals, pix = [], np.ones((hm, wm), bool)
    for i in range(C):
        hh, ww = (hm // 2, wm // 2) if (sub and i) else (hm, wm)
        v, d = inverse(ks[i, :hh, :ww], tc if i else tl)
        if sub and i:
            v, d = v.repeat(2, axis=0).repeat(2, axis=1), d.repeat(2, axis=0).repeat(2, axis=1)
        vals.append(v[:H, :W])
        pix &= d
    lev = np.stack(ycc_to_rgb(*vals)) if C == 3 else np.stack(vals)
    return SimpleNamespace(out=lev / _c(255), coef=ks.astype(np.int16), coef_valid=valid, coef_decided=decided & valid,
                           pix_decided=pix[:H, :W])


# ---- the inputs of the device test (and of the CPU test of its caps) ----------------------------------------------------------------

SHAPES = ((72, 72), (61, 45), (8, 8), (16, 16), (1, 1), (7, 130))
QUALITIES = (50, 0, 5, 100, 90)          # one per sample of the batch of five: per-sample indexing and the pass-through in one launch
SENTINEL = -32768                        # coef_out is pre-filled with it; no quantised coefficient reaches it (|k| <= 8 * 128)


def smooth_u8(rng, C, H, W):
    yy, xx = np.mgrid[0:H, 0:W]
    out = []
    for _ in range(C):
        a, b, c, d = rng.uniform(0.02, 0.25, 4)
        ph = rng.uniform(0, 6.28, 2)
        out.append(127.5 + 70 * np.sin(a * yy + b * xx + ph[0]) + 45 * np.cos(c * yy - d * xx + ph[1]) + rng.normal(0, 2.0, (H, W)))
    return np.clip(np.rint(np.stack(out)), 0, 255)


def make_batch(C: int, H: int, W: int, seed: int = 0) -> np.ndarray:
    """fp32 [5][C][H][W]: k / 255 images, smooth (even samples) and uniform noise (odd), ~3 % of the values replaced by off-grid floats,
    values outside [0, 1] and a few NaNs (step 1)."""
    rng = np.random.default_rng(1000003 * seed + 1009 * C + 31 * H + W)
    xs = []
    for b in range(5):
        lev = smooth_u8(rng, C, H, W) if b % 2 == 0 else rng.integers(0, 256, (C, H, W)).astype(np.float64)
        x = (lev.astype(np.float32) / _c(255)).astype(np.float32)
        pick = rng.random(x.shape)
        x = np.where(pick < 0.015, rng.uniform(0, 1, x.shape).astype(np.float32), x)
        x = np.where((pick >= 0.015) & (pick < 0.025), rng.uniform(-0.5, 1.5, x.shape).astype(np.float32), x)
        x = np.where((pick >= 0.025) & (pick < 0.03), np.float32(np.nan), x)
        xs.append(x.astype(np.float32))
    return np.stack(xs)


def cases():
    for (H, W) in SHAPES:
        for C in (1, 3):
            for sub in (0, 1):
                yield C, H, W, sub
