"""fp64 / bit-level numpy restatement of the scale-1 restoration pairs (include/srk.h: srk_noise_f32, srk_crop_restore_u8).

It imports, and does not restate, the Philox / Box-Muller noise of tests/degrade_ref.py (`normal_field`, `add_noise`) and the JPEG
round trip of tests/jpeg_ref.py (`roundtrip`, with its decided / undecided rules).  What it adds is the integer luma and the window
rule: the degraded patch is the window at (top, left) of jpeg_roundtrip(noise(convert(whole image))) -- noise keyed on image
coordinates, blocks anchored at the image's (0, 0), the image extended by replication.  Pinned in tests/test_restore_ref.py (known
answers, negative controls); the reference of tests/test_gpu_restore.py.  `chain(..., variant=)` builds the negative controls."""
import functools

import numpy as np

import degrade_ref as D
import jpeg_ref as J

LUMA = (4899, 9617, 1868)          # / 16384
VARIANTS = ("patch_blocks", "patch_noise", "float_luma", "zero_pad", "noise_after_jpeg")


def luma(a, variant=""):
    """[..., 3] uint8 / uint16 stored samples -> [...] of the same dtype: (4899 R + 9617 G + 1868 B + 8192) >> 14."""
    a = np.asarray(a)
    assert a.dtype in (np.uint8, np.uint16) and a.shape[-1] == 3
    if variant == "float_luma":          # a negative control: rounded float coefficients
        return np.rint(0.299 * a[..., 0] + 0.587 * a[..., 1] + 0.114 * a[..., 2]).astype(a.dtype)
    v = a.astype(np.int64)
    return ((LUMA[0] * v[..., 0] + LUMA[1] * v[..., 1] + LUMA[2] * v[..., 2] + 8192) >> 14).astype(a.dtype)


def convert(a, out_chans, variant=""):
    """uint8 / uint16 [H,W] or [H,W,3] -> the CODED planes fp32 [Cc,H,W] in [0, 1], Cc = 3 for an RGB source at out_chans 3, else 1 (a
    gray source, or the luma of an RGB source at out_chans 1); u8 / 255, u16 / 65535 in fp32."""
    a = np.asarray(a)
    if a.ndim == 3 and a.shape[2] == 1:
        a = a[:, :, 0]
    if a.ndim == 3 and out_chans == 1:
        a = luma(a, variant)
    v = a.astype(np.float32) / np.float32(65535.0 if a.dtype == np.uint16 else 255.0)
    return v[None] if v.ndim == 2 else np.ascontiguousarray(v.transpose(2, 0, 1))


def expand(x, out_chans):
    """coded planes [Cc,...] -> [out_chans,...]: one plane is written out_chans times."""
    return x if x.shape[0] == out_chans else np.repeat(x, out_chans, axis=0)


def noised(img, sigma, noise_id, gray, y0=0, x0=0):
    """img [C,h,w] (fp32 values) whose pixel (0, 0) is image pixel (y0, x0) -> (fp64 unquantised noised values, bound per element).
    The bound is the 7k noise term C_NOISE u (r + |z|) std plus 4 u (|v| + std |z|): the device rounds the sum once (u of the result)
    and std three times (product, sum, root: <= 2.5 u relative), and the reference's v is the device's fp32 v exactly."""
    v = np.asarray(img, np.float64)
    C, h, w = v.shape
    if D.f32(sigma) == 0.0:
        return v, np.zeros_like(v)
    z, r = D.normal_field(C, y0, x0, h, w, noise_id, gray or C == 1)
    std = D.noise_std(v, sigma, 0.0)
    return D.add_noise(v, z, sigma, 0.0), D.C_NOISE * D.U * (r + np.abs(z)) * std + 4.0 * D.U * (np.abs(v) + std * np.abs(z))


def chain(a, out_chans, sigma, noise_id, gray, quality, subsample=False, quant_bits=0, variant="", window=None):
    """The degraded image [out_chans,H,W] fp32 of the whole-image chain (window None), or its negative controls on the window
    (top, left, P): 'patch_blocks' = the chain's JPEG stage run on the noised patch (blocks anchored at the patch); 'patch_noise' =
    noise keyed on patch coordinates; 'zero_pad' = zero padding in place of replication; 'noise_after_jpeg'; 'float_luma'."""
    x = convert(a, out_chans, variant)
    y0 = x0 = 0
    if window is not None and variant in ("patch_blocks", "patch_noise"):
        top, left, P = window
        x = x[:, top:top + P, left:left + P]
        y0, x0 = (top, left) if variant == "patch_blocks" else (0, 0)
    q8 = (lambda v: D.quant8(v)[0]) if quant_bits == 8 else (lambda v: np.asarray(v, np.float32))
    if variant == "noise_after_jpeg":
        y = J.roundtrip(x, quality, subsample).out
        y = q8(noised(y, sigma, noise_id, gray)[0])
    else:
        y = q8(noised(x, sigma, noise_id, gray, y0, x0)[0])
        y = J.roundtrip(y, quality, subsample, variant="zero_pad" if variant == "zero_pad" else "").out
    y = expand(np.asarray(y, np.float32), out_chans)
    if window is not None and variant not in ("patch_blocks", "patch_noise"):
        top, left, P = window
        y = y[:, top:top + P, left:left + P]
    return y


# ---- the cases tests/test_restore_ref.py (CPU: the cap) and tests/test_gpu_restore.py (device) share ---------------------------------
QUALITIES = (50, 0, 5, 100, 90)
SOURCES = (("rgb8", 45, 61), ("gray8", 40, 72), ("rgb16", 33, 50))          # nothing is a multiple of 16
NOISE_ID0 = 0x9E3779B97F4A7C15          # bit 63 set: the id travels as a signed 64-bit integer
SIGMA = 10.0 / 255.0


def case_image(k):
    kind, H, W = SOURCES[k]
    rng = np.random.default_rng(700 + k)
    C = 3 if kind.startswith("rgb") else 1
    lev = J.smooth_u8(rng, C, H, W)          # smooth: blocks that keep few coefficients, as photographs have
    if kind == "rgb16":
        a = np.clip(np.rint(lev * 257.0 + rng.integers(-128, 129, lev.shape)), 0, 65535).astype(np.uint16)
    else:
        a = lev.astype(np.uint8)
    return np.ascontiguousarray(a.transpose(1, 2, 0)) if C == 3 else a[0]


def offsets(k, P):
    """(top, left) x 5: the corner, the far corner (the replicated edge), an odd phase, an aligned one, and one inside."""
    _, H, W = SOURCES[k]
    far = (H - P, W - P)
    return [(0, 0), far, (min(3, far[0]), min(5, far[1])), (min(8, far[0]), min(16, far[1])), (min(13, far[0]), min(7, far[1]))]


@functools.lru_cache(maxsize=None)
def noise_reference(k, out_chans, gray):
    """(fp64 unquantised noised coded planes [5][Cc][H][W], bound) of image k, one noise id per sample of the batch; shared, read-only."""
    x = convert(case_image(k), out_chans)
    vs, bs = zip(*(noised(x, SIGMA, NOISE_ID0 + 7 * b + k, gray) for b in range(5)))
    v, b = np.stack(vs), np.stack(bs)
    v.setflags(write=False)
    b.setflags(write=False)
    return v, b
