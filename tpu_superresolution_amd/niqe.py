"""No-reference quality: NIQE (Mittal et al., "Making a completely blind image quality analyzer") in the form of BasicSR's
`calculate_niqe` -- the score the Real-ESRGAN / BSRGAN / SwinIR real-SR papers print for files without ground truth.  Restated from the
published algorithm, **parity unpinned** (include/srk.h "No-reference quality (NIQE)").

    python -m tpu_superresolution_amd.niqe fit   --input DIR --out F.npz [--sharpness 0.75] [--crop_border N]
    python -m tpu_superresolution_amd.niqe score --input FILE|DIR --params F.npz [--crop_border N] [--batch_size N] [--device D]

`fit` estimates the 36-dimensional Gaussian of pristine images (the HR training directory) and writes BasicSR's `niqe_pris_params.npz`
format: `mu_pris_param [1,36]`, `cov_pris_param [36,36]`, `gaussian_window [7,7]` (fspecial('gaussian', 7, 7/6)); the published file can be
dropped in.  `score` prints `[niqe] <name> <score>` per file and `[done] n images | mean`; lower is better.

The device computes the four stages of csrc/niqe.hip on fp32 CUDA tensors (`niqe_moments`: one plane launch, one half-size launch, two
MSCN launches, two moments launches, one download); a CPU tensor takes the numpy form of the same definition.  From the block moments on,
everything is host fp64: `niqe_features` (AGGD moment matching on BasicSR's grid), `niqe_distance`, `niqe`, `niqe_fit`.
"""
from __future__ import annotations

import argparse
import math
import numbers
from pathlib import Path
from typing import Iterable, Optional, Tuple

import numpy as np
import torch

NIQE_BLOCK = 96          # the published block side
NIQE_KEYS = ("mu_pris_param", "cov_pris_param", "gaussian_window")
HALF_TAPS = (-3, -9, 29, 111, 111, 29, -9, -3)          # / 256: antialiased cubic (a = -0.5) at scale 1/2


def niqe_window() -> np.ndarray:
    """fspecial('gaussian', 7, 7/6), normalised in fp64 -> [7, 7]."""
    r = np.arange(-3, 4, dtype=np.float64)
    g = np.exp(-(r[:, None] ** 2 + r[None, :] ** 2) / (2.0 * (7.0 / 6.0) ** 2))
    return g / g.sum()


# ---- the parameter file ---------------------------------------------------------------------------------------------------------------
def check_niqe_params(mu, cov, window, what: str = "niqe parameters") -> dict:
    """-> {'mu' [36], 'cov' [36,36], 'window' [7,7]} in fp64; ValueError for wrong shapes, non-finite values or an asymmetric covariance."""
    mu, cov, window = (np.asarray(v, dtype=np.float64) for v in (mu, cov, window))
    if mu.size != 36 or mu.ndim > 2 or cov.shape != (36, 36) or window.shape != (7, 7):
        raise ValueError(f"{what}: expected mu_pris_param [1,36], cov_pris_param [36,36], gaussian_window [7,7] "
                         f"(got {mu.shape}, {cov.shape}, {window.shape})")
    for name, v in (("mu_pris_param", mu), ("cov_pris_param", cov), ("gaussian_window", window)):
        if not np.all(np.isfinite(v)):
            raise ValueError(f"{what}: {name} holds non-finite values")
    if not np.allclose(cov, cov.T, rtol=1e-8, atol=1e-12 * max(1.0, float(np.abs(cov).max()))):
        raise ValueError(f"{what}: cov_pris_param is not symmetric")
    return {"mu": mu.reshape(36), "cov": cov, "window": window}


def load_niqe_params(path) -> dict:
    """Reads a `niqe_pris_params.npz` (BasicSR's format) -> check_niqe_params' dict; ValueError names what is wrong with the file."""
    try:
        f = np.load(str(path), allow_pickle=False)
    except Exception as e:          # a missing file, a file that is no archive
        raise ValueError(f"{path}: cannot be read as a NIQE parameter file ({type(e).__name__})") from e
    if not hasattr(f, "files"):
        raise ValueError(f"{path}: cannot be read as a NIQE parameter file (one array, not an .npz archive)")
    with f:
        missing = [k for k in NIQE_KEYS if k not in f.files]
        if missing:
            raise ValueError(f"{path}: not a NIQE parameter file: lacks {missing} (has {sorted(f.files)})")
        try:
            mu, cov, window = (f[k] for k in NIQE_KEYS)
        except Exception as e:
            raise ValueError(f"{path}: cannot be read as a NIQE parameter file ({type(e).__name__})") from e
    return check_niqe_params(mu, cov, window, what=str(path))


def save_niqe_params(path, mu, cov, window=None) -> None:
    p = check_niqe_params(mu, cov, niqe_window() if window is None else window)
    with open(str(path), "wb") as f:
        np.savez(f, mu_pris_param=p["mu"].reshape(1, 36), cov_pris_param=p["cov"], gaussian_window=p["window"])


# ---- stages ---------------------------------------------------------------------------------------------------------------------------
def niqe_plane_shape(shape, border: int = 0, bs: int = NIQE_BLOCK) -> Tuple[int, int, int, int]:
    """[B, C, H, W] -> (Hk, Wk, nbh, nbw) of the plane srk_niqe_plane_f32 keeps; ValueError for what it refuses, fewer than one block included."""
    if len(shape) != 4:
        raise ValueError(f"niqe: images must be [B, C, H, W] (got {tuple(shape)})")
    B, C, H, W = (int(v) for v in shape)
    if isinstance(border, bool) or not isinstance(border, numbers.Integral) or border < 0:
        raise ValueError(f"niqe: crop border must be an integer >= 0 (got {border!r})")
    if isinstance(bs, bool) or not isinstance(bs, numbers.Integral) or bs < 8 or bs % 2:
        raise ValueError(f"niqe: the block side must be an even integer >= 8 (got {bs!r})")
    if min(B, H, W) < 1 or C not in (1, 3) or B > 1024:
        raise ValueError(f"niqe: needs 1 <= B <= 1024, C 1 or 3 and non-empty images (got {tuple(shape)})")
    nbh, nbw = max(0, H - 2 * border) // bs, max(0, W - 2 * border) // bs
    if nbh < 1 or nbw < 1:
        raise ValueError(f"niqe: {H} x {W} with a border of {border} holds no block of {bs} x {bs}")
    return nbh * bs, nbw * bs, nbh, nbw


_WIN_CACHE = {}


def _device_window(window: np.ndarray, device) -> torch.Tensor:
    w32 = np.ascontiguousarray(window, dtype=np.float32).reshape(49)
    key = (str(device), w32.tobytes())
    if key not in _WIN_CACHE:
        _WIN_CACHE.clear()
        _WIN_CACHE[key] = torch.from_numpy(w32.copy()).to(device)
    return _WIN_CACHE[key]


def half_host(plane: np.ndarray) -> np.ndarray:
    """The half-size filter of srk_niqe_half_f32 on an integer-valued [..., H, W] plane (H, W even), in exact integers -> fp32."""
    s = np.rint(plane).astype(np.int64)
    for axis in (-1, -2):
        n = s.shape[axis]
        pad = [(0, 0)] * s.ndim
        pad[axis] = (3, 3)
        p = np.moveaxis(np.pad(s, pad, mode="symmetric"), axis, -1)
        acc = sum(t * p[..., k:k + n:2] for k, t in enumerate(HALF_TAPS))
        s = np.moveaxis(acc, -1, axis)
    return s.astype(np.float32) * np.float32(2.0 ** -16)


def mscn_host(plane: np.ndarray, window: np.ndarray):
    """The centred MSCN form on [..., H, W] (replicate border), accumulated in fp64 with the fp32 taps -> (m, sigma) in fp32."""
    v = np.asarray(plane, dtype=np.float64)
    w = np.asarray(window, dtype=np.float32).astype(np.float64).reshape(7, 7)
    H, W = v.shape[-2:]
    p = np.pad(v, [(0, 0)] * (v.ndim - 2) + [(3, 3), (3, 3)], mode="edge")
    a, b = np.zeros_like(v), np.zeros_like(v)
    for dy in range(7):
        for dx in range(7):
            d = p[..., dy:dy + H, dx:dx + W] - v
            a += w[dy, dx] * d
            b += w[dy, dx] * d * d
    sigma = np.sqrt(np.abs(b - a * a))
    return (-a / (sigma + 1.0)).astype(np.float32), sigma.astype(np.float32)


_SHIFTS = ((0, 1), (1, 0), (1, 1), (1, -1))


def moments_host(m: np.ndarray, bs: int, sigma: Optional[np.ndarray] = None):
    """The block moments of srk_niqe_moments_f32 from an fp32 map [B, H, W] (products in fp32, sums in fp64, stored as fp32)."""
    m = np.asarray(m, dtype=np.float32)
    B, H, W = m.shape
    nbh, nbw = H // bs, W // bs
    blk = m.reshape(B, nbh, bs, nbw, bs).transpose(0, 1, 3, 2, 4)
    mom = np.empty((B, nbh * nbw, 5, 5), dtype=np.float32)
    for k, p in enumerate([blk] + [blk * np.roll(blk, s, axis=(3, 4)) for s in _SHIFTS]):
        p = p.reshape(B, nbh * nbw, bs * bs)
        neg, pos, sq = p < 0, p > 0, p.astype(np.float64) ** 2
        mom[:, :, k, 0], mom[:, :, k, 1] = neg.sum(-1), np.where(neg, sq, 0.0).sum(-1)
        mom[:, :, k, 2], mom[:, :, k, 3] = pos.sum(-1), np.where(pos, sq, 0.0).sum(-1)
        mom[:, :, k, 4] = np.abs(p.astype(np.float64)).sum(-1)
    sharp = None
    if sigma is not None:
        sg = np.asarray(sigma, dtype=np.float64).reshape(B, nbh, bs, nbw, bs).transpose(0, 1, 3, 2, 4)
        sharp = sg.reshape(B, nbh * nbw, bs * bs).mean(-1).astype(np.float32)
    return mom, sharp


def niqe_moments(x: torch.Tensor, border: int = 0, bs: int = NIQE_BLOCK, window: Optional[np.ndarray] = None):
    """fp32 [B, C, H, W] in [0, 1], C 1 or 3 -> (mom1, mom2 fp32 [B, nb, 5, 5], sharp fp32 [B, nb]) as numpy arrays: the block moments of
    both scales and the scale-1 block means of sigma (srk.h).  A CUDA tensor takes the kernels: six launches, one download."""
    Hk, Wk, nbh, nbw = niqe_plane_shape(x.shape, border, bs)
    window = niqe_window() if window is None else np.asarray(window, dtype=np.float64)
    if window.shape != (7, 7):
        raise ValueError(f"niqe: the window must be [7, 7] (got {window.shape})")
    B, C, H, W = x.shape
    nb = nbh * nbw
    if x.is_cuda:
        from ._lib import _p, _stream, check, lib
        x = x.detach().to(torch.float32).contiguous()
        dev, f32 = x.device, torch.float32
        win = _device_window(window, dev)
        plane, half = torch.empty((B, Hk, Wk), dtype=f32, device=dev), torch.empty((B, Hk // 2, Wk // 2), dtype=f32, device=dev)
        m1, sg = torch.empty_like(plane), torch.empty_like(plane)
        m2 = torch.empty_like(half)
        out = torch.empty(B * nb * 51, dtype=f32, device=dev)
        mom1, mom2, sharp = out[:B * nb * 25], out[B * nb * 25:B * nb * 50], out[B * nb * 50:]
        L, s = lib(), _stream()
        check(L.srk_niqe_plane_f32(_p(x), _p(plane), B, C, H, W, int(border), int(bs), s))
        check(L.srk_niqe_half_f32(_p(plane), _p(half), B, Hk, Wk, s))
        check(L.srk_niqe_mscn_f32(_p(plane), _p(win), _p(m1), _p(sg), B, Hk, Wk, s))
        check(L.srk_niqe_mscn_f32(_p(half), _p(win), _p(m2), None, B, Hk // 2, Wk // 2, s))
        check(L.srk_niqe_moments_f32(_p(m1), _p(sg), mom1.data_ptr(), sharp.data_ptr(), B, Hk, Wk, int(bs), s))
        check(L.srk_niqe_moments_f32(_p(m2), None, mom2.data_ptr(), None, B, Hk // 2, Wk // 2, int(bs) // 2, s))
        host = out.cpu().numpy()
        return (host[:B * nb * 25].reshape(B, nb, 5, 5), host[B * nb * 25:B * nb * 50].reshape(B, nb, 5, 5), host[B * nb * 50:].reshape(B, nb))
    from .metrics import bench_planes_torch
    plane = bench_planes_torch(x.detach(), int(border), "y").round()[:, 0, :Hk, :Wk].numpy()
    m1, sg = mscn_host(plane, window)
    m2, _ = mscn_host(half_host(plane), window)
    mom1, sharp = moments_host(m1, int(bs), sg)
    mom2, _ = moments_host(m2, int(bs) // 2)
    return mom1, mom2, sharp


# ---- features and distance: host fp64 --------------------------------------------------------------------------------------------------
_GRID = None


def _aggd_grid():
    """BasicSR's grid arange(0.2, 10.001, 0.001) with lgamma(1/g), lgamma(2/g), lgamma(3/g) and r(g) = G(2/g)^2 / (G(1/g) G(3/g))."""
    global _GRID
    if _GRID is None:
        gam = np.arange(0.2, 10.001, 0.001)
        lg = [np.array([math.lgamma(k / g) for g in gam]) for k in (1, 2, 3)]
        _GRID = (gam, lg[0], lg[1], lg[2], np.exp(2.0 * lg[1] - lg[0] - lg[2]))
    return _GRID


def niqe_features(mom, npix: int) -> np.ndarray:
    """Block moments [..., 5, 5] of blocks of `npix` pixels -> the 18 features [..., 18] of BasicSR's compute_feature in fp64: AGGD moment
    matching (estimate_aggd_param) per map, [alpha, (beta_l + beta_r) / 2] of the MSCN map, then [alpha, (beta_r - beta_l) G(2/alpha) /
    G(1/alpha), beta_l, beta_r] per shift.  A map with an empty side gives NaN there, as in BasicSR."""
    mom = np.asarray(mom, dtype=np.float64)
    if mom.shape[-2:] != (5, 5) or int(npix) < 1:
        raise ValueError(f"niqe_features takes moments [..., 5, 5] and a pixel count >= 1 (got {mom.shape}, {npix!r})")
    lead = mom.shape[:-2]
    s = mom.reshape(-1, 5)
    gam, lg1, lg2, lg3, r_gam = _aggd_grid()
    with np.errstate(divide="ignore", invalid="ignore"):
        left, right = np.sqrt(s[:, 1] / s[:, 0]), np.sqrt(s[:, 3] / s[:, 2])
        gh = left / right
        rhat = (s[:, 4] / npix) ** 2 / ((s[:, 1] + s[:, 3]) / npix)
        rnorm = rhat * (gh ** 3 + 1) * (gh + 1) / (gh ** 2 + 1) ** 2
        pos = np.empty(s.shape[0], dtype=np.int64)
        for i in range(0, s.shape[0], 512):          # argmin of the squared distance on the grid; a NaN row takes index 0, as np.argmin does
            pos[i:i + 512] = np.argmin((r_gam[None, :] - rnorm[i:i + 512, None]) ** 2, axis=1)
        alpha = gam[pos]
        scale = np.exp(0.5 * (lg1[pos] - lg3[pos]))
        bl, br = left * scale, right * scale
        mean = (br - bl) * np.exp(lg2[pos] - lg1[pos])
    alpha, bl, br, mean = (v.reshape(-1, 5) for v in (alpha, bl, br, mean))
    feat = [alpha[:, 0], (bl[:, 0] + br[:, 0]) / 2.0]
    for k in range(1, 5):
        feat += [alpha[:, k], mean[:, k], bl[:, k], br[:, k]]
    return np.stack(feat, axis=-1).reshape(*lead, 18)


def niqe_distance(rows, mu_p, cov_p) -> float:
    """rows [n, 36] (scale-1 and scale-2 features side by side) against the pristine Gaussian: mu_d = nanmean of the rows, cov_d = np.cov
    of the NaN-free rows, sqrt((mu_p - mu_d) pinv((cov_p + cov_d) / 2) (mu_p - mu_d)^T).  Fewer than 2 NaN-free rows: ValueError."""
    rows = np.asarray(rows, dtype=np.float64)
    if rows.ndim != 2 or rows.shape[1] != 36:
        raise ValueError(f"niqe_distance takes rows [n, 36] (got {rows.shape})")
    clean = rows[~np.isnan(rows).any(axis=1)]
    if clean.shape[0] < 2:
        raise ValueError(f"niqe: {clean.shape[0]} of {rows.shape[0]} blocks have finite features; the covariance needs at least 2")
    mu_d = np.nanmean(rows, axis=0)
    cov_d = np.cov(clean, rowvar=False)
    d = (np.asarray(mu_p, dtype=np.float64).reshape(1, 36) - mu_d.reshape(1, 36))
    inv = np.linalg.pinv((np.asarray(cov_p, dtype=np.float64) + cov_d) / 2.0)
    return float(np.sqrt(d @ inv @ d.T).reshape(()))


def niqe_rows(mom1, mom2, bs: int = NIQE_BLOCK) -> np.ndarray:
    """Block moments of both scales [..., 5, 5] -> rows [..., 36]."""
    return np.concatenate([niqe_features(mom1, bs * bs), niqe_features(mom2, (bs // 2) ** 2)], axis=-1)


def _params(params) -> dict:
    if isinstance(params, dict) and {"mu", "cov", "window"} <= set(params):
        return params
    if isinstance(params, (str, Path)):
        return load_niqe_params(params)
    return check_niqe_params(*params)


def niqe(x: torch.Tensor, params, crop_border: int = 0, bs: int = NIQE_BLOCK) -> torch.Tensor:
    """NIQE of fp32 [B, C, H, W] images in [0, 1] (C 3: on the rounded BT.601 luma; C 1: as they are) -> fp64 [B] on the CPU; lower is
    better.  params: load_niqe_params' dict, a path, or (mu, cov, window).  The images are quantised to 8 bits first, as a written file is."""
    p = _params(params)
    mom1, mom2, _ = niqe_moments(x, crop_border, bs, p["window"])
    rows = niqe_rows(mom1, mom2, bs)
    return torch.tensor([niqe_distance(rows[b], p["mu"], p["cov"]) for b in range(rows.shape[0])], dtype=torch.float64)


def niqe_fit(batches: Iterable[torch.Tensor], sharpness: float = 0.75, crop_border: int = 0, bs: int = NIQE_BLOCK,
             window: Optional[np.ndarray] = None):
    """The pristine model (estimatemodelparam.m): per image the blocks whose sharpness (block mean of sigma at scale 1) is above
    `sharpness` x the image's largest are kept; -> (mu [36] = nanmean of the kept rows of all images, cov [36, 36] = covariance of the
    NaN-free ones).  batches: fp32 [B, C, H, W] tensors, any mix of sizes."""
    if not (isinstance(sharpness, numbers.Real) and 0.0 <= float(sharpness) < 1.0):
        raise ValueError(f"niqe_fit: sharpness must be in [0, 1) (got {sharpness!r})")
    kept = []
    for x in batches:
        mom1, mom2, sharp = niqe_moments(x, crop_border, bs, window)
        rows = niqe_rows(mom1, mom2, bs)
        for b in range(rows.shape[0]):
            kept.append(rows[b][sharp[b] > np.float32(sharpness) * sharp[b].max()])
    rows = np.concatenate(kept, axis=0) if kept else np.empty((0, 36))
    clean = rows[~np.isnan(rows).any(axis=1)]
    if clean.shape[0] < 2:
        raise ValueError(f"niqe_fit: {clean.shape[0]} kept blocks with finite features; the covariance needs at least 2")
    return np.nanmean(rows, axis=0), np.cov(clean, rowvar=False)


# ---- the command line -----------------------------------------------------------------------------------------------------------------
def parse_args(argv=None):
    ap = argparse.ArgumentParser(prog="python -m tpu_superresolution_amd.niqe", description="NIQE: fit the pristine model, score image files without ground truth")
    sub = ap.add_subparsers(dest="cmd", required=True)
    fit = sub.add_parser("fit", help="fit the pristine Gaussian on a directory of good images (the HR training set)")
    fit.add_argument("--input", type=str, required=True, help="an image file, or a directory of them (not recursive, sorted by name)")
    fit.add_argument("--out", type=str, required=True, help="the .npz to write (BasicSR's niqe_pris_params.npz format)")
    fit.add_argument("--sharpness", type=float, default=0.75, help="keep the blocks whose sharpness is above this share of the image's largest")
    score = sub.add_parser("score", help="score image files against a parameter file")
    score.add_argument("--input", type=str, required=True, help="an image file, or a directory of them (not recursive, sorted by name)")
    score.add_argument("--params", type=str, required=True, help="niqe_pris_params.npz: the published file, or one written by `fit`")
    for p in (fit, score):
        p.add_argument("--crop_border", type=int, default=0, help="pixels cropped on every side before the blocks are cut")
        p.add_argument("--batch_size", type=int, default=1, help="consecutive files of equal size and mode, up to N, form one batch")
        p.add_argument("--device", type=str, default=None, help="force 'cpu' / 'cuda' (default: cuda if available)")
    args = ap.parse_args(argv)
    if args.crop_border < 0:
        ap.error(f"--crop_border must be >= 0 (got {args.crop_border})")
    if args.batch_size < 1:
        ap.error(f"--batch_size must be >= 1 (got {args.batch_size})")
    if args.cmd == "fit" and not 0.0 <= args.sharpness < 1.0:
        ap.error(f"--sharpness must be in [0, 1) (got {args.sharpness})")
    if args.cmd == "score":
        try:
            args.niqe_params = load_niqe_params(args.params)
        except ValueError as e:
            ap.error(f"--params {e}")
    return args


def _batches(files, batch_size: int, device, log):
    """Decoded files in runs of equal (shape, dtype, mode), up to batch_size -> (names, fp32 [B, C, H, W] on `device`); alpha is dropped."""
    from . import ops
    from .predict import _key, _to_device, load_image
    i, ahead = 0, None
    while i < len(files):
        arrays, mode0 = [], None
        while i + len(arrays) < len(files) and len(arrays) < batch_size:
            a, mode = ahead if ahead is not None else load_image(files[i + len(arrays)], log=log)
            ahead = None
            if arrays and (_key(a) != _key(arrays[0]) or mode != mode0):
                ahead = (a, mode)
                break
            arrays.append(a)
            mode0 = mode
        stack = np.stack([a[:, :, None] if a.ndim == 2 else a for a in arrays])
        x, _ = ops.image_unpack(_to_device(stack, device), 3 if stack.shape[3] >= 3 else 1)
        yield [p.name for p in files[i:i + len(arrays)]], x
        i += len(arrays)


def main(argv=None, log=print) -> dict:
    args = parse_args(argv)
    from .predict import discover
    device = torch.device(args.device) if args.device else torch.device("cuda" if torch.cuda.is_available() else "cpu")
    log(f"[device] {device}")
    files = discover(args.input, log=log)
    if not files:
        raise SystemExit(f"--input {args.input}: no image that PIL can open (see the [skip] lines)")
    if args.cmd == "fit":
        used = []

        def gen():
            for names, x in _batches(files, args.batch_size, device, log):
                try:
                    niqe_plane_shape(x.shape, args.crop_border)
                except ValueError as e:
                    for n in names:
                        log(f"[niqe] {n}: skipped ({e})")
                    continue
                used.extend(names)
                yield x

        try:
            mu, cov = niqe_fit(gen(), sharpness=args.sharpness, crop_border=args.crop_border)
        except ValueError as e:
            raise SystemExit(f"--input {args.input}: {e}")
        save_niqe_params(args.out, mu, cov)
        log(f"[done] fitted on {len(used)} images -> {args.out}")
        return {"n": len(used), "files": used, "out": str(args.out), "mu": mu, "cov": cov}
    p = args.niqe_params
    scores = {}
    for names, x in _batches(files, args.batch_size, device, log):
        try:
            _, _, nbh, nbw = niqe_plane_shape(x.shape, args.crop_border)
            if nbh * nbw < 2:
                raise ValueError(f"{x.shape[2]} x {x.shape[3]} with a border of {args.crop_border} holds {nbh * nbw} block of "
                                 f"{NIQE_BLOCK} x {NIQE_BLOCK}; the score needs at least 2")
            mom1, mom2, _ = niqe_moments(x, args.crop_border, NIQE_BLOCK, p["window"])
        except ValueError as e:
            for n in names:
                log(f"[niqe] {n}: skipped ({e})")
            continue
        rows = niqe_rows(mom1, mom2)
        for b, n in enumerate(names):
            try:
                scores[n] = niqe_distance(rows[b], p["mu"], p["cov"])
            except ValueError as e:
                log(f"[niqe] {n}: skipped ({e})")
                continue
            log(f"[niqe] {n} {scores[n]:.4f}")
    if not scores:
        raise SystemExit(f"--input {args.input}: no file could be scored (see the [niqe] lines)")
    mean = float(np.mean(list(scores.values())))
    log(f"[done] {len(scores)} images | mean {mean:.4f}")
    return {"n": len(scores), "scores": scores, "mean": mean}


if __name__ == "__main__":
    main()
