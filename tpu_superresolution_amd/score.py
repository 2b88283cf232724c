"""Score image files against ground truth: benchmark-protocol PSNR / SSIM, PSNR-B and MS-SSIM.

    python -m tpu_superresolution_amd.score --sr FILE|DIR --gt FILE|DIR [--metrics psnr ssim psnrb ms_ssim] [--mode y|rgb]
        [--crop_border N] [--suffix _sr] [--gt_modcrop S] [--batch_size N] [--device D]

An SR file pairs with the ground-truth file whose stem equals its own with --suffix stripped (`predict` appends `_sr`); two files given
directly are one pair whatever their names.  Every score is taken on the 8-bit, border-cropped planes of the SwinIR / HAT / DAT test
protocol: the BT.601 luma (--mode y) or the colour planes (--mode rgb), scale 0..255.  `psnr` and `ssim` are ``metrics.bench_metrics``,
`psnrb` and `ms_ssim` ``metrics.psnrb`` and ``metrics.ms_ssim``; PSNR-B rates the SR file as the restored image.  A pair too small for a
metric (cropped planes below 11 x 11 for ssim, 16 x 16 for psnrb, 161 x 161 for ms_ssim) prints `-` for it and stays out of its mean.
SSIM, PSNR-B and MS-SSIM are restated from the published algorithms: **parity with the third-party scripts unpinned**.
"""
from __future__ import annotations

import argparse
from pathlib import Path

import numpy as np
import torch

METRICS = ("psnr", "ssim", "psnrb", "ms_ssim")
MIN_SIDE = {"psnr": 1, "ssim": 11, "psnrb": 16, "ms_ssim": 161}          # of the cropped planes
_FMT = {"psnr": "{:.4f}", "ssim": "{:.6f}", "psnrb": "{:.4f}", "ms_ssim": "{:.6f}"}


def parse_args(argv=None):
    ap = argparse.ArgumentParser(prog="python -m tpu_superresolution_amd.score", description="score image files against ground truth")
    ap.add_argument("--sr", type=str, required=True, help="a restored / upscaled image file, or a directory of them (not recursive, sorted by name)")
    ap.add_argument("--gt", type=str, required=True, help="the ground-truth file, or the directory of ground-truth files")
    ap.add_argument("--metrics", type=str, nargs="+", choices=METRICS, default=["psnr", "ssim"], help="the scores to print, in this order")
    ap.add_argument("--mode", type=str, choices=("y", "rgb"), default="y", help="BT.601 luma (the papers' tables) or the colour planes")
    ap.add_argument("--crop_border", type=int, default=0, help="pixels cropped on every side (the papers crop the scale factor)")
    ap.add_argument("--suffix", type=str, default="_sr", help="stripped from an SR stem before it is matched with a ground-truth stem")
    ap.add_argument("--gt_modcrop", type=int, default=1, help="crop the ground truth to multiples of S from the top left (the scale factor)")
    ap.add_argument("--batch_size", type=int, default=1, help="consecutive pairs of equal size and mode, up to N, form one batch")
    ap.add_argument("--device", type=str, default=None, help="force 'cpu' / 'cuda' (default: cuda if available)")
    args = ap.parse_args(argv)
    if args.crop_border < 0:
        ap.error(f"--crop_border must be >= 0 (got {args.crop_border})")
    if args.batch_size < 1:
        ap.error(f"--batch_size must be >= 1 (got {args.batch_size})")
    if args.gt_modcrop < 1:
        ap.error(f"--gt_modcrop must be >= 1 (got {args.gt_modcrop})")
    args.metrics = list(dict.fromkeys(args.metrics))
    return args


def pair_files(sr_files, gt_files, suffix: str, direct: bool = False):
    """-> (pairs [(sr, gt)] in SR order, the number of ground-truth files without an SR file).  Every SR file without a partner is named
    in one error."""
    if direct:
        return [(sr_files[0], gt_files[0])], 0
    by_stem = {}
    for g in gt_files:
        if g.stem in by_stem:
            raise SystemExit(f"--gt: {by_stem[g.stem].name} and {g.name} share the stem {g.stem!r}")
        by_stem[g.stem] = g
    pairs, missing = [], []
    for s in sr_files:
        stem = s.stem[:-len(suffix)] if suffix and s.stem.endswith(suffix) else s.stem
        if stem in by_stem:
            pairs.append((s, by_stem[stem]))
        else:
            missing.append(f"{s.name} (no ground-truth file with the stem {stem!r})")
    if missing:
        raise SystemExit(f"--sr: {len(missing)} of {len(sr_files)} files have no partner in --gt: " + "; ".join(missing))
    used = {g for _, g in pairs}
    return pairs, sum(1 for g in gt_files if g not in used)


def _colours(a: np.ndarray) -> int:
    return 3 if (a.ndim == 3 and a.shape[2] >= 3) else 1


def _load_pair(sr, gt, modcrop: int, log):
    from .predict import load_image
    a, _ = load_image(sr, log=log)
    g, _ = load_image(gt, log=log)
    g = g[:g.shape[0] - g.shape[0] % modcrop, :g.shape[1] - g.shape[1] % modcrop]
    if a.shape[:2] != g.shape[:2] or _colours(a) != _colours(g):
        crop = f" after --gt_modcrop {modcrop}" if modcrop > 1 else ""
        raise SystemExit(f"{sr.name} is {a.shape[0]} x {a.shape[1]} with {_colours(a)} colour channel(s), {gt.name} is {g.shape[0]} x {g.shape[1]} "
                         f"with {_colours(g)}{crop}: a pair must have one size and one channel count")
    return a, np.ascontiguousarray(g)


def _unpack(arrays, device) -> torch.Tensor:
    from . import ops
    from .predict import _to_device
    stack = np.stack([a[:, :, None] if a.ndim == 2 else a for a in arrays])
    return ops.image_unpack(_to_device(stack, device), 3 if stack.shape[3] >= 3 else 1)[0]


def _batches(pairs, args, device, log):
    """Loaded pairs in runs of equal (shape, dtype) of both files, up to --batch_size -> (SR names, sr, gt: fp32 [B, C, H, W] on `device`)."""
    from .predict import _key
    i, ahead = 0, None
    while i < len(pairs):
        srs, gts = [], []
        while i + len(srs) < len(pairs) and len(srs) < args.batch_size:
            a, g = ahead if ahead is not None else _load_pair(*pairs[i + len(srs)], args.gt_modcrop, log)
            ahead = None
            if srs and (_key(a), _key(g)) != (_key(srs[0]), _key(gts[0])):
                ahead = (a, g)
                break
            srs.append(a)
            gts.append(g)
        yield [s.name for s, _ in pairs[i:i + len(srs)]], _unpack(srs, device), _unpack(gts, device)
        i += len(srs)


def score_batch(sr: torch.Tensor, gt: torch.Tensor, metrics_wanted, crop_border: int, mode: str) -> dict:
    """-> {metric: list of B floats, or None when the cropped planes are too small for it}."""
    from . import metrics as M
    from .ops import bench_plane_shape
    try:
        side = min(bench_plane_shape(sr.shape, crop_border, mode)[2:])
    except ValueError:
        side = 0
    out = {m: None for m in metrics_wanted}
    ok = [m for m in metrics_wanted if side >= MIN_SIDE[m]]
    if "psnr" in ok or "ssim" in ok:
        ps, ss = M.bench_metrics(sr, gt, crop_border, mode, with_ssim="ssim" in ok)
        if "psnr" in ok:
            out["psnr"] = [float(v) for v in ps.cpu()]
        if "ssim" in ok:
            out["ssim"] = [float(v) for v in ss.cpu()]
    if "psnrb" in ok:
        out["psnrb"] = [float(v) for v in M.psnrb(sr, gt, crop_border, mode).cpu()]
    if "ms_ssim" in ok:
        pp, pt = M.bench_planes_pair(sr, gt, crop_border, mode)
        out["ms_ssim"] = [float(v) for v in M.ms_ssim(pp, pt, data_range=255.0, size_average=False).cpu()]
    return out


def main(argv=None, log=print) -> dict:
    args = parse_args(argv)
    from .predict import discover
    device = torch.device(args.device) if args.device else torch.device("cuda" if torch.cuda.is_available() else "cpu")
    log(f"[device] {device}")
    try:
        sr_files, gt_files = discover(args.sr, log=log), discover(args.gt, log=log)
    except FileNotFoundError as e:
        raise SystemExit(str(e).replace("--input", "--sr / --gt"))
    for flag, files, where in (("--sr", sr_files, args.sr), ("--gt", gt_files, args.gt)):
        if not files:
            raise SystemExit(f"{flag} {where}: no image that PIL can open (see the [skip] lines)")
    pairs, unmatched = pair_files(sr_files, gt_files, args.suffix, direct=Path(args.sr).is_file() and Path(args.gt).is_file())
    if unmatched:
        log(f"[pair] {unmatched} ground-truth files have no SR file")
    scores = {}
    with torch.no_grad():
        for names, sr, gt in _batches(pairs, args, device, log):
            got = score_batch(sr, gt, args.metrics, args.crop_border, args.mode)
            for b, n in enumerate(names):
                scores[n] = {m: (None if got[m] is None else got[m][b]) for m in args.metrics}
                log(f"[score] {n} " + " ".join(f"{m}=" + ("-" if scores[n][m] is None else _FMT[m].format(scores[n][m])) for m in args.metrics))
    mean = {}
    for m in args.metrics:
        vals = [s[m] for s in scores.values() if s[m] is not None]
        if not vals:
            raise SystemExit(f"--metrics {m}: no pair could be scored (cropped planes of at least {MIN_SIDE[m]} x {MIN_SIDE[m]} are needed; see the "
                             f"[score] lines)")
        mean[m] = float(np.mean(vals))
    log(f"[done] {len(scores)} pairs | " + " ".join(f"{m}={_FMT[m].format(mean[m])}" for m in args.metrics))
    return {"n": len(scores), "scores": scores, "mean": mean, "unmatched_gt": unmatched}


if __name__ == "__main__":
    main()
