"""Test-set evaluation entry point with the reference's command line (modules/evaluate.py:54-234).

    python -m tpu_superresolution_amd.evaluate --scale X2 --data_root D --ckpt best_X2.pt [--save_dir preds ...]

Same ten flags, same pipeline and prints: eval transform (grayscale -> bicubic LR to HR size -> [0,1], :78) ->
``Shuffled2DPaired(split="test")`` -> min/max peek (:96-112) -> bicubic baseline PSNR/SSIM (:115-134) -> ``MS_ResUNet()``
+ checkpoint (``{"model": sd}``, ``{"params": sd}``, ``{"params_ema": sd}`` or a raw state_dict, strict, :136-145) -> per-batch fp32 PSNR (:24-29) and SSIM,
non-finite guard (:172-178), optional bilinear resize to the HR size (:181-184), PNG dumps
``idx_%06d_{lr,hr,sr}.png`` under the policy --save_indices > --save_every/--save_start > first --save_n, always capped
by --save_n (:199-225) -> summary (:229-234).

BASELINE config 1 runs this on the CPU with stock torch operators (MS_ResUNet has no kernel in scope).
Additive: ``--arch swinir | hat | dat`` evaluates the MI355X SwinIR / HAT / DAT path (finetune_swinir.py model, RGB un-upscaled LR input, needs a
GPU + libsrk); ``--self_ensemble`` averages the eight flipped / rotated predictions (any --arch); ``--tile N`` predicts on overlapping
N x N tiles of the model's input and merges them (tiling.tiled_forward; any --arch; inside the self-ensemble when both are given);
``--synth_lr [--synth_lr_bits 0|8]`` (--arch swinir | hat | dat) needs only the HR directory of the test split: LR is its antialiased
bicubic downscale, formed on the device (ops.resize_aa), with ``--degrade blind --blur_sigma SY SX --noise_sigma N --noise_gain G`` blurred and
noised there with fixed parameters (ops.degrade_blind), with ``--jpeg_quality Q [--jpeg_subsample 444|420]`` then sent through a baseline
JPEG round trip (ops.jpeg_roundtrip), with ``--blur_theta DEG`` or ``--blur_psf FILE`` blurred with a 2-D table instead (ops.degrade_psf,
DESIGN 7n); ``main(argv)`` is callable from tests.  SSIM is ``metrics.ssim`` (restated, parity unpinned).
``--bench_metric y | rgb [--crop_border N]`` (any --arch, any of the options above: it looks at (pred, hr) only) adds ``[bench]`` lines
and ``bench_*`` keys with the scores of the papers' protocol -- 8-bit, border-cropped (default: the scale), BT.601 luma or RGB, 0..255
scale, mean over images (metrics.bench_metrics); the other lines and keys stay as they are.
``--synth_lr --degrade second_order`` degrades the HR images with the fixed second-order chain (SecondOrderSpec.fixed, ops.degrade_second_order,
DESIGN 7p); with ``--gt_usm [--usm_weight W --usm_threshold T --usm_radius R]`` the HR images are unsharp-masked first (ops.usm_sharpen), the chain
runs on the sharpened images and every score is taken against them.
``--task dn | car --scale X1 --arch swinir [--channels 1|3 --dn_sigma S --jpeg_quality Q]`` scores the scale-1 restoration models: the clean test
images are noised / JPEG-coded as whole images on the device (ops.restore_degrade) and the baseline line is the degraded input itself.
"""
from __future__ import annotations

import argparse
import re
import time
from functools import partial
from pathlib import Path

import torch
from PIL import Image
from torch.utils.data import DataLoader

from .data_cli import (BLIND, SCALES, SECOND, USM_FLAGS, default_window_size, eval_lines, eval_psf, eval_restore, eval_specs,          # noqa: F401
                       flag, shared_flags, usm_spec as eval_usm)          # eval_usm: training's rule, the same object as finetune_swinir.usm_spec
from .metrics import psnr, ssim
from .ms_resunet import MS_ResUNet
from .sr_datasets import PairTransformValid, RestoreBatches, Shuffled2DHR, Shuffled2DPaired, SynthLRBatches, clean_to_tensor, hr_to_tensor3
from .sr_transforms import build_pair_transform_eval


def save_tensor_as_png(x: torch.Tensor, path: Path, per_image_rescale: bool = False):
    """evaluate.py:31-51: [C,H,W] in [0,1] -> 8-bit PNG (clamp, or per-image min-max when asked; x255 then truncation, as
    torchvision's ToPILImage does for float tensors)."""
    x = x.detach().float().cpu()
    if per_image_rescale:
        lo, hi = float(x.min()), float(x.max())
        x = torch.zeros_like(x) if hi <= lo + 1e-8 else (x - lo) / (hi - lo)
    else:
        x = x.clamp(0.0, 1.0)
    a = x.mul(255).byte().numpy()
    img = Image.fromarray(a[0], mode="L") if a.shape[0] == 1 else Image.fromarray(a.transpose(1, 2, 0))
    img.save(str(path))


PARAM_KEYS = ("model", "params", "params_ema")          # envelopes, in the order 'auto' tries them


def _load_state(path: str, param_key: str = "auto", keys=PARAM_KEYS):
    """-> (state_dict, message).  'auto': the first of `keys` the file has (the published HAT / DAT files hold only 'params_ema', the
    exponential moving average of the weights; finetune_swinir --weights tries 'params' first), else a raw state_dict.  A named key must exist."""
    ckpt = torch.load(path, map_location="cpu", weights_only=True)
    if param_key != "auto":
        if param_key not in PARAM_KEYS:
            raise ValueError(f"param_key must be 'auto' or one of {PARAM_KEYS} (got {param_key!r})")
        if not isinstance(ckpt, dict) or param_key not in ckpt:
            have = [str(k) for k in ckpt] if isinstance(ckpt, dict) else []
            raise KeyError(f"{path}: no '{param_key}' key; the file has {have[:12]}{' ...' if len(have) > 12 else ''}")
        return ckpt[param_key], f"[ckpt] loaded state_dict from '{param_key}' key"
    if isinstance(ckpt, dict):
        for k in keys:
            if k in ckpt:
                return ckpt[k], f"[ckpt] loaded state_dict from '{k}' key"
    return ckpt, "[ckpt] loaded raw state_dict"


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=str, choices=["X1", "X2", "X4"], required=True,
                    help="dataset configuration; X1 (input and target of one size) with --task dn | car")
    ap.add_argument("--data_root", type=str, default="DeepRockSR-2D")
    ap.add_argument("--batch_size", type=int, default=4)
    ap.add_argument("--workers", type=int, default=0)
    ap.add_argument("--ckpt", type=str, required=True)
    ap.add_argument("--save_dir", type=str, default="preds")
    ap.add_argument("--save_n", type=int, default=16)
    ap.add_argument("--save_every", type=int, default=0, help="save every N-th sample by dataset index (0 = off)")
    ap.add_argument("--save_start", type=int, default=0, help="first index of the periodic saving (for save_every)")
    ap.add_argument("--save_indices", type=str, default="",
                    help="explicit comma-separated indices, e.g. '0,100,200'; takes priority over save_every")
    ap.add_argument("--arch", type=str, choices=["ms_resunet", "swinir", "hat", "dat"], default="ms_resunet")       # additive
    ap.add_argument("--param_key", type=str, choices=["auto", *PARAM_KEYS], default="auto",
                    help="additive: which envelope of the checkpoint to load (auto: model, then params, then params_ema)")
    ap.add_argument("--device", type=str, default=None, help="additive: force 'cpu' / 'cuda' (default: cuda if available)")
    ap.add_argument("--window_size", type=int, default=None,
                    help="additive, --arch swinir: SwinIR(window_size=N), N in 2..8 (default: 8, or 7 with --task car)")
    flag(ap, "task", str, "sr", choices=["sr", "dn", "car"],
         text="--arch swinir: dn = denoising, car = JPEG compression-artifact reduction -- the published scale-1 models "
              "(finetune_swinir.build_restoration_model), scored from the HR directory of the test split alone: each image is degraded on the "
              "device as a whole (ops.restore_degrade; the noise id of an image is its index in the split) and the baseline is the degraded input "
              "itself.  They need --scale X1")
    shared_flags(ap, "channels")
    flag(ap, "dn_sigma", float, None, metavar="S",
         text="with --task dn (required) | car: the Gaussian noise sigma on the 0..255 scale of the papers (15 / 25 / 50)")
    shared_flags(ap, "dn_bits")
    ap.add_argument("--self_ensemble", action="store_true",
                    help="additive: predict with the x8 self-ensemble (the '+' of SwinIR+ / HAT+ / DAT+): the mean of the eight "
                         "inverse-transformed predictions on the flipped / rotated inputs (augment.self_ensemble)")
    ap.add_argument("--tile", type=int, default=0,
                    help="additive: predict on overlapping tiles of N x N input pixels and merge them (tiling.tiled_forward; 0 = off, "
                         "the whole image in one call; a tile at least as large as the image is the whole image too)")
    ap.add_argument("--tile_overlap", type=int, default=32, help="additive, with --tile: input pixels two neighbouring tiles share")
    ap.add_argument("--tile_batch", type=int, default=1, help="additive, with --tile: tiles per model call")
    ap.add_argument("--tile_blend", type=str, choices=["mean", "center"], default="mean",
                    help="additive, with --tile: mean = average the tiles covering a pixel (SwinIR's test script), center = take each "
                         "pixel from the tile whose border is farthest (what the tile_pad of the HAT / DAT scripts aims at)")
    ap.add_argument("--synth_lr", action="store_true",
                    help="additive, --arch swinir|hat|dat: evaluate from the HR directory of the test split alone; LR is its antialiased bicubic "
                         "(PIL BICUBIC convention) downscale, formed on the device (ops.resize_aa)")
    shared_flags(ap, "synth_lr_bits")
    flag(ap, "degrade", str, "bicubic", choices=["bicubic", "blind", "second_order"],
         text="with --synth_lr: blind = LR is blurred and noised with the fixed parameters below (ops.degrade_blind; the noise id of an image is "
              "its index in the split); second_order = the fixed second-order chain (sr_datasets.SecondOrderSpec.fixed, ops.degrade_second_order, "
              "DESIGN 7p): that blur and noise as stage 1, --jpeg_quality Q as the first JPEG's quality (default: the middle of 30..95), then the "
              "documented midpoints; it needs --synth_lr_bits 8")
    flag(ap, "blur_sigma", float, [1.1, 1.1], BLIND + "sigma of the Gaussian blur in HR pixels along y and x, within [0, 2.5]", nargs=2,
          metavar=("SY", "SX"))
    flag(ap, "noise_sigma", float, 5.0, BLIND + "noise sigma in 8-bit levels")
    flag(ap, "noise_gain", float, 0.0, BLIND + "gain of the signal-dependent noise")
    flag(ap, "blur_theta", float, None, metavar="DEG",
         text=BLIND + "the Gaussian of --blur_sigma turned by DEG degrees, applied as a 2-D table (blur_kernels.gaussian, ops.degrade_psf, "
              "csrc/blur2d.hip); 0 is the axis-aligned Gaussian on the 2-D path")
    flag(ap, "blur_psf", str, None, metavar="FILE",
         text=BLIND + "blur with table 0 of a measured point-spread function, .npy [k][k] or [n][k][k] (k odd <= 21, taps >= 0 summing to 1), instead "
              "of the Gaussian")
    flag(ap, "jpeg_quality", int, None, metavar="Q",
         text="with --synth_lr --synth_lr_bits 8 (either --degrade): the LR image makes a round trip through baseline JPEG at quality Q in 1..100 "
              "on the device (ops.jpeg_roundtrip, csrc/jpeg.hip), before any tiling or self-ensemble")
    shared_flags(ap, "jpeg_subsample")
    ap.add_argument("--gt_usm", action="store_true",
                    help="additive, " + SECOND + "score a model trained with finetune_swinir --gt_usm -- the HR image is unsharp-masked on the device "
                         "(ops.usm_sharpen, csrc/usm.hip, DESIGN 7r), the fixed chain (bicubic resizes) runs on the sharpened image and every score "
                         "is taken against it")
    shared_flags(ap, *USM_FLAGS)
    ap.add_argument("--bench_metric", type=str, choices=["y", "rgb"], default=None,
                    help="additive: also report PSNR / SSIM by the protocol of the SwinIR / HAT / DAT papers (metrics.bench_metrics): "
                         "8-bit, border-cropped, y = BT.601 luma of RGB (a single-channel image is its own luma), rgb = every channel, "
                         "0..255 scale, mean over images")
    ap.add_argument("--crop_border", type=int, default=None, metavar="N",
                    help="additive, with --bench_metric: pixels cropped on every side before scoring (default: the scale)")
    args = ap.parse_args(argv)
    if args.window_size is None:
        args.window_size = default_window_size(args.task)
    eval_specs(args, ap.error)          # the data-path flags in their order; nothing is kept: main() builds the run's specs
    if args.tile < 0 or args.tile_batch < 1 or args.tile_overlap < 0 or (args.tile and args.tile_overlap >= args.tile):
        ap.error(f"--tile must be >= 0, --tile_batch >= 1 and 0 <= --tile_overlap < --tile (got --tile {args.tile} "
                 f"--tile_overlap {args.tile_overlap} --tile_batch {args.tile_batch})")
    if not 2 <= args.window_size <= 8 or (args.window_size != 8 and args.arch != "swinir"):
        ap.error(f"--window_size must be in 2..8 and is an option of --arch swinir (got {args.window_size} with --arch {args.arch})")
    return args


def build_loader(args, specs, scale_int, swin, device):
    """-> (test_ds, test_loader) of the run's branch (--task dn | car and --synth_lr read the HR directory alone); the loader is wrapped so
    that the (degraded, clean) or (lr, hr) batches are formed on the device.  specs: the run's, from eval_specs."""
    tf_test = PairTransformValid(scale_int) if swin else build_pair_transform_eval()
    if specs.restore is not None:
        test_ds = Shuffled2DHR(args.data_root, split="test", transform=partial(clean_to_tensor, out_chans=args.channels))
    elif args.synth_lr:
        test_ds = Shuffled2DHR(args.data_root, split="test", transform=hr_to_tensor3)
    else:
        test_ds = Shuffled2DPaired(args.data_root, split="test", scale=args.scale, transform_pair=tf_test)
    test_loader = DataLoader(test_ds, batch_size=args.batch_size, shuffle=False, num_workers=args.workers,
                             pin_memory=(device.type == "cuda"), persistent_workers=False)
    if specs.restore is not None:
        test_loader = RestoreBatches(test_loader, args.channels, specs.restore, args.dn_bits, device)
    if args.synth_lr:
        test_loader = SynthLRBatches(test_loader, scale_int, args.synth_lr_bits, device, degrade=specs.degrade,
                                     jpeg=specs.jpeg, jpeg_subsample=args.jpeg_subsample == "420", psf=specs.psf, second_order=specs.second_order,
                                     usm=specs.usm)
    return test_ds, test_loader


def main(argv=None):
    args = parse_args(argv)

    device = torch.device(args.device) if args.device else torch.device("cuda" if torch.cuda.is_available() else "cpu")
    print("[device]", device, torch.cuda.get_device_name(0) if device.type == "cuda" else "-")
    swin = args.arch in ("swinir", "hat", "dat")
    if swin and device.type != "cuda":
        raise SystemExit(f"--arch {args.arch} runs on the MI355X HIP path only (no CPU fallback)")
    scale_int = SCALES[args.scale.upper()]
    specs = eval_specs(args)          # the run's fixed degradation, built once: the device wrapper and the lines share it
    restore = specs.restore is not None

    test_ds, test_loader = build_loader(args, specs, scale_int, swin, device)
    for line in eval_lines(args, specs, scale_int):
        print(line)
    print(f"[data] test samples: {len(test_ds)} | steps: {len(test_loader)}")

    def upscaled(lr, hr):
        """What is compared with HR as the 'bicubic' prediction: the eval transform already upscaled LR for MS_ResUNet; for
        SwinIR (raw LR input) it is done here."""
        if lr.shape[-2:] == hr.shape[-2:]:
            return lr
        return torch.nn.functional.interpolate(lr, size=hr.shape[-2:], mode="bicubic", align_corners=False).clamp(0, 1)

    for lr, hr in test_loader:                          # _peek_batch, :96-112
        lf, hf = torch.isfinite(lr), torch.isfinite(hr)
        print("[peek] lr min/max:", float(lr[lf].min()) if lf.any() else float("nan"), float(lr[lf].max()) if lf.any() else float("nan"),
              "| hr min/max:", float(hr[hf].min()) if hf.any() else float("nan"), float(hr[hf].max()) if hf.any() else float("nan"),
              "| shapes:", tuple(lr.shape), tuple(hr.shape))
        break

    bench = args.bench_metric is not None
    border = scale_int if args.crop_border is None else args.crop_border
    if bench:
        from .metrics import bench_metrics
    bench_ps, bench_ss, bench_bic_ps, bench_bic_ss = [], [], [], []          # per-image tensors, read once after each loop

    with torch.no_grad():                               # bicubic baseline, :115-134
        ps, ss = [], []
        for lr, hr in test_loader:
            lr, hr = lr.to(device, dtype=torch.float32), hr.to(device, dtype=torch.float32)
            up = upscaled(lr, hr)
            ps.append(psnr(up, hr, max_val=1.0))
            ss.append(float(ssim(up, hr, data_range=1.0, size_average=True)))
            if bench:
                bp, bs = bench_metrics(up, hr, border, args.bench_metric)
                bench_bic_ps.append(bp)
                bench_bic_ss.append(bs)
    base_name = "Degraded input" if restore else "Bicubic"          # at scale 1 the baseline is the degraded input itself
    print(f"[baseline] {base_name} PSNR: {sum(ps) / len(ps):.2f} dB | SSIM: {sum(ss) / len(ss):.4f}")
    more = {}
    if bench:
        tag = args.bench_metric.upper()

        def bench_line(what, p_list, s_list):
            """The mean over IMAGES (not over batches: a short last batch weighs what its images weigh)."""
            p_all, s_all = torch.cat(p_list), torch.cat(s_list)
            mp, ms = float(p_all.double().mean()), float(s_all.double().mean())
            print(f"[bench] {what}PSNR-{tag}: {mp:.2f} dB | SSIM-{tag}: {ms:.4f} (8-bit, border {border}, mean over {p_all.numel()} images)")
            return mp, ms

        more["bench_bicubic_psnr"], more["bench_bicubic_ssim"] = bench_line(base_name + " ", bench_bic_ps, bench_bic_ss)

    if swin:
        from .finetune_swinir import build_restoration_model, build_sr_model
        model = (build_restoration_model(args.task, args.channels, 0.0, args.window_size) if restore else
                 build_sr_model(args.arch, scale_int, drop_path_rate=0.0, window_size=args.window_size))
    else:
        model = MS_ResUNet()
    state, msg = _load_state(args.ckpt, args.param_key)
    model.load_state_dict(state, strict=True)
    print(msg)
    model = model.to(device).eval()
    predict = model
    if args.tile:
        from .tiling import tiled_forward
        predict = partial(tiled_forward, model, tile=args.tile, overlap=args.tile_overlap, tile_batch=args.tile_batch, blend=args.tile_blend)
        print(f"[tile] {args.tile} overlap {args.tile_overlap} batch {args.tile_batch} blend {args.tile_blend}")
    if args.self_ensemble:
        from .augment import self_ensemble
        predict = partial(self_ensemble, predict)
        print("[self_ensemble] x8")

    t0 = time.time()
    psnr_vals, ssim_vals = [], []
    out_dir = Path(args.save_dir)
    out_dir.mkdir(parents=True, exist_ok=True)
    saved = 0
    save_set = None
    if args.save_indices.strip():
        save_set = {int(x) for x in re.split(r"[,\s]+", args.save_indices.strip()) if x != ""}
        print(f"[save] explicit indices: {sorted(save_set)[:20]}{'...' if len(save_set) > 20 else ''}")
    elif args.save_every and args.save_every > 0:
        print(f"[save] every {args.save_every} samples starting at {args.save_start}")
    else:
        print(f"[save] first {args.save_n} samples (default mode)")

    global_idx = 0
    with torch.no_grad():
        for lr, hr in test_loader:
            lr, hr = lr.to(device, non_blocking=True), hr.to(device, non_blocking=True)
            with torch.amp.autocast("cuda", enabled=(device.type == "cuda" and not swin)):
                pred = predict(lr)
                if not torch.isfinite(pred).all():
                    bad = (~torch.isfinite(pred)).float().mean().item()
                    raise RuntimeError(f"Pred has non-finite values: share={bad:.6f}, min={torch.nanmin(pred).item():.4g}, "
                                       f"max={torch.nanmax(pred).item():.4g}")
            if pred.shape[-2:] != hr.shape[-2:]:
                pred = torch.nn.functional.interpolate(pred, size=hr.shape[-2:], mode="bilinear", align_corners=False)
            pred_f, hr_f = pred.to(torch.float32), hr.to(torch.float32)
            psnr_vals.append(psnr(pred_f, hr_f, max_val=1.0))
            ssim_vals.append(float(ssim(pred_f, hr_f, data_range=1.0, size_average=True)))
            if bench:
                bp, bs = bench_metrics(pred_f, hr_f, border, args.bench_metric)
                bench_ps.append(bp)
                bench_ss.append(bs)
            for b in range(pred.size(0)):
                idx = global_idx + b
                if save_set is not None:
                    want = idx in save_set
                elif args.save_every and args.save_every > 0:
                    want = idx >= args.save_start and (idx - args.save_start) % args.save_every == 0
                else:
                    want = saved < args.save_n
                if not want or saved >= args.save_n:       # --save_n caps every mode (:213-215)
                    continue
                stem = f"idx_{idx:06d}"
                save_tensor_as_png(lr[b], out_dir / f"{stem}_lr.png")
                save_tensor_as_png(hr[b], out_dir / f"{stem}_hr.png")
                save_tensor_as_png(pred[b], out_dir / f"{stem}_sr.png")
                saved += 1
            global_idx += pred.size(0)

    dt = time.time() - t0
    mean_psnr = sum(psnr_vals) / max(1, len(psnr_vals))
    mean_ssim = sum(ssim_vals) / max(1, len(ssim_vals))
    print(f"[done] test PSNR: {mean_psnr:.2f} dB | SSIM: {mean_ssim:.4f} | time: {dt:.1f}s for {len(test_ds)} samples")
    if bench:
        more["bench_psnr"], more["bench_ssim"] = bench_line("", bench_ps, bench_ss)
    print(f"[saved] examples in: {out_dir.resolve()}")
    return {"psnr": mean_psnr, "ssim": mean_ssim, "bicubic_psnr": sum(ps) / len(ps), "bicubic_ssim": sum(ss) / len(ss),
            "saved": saved, "n": len(test_ds), **more}


if __name__ == "__main__":
    main()
