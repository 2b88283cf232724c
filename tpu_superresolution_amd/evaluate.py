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
from pathlib import Path

import torch
from PIL import Image
from torch.utils.data import DataLoader

from .metrics import psnr, ssim
from .ms_resunet import MS_ResUNet
from .sr_datasets import Shuffled2DPaired
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


def _load_state(path: str, param_key: str = "auto"):
    """-> (state_dict, message).  'auto': the first of 'model', 'params', 'params_ema' the file has (the published HAT / DAT files hold
    only 'params_ema', the exponential moving average of the weights), else the file is a raw state_dict.  A named key must exist."""
    ckpt = torch.load(path, map_location="cpu", weights_only=True)
    if param_key != "auto":
        if param_key not in PARAM_KEYS:
            raise ValueError(f"param_key must be 'auto' or one of {PARAM_KEYS} (got {param_key!r})")
        if not isinstance(ckpt, dict) or param_key not in ckpt:
            have = [str(k) for k in ckpt] if isinstance(ckpt, dict) else []
            raise KeyError(f"{path}: no '{param_key}' key; the file has {have[:12]}{' ...' if len(have) > 12 else ''}")
        return ckpt[param_key], f"[ckpt] loaded state_dict from '{param_key}' key"
    if isinstance(ckpt, dict):
        for k in PARAM_KEYS:
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
    ap.add_argument("--task", type=str, choices=["sr", "dn", "car"], default="sr",
                    help="additive, --arch swinir: dn = denoising, car = JPEG compression-artifact reduction -- the published scale-1 "
                         "models (finetune_swinir.build_restoration_model), scored from the HR directory of the test split alone: each "
                         "image is degraded on the device as a whole (ops.restore_degrade; the noise id of an image is its index in the "
                         "split) and the baseline is the degraded input itself.  They need --scale X1")
    ap.add_argument("--channels", type=int, choices=[1, 3], default=3,
                    help="additive, with --task dn | car: 3 = colour, 1 = gray (an RGB file becomes its integer BT.601 luma, ops.to_gray)")
    ap.add_argument("--dn_sigma", type=float, default=None, metavar="S",
                    help="additive, with --task dn (required) | car: the Gaussian noise sigma on the 0..255 scale of the papers (15 / 25 / 50)")
    ap.add_argument("--dn_bits", type=int, choices=[0, 8], default=0,
                    help="additive, with --task dn | car: 0 = the noisy input is neither clipped nor rounded, 8 = rounded to k / 255")
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
                    help="additive, --arch swinir|hat|dat: evaluate from the HR directory of the test split alone; LR is its antialiased "
                         "bicubic (PIL BICUBIC convention) downscale, formed on the device (ops.resize_aa)")
    ap.add_argument("--synth_lr_bits", type=int, choices=[0, 8], default=8,
                    help="additive, with --synth_lr: 8 = LR rounded to k / 255 as an 8-bit LR file would hold it, 0 = the filtered values")
    ap.add_argument("--degrade", type=str, choices=["bicubic", "blind", "second_order"], default="bicubic",
                    help="additive, with --synth_lr: blind = LR is blurred and noised with the fixed parameters below (ops.degrade_blind; "
                         "the noise id of an image is its index in the split); second_order = the fixed second-order chain "
                         "(sr_datasets.SecondOrderSpec.fixed, ops.degrade_second_order, DESIGN 7p): that blur and noise as stage 1, "
                         "--jpeg_quality Q as the first JPEG's quality (default: the middle of 30..95), then the documented midpoints; it "
                         "needs --synth_lr_bits 8")
    ap.add_argument("--blur_sigma", type=float, nargs=2, default=[1.1, 1.1], metavar=("SY", "SX"),
                    help="additive, with --degrade blind: sigma of the Gaussian blur in HR pixels along y and x, within [0, 2.5]")
    ap.add_argument("--noise_sigma", type=float, default=5.0, help="additive, with --degrade blind: noise sigma in 8-bit levels")
    ap.add_argument("--noise_gain", type=float, default=0.0, help="additive, with --degrade blind: gain of the signal-dependent noise")
    ap.add_argument("--blur_theta", type=float, default=None, metavar="DEG",
                    help="additive, with --degrade blind: the Gaussian of --blur_sigma turned by DEG degrees, applied as a 2-D table "
                         "(blur_kernels.gaussian, ops.degrade_psf, csrc/blur2d.hip); 0 is the axis-aligned Gaussian on the 2-D path")
    ap.add_argument("--blur_psf", type=str, default=None, metavar="FILE",
                    help="additive, with --degrade blind: blur with table 0 of a measured point-spread function, .npy [k][k] or [n][k][k] "
                         "(k odd <= 21, taps >= 0 summing to 1), instead of the Gaussian")
    ap.add_argument("--jpeg_quality", type=int, default=None, metavar="Q",
                    help="additive, with --synth_lr --synth_lr_bits 8 (either --degrade): the LR image makes a round trip through baseline "
                         "JPEG at quality Q in 1..100 on the device (ops.jpeg_roundtrip, csrc/jpeg.hip), before any tiling or self-ensemble")
    ap.add_argument("--jpeg_subsample", type=str, choices=["444", "420"], default="444",
                    help="additive, with --jpeg_quality: chroma at 4:4:4, or 4:2:0 (2 x 2 means, upsampled by replication)")
    ap.add_argument("--gt_usm", action="store_true",
                    help="additive, with --degrade second_order: score a model trained with finetune_swinir --gt_usm -- the HR image is "
                         "unsharp-masked on the device (ops.usm_sharpen, csrc/usm.hip, DESIGN 7r), the fixed chain (bicubic resizes) runs "
                         "on the sharpened image and every score is taken against it")
    ap.add_argument("--usm_radius", type=int, default=None, help="additive, with --gt_usm: Real-ESRGAN's radius, 1..51 (default 50)")
    ap.add_argument("--usm_weight", type=float, default=None, help="additive, with --gt_usm: weight of the residual (default 0.5)")
    ap.add_argument("--usm_threshold", type=float, default=None, help="additive, with --gt_usm: threshold of the mask in 8-bit levels (default 10)")
    ap.add_argument("--bench_metric", type=str, choices=["y", "rgb"], default=None,
                    help="additive: also report PSNR / SSIM by the protocol of the SwinIR / HAT / DAT papers (metrics.bench_metrics): "
                         "8-bit, border-cropped, y = BT.601 luma of RGB (a single-channel image is its own luma), rgb = every channel, "
                         "0..255 scale, mean over images")
    ap.add_argument("--crop_border", type=int, default=None, metavar="N",
                    help="additive, with --bench_metric: pixels cropped on every side before scoring (default: the scale)")
    args = ap.parse_args(argv)
    if args.window_size is None:
        args.window_size = 7 if args.task == "car" else 8
    if args.task == "sr":
        if args.scale == "X1":
            ap.error("--scale X1 is the scale of --task dn | car; --task sr takes X2 | X4")
        if args.channels != 3 or args.dn_sigma is not None or args.dn_bits != 0:
            ap.error("--channels, --dn_sigma and --dn_bits are options of --task dn | car")
    else:
        if args.scale != "X1":
            ap.error(f"--task {args.task} restores at one size: it needs --scale X1 (got {args.scale})")
        if args.arch != "swinir":
            ap.error(f"--task {args.task} is built for --arch swinir only (HAT and DAT end in a pixel-shuffle tail; got --arch {args.arch})")
        if args.synth_lr or args.degrade != "bicubic":
            ap.error(f"--synth_lr and --degrade form LR images for --task sr; --task {args.task} degrades at scale 1 on its own")
        if args.task == "dn" and args.dn_sigma is None:
            ap.error("--task dn needs --dn_sigma S (0..255 scale, e.g. 25)")
        if args.task == "dn" and args.jpeg_quality is not None:
            ap.error("--jpeg_quality with noise is --task car --dn_sigma S; --task dn has no JPEG stage")
        if args.task == "car" and args.jpeg_quality is None:
            ap.error("--task car needs --jpeg_quality Q")
        if args.bench_metric is not None and args.channels == 1:
            ap.error("--bench_metric is not offered with --channels 1 (the benchmark-protocol scores take RGB predictions)")
        try:
            eval_restore(args)
        except ValueError as e:
            ap.error(f"--task {args.task}: {e}")
    if args.crop_border is not None:
        if args.bench_metric is None:
            ap.error("--crop_border is an option of the benchmark-protocol scores: it needs --bench_metric y | rgb")
        if args.crop_border < 0:
            ap.error(f"--crop_border must be >= 0 (got {args.crop_border})")
    if args.synth_lr and args.arch == "ms_resunet":
        ap.error("--synth_lr is an option of --arch swinir | hat | dat (MS_ResUNet takes the pre-upscaled LR of the eval transform)")
    if args.degrade == "second_order" and args.synth_lr_bits != 8:
        ap.error("--degrade second_order codes 8-bit LR images: it needs --synth_lr_bits 8")
    if args.degrade in ("blind", "second_order"):
        if not args.synth_lr:
            ap.error(f"--degrade {args.degrade} degrades the HR images on the device: it needs --synth_lr")
        try:
            from .ops import pack_degrade_params
            pack_degrade_params(args.blur_sigma, (args.noise_sigma / 255.0, args.noise_gain), 0, False)
        except ValueError as e:
            ap.error(f"--degrade {args.degrade}: {e}")
    usm_opts = [n for n in ("usm_radius", "usm_weight", "usm_threshold") if getattr(args, n) is not None]
    if args.gt_usm and args.degrade != "second_order":
        ap.error("--gt_usm sharpens the target of --degrade second_order: it needs it")
    if usm_opts and not args.gt_usm:
        ap.error(f"--{usm_opts[0]} is an option of --gt_usm")
    try:
        eval_usm(args)
    except ValueError as e:
        ap.error(f"--gt_usm: {e}")
    if (args.blur_theta is not None or args.blur_psf is not None) and args.degrade not in ("blind", "second_order"):
        ap.error("--blur_theta and --blur_psf shape the blur of --degrade blind | second_order: they need it")
    if args.blur_theta is not None and args.blur_psf is not None:
        ap.error("--blur_psf FILE replaces the Gaussian: it does not go with --blur_theta")
    try:
        eval_psf(args)
    except (ValueError, OSError) as e:
        ap.error(f"--blur_theta / --blur_psf: {e}")
    if args.jpeg_quality is None:
        if args.jpeg_subsample != "444" and args.degrade != "second_order":
            ap.error("--jpeg_subsample is an option of the JPEG stage: it needs --jpeg_quality Q")
    elif args.task == "sr":
        if not args.synth_lr:
            ap.error("--jpeg_quality codes the LR images formed on the device: it needs --synth_lr")
        if args.synth_lr_bits != 8:
            ap.error("--jpeg_quality codes 8-bit LR images: it needs --synth_lr_bits 8")
        if not 1 <= args.jpeg_quality <= 100:
            ap.error(f"--jpeg_quality must be in 1..100 (got {args.jpeg_quality})")
    if args.tile < 0 or args.tile_batch < 1 or args.tile_overlap < 0 or (args.tile and args.tile_overlap >= args.tile):
        ap.error(f"--tile must be >= 0, --tile_batch >= 1 and 0 <= --tile_overlap < --tile (got --tile {args.tile} "
                 f"--tile_overlap {args.tile_overlap} --tile_batch {args.tile_batch})")
    if not 2 <= args.window_size <= 8 or (args.window_size != 8 and args.arch != "swinir"):
        ap.error(f"--window_size must be in 2..8 and is an option of --arch swinir (got {args.window_size} with --arch {args.arch})")
    return args


def eval_restore(args):
    """The FixedRestore of the command line (None for --task sr); --dn_sigma is given on the 0..255 scale."""
    if args.task == "sr":
        return None
    from .ops import pack_restore_params
    from .sr_datasets import FixedRestore
    fx = FixedRestore((args.dn_sigma or 0.0) / 255.0, args.jpeg_quality or 0, False, args.jpeg_subsample == "420")
    pack_restore_params(fx.jpeg_quality, (fx.sigma, 0.0), 0, False)          # the ranges
    return fx


def eval_usm(args):
    """The UsmSpec of the command line (None without --gt_usm): training's rule, finetune_swinir.usm_spec."""
    from .finetune_swinir import usm_spec
    return usm_spec(args)


def eval_psf(args):
    """The 2-D blur table of the command line: table 0 of --blur_psf, the rotated Gaussian of --blur_theta (sigma_x along the columns at
    0 degrees, as on the separable path; a sigma of 0 is floored as in sr_datasets.PsfSpec), or None."""
    if args.blur_psf is not None:
        from .blur_kernels import load_psf_file
        return load_psf_file(args.blur_psf)[0]
    if args.blur_theta is None:
        return None
    import math

    from .blur_kernels import gaussian
    from .sr_datasets import PSF_SIGMA_FLOOR
    if not math.isfinite(args.blur_theta):
        raise ValueError(f"--blur_theta must be finite (got {args.blur_theta})")
    sy, sx = (max(float(v), PSF_SIGMA_FLOOR) for v in args.blur_sigma)
    return gaussian(2 * min(math.ceil(3.0 * max(float(v) for v in args.blur_sigma)), 10) + 1, sx, sy, math.radians(args.blur_theta))


def main(argv=None):
    args = parse_args(argv)

    device = torch.device(args.device) if args.device else torch.device("cuda" if torch.cuda.is_available() else "cpu")
    print("[device]", device, torch.cuda.get_device_name(0) if device.type == "cuda" else "-")
    swin = args.arch in ("swinir", "hat", "dat")
    if swin and device.type != "cuda":
        raise SystemExit(f"--arch {args.arch} runs on the MI355X HIP path only (no CPU fallback)")
    scale_int = {"X1": 1, "X2": 2, "X4": 4}[args.scale.upper()]
    restore = args.task != "sr"

    if swin:
        from .sr_datasets import PairTransformValid
        tf_test = PairTransformValid(scale_int)
    else:
        tf_test = build_pair_transform_eval()
    if restore:
        from functools import partial

        from .sr_datasets import RestoreBatches, Shuffled2DHR, clean_to_tensor
        test_ds = Shuffled2DHR(args.data_root, split="test", transform=partial(clean_to_tensor, out_chans=args.channels))
    elif args.synth_lr:
        from .sr_datasets import Shuffled2DHR, SynthLRBatches, hr_to_tensor3
        test_ds = Shuffled2DHR(args.data_root, split="test", transform=hr_to_tensor3)
    else:
        test_ds = Shuffled2DPaired(args.data_root, split="test", scale=args.scale, transform_pair=tf_test)
    test_loader = DataLoader(test_ds, batch_size=args.batch_size, shuffle=False, num_workers=args.workers,
                             pin_memory=(device.type == "cuda"), persistent_workers=False)
    if restore:          # (degraded, clean) batches formed on the device
        fx = eval_restore(args)
        test_loader = RestoreBatches(test_loader, args.channels, fx, args.dn_bits, device)
        print(f"[task {args.task}] {args.channels} channel(s); degraded = whole image on the device: noise sigma={fx.sigma * 255.0:.4g} / 255 "
              f"({args.dn_bits or 'no'}-bit rounding), jpeg quality {fx.jpeg_quality or 'none'} chroma {args.jpeg_subsample}, noise id = image index")
    if args.synth_lr:          # (lr, hr) batches formed on the device, before the peek, the baseline and the prediction loop
        fixed = second = None
        if args.degrade in ("blind", "second_order"):
            from .sr_datasets import FixedDegrade
            fixed = FixedDegrade(tuple(args.blur_sigma), (args.noise_sigma / 255.0, args.noise_gain))
        if args.degrade == "second_order":
            from .sr_datasets import SecondOrderSpec
            second = SecondOrderSpec() if args.jpeg_quality is None else SecondOrderSpec(jpeg_quality=(args.jpeg_quality,) * 2)
        test_loader = SynthLRBatches(test_loader, scale_int, args.synth_lr_bits, device, degrade=fixed,
                                     jpeg=None if second is not None else args.jpeg_quality, jpeg_subsample=args.jpeg_subsample == "420",
                                     psf=eval_psf(args), second_order=second, usm=eval_usm(args))
        print(f"[synth_lr] LR = antialiased bicubic /{scale_int} of HR on the device, {args.synth_lr_bits or 'no'}-bit rounding")
        if fixed is not None:
            print(f"[degrade] blind: blur sigma=({fixed.blur[0]:.4g}, {fixed.blur[1]:.4g}) HR px, noise sigma={args.noise_sigma:.4g} / 255 "
                  f"gain={args.noise_gain:.4g}, noise id = image index")
        if eval_psf(args) is not None:
            k = eval_psf(args)
            print(f"[degrade] blur kernel: {k.shape[0]} x {k.shape[0]} table, " + (f"table 0 of {args.blur_psf}" if args.blur_psf is not None else
                                                                                    f"the Gaussian turned by {args.blur_theta:g} degrees"))
        if second is not None:
            fx2 = second.fixed(None, fixed.noise)
            print(f"[degrade] second order, fixed: resize x{fx2.r1:.4g}, jpeg {fx2.q1}, blur 2 {fx2.k2.shape[0]} taps, resize x{fx2.r2:.4g} of LR, "
                  f"noise sigma={fx2.noise2[0] * 255.0:.4g} / 255, jpeg {fx2.q2}, final filter {fx2.k3.shape[0]} taps, chroma {args.jpeg_subsample}")
            if args.gt_usm:
                us = eval_usm(args)
                print(f"[degrade] gt_usm: HR is unsharp-masked ({us.ks} taps, weight {us.weight:g}, threshold {us.threshold:g} / 255); LR is "
                      f"degraded from it and every score is taken against it")
        elif args.jpeg_quality is not None:
            print(f"[degrade] jpeg: quality {args.jpeg_quality}, chroma {args.jpeg_subsample}")
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
        from functools import partial

        from .tiling import tiled_forward
        predict = partial(tiled_forward, model, tile=args.tile, overlap=args.tile_overlap, tile_batch=args.tile_batch, blend=args.tile_blend)
        print(f"[tile] {args.tile} overlap {args.tile_overlap} batch {args.tile_batch} blend {args.tile_blend}")
    if args.self_ensemble:
        from functools import partial

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
