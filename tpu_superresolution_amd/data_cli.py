"""The command-line layer of the data path, shared by finetune_swinir.py and evaluate.py: the scale and task tables, the
declarations of training's flags from --synth_lr on and of the flags both scripts take alike, the cross-flag checks (written once, the
words that differ passed in), the spec builders, ``saved_args`` (derived from the parser's own defaults) and a run's [task ...] / [degrade]
lines.  ``train_specs`` / ``eval_specs`` check a script's flags in a fixed order and build each spec once, where its errors are reported:
parse_args calls them with ``ap.error`` and drops the result (vars(args) is what a checkpoint saves), main() calls them again.  Host code."""
from __future__ import annotations

import math
from collections import namedtuple

from .blur_kernels import gaussian, load_psf_file
from .degrade_specs import (PSF_SIGMA_FLOOR, DegradeSpec, FixedDegrade, FixedRestore, JpegSpec, PsfSpec, RestoreSpec, SecondOrderSpec, UsmSpec)
from .image_ops import pack_degrade_params, pack_restore_params

SCALES = {"X1": 1, "X2": 2, "X4": 4}
RESTORATION_TASKS = {"dn": dict(window_size=8, img_size=128, img_range=1.0), "car": dict(window_size=7, img_size=126, img_range=255.0)}
SECOND_ORDER_FLAGS = ("blur2_sigma", "blur2_p", "noise2_sigma", "jpeg2_quality", "resize_range", "resize_prob", "resize2_range", "resize2_prob",
                      "sinc_p", "final_sinc_p", "degrade_margin", "resize_mode_prob")
USM_FLAGS = ("usm_radius", "usm_weight", "usm_threshold")
TWO_D = ("blind", "second_order")          # the --degrade values that blur and noise


def default_window_size(task: str) -> int:
    """--window_size when it is not given: the task's published window (7 for car), 8 for super-resolution."""
    return RESTORATION_TASKS[task]["window_size"] if task != "sr" else 8


RANGE, UP_DOWN_KEEP = dict(nargs=2, metavar=("LO", "HI")), dict(nargs=3, metavar=("UP", "DOWN", "KEEP"))
BLIND, MIXED, SECOND = "with --degrade blind: ", "with --blur_kernel mixed: ", "with --degrade second_order: "


def flag(ap, name, typ, default, text, **kw) -> None:
    """Declares --name; every flag of the data path is additive to the reference's command line, and its help says so first."""
    ap.add_argument("--" + name, type=typ, default=default, help="additive, " + text, **kw)


SHARED_FLAGS = {          # declared alike by both scripts: shared_flags(ap, name) at the flag's place in either parser
    "channels": (int, 3, "with --task dn | car: 3 = colour, 1 = gray (an RGB file becomes its integer BT.601 luma, ops.to_gray)", [1, 3]),
    "dn_bits": (int, 0, "with --task dn | car: 0 = the noisy input is neither clipped nor rounded, as the published training has it; 8 = rounded "
                        "to k / 255", [0, 8]),
    "synth_lr_bits": (int, 8, "with --synth_lr: 8 = round the LR values to k / 255, as an 8-bit LR file would hold them; 0 = keep the filtered fp32 "
                              "values", [0, 8]),
    "jpeg_subsample": (str, "444", "with --jpeg_quality: chroma at 4:4:4, or 4:2:0 (2 x 2 means, upsampled by replication)", ["444", "420"]),
    "usm_radius": (int, None, "with --gt_usm: Real-ESRGAN's radius, 1..51 (default 50: 51 taps, sigma 8)", None),
    "usm_weight": (float, None, "with --gt_usm: weight of the residual (default 0.5)", None),
    "usm_threshold": (float, None, "with --gt_usm: threshold of the mask in 8-bit levels (default 10)", None),
}


def shared_flags(ap, *names) -> None:
    for n in names:
        flag(ap, n, *SHARED_FLAGS[n][:3], choices=SHARED_FLAGS[n][3])


def add_train_data_flags(ap) -> None:
    """finetune_swinir's flags from --synth_lr on: how the (LR, HR) pairs of a run are made on the device."""
    ap.add_argument("--synth_lr", action="store_true",
                    help="additive, with --gpu_data: train and validate from the HR directories alone -- every LR patch is the antialiased bicubic "
                         "(PIL BICUBIC convention) downscale of its HR image, computed on the device in the launch that crops the HR patch "
                         "(sr_datasets.DeviceHRPool); no LR directory is required or read")
    shared_flags(ap, "synth_lr_bits")
    flag(ap, "degrade", str, "bicubic", choices=["bicubic", "blind", "second_order"],
         text="with --synth_lr: blind = every LR training patch is blurred (Gaussian, composed into the bicubic taps) and noised with random "
              "per-sample parameters on the device (sr_datasets.DegradeSpec, csrc/degrade.hip); validation uses the midpoints of the ranges and "
              "fixed noise, the same LR images every epoch.  second_order = Real-ESRGAN's chain on the device -- blur, resize, noise, JPEG, twice, "
              "each sample at its own intermediate sizes, then a sinc filter (sr_datasets.SecondOrderSpec / DeviceHR2Pool, csrc/filter2d.hip, "
              "csrc/ragged.hip; DESIGN 7p).  Stage 1 takes the options of blind (--blur_sigma, --blur_kernel*, --noise_sigma, --noise_gain, "
              "--gray_noise_p, --jpeg_quality); it needs --synth_lr_bits 8")
    flag(ap, "blur_sigma", float, [0.2, 2.0], BLIND + "range of the blur sigma in HR pixels, within [0, 2.5]", **RANGE)
    flag(ap, "blur_aniso_p", float, 0.5, BLIND + "probability of an independent sigma_x (otherwise sigma_x = sigma_y)")
    flag(ap, "noise_sigma", float, [0.0, 10.0], BLIND + "range of the signal-independent noise sigma in 8-bit levels (divided by 255)", **RANGE)
    flag(ap, "noise_gain", float, [0.0, 0.0], BLIND + "range of the gain of the signal-dependent (Poisson-like) noise variance gain * v", **RANGE)
    flag(ap, "gray_noise_p", float, 0.4, BLIND + "probability that a colour image gets one noise draw for its three channels")
    flag(ap, "degrade_seed", int, 0, BLIND + "seed of the degradation parameters' own generator (+ rank)")
    flag(ap, "jpeg_quality", int, None, **RANGE,
         text="with --synth_lr --synth_lr_bits 8 (either --degrade): every LR training patch makes a round trip through baseline JPEG on the device "
              "at a quality uniform in LO..HI (1..100; sr_datasets.JpegSpec, csrc/jpeg.hip; its own generator, seeded by --degrade_seed + rank); "
              "validation uses the middle of the range")
    flag(ap, "jpeg_p", float, 1.0, "with --jpeg_quality: probability that a training patch takes the JPEG stage (otherwise it passes through)")
    shared_flags(ap, "jpeg_subsample")
    flag(ap, "blur_kernel", str, "axis", choices=["axis", "rotated", "mixed"],
         text=BLIND + "the blur of a training patch -- 'axis': the axis-aligned Gaussian composed into the bicubic taps; 'rotated': the same Gaussian "
              "turned by a random angle; 'mixed': Real-ESRGAN's pool of (an)isotropic, generalized and plateau kernels -- as a 2-D table on the "
              "device (sr_datasets.PsfSpec, csrc/blur2d.hip; its own generator, seeded by --degrade_seed + rank); validation keeps the isotropic "
              "midpoints")
    flag(ap, "blur_kernel_prob", float, None, nargs=6, metavar="P",
         text=MIXED + "probabilities of iso, aniso, generalized iso, generalized aniso, plateau iso, plateau aniso (default 0.45 0.25 0.12 0.03 "
              "0.12 0.03)")
    flag(ap, "blur_beta_g", float, None, MIXED + "range of the generalized Gaussian's shape beta (default 0.5 4)", **RANGE)
    flag(ap, "blur_beta_p", float, None, MIXED + "range of the plateau kernel's shape beta (default 1 2)", **RANGE)
    flag(ap, "blur_ksize", int, None, MIXED + "range of the odd table size (default 7 21)", **RANGE)
    flag(ap, "blur_psf", str, None, metavar="FILE",
         text=BLIND + "a measured point-spread function, .npy [k][k] or [n][k][k] (k odd <= 21, taps >= 0 summing to 1); every training patch is "
              "blurred with one of its tables, validation with table 0")
    flag(ap, "degrade_tables", str, "host", choices=["host", "device"],
         text="with --degrade blind and --blur_kernel rotated | mixed or --blur_psf, or with --degrade second_order: where the blur and sinc tables "
              "of a training batch are evaluated -- 'host': in fp64 numpy, then uploaded; 'device': on the GPU from eight numbers per table "
              "(csrc/tables.hip, DESIGN 7q), the same draws and decisions, every tap within one fp32 spacing of the host's.  Validation keeps its "
              "fixed host tables")
    flag(ap, "blur2_sigma", float, None, SECOND + "range of the sigmas of the second blur, a rotated Gaussian (default 0.2 1.5)", **RANGE)
    flag(ap, "blur2_p", float, None, SECOND + "probability of the second blur (default 0.8)")
    flag(ap, "noise2_sigma", float, None, SECOND + "range of the second noise sigma in 8-bit levels (default 1 25)", **RANGE)
    flag(ap, "jpeg2_quality", int, None, SECOND + "quality range of the second JPEG (default 30 95; --jpeg_quality is the first's)", **RANGE)
    flag(ap, "resize_range", float, None, SECOND + "factors of the first resize, LO <= 1 <= HI (default 0.15 1.5)", **RANGE)
    flag(ap, "resize_prob", float, None, SECOND + "probabilities of the first resize going up, down, or staying (default 0.2 0.7 0.1)", **UP_DOWN_KEEP)
    flag(ap, "resize2_range", float, None, SECOND + "factors of the second resize, relative to the LR size (default 0.3 1.2)", **RANGE)
    flag(ap, "resize2_prob", float, None, SECOND + "probabilities of the second resize (default 0.3 0.4 0.3)", **UP_DOWN_KEEP)
    flag(ap, "sinc_p", float, None, SECOND + "probability that a blur is a sinc (ringing) filter, at both stages (default 0.1)")
    flag(ap, "final_sinc_p", float, None, SECOND + "probability of the final sinc filter (default 0.8)")
    flag(ap, "degrade_margin", int, None, SECOND + "LR pixels around the patch that the chain also runs on (default 8)")
    flag(ap, "resize_mode_prob", float, None, nargs=3, metavar=("AREA", "BILINEAR", "BICUBIC"),
         text=SECOND + "probabilities of the rule of each of the three resizes of a training patch (csrc/resize_modes.hip, DESIGN 7r; Real-ESRGAN draws "
              "among the three; default 0 0 1, the antialiased cubic).  Validation keeps the cubic")
    ap.add_argument("--gt_usm", action="store_true",
                    help="additive, " + SECOND + "Real-ESRGAN's gt_usm -- the HR window is unsharp-masked once on the device (csrc/usm.hip, DESIGN 7r), "
                         "the LR patch is degraded from the sharpened window and the loss is taken against it; validation scores against the "
                         "sharpened image.  --degrade_margin 13 at X4 (25 at X2) keeps the window's reflected edge out of the patch")
    shared_flags(ap, *USM_FLAGS)
    ap.add_argument("--task", type=str, choices=["sr", "dn", "car"], default="sr",
                    help="additive: sr = super-resolution (as ever); dn = denoising, car = JPEG compression-artifact reduction: the published "
                         "scale-1 SwinIR models (build_restoration_model), trained from the HR directories alone -- every patch is cut at any image "
                         "pixel and degraded on the device as a window of the whole-image degradation (sr_datasets.DeviceRestorePool, "
                         "csrc/restore.hip).  They need --scale X1 and imply --gpu_data")
    shared_flags(ap, "channels")
    flag(ap, "dn_sigma", float, None, **RANGE,
         text="with --task dn (required) | car: range of the Gaussian noise sigma on the 0..255 scale of the papers (15 / 25 / 50; divided by 255); "
              "validation uses the midpoint")
    shared_flags(ap, "dn_bits")


def degrade_spec(args):
    """The DegradeSpec of the command line (None for --degrade bicubic); --noise_sigma is given in 8-bit levels."""
    if args.degrade not in TWO_D:
        return None
    return DegradeSpec(blur_sigma=tuple(args.blur_sigma), blur_aniso_p=args.blur_aniso_p, noise_sigma=tuple(v / 255.0 for v in args.noise_sigma),
                       noise_gain=tuple(args.noise_gain), gray_noise_p=args.gray_noise_p, seed=args.degrade_seed)


def psf_spec(args):
    """The PsfSpec of the command line (None for --blur_kernel axis without --blur_psf); it reuses --degrade_seed.  Every call reads FILE."""
    if args.blur_psf is not None:
        return PsfSpec(mode="file", file=args.blur_psf, seed=args.degrade_seed)
    if args.blur_kernel == "axis":
        return None
    opts = {k: tuple(v) for k, v in (("kernel_prob", args.blur_kernel_prob), ("beta_g", args.blur_beta_g), ("beta_p", args.blur_beta_p),
                                     ("ksize", args.blur_ksize)) if v is not None}
    return PsfSpec(mode=args.blur_kernel, seed=args.degrade_seed, **opts)


def jpeg_spec(args):
    """The JpegSpec of the command line (None without --jpeg_quality, and with --degrade second_order, whose first JPEG takes the
    range); it reuses --degrade_seed."""
    if args.jpeg_quality is None or args.degrade == "second_order":
        return None
    return JpegSpec(quality=tuple(args.jpeg_quality), p=args.jpeg_p, subsample=args.jpeg_subsample == "420", seed=args.degrade_seed)


def usm_spec(args):
    """The UsmSpec of the command line (None without --gt_usm): the flags that were given replace Real-ESRGAN's defaults.  Both scripts."""
    if not args.gt_usm:
        return None
    return UsmSpec(**{k: v for k, v in (("radius", args.usm_radius), ("weight", args.usm_weight), ("threshold", args.usm_threshold)) if v is not None})


def second_order_spec(args):
    """The SecondOrderSpec of the command line (None unless --degrade second_order): the flags that were given replace Real-ESRGAN's
    defaults; --noise2_sigma is given in 8-bit levels, --jpeg_quality is the first JPEG's range; it reuses --degrade_seed,
    --gray_noise_p and --blur_ksize."""
    if args.degrade != "second_order":
        return None
    opts = {k: (v if isinstance(v, float) else tuple(v)) for k, v in (
        ("blur2_sigma", args.blur2_sigma), ("blur2_p", args.blur2_p), ("jpeg2_quality", args.jpeg2_quality), ("resize_range", args.resize_range),
        ("resize_prob", args.resize_prob), ("resize2_range", args.resize2_range), ("resize2_prob", args.resize2_prob), ("sinc_p", args.sinc_p),
        ("final_sinc_p", args.final_sinc_p), ("jpeg_quality", args.jpeg_quality), ("ksize", args.blur_ksize),
        ("resize_mode_prob", args.resize_mode_prob)) if v is not None}
    if args.noise2_sigma is not None:
        opts["noise2_sigma"] = tuple(v / 255.0 for v in args.noise2_sigma)
    return SecondOrderSpec(gray_noise_p=args.gray_noise_p, seed=args.degrade_seed, **opts)


def restore_spec(args):
    """The RestoreSpec of the command line (None for --task sr); --dn_sigma is given on the 0..255 scale; it reuses --degrade_seed and
    --gray_noise_p is not consulted: a colour image gets colour noise, as in the published training."""
    if args.task == "sr":
        return None
    sigma = (0.0, 0.0) if args.dn_sigma is None else tuple(v / 255.0 for v in args.dn_sigma)
    return RestoreSpec(sigma=sigma, jpeg_quality=None if args.jpeg_quality is None else tuple(args.jpeg_quality),
                       subsample=args.jpeg_subsample == "420", seed=args.degrade_seed)


def eval_restore(args):
    """The FixedRestore of evaluate's command line (None for --task sr); --dn_sigma is given on the 0..255 scale."""
    if args.task == "sr":
        return None
    fx = FixedRestore((args.dn_sigma or 0.0) / 255.0, args.jpeg_quality or 0, False, args.jpeg_subsample == "420")
    pack_restore_params(fx.jpeg_quality, (fx.sigma, 0.0), 0, False)          # the ranges
    return fx


def eval_psf(args):
    """The 2-D blur table of evaluate's command line: table 0 of --blur_psf, the rotated Gaussian of --blur_theta (sigma_x along the
    columns at 0 degrees, as on the separable path; a sigma of 0 is floored as in sr_datasets.PsfSpec), or None."""
    if args.blur_psf is not None:
        return load_psf_file(args.blur_psf)[0]
    if args.blur_theta is None:
        return None
    if not math.isfinite(args.blur_theta):
        raise ValueError(f"--blur_theta must be finite (got {args.blur_theta})")
    sy, sx = (max(float(v), PSF_SIGMA_FLOOR) for v in args.blur_sigma)
    return gaussian(2 * min(math.ceil(3.0 * max(float(v) for v in args.blur_sigma)), 10) + 1, sx, sy, math.radians(args.blur_theta))


def _raise(message: str):
    raise ValueError(message)


def _built(fail, prefix, build, args, errors=(ValueError,)):
    """build(args), its refusal reported as '<prefix>: <reason>'."""
    try:
        return build(args)
    except errors as e:
        fail(f"{prefix}: {e}")


def check_task(args, fail, build, sigma="LO HI", sigma_eg="25 25", quality="LO HI", bench="val_bench_metric", jpeg_p=1.0):
    """The --task sr | dn | car block -> the restoration spec (None for sr).  The defaults word training's messages; jpeg_p is its flag."""
    if args.task == "sr":
        if args.scale == "X1":
            fail("--scale X1 is the scale of --task dn | car; --task sr takes X2 | X4")
        if args.channels != 3 or args.dn_sigma is not None or args.dn_bits != 0:
            fail("--channels, --dn_sigma and --dn_bits are options of --task dn | car")
        return None
    if args.scale != "X1":
        fail(f"--task {args.task} restores at one size: it needs --scale X1 (got {args.scale})")
    if args.arch != "swinir":
        fail(f"--task {args.task} is built for --arch swinir only (HAT and DAT end in a pixel-shuffle tail; got --arch {args.arch})")
    if args.synth_lr or args.degrade != "bicubic":
        fail(f"--synth_lr and --degrade form LR images for --task sr; --task {args.task} degrades at scale 1 on its own")
    if args.task == "dn" and args.dn_sigma is None:
        fail(f"--task dn needs --dn_sigma {sigma} (0..255 scale, e.g. {sigma_eg})")
    if args.task == "dn" and args.jpeg_quality is not None:
        fail(f"--jpeg_quality with noise is --task car --dn_sigma {sigma}; --task dn has no JPEG stage")
    if args.task == "car" and args.jpeg_quality is None:
        fail(f"--task car needs --jpeg_quality {quality}")
    if jpeg_p != 1.0:
        fail(f"--jpeg_p is an option of the JPEG stage of --synth_lr; with --task {args.task} every patch is coded")
    if getattr(args, bench) is not None and args.channels == 1:
        fail(f"--{bench} is not offered with --channels 1 (the benchmark-protocol scores take RGB predictions)")
    return _built(fail, f"--task {args.task}", build, args)


def check_degrade(args, fail, build, what="HR patches"):
    """--degrade blind | second_order needs --synth_lr and parameters in range -> the blur-and-noise spec (None for bicubic)."""
    if args.degrade in TWO_D and not args.synth_lr:
        fail(f"--degrade {args.degrade} degrades {what} on the device: it needs --synth_lr")
    return _built(fail, f"--degrade {args.degrade}", build, args)


def check_usm(args, fail):
    """The --gt_usm / --usm_* block -> the UsmSpec (None without --gt_usm)."""
    usm_opts = [n for n in USM_FLAGS if getattr(args, n) is not None]
    if args.gt_usm and args.degrade != "second_order":
        fail("--gt_usm sharpens the target of --degrade second_order: it needs it")
    if usm_opts and not args.gt_usm:
        fail(f"--{usm_opts[0]} is an option of --gt_usm")
    return _built(fail, "--gt_usm", usm_spec, args)


def check_blur(args, fail, other: str, other_on: bool, clash: str):
    """The 2-D blur flags: --blur_psf and `other` (training's --blur_kernel, evaluate's --blur_theta) need a --degrade and exclude each other."""
    if (other_on or args.blur_psf is not None) and args.degrade not in TWO_D:
        fail(f"--{other} and --blur_psf shape the blur of --degrade blind | second_order: they need it")
    if args.blur_psf is not None and other_on:
        fail(f"--blur_psf FILE replaces the {clash}")


def check_jpeg(args, fail, stray: bool, stray_message: str, on_device: bool, off_device_message: str) -> bool:
    """The --jpeg_quality block of --task sr -> whether there is a JPEG stage, which the caller validates.  stray: an option without its stage."""
    if args.jpeg_quality is None:
        if stray:
            fail(stray_message)
        return False
    if args.task != "sr":
        return False
    if not on_device:
        fail(off_device_message)
    if args.synth_lr_bits != 8:
        fail("--jpeg_quality codes 8-bit LR images: it needs --synth_lr_bits 8")
    return True


# a run's specs (None where a stage is off): RestoreSpec, DegradeSpec, SecondOrderSpec, UsmSpec, PsfSpec, JpegSpec -- or evaluate's fixed ones
Specs = namedtuple("Specs", "restore degrade second_order usm psf jpeg")


def train_specs(args, fail=_raise) -> Specs:
    """Checks finetune_swinir's data-path flags, in this order, and builds the run's specs; fail(message) does not return."""
    restore = check_task(args, fail, restore_spec, jpeg_p=args.jpeg_p)
    if args.synth_lr and not args.gpu_data:
        fail("--synth_lr forms the LR patches on the device: it needs --gpu_data")
    degrade = check_degrade(args, fail, degrade_spec)
    second = [n for n in SECOND_ORDER_FLAGS if getattr(args, n) is not None]
    if args.degrade == "second_order":
        if args.synth_lr_bits != 8:
            fail("--degrade second_order codes 8-bit LR images: it needs --synth_lr_bits 8")
        if args.jpeg_p != 1.0:
            fail("--jpeg_p is an option of the single JPEG stage; --degrade second_order codes every patch twice")
    elif second:
        fail(f"--{second[0]} is an option of --degrade second_order")
    second_order = _built(fail, "--degrade second_order", second_order_spec, args)
    if args.degrade_margin is not None and not 0 <= args.degrade_margin <= 64:
        fail(f"--degrade_margin must be in 0..64 LR pixels (got {args.degrade_margin})")
    usm = check_usm(args, fail)
    check_blur(args, fail, "blur_kernel", args.blur_kernel != "axis", "generated kernels: it does not go with --blur_kernel rotated | mixed")
    mixed_opts = [n for n in ("blur_kernel_prob", "blur_beta_g", "blur_beta_p", "blur_ksize") if getattr(args, n) is not None]
    if mixed_opts and args.blur_kernel != "mixed":
        fail(f"--{mixed_opts[0]} is an option of --blur_kernel mixed")
    psf = _built(fail, "--blur_kernel / --blur_psf", psf_spec, args, (ValueError, OSError))
    if args.degrade_tables != "host" and not (args.degrade == "second_order" or (args.degrade == "blind" and psf is not None)):
        fail("--degrade_tables device builds the 2-D tables of --degrade blind with --blur_kernel rotated | mixed or --blur_psf, or of "
             "--degrade second_order: it needs one of them")
    stage = check_jpeg(args, fail, args.jpeg_p != 1.0 or (args.jpeg_subsample != "444" and args.degrade != "second_order"),
                       "--jpeg_p and --jpeg_subsample are options of the JPEG stage: they need --jpeg_quality LO HI", args.gpu_data and args.synth_lr,
                       "--jpeg_quality codes the LR patches formed on the device: it needs --gpu_data --synth_lr")
    return Specs(restore, degrade, second_order, usm, psf, _built(fail, "--jpeg_quality", jpeg_spec, args) if stage else None)


def eval_degrade(args):
    """The FixedDegrade of evaluate's command line (None for --degrade bicubic), its ranges checked; --noise_sigma is given in 8-bit levels."""
    if args.degrade not in TWO_D:
        return None
    fixed = FixedDegrade(tuple(args.blur_sigma), (args.noise_sigma / 255.0, args.noise_gain))
    pack_degrade_params(fixed.blur, fixed.noise, 0, False)
    return fixed


def eval_specs(args, fail=_raise) -> Specs:
    """The same for evaluate (--crop_border and --arch ms_resunet have their place in the order); jpeg: the quality of the single JPEG stage."""
    restore = check_task(args, fail, eval_restore, "S", "25", "Q", "bench_metric")
    if args.crop_border is not None:
        if args.bench_metric is None:
            fail("--crop_border is an option of the benchmark-protocol scores: it needs --bench_metric y | rgb")
        if args.crop_border < 0:
            fail(f"--crop_border must be >= 0 (got {args.crop_border})")
    if args.synth_lr and args.arch == "ms_resunet":
        fail("--synth_lr is an option of --arch swinir | hat | dat (MS_ResUNet takes the pre-upscaled LR of the eval transform)")
    if args.degrade == "second_order" and args.synth_lr_bits != 8:
        fail("--degrade second_order codes 8-bit LR images: it needs --synth_lr_bits 8")
    degrade = check_degrade(args, fail, eval_degrade, "the HR images")
    usm = check_usm(args, fail)
    check_blur(args, fail, "blur_theta", args.blur_theta is not None, "Gaussian: it does not go with --blur_theta")
    psf = _built(fail, "--blur_theta / --blur_psf", eval_psf, args, (ValueError, OSError))
    stage = check_jpeg(args, fail, args.jpeg_subsample != "444" and args.degrade != "second_order",
                       "--jpeg_subsample is an option of the JPEG stage: it needs --jpeg_quality Q", args.synth_lr,
                       "--jpeg_quality codes the LR images formed on the device: it needs --synth_lr")
    if stage and not 1 <= args.jpeg_quality <= 100:
        fail(f"--jpeg_quality must be in 1..100 (got {args.jpeg_quality})")
    if args.degrade != "second_order":
        return Specs(restore, degrade, None, usm, psf, args.jpeg_quality)
    second_order = SecondOrderSpec() if args.jpeg_quality is None else SecondOrderSpec(jpeg_quality=(args.jpeg_quality,) * 2)
    return Specs(restore, degrade, second_order, usm, psf, None)


ALWAYS_SAVED = frozenset((          # the reference's flags and the earliest additive ones: in every checkpoint, at any value
    "data_root", "scale", "weights", "epochs", "batch_size", "lr_patch", "lr", "weight_decay", "workers", "seed", "no_pin", "no_persistent",
    "freeze_regex", "scheduler", "min_lr", "grad_clip", "drop_path_rate", "gpu_data", "gpu_data_shard_mb", "arch", "graph", "freeze_bn",
    "window_size", "augment"))
FOLLOWS = {"fft_norm": "fft_weight", "val_tile_overlap": "val_tile", "synth_lr_bits": "synth_lr"}          # option -> the flag that turns it on


def saved_args(args, parser) -> dict:
    """What a checkpoint keeps of the command line: the ALWAYS_SAVED flags, and of the others -- every flag added since, and every flag
    added later -- those that differ from the default their own add_argument declared (an option of FOLLOWS only while its owner does)."""
    def at_default(k):
        return getattr(args, k) == parser.get_default(k)
    return {k: v for k, v in vars(args).items() if k in ALWAYS_SAVED or not (at_default(k) or (k in FOLLOWS and at_default(FOLLOWS[k])))}


def train_lines(args, specs, scale_int: int, pool) -> list:
    """The [task ...] / [synth_lr] / [degrade] / [gpu_data] lines of a training run on a device pool.  Of the pool they quote its length,
    shard count and decoded MiB and, with --degrade second_order, DeviceHR2Pool's window (extent, HR pixels) and margin (LR pixels)."""
    held = f"in {pool.num_shards} shard(s), {sum(t.numel() for t in pool._host) / 2**20:.1f} MiB decoded"
    if specs.restore is not None:
        fx = specs.restore.fixed()
        return [f"[task {args.task}] {len(pool)} clean images {held}; {args.channels} channel(s), patches of {args.lr_patch} cut at any pixel and "
                f"degraded on the device",
                f"[degrade] noise sigma in {[0.0, 0.0] if args.dn_sigma is None else args.dn_sigma} / 255 ({args.dn_bits or 'no'}-bit "
                f"rounding), jpeg quality in {args.jpeg_quality} chroma {args.jpeg_subsample}, blocks on the image's grid, seed "
                f"{args.degrade_seed}; validation: sigma={fx.sigma * 255.0:.4g} / 255 quality {fx.jpeg_quality or 'none'}, noise id = image index"]
    if not args.synth_lr:
        return [f"[gpu_data] {len(pool)} pairs {held}"]
    so, us, ps, js = specs.second_order, specs.usm, specs.psf, specs.jpeg
    lines = [f"[synth_lr] {len(pool)} HR images {held}; LR = antialiased bicubic /{scale_int} on the device, {args.synth_lr_bits or 'no'}-bit rounding"]
    if so is not None:
        lines.append(f"[degrade] second order: window {pool.extent} x {pool.extent} HR px (margin {pool.margin} LR px), resize {list(so.resize_range)} "
                     f"p={list(so.resize_prob)} then {list(so.resize2_range)} p={list(so.resize2_prob)}, blur 2 p={so.blur2_p:g}, sinc p={so.sinc_p:g} "
                     f"final p={so.final_sinc_p:g}, jpeg {list(so.jpeg_quality)} then {list(so.jpeg2_quality)} chroma {args.jpeg_subsample}, seed "
                     f"{args.degrade_seed}; validation: the fixed chain (SecondOrderSpec.fixed), noise id = image index")
        if so.resize_mode_prob != (0.0, 0.0, 1.0):
            lines.append(f"[degrade] resize rules: area / bilinear / bicubic with p={list(so.resize_mode_prob)} at each of the three resizes; "
                         f"validation: bicubic")
        if us is not None:
            lines.append(f"[degrade] gt_usm: the HR window is unsharp-masked ({us.ks} taps, weight {us.weight:g}, threshold {us.threshold:g} / 255); "
                         f"LR is degraded from it and the loss is taken against it; margin {pool.margin} x scale {scale_int} "
                         f"{'>=' if pool.margin * scale_int >= us.ks - 1 else '<'} 2R = {us.ks - 1}")
    if specs.degrade is not None:
        fx = specs.degrade.fixed()
        lines.append(f"[degrade] blind: blur sigma in {args.blur_sigma} HR px (aniso p={args.blur_aniso_p}), noise sigma in "
                     f"{args.noise_sigma} / 255, gain in {args.noise_gain}, gray p={args.gray_noise_p}, seed {args.degrade_seed}; "
                     f"validation: sigma=({fx.blur[0]:.4g}, {fx.blur[1]:.4g}) noise sigma={fx.noise[0] * 255.0:.4g} / 255 "
                     f"gain={fx.noise[1]:.4g}, noise id = image index")
    if ps is not None:
        what = (f"{len(ps.tables)} measured table(s) of {args.blur_psf}, {ps.tables.shape[-1]} x {ps.tables.shape[-1]}; validation: table 0"
                if ps.mode == "file" else f"{ps.mode} 2-D kernels; validation: the isotropic midpoints")
        lines.append(f"[degrade] blur kernel: {what}, seed {args.degrade_seed}")
    if args.degrade_tables == "device":
        lines.append("[degrade] tables: built on the device from descriptors (csrc/tables.hip)")
    if js is not None:          # with --degrade second_order the range is the first JPEG's, quoted in that line
        lines.append(f"[degrade] jpeg: quality in {list(js.quality)} with p={js.p:g}, chroma {args.jpeg_subsample}, seed {args.degrade_seed}; "
                     f"validation: quality {js.fixed()}")
    return lines


def eval_lines(args, specs, scale_int: int) -> list:
    """The [task ...] / [synth_lr] / [degrade] lines of an evaluation run."""
    if specs.restore is not None:
        fx = specs.restore
        return [f"[task {args.task}] {args.channels} channel(s); degraded = whole image on the device: noise sigma={fx.sigma * 255.0:.4g} / 255 "
                f"({args.dn_bits or 'no'}-bit rounding), jpeg quality {fx.jpeg_quality or 'none'} chroma {args.jpeg_subsample}, noise id = image index"]
    if not args.synth_lr:
        return []
    fixed, second, k, us = specs.degrade, specs.second_order, specs.psf, specs.usm
    lines = [f"[synth_lr] LR = antialiased bicubic /{scale_int} of HR on the device, {args.synth_lr_bits or 'no'}-bit rounding"]
    if fixed is not None:
        lines.append(f"[degrade] blind: blur sigma=({fixed.blur[0]:.4g}, {fixed.blur[1]:.4g}) HR px, noise sigma={args.noise_sigma:.4g} / 255 "
                     f"gain={args.noise_gain:.4g}, noise id = image index")
    if k is not None:
        lines.append(f"[degrade] blur kernel: {k.shape[0]} x {k.shape[0]} table, " + (f"table 0 of {args.blur_psf}" if args.blur_psf is not None else
                                                                                      f"the Gaussian turned by {args.blur_theta:g} degrees"))
    if second is not None:
        fx2 = second.fixed(None, fixed.noise)
        lines.append(f"[degrade] second order, fixed: resize x{fx2.r1:.4g}, jpeg {fx2.q1}, blur 2 {fx2.k2.shape[0]} taps, resize x{fx2.r2:.4g} of LR, "
                     f"noise sigma={fx2.noise2[0] * 255.0:.4g} / 255, jpeg {fx2.q2}, final filter {fx2.k3.shape[0]} taps, chroma {args.jpeg_subsample}")
        if us is not None:
            lines.append(f"[degrade] gt_usm: HR is unsharp-masked ({us.ks} taps, weight {us.weight:g}, threshold {us.threshold:g} / 255); LR is "
                         f"degraded from it and every score is taken against it")
    elif args.jpeg_quality is not None:
        lines.append(f"[degrade] jpeg: quality {args.jpeg_quality}, chroma {args.jpeg_subsample}")
    return lines
