"""SwinIR fine-tuning entry point with the reference's command line (modules/finetune_swinir.py:213-236),
running on MI355X through libsrk.

    python -m tpu_superresolution_amd.finetune_swinir --data_root D --scale X4 --weights swinir.pth [...]
    torchrun --nproc-per-node 8 -m tpu_superresolution_amd.finetune_swinir ...      (data parallel, RCCL)

Same flags, same model configuration (:269-281), same checkpoint envelopes in ({"params": sd} or raw) and
out ("best_swinir_finetune_<scale>.pt", "bestpsnr_swinir_finetune_<scale>.pt" with key "model", :345-371),
same epoch print line (:337-342).  Differences, all additive: bf16 MFMA is built into the kernels (no autocast
context), the step uses the fused L1 / clip / AdamW kernels, `--weights` may be omitted (random init) and
`--drop_path_rate` exposes the constructor default (0.1) that the reference leaves implicit.  `--augment flip|d4` (default none) trains
on flipped / rotated patches (augment.py; on the device with `--gpu_data`).  `--loss l1|mse|charbonnier` (default l1) and
`--ssim_weight W` (default 0) choose the objective: the pixel loss plus W * (1 - SSIM), value and gradient from the fused kernels of
csrc/loss.hip (training.make_loss); with W > 0 validation also reports the mean per-image SSIM and checkpoints gain 'val_ssim'.
`--fft_weight W [--fft_norm backward|ortho]` (default 0) adds W * mean(|Re D| + |Im D|), D = rfft2(pred - hr): the frequency loss of the
SwinFIR / HAT recipes (csrc/fft_loss.hip; HR patches of at most 512 x 512).
`--val_tile N` (default 0 = whole images) validates on overlapping N x N LR tiles merged on the device (tiling.tiled_forward).
`--val_bench_metric y|rgb [--val_crop_border N]` adds the papers' scores to the epoch line and the checkpoints ('val_bench_psnr',
'val_bench_ssim'): 8-bit, border-cropped (default: the scale), BT.601 luma or RGB, 0..255 scale (metrics.bench_metrics).
`--gpu_data --synth_lr [--synth_lr_bits 0|8]` trains and validates from the HR directories alone: every LR patch is the antialiased
bicubic downscale of its HR image, made on the device (sr_datasets.DeviceHRPool, csrc/resize.hip); no LR directory is read.
`--degrade blind [--blur_sigma LO HI --noise_sigma LO HI ...]` blurs and noises every such patch with random parameters in the same
launch (csrc/degrade.hip); validation uses the midpoints of the ranges and the same noise every epoch.
`--task dn|car --scale X1 [--channels 1|3 --dn_sigma LO HI --dn_bits 0|8]` trains the published scale-1 SwinIR models (denoising; JPEG
compression-artifact reduction with --jpeg_quality LO HI) from the HR directories alone: every patch is cut at any image pixel and is the
window of the whole-image degradation, JPEG blocks anchored at the image's (0, 0) (sr_datasets.DeviceRestorePool, csrc/restore.hip).
`--jpeg_quality LO HI [--jpeg_p P --jpeg_subsample 444|420]` (with either --degrade) sends every 8-bit LR patch through a baseline JPEG
round trip at a random per-sample quality in a second launch (csrc/jpeg.hip); validation uses the middle of the range.
`--degrade second_order` runs Real-ESRGAN's chain on the device instead -- blur, resize, noise, JPEG, twice, every sample at its own
intermediate sizes, then a sinc filter (sr_datasets.DeviceHR2Pool, csrc/filter2d.hip, csrc/ragged.hip).
`--degrade_tables device` (with the 2-D kernels of --degrade blind, or --degrade second_order) builds the blur and sinc tables of every
training batch on the device instead of in numpy on the training thread (csrc/tables.hip).
`--gt_usm [--usm_weight W --usm_threshold T --usm_radius R]` (with --degrade second_order) unsharp-masks the HR window on the device, degrades
the LR patch from the sharpened window and takes the loss against it; `--resize_mode_prob AREA BILINEAR BICUBIC` draws the rule of each of
the chain's three resizes per sample (csrc/usm.hip, csrc/resize_modes.hip).
`--blur_kernel rotated|mixed` or `--blur_psf FILE` (with --degrade blind) blurs every patch with a 2-D table -- a rotated, generalized or
plateau Gaussian, or a measured point-spread function -- in the same single launch (csrc/blur2d.hip).
The flags from --synth_lr on are declared, checked, turned into specs and worded for the [degrade] lines in data_cli.py.

Also additive: `--arch hat|dat` fine-tunes HAT / DAT (build_sr_model) through the same loop -- the fused, device-gated clip + AdamW step
over their parameter lists (optim.FusedAdamW, csrc/optim_multi.hip), checkpoints "best_<arch>_finetune_<scale>.pt" /
"bestpsnr_<arch>_finetune_<scale>.pt" -- and `--graph` replays their whole train step as one hipGraph (training.GraphedTrainStep; one
process, fixed batch shape).  With more than one process HAT / DAT average their gradients through distributed.ListGradSynchronizer.
"""
from __future__ import annotations

import argparse
import os
import random
import re
import time
from contextlib import nullcontext
from datetime import timedelta
from functools import partial

import torch
from torch.utils.data import DataLoader
from torch.utils.data.distributed import DistributedSampler

from . import SwinIR, data_cli
from .data_cli import (RESTORATION_TASKS, SCALES, SECOND_ORDER_FLAGS, USM_FLAGS, add_train_data_flags,          # noqa: F401
                       default_window_size, degrade_spec, jpeg_spec, psf_spec, restore_spec, second_order_spec, train_lines, train_specs, usm_spec)
from .distributed import DataParallelSwinIR, init_from_env
from .optim import FusedAdamW
from .sr_datasets import (DeviceHR2Pool, DeviceHRPool, DevicePairPool, DeviceRestorePool, PairTransformTrain, PairTransformValid, RestoreBatches,
                          Shuffled2DHR, Shuffled2DPaired, SynthLRBatches, clean_to_tensor, hr_to_tensor3)
from .training import assert_finite_step, freeze_batchnorm, l1_loss, loss_name, make_loss, train_step


def fmt(seconds: float) -> str:
    return str(timedelta(seconds=int(seconds)))


def seed_everything(seed: int = 42):
    random.seed(seed)
    torch.manual_seed(seed)
    torch.cuda.manual_seed_all(seed)


def batch_psnr(pred: torch.Tensor, target: torch.Tensor, max_val: float = 1.0) -> torch.Tensor:
    """finetune_swinir.py:69-74."""
    pred, target = pred.clamp(0.0, 1.0), target.clamp(0.0, 1.0)
    mse = ((pred - target) ** 2).reshape(pred.size(0), -1).mean(dim=1)
    return 20.0 * torch.log10(max_val / torch.sqrt(mse + 1e-8))


def make_loader(ds, batch_size, workers, pin=True, shuffle=False, drop_last=False, persistent=False, sampler=None):
    kw = dict(dataset=ds, batch_size=batch_size, shuffle=shuffle and sampler is None, drop_last=drop_last, num_workers=workers,
              pin_memory=pin, sampler=sampler)
    if workers and workers > 0:
        kw["persistent_workers"] = persistent
        kw["prefetch_factor"] = 2
    return DataLoader(**kw)


class DevicePoolLoader:
    """Drop-in for the training DataLoader when the training set is held pre-decoded in GPU memory (`--gpu_data`,
    sr_datasets.DevicePairPool): same epoch semantics as DataLoader(shuffle=True, drop_last=True) with an optional
    DistributedSampler-style rank shard (per-epoch permutation from torch.Generator(seed + epoch), ranks take strided
    slices of it); the crop corners come from the process-global `random`, as in the host transform."""

    def __init__(self, pool, batch_size: int, rank: int = 0, world: int = 1, seed: int = 0):
        self.pool, self.batch_size, self.rank, self.world, self.seed, self.epoch = pool, batch_size, rank, world, seed, 0

    def set_epoch(self, epoch: int) -> None:
        self.epoch = epoch

    def __len__(self):
        return (len(self.pool) // self.world) // self.batch_size

    def __iter__(self):
        g = torch.Generator().manual_seed(self.seed + self.epoch)
        perm = torch.randperm(len(self.pool), generator=g).tolist()
        mine = perm[self.rank:len(perm) - len(perm) % self.world:self.world] if self.world > 1 else perm
        if getattr(self.pool, "num_shards", 1) > 1:
            # sharded pool (pinned host shards, two resident on the device): walk the epoch shard by shard -- shuffled order of
            # shards, shuffled images inside each -- so that the copy of the next shard overlaps the steps on this one
            order = torch.randperm(self.pool.num_shards, generator=g).tolist()
            by_shard = {s: [i for i in mine if self.pool.shard_of(i) == s] for s in order}
            for s in order:
                idx = by_shard[s]
                for b in range(len(idx) // self.batch_size):
                    yield self.pool.sample(idx[b * self.batch_size:(b + 1) * self.batch_size])
            return
        for b in range(len(self)):
            yield self.pool.sample(mine[b * self.batch_size:(b + 1) * self.batch_size])


def train_one_epoch(model, loader, optimizer, device, sync=None, check_finite=True, graphed=None, freeze_bn=False, loss_fn=None):
    """loss_fn: the objective of train_step (training.make_loss; None = L1).
    graphed: a training.GraphedTrainStep over (model, optimizer) that runs the step instead of train_step (--graph).
    freeze_bn: every BatchNorm stays in eval mode (running statistics, no buffer moves): re-applied here because model.train() switches
    them all back on, and before the first graphed step captures the launch sequence."""
    model.train()
    if freeze_bn:
        freeze_batchnorm(model)
    total, n, t0 = 0.0, 0, time.time()
    for lr, hr in loader:
        lr, hr = lr.to(device, non_blocking=True), hr.to(device, non_blocking=True)
        loss, bad = graphed(lr, hr) if graphed is not None else train_step(model, optimizer, lr, hr, sync, loss_fn)
        if check_finite:
            assert_finite_step(loss, bad)          # RuntimeError like finetune_swinir.py:133-143
        total += float(loss)
        n += 1
    return total / max(1, n), time.time() - t0


@torch.no_grad()
def validate(model, loader, device, with_ssim=False, predict=None):
    """-> (mean L1 over batches, mean per-image PSNR, seconds); with_ssim (device only): also the mean per-image SSIM (ops.ssim,
    data_range 1), inserted before the seconds.  predict: what maps an LR batch to the prediction instead of the model itself
    (--val_tile: tiling.tiled_forward around the model)."""
    return _validate(model, loader, device, with_ssim, predict, None, 0)


@torch.no_grad()
def validate_bench(model, loader, device, bench_metric, crop_border, with_ssim=False, predict=None):
    """``validate`` plus the mean per-image PSNR and SSIM of the papers' protocol (bench_metric 'y' | 'rgb'; metrics.bench_metrics: 8-bit,
    crop_border cropped, luma or RGB, 0..255 scale), the two of them inserted before the seconds; they are summed on the device and
    read once, after the loop.  bench_metric None is ``validate`` itself."""
    return _validate(model, loader, device, with_ssim, predict, bench_metric, crop_border)


def _validate(model, loader, device, with_ssim, predict, bench_metric, crop_border):
    model.eval()
    predict = model if predict is None else predict
    if bench_metric is not None:
        from .metrics import bench_metrics
        bench_acc = torch.zeros(2, dtype=torch.float32, device=device)
    total, n, sum_psnr, n_imgs, t0 = 0.0, 0, 0.0, 0, time.time()
    ssim_acc = torch.zeros(1, dtype=torch.float32, device=device) if with_ssim else None
    on_gpu = torch.device(device).type == "cuda"
    if on_gpu:
        # fused L1 + per-image PSNR pass (csrc/misc.hip psnr_*_kernel); the sums stay on the device until the loop ends
        # (the reference reads two scalars back per batch, finetune_swinir.py:196-201)
        from . import ops
        psnr_acc = torch.zeros(1, dtype=torch.float32, device=device)
        l1_acc = torch.zeros(1, dtype=torch.float32, device=device)
    for lr, hr in loader:
        lr, hr = lr.to(device, non_blocking=True), hr.to(device, non_blocking=True)
        out = predict(lr)
        if on_gpu:
            batch_abs = torch.zeros(1, dtype=torch.float32, device=device)
            ops.batch_psnr(out.float(), hr.float(), 1.0, psnr_sum=psnr_acc, abs_sum=batch_abs)
            l1_acc += batch_abs / out.numel()          # mean over the batch, like F.l1_loss; batches may differ in size
            if with_ssim:
                ssim_acc += ops.ssim(out.float(), hr.float(), 1.0)[0].sum()
        else:
            total += float(l1_loss(out, hr))
            sum_psnr += float(batch_psnr(out, hr).sum())
        if bench_metric is not None:
            bench_acc += torch.stack([v.sum() for v in bench_metrics(out.float(), hr.float(), crop_border, bench_metric)])
        n += 1
        n_imgs += lr.size(0)
    if on_gpu:
        total, sum_psnr = float(l1_acc), float(psnr_acc)
    more = (float(ssim_acc) / max(1, n_imgs),) if with_ssim else ()
    if bench_metric is not None:
        more += tuple(v / max(1, n_imgs) for v in bench_acc.tolist())
    return (total / max(1, n), sum_psnr / max(1, n_imgs), *more, time.time() - t0)


def build_model(scale_int: int, drop_path_rate: float = 0.1, window_size: int = 8) -> SwinIR:
    """finetune_swinir.py:269-281; window_size (additive): 8 as the script has it, or 2..7 (7: the published JPEG-artifact models).
    img_size -- which only sizes the attn_mask buffers of the state_dict -- is 64 rounded down to a multiple of the window (63 at
    window 7: the reference's constructor cannot build its masks otherwise)."""
    return SwinIR(upscale=scale_int, in_chans=3, img_size=64 // window_size * window_size, window_size=window_size, img_range=1.0,
                  depths=[6] * 6, embed_dim=180,
                  num_heads=[6] * 6, mlp_ratio=2, upsampler="pixelshuffle", resi_connection="1conv",
                  drop_path_rate=drop_path_rate)


def build_restoration_model(task: str, channels: int = 3, drop_path_rate: float = 0.1, window_size: int = None) -> SwinIR:
    """The published scale-1 SwinIR configurations: 'dn' (gray / colour denoising: window 8, img_size 128, img_range 1) and 'car' (JPEG
    compression-artifact reduction: window 7, img_size 126, img_range 255); upscale 1, upsampler '', in_chans = channels (1 | 3).
    window_size: None = the task's; another window rounds img_size -- which only sizes the attn_mask buffers -- down to its multiple."""
    if task not in RESTORATION_TASKS:
        raise ValueError(f"task must be one of {tuple(RESTORATION_TASKS)} (got {task!r})")
    if channels not in (1, 3):
        raise ValueError(f"channels must be 1 or 3 (got {channels!r})")
    cfg = RESTORATION_TASKS[task]
    ws = cfg["window_size"] if window_size is None else int(window_size)
    if not 2 <= ws <= 8:
        raise ValueError(f"window_size must be in 2..8 (got {window_size!r})")
    return SwinIR(upscale=1, in_chans=channels, img_size=cfg["img_size"] // ws * ws, window_size=ws, img_range=cfg["img_range"],
                  depths=[6] * 6, embed_dim=180, num_heads=[6] * 6, mlp_ratio=2, upsampler="", resi_connection="1conv",
                  drop_path_rate=drop_path_rate)


def build_sr_model(arch: str, scale_int: int, drop_path_rate: float = 0.1, window_size: int = 8):
    """The transformer SR models of modules/ at their published x2 / x4 hyper-parameters, on the HIP path: 'swinir'
    (finetune_swinir.py:269-281), 'hat' (HAT-SRx4 configuration of hat_arch.py's constructor defaults: window 16, overlap 0.5, CAB),
    'dat' (official DAT configuration: split [8, 32], expansion 4; dat_arch.py:721-741).  Used by train.py / evaluate.py --arch."""
    if arch == "swinir":
        return build_model(scale_int, drop_path_rate, window_size)
    if window_size != 8:
        raise ValueError(f"window_size={window_size} is an option of arch 'swinir' ('{arch}' has its published window)")
    if arch == "hat":
        from .hat_arch import HAT
        return HAT(upscale=scale_int, in_chans=3, img_size=64, window_size=16, compress_ratio=3, squeeze_factor=30, conv_scale=0.01,
                   overlap_ratio=0.5, img_range=1.0, depths=[6] * 6, embed_dim=180, num_heads=[6] * 6, mlp_ratio=2,
                   upsampler="pixelshuffle", resi_connection="1conv", drop_path_rate=drop_path_rate)
    if arch == "dat":
        from .dat_arch import DAT
        return DAT(upscale=scale_int, in_chans=3, img_size=64, img_range=1.0, depth=[6] * 6, embed_dim=180, num_heads=[6] * 6,
                   expansion_factor=4, resi_connection="1conv", split_size=[8, 32], upsampler="pixelshuffle", drop_path_rate=drop_path_rate)
    raise ValueError(f"unknown arch {arch!r}")


def build_parser() -> argparse.ArgumentParser:
    """The reference's flags and the additive ones of the training loop; the data-path flags (--synth_lr on) are data_cli's."""
    ap = argparse.ArgumentParser()
    ap.add_argument("--data_root", type=str, required=True)
    ap.add_argument("--scale", type=str, choices=["X1", "X2", "X4"], required=True,
                    help="X2 | X4 with --task sr; X1 (input and target of one size) with --task dn | car")
    ap.add_argument("--weights", type=str, default=None, help="Path to SwinIR pretrained checkpoint (.pth/.pt)")
    ap.add_argument("--epochs", type=int, default=10)
    ap.add_argument("--batch_size", type=int, default=8, help="per-process batch size")
    ap.add_argument("--lr_patch", type=int, default=64, help="LR patch size (HR patch = lr_patch*scale)")
    ap.add_argument("--lr", type=float, default=2e-5)
    ap.add_argument("--weight_decay", type=float, default=0.0)
    ap.add_argument("--workers", type=int, default=None)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--no_pin", action="store_true")
    ap.add_argument("--no_persistent", action="store_true")
    ap.add_argument("--freeze_regex", type=str, default=None)
    ap.add_argument("--scheduler", type=str, choices=["None", "Cosine"], default="Cosine")
    ap.add_argument("--min_lr", type=float, default=2e-6)
    ap.add_argument("--grad_clip", type=float, default=1.0)
    ap.add_argument("--drop_path_rate", type=float, default=0.1)      # additive
    ap.add_argument("--gpu_data", action="store_true",
                    help="additive: decode the training set once and crop/convert on the device")
    ap.add_argument("--gpu_data_shard_mb", type=int, default=0,
                    help="additive, with --gpu_data: keep the decoded set in pinned host shards of this size and prefetch them "
                         "to the device one ahead (0 = whole set resident on the device)")
    ap.add_argument("--arch", type=str, choices=["swinir", "hat", "dat"], default="swinir",
                    help="additive: the model to fine-tune (build_sr_model)")
    ap.add_argument("--graph", action="store_true",
                    help="additive, --arch hat|dat, one process: capture the train step into a hipGraph and replay it")
    ap.add_argument("--freeze_bn", action="store_true",
                    help="additive, --arch dat: fine-tune with every BatchNorm in eval mode (running statistics, no buffer moves; "
                         "allows --batch_size 1); swinir / hat have no BatchNorm")
    ap.add_argument("--ema_decay", type=float, default=0.0,
                    help="additive: keep an exponential moving average of the weights inside the fused optimizer step (0 = off; "
                         "published recipes use 0.999); validation runs on it and checkpoints gain 'params_ema'")
    ap.add_argument("--window_size", type=int, default=None,
                    help="additive, --arch swinir: build SwinIR(window_size=N); 2..7 train through enable_small_window_training() "
                         "(7 is the window of the published JPEG-artifact models) and allow --graph.  Default: 8, or 7 with --task car")
    ap.add_argument("--augment", type=str, choices=["none", "flip", "d4"], default="none",
                    help="additive: training augmentation by the symmetries of the square, one drawn per sample after its crop corners "
                         "and applied to LR and HR alike (validation is never augmented).  flip: horizontal and vertical flip, each "
                         "with p = 0.5 -- the distribution of the reference's PairFlips, drawn from `random` and not from its "
                         "torch.rand stream; d4: the flips and the 90-degree rotations (all eight symmetries).  With --gpu_data the "
                         "transform is one kernel launch per batch side")
    ap.add_argument("--loss", type=str, choices=["l1", "mse", "charbonnier"], default="l1",
                    help="additive: the pixel objective (training.make_loss): l1 as the reference, mse, or charbonnier = "
                         "mean sqrt(d^2 + eps^2)")
    ap.add_argument("--charbonnier_eps", type=float, default=1e-3, help="additive: the eps of --loss charbonnier")
    ap.add_argument("--ssim_weight", type=float, default=0.0,
                    help="additive: add ssim_weight * (1 - SSIM(pred, hr)) to the objective (0 = off; needs HR patches of at least "
                         "11 x 11); validation then also reports the SSIM and checkpoints gain 'val_ssim'")
    ap.add_argument("--fft_weight", type=float, default=0.0,
                    help="additive: add fft_weight * mean(|Re D| + |Im D|), D = rfft2(pred - hr), to the objective: the frequency "
                         "loss of the SwinFIR / HAT fine-tuning recipes (0 = off; typical 0.05 .. 0.1; needs HR patches of at most "
                         "512 x 512; csrc/fft_loss.hip)")
    ap.add_argument("--fft_norm", type=str, choices=["backward", "ortho"], default="backward",
                    help="additive, with --fft_weight: the normalisation of the transform (ortho divides by sqrt(H W))")
    ap.add_argument("--val_tile", type=int, default=0,
                    help="additive: validate on overlapping tiles of N x N LR pixels merged by their mean (tiling.tiled_forward; 0 = "
                         "off, the whole image in one call)")
    ap.add_argument("--val_tile_overlap", type=int, default=32, help="additive, with --val_tile: LR pixels two neighbouring tiles share")
    ap.add_argument("--val_bench_metric", type=str, choices=["y", "rgb"], default=None,
                    help="additive: validation also reports PSNR / SSIM by the protocol of the SwinIR / HAT / DAT papers "
                         "(metrics.bench_metrics: 8-bit, border-cropped, y = BT.601 luma, rgb = every channel, 0..255 scale, mean over "
                         "images); checkpoints gain 'val_bench_psnr' / 'val_bench_ssim'; which checkpoint is best does not change")
    ap.add_argument("--val_crop_border", type=int, default=None, metavar="N",
                    help="additive, with --val_bench_metric: pixels cropped on every side before scoring (default: the scale)")
    add_train_data_flags(ap)
    return ap


def parse_args(argv=None):
    ap = build_parser()
    args = ap.parse_args(argv)
    if args.window_size is None:
        args.window_size = default_window_size(args.task)
    train_specs(args, ap.error)          # the data-path flags in their order; nothing is kept: main() builds the run's specs
    args.gpu_data |= args.task != "sr"          # dn | car: the pairs are made on the device; the HR directories alone are read
    if args.val_tile < 0 or args.val_tile_overlap < 0 or (args.val_tile and args.val_tile_overlap >= args.val_tile):
        ap.error(f"--val_tile must be >= 0 and 0 <= --val_tile_overlap < --val_tile (got --val_tile {args.val_tile} "
                 f"--val_tile_overlap {args.val_tile_overlap})")
    if args.val_crop_border is not None and (args.val_bench_metric is None or args.val_crop_border < 0):
        ap.error(f"--val_crop_border must be >= 0 and is an option of --val_bench_metric y | rgb (got {args.val_crop_border})")
    for n in ("ssim_weight", "fft_weight"):
        if not 0.0 <= getattr(args, n) < float("inf"):          # also refuses NaN
            ap.error(f"--{n} must be a finite number >= 0 (got {getattr(args, n)})")
    hr_patch = args.lr_patch * SCALES[args.scale.upper()]
    if args.fft_weight > 0 and hr_patch > 512:
        ap.error(f"--fft_weight needs HR patches of at most 512 x 512 (lr_patch * scale = {hr_patch})")
    if not args.charbonnier_eps > 0.0:
        ap.error(f"--charbonnier_eps must be > 0 (got {args.charbonnier_eps})")
    if args.ssim_weight > 0 and hr_patch < 11:
        ap.error(f"--ssim_weight needs HR patches of at least 11 x 11 (lr_patch * scale = {hr_patch})")
    if not 0.0 <= args.ema_decay < 1.0:          # also refuses NaN
        ap.error(f"--ema_decay must be in [0, 1) (got {args.ema_decay})")
    if not 2 <= args.window_size <= 8:
        ap.error(f"--window_size must be in 2..8 (got {args.window_size})")
    if args.window_size != 8 and args.arch != "swinir":
        ap.error("--window_size is an option of --arch swinir")
    if args.graph and args.arch == "swinir" and args.window_size == 8:
        ap.error("--graph captures the host-orchestrated train step of --arch hat / dat and of --arch swinir --window_size 2..7 "
                 "(the window-8 SwinIR step is one C call already)")
    return args


def saved_args(args) -> dict:
    """What a checkpoint keeps of the command line: additive flags leave no trace in the files at the defaults their add_argument declared."""
    return data_cli.saved_args(args, build_parser())


def build_loaders(args, specs, scale_int, device, rank, world):
    """-> (train_loader, sampler, valid_loader, lines): a DevicePoolLoader over the pool of the run's branch (--task dn | car, --synth_lr,
    --gpu_data) or the host DataLoader; what takes set_epoch (or None); the validation loader with its device wrapper; the pool's lines
    for rank 0 to print (data_cli.train_lines).  specs: the run's, from train_specs."""
    shard_bytes, pool = (args.gpu_data_shard_mb << 20) or None, None
    if specs.restore is not None:
        raw = Shuffled2DHR(args.data_root, split="train")
        pool = DeviceRestorePool((raw[i] for i in range(len(raw))), args.lr_patch, args.channels, specs.restore, device=device,
                                 shard_bytes=shard_bytes, augment=args.augment, quant_bits=args.dn_bits, rank=rank)
        train_loader = sampler = DevicePoolLoader(pool, args.batch_size, rank, world, args.seed)
        valid_ds = Shuffled2DHR(args.data_root, split="valid", transform=partial(clean_to_tensor, out_chans=args.channels))
    elif args.synth_lr:
        raw = Shuffled2DHR(args.data_root, split="train")
        if specs.second_order is not None:
            pool = DeviceHR2Pool((raw[i] for i in range(len(raw))), args.lr_patch, scale_int, specs.second_order, specs.degrade, device=device,
                                 shard_bytes=shard_bytes, augment=args.augment, rank=rank, psf=specs.psf,
                                 margin=8 if args.degrade_margin is None else args.degrade_margin, subsample=args.jpeg_subsample == "420",
                                 names=[f.name for f in raw.files], tables=args.degrade_tables, usm=specs.usm)
        else:
            pool = DeviceHRPool((raw[i] for i in range(len(raw))), args.lr_patch, scale_int, device=device,
                                shard_bytes=shard_bytes, augment=args.augment, quant_bits=args.synth_lr_bits,
                                degrade=specs.degrade, rank=rank, jpeg=specs.jpeg, psf=specs.psf, tables=args.degrade_tables)
        train_loader = sampler = DevicePoolLoader(pool, args.batch_size, rank, world, args.seed)
        valid_ds = Shuffled2DHR(args.data_root, split="valid", transform=hr_to_tensor3)
    else:
        train_ds = Shuffled2DPaired(args.data_root, split="train", scale=args.scale,
                                    transform_pair=PairTransformTrain(args.lr_patch, scale_int, args.augment))
        valid_ds = Shuffled2DPaired(args.data_root, split="valid", scale=args.scale, transform_pair=PairTransformValid(scale_int))
        sampler = DistributedSampler(train_ds, num_replicas=world, rank=rank, shuffle=True, seed=args.seed) if world > 1 else None
        train_loader = make_loader(train_ds, args.batch_size, args.workers, pin=not args.no_pin, shuffle=True, drop_last=True,
                                   persistent=not args.no_persistent, sampler=sampler)
        if args.gpu_data:
            raw = Shuffled2DPaired(args.data_root, split="train", scale=args.scale, transform_pair=None)
            pool = DevicePairPool((raw[i] for i in range(len(raw))), args.lr_patch, scale_int, device=device,
                                  shard_bytes=shard_bytes, augment=args.augment)
            train_loader = sampler = DevicePoolLoader(pool, args.batch_size, rank, world, args.seed)
    valid_loader = make_loader(valid_ds, max(1, args.batch_size // 2), args.workers, pin=not args.no_pin, shuffle=False,
                               drop_last=False, persistent=not args.no_persistent)
    if specs.restore is not None:
        valid_loader = RestoreBatches(valid_loader, args.channels, specs.restore, args.dn_bits, device)
    if args.synth_lr:
        valid_loader = SynthLRBatches(valid_loader, scale_int, args.synth_lr_bits, device, degrade=specs.degrade, jpeg=specs.jpeg,
                                      jpeg_subsample=args.jpeg_subsample == "420", psf=specs.psf, second_order=specs.second_order,
                                      usm=specs.usm)
    return train_loader, sampler, valid_loader, [] if pool is None else train_lines(args, specs, scale_int, pool)


def main(argv=None):
    args = parse_args(argv)
    rank, world, local = init_from_env()
    if args.graph and world > 1:
        raise SystemExit("--graph is for one process (gradient all-reduce stays outside graphs)")
    seed_everything(args.seed)
    if args.workers is None:
        cpu = os.cpu_count() or 4
        args.workers = min(8, max(2, cpu // 2))
    if not torch.cuda.is_available():
        raise SystemExit("the MI355X HIP path needs a GPU (no CPU fallback)")
    device = torch.device("cuda", local)
    torch.cuda.set_device(device)
    if rank == 0:
        print("[device]", device, torch.cuda.get_device_name(local), f"world={world}")
    scale_int = SCALES[args.scale.upper()]

    specs = train_specs(args)          # the run's degradation specs, built once: the pool, the validation wrapper and the lines share them
    train_loader, sampler, valid_loader, lines = build_loaders(args, specs, scale_int, device, rank, world)
    for line in lines if rank == 0 else ():
        print(line)

    if args.task != "sr":
        model = build_restoration_model(args.task, args.channels, args.drop_path_rate, args.window_size)
    else:
        model = (build_model(scale_int, args.drop_path_rate, args.window_size) if args.arch == "swinir" else
                 build_sr_model(args.arch, scale_int, args.drop_path_rate))
    small = args.arch == "swinir" and args.window_size < 8
    if small:
        model.enable_small_window_training()          # before the optimizer is constructed: the model steps on the multi-tensor path
    if args.weights:
        from .evaluate import _load_state          # envelopes, in this script's order; 'params_ema' is what published HAT / DAT files hold
        state, _ = _load_state(args.weights, keys=("params", "model", "params_ema"))
        missing, unexpected = model.load_state_dict(state, strict=True)
        if rank == 0:
            print(f"[weights] loaded: {args.weights}")
            print(f"[weights] missing={len(missing)}, unexpected={len(unexpected)}")
    model = model.to(device)
    if args.freeze_regex:
        pattern, froze = re.compile(args.freeze_regex), 0
        for name, p in model.named_parameters():
            if pattern.search(name):
                p.requires_grad = False
                froze += 1
        if rank == 0:
            print(f"[freeze] regex='{args.freeze_regex}', froze_params={froze}")
    if args.freeze_bn:
        n_bn = freeze_batchnorm(model)          # train_one_epoch re-applies it after every model.train()
    if args.freeze_bn and rank == 0:
        print(f"[freeze_bn] {n_bn} BatchNorm layers use their running statistics" if n_bn else
              f"[freeze_bn] --arch {args.arch} has no BatchNorm layer: nothing to freeze")
    if rank == 0:
        n_train = sum(1 for p in model.parameters() if p.requires_grad)
        print(f"[params] trainable tensors: {n_train} / total: {len(list(model.parameters()))}")

    if args.arch == "swinir" and not small:
        dp = DataParallelSwinIR(model)
        dp.attach(device)                 # weights are now identical on every rank (broadcast from rank 0)
    else:
        dp = None
        if world > 1:
            # HAT / DAT / small-window SwinIR: separate parameter tensors.  Same weights (and BatchNorm statistics) everywhere, then per-segment gradient
            # SUMS overlapped with the backward (hat_train / dat_train call model.grad_sync); the optimizer divides by the world size
            import torch.distributed as dist
            from .distributed import ListGradSynchronizer
            for t in [*model.parameters(), *model.buffers()]:
                dist.broadcast(t.data, src=0)
            dp = model.grad_sync = ListGradSynchronizer(average=False)
    if world > 1:
        # per-rank randomness from here on: DropPath masks and crop corners must differ between ranks, or stochastic
        # depth / crop diversity would not scale with the world size (bench.py seeds 1234 + rank the same way)
        seed_everything(args.seed + rank)
    opt = FusedAdamW(model, lr=args.lr, weight_decay=args.weight_decay,
                     max_grad_norm=args.grad_clip if args.grad_clip and args.grad_clip > 0 else None, grad_div=float(world),
                     ema_decay=args.ema_decay or None)
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=args.epochs, eta_min=args.min_lr) if args.scheduler == "Cosine" else None

    custom = args.loss != "l1" or args.ssim_weight > 0 or args.fft_weight > 0          # at the defaults: the L1 step, lines and files of ever
    loss_fn = make_loss(args.loss, args.charbonnier_eps, args.ssim_weight, fft_weight=args.fft_weight,
                        fft_norm=args.fft_norm) if custom else None
    with_ssim = args.ssim_weight > 0
    graphed = None
    if args.graph:
        from .training import GraphedTrainStep
        graphed = GraphedTrainStep(model, opt, loss_fn=loss_fn)          # drop_last=True keeps the batch shape fixed

    predict = None
    if args.val_tile:
        from .tiling import tiled_forward
        predict = partial(tiled_forward, model, tile=args.val_tile, overlap=args.val_tile_overlap)
        if rank == 0:
            print(f"[val_tile] {args.val_tile} overlap {args.val_tile_overlap}")

    validate_fn, val_border = validate, None          # without --val_bench_metric: the validation call of ever
    if args.val_bench_metric is not None:
        val_border = scale_int if args.val_crop_border is None else args.val_crop_border
        validate_fn = partial(validate_bench, bench_metric=args.val_bench_metric, crop_border=val_border)

    best_loss, best_psnr, t_all = float("inf"), -float("inf"), time.time()
    for epoch in range(1, args.epochs + 1):
        if sampler is not None:
            sampler.set_epoch(epoch)
        tr_loss, tr_t = train_one_epoch(model, train_loader, opt, device, dp if world > 1 else None, graphed=graphed,
                                        freeze_bn=args.freeze_bn, loss_fn=loss_fn)
        with opt.swap_ema() if args.ema_decay else nullcontext():          # validate what gets shipped: the averaged weights (the same on every rank)
            val = validate_fn(model, valid_loader, device, with_ssim=with_ssim, predict=predict)
        val_loss, val_psnr, val_t = val[0], val[1], val[-1]
        if sched is not None:
            sched.step()
        if rank != 0:
            continue
        train_name = f"loss[{loss_name(args.loss, args.ssim_weight, args.fft_weight)}]" if custom else "L1"
        val_more = f", SSIM={val[2]:.4f}" if with_ssim else ""
        if val_border is not None:
            tag = args.val_bench_metric.upper()
            val_more += f", bench PSNR-{tag}={val[-3]:.2f}dB SSIM-{tag}={val[-2]:.4f} (8-bit, border {val_border})"
        if args.gt_usm:
            val_more += " [against the USM-sharpened target]"
        print(f"[{args.scale}] epoch {epoch:03d}/{args.epochs} | lr={opt.param_groups[0]['lr']:.2e} | "
              f"train {train_name}={tr_loss:.6f} ({tr_t:.1f}s) | val L1={val_loss:.6f}, PSNR={val_psnr:.2f}dB{val_more} ({val_t:.1f}s)")
        sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}     # un-prefixed keys, like the reference
        # with --ema_decay: the average next to the raw weights, under the key of the published checkpoints; without: the files as ever
        more = {"params_ema": opt.ema_state_dict()} if args.ema_decay else {}
        if with_ssim:
            more["val_ssim"] = val[2]
        if val_border is not None:
            more["val_bench_psnr"], more["val_bench_ssim"] = val[-3], val[-2]
        ckpt_args = saved_args(args)
        if val_loss < best_loss:
            best_loss = val_loss
            torch.save({"model": sd, **more, "epoch": epoch, "best_val_loss": best_loss, "val_psnr": val_psnr, "args": ckpt_args},
                       f"best_{args.arch}_finetune_{args.scale}.pt")
        if val_psnr > best_psnr:
            best_psnr = val_psnr
            torch.save({"model": sd, **more, "epoch": epoch, "best_val_psnr": best_psnr, "val_loss": val_loss, "args": ckpt_args},
                       f"bestpsnr_{args.arch}_finetune_{args.scale}.pt")
    if rank == 0:
        print(f"[time] total: {fmt(time.time() - t_all)}")
        print(f"[done] best_val_loss={best_loss:.6f}, best_val_psnr={best_psnr:.2f} dB")


if __name__ == "__main__":
    main()
