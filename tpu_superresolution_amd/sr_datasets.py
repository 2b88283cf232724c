"""Paired LR/HR PNG dataset of the reference (modules/sr_datasets.py:14-73), host side, PIL only.

Directory contract (DeepRockSR-2D "shuffled2D"):
    <root>/shuffled2D/shuffled2D_<split>_HR/*.png
    <root>/shuffled2D/shuffled2D_<split>_LR_default_<X2|X4>/*x2.png  (stem = HR stem + optional [_-]x<k>)
Pairs are matched by stem; ``transform_pair(lr_pil, hr_pil) -> (lr_tensor, hr_tensor)``.
"""
from __future__ import annotations

import math
import random
import re
from pathlib import Path
from typing import Callable, Optional, Tuple

import numpy as np
import torch
from PIL import Image
from torch.utils.data import Dataset

from ._lib import check, lib
from .augment import AUGMENT_MODES, apply_op_host, dihedral, draw_op
from .degrade_specs import (PSF_MODES, PSF_SIGMA_FLOOR, SECOND_ORDER_VARIATES, TABLE_MODES, DegradeSpec, FixedDegrade, FixedRestore,  # noqa: F401
                            JpegSpec, PsfSpec, RestoreSpec, SecondOrderSpec, UsmSpec, _check_factors, _check_prob3, _check_range)
from .image_ops import (_quant_bits, check_jpeg_quality, degrade_aa, degrade_blind, degrade_psf, degrade_second_order, jpeg_roundtrip,
                        kernel_tables, pack_degrade_params, pack_psf, pack_restore_params, restore_degrade, to_gray)


def _dirs(root: str, split: str, scale: str) -> Tuple[Path, Path]:
    base = Path(root) / "shuffled2D"
    hr, lr = base / f"shuffled2D_{split}_HR", base / f"shuffled2D_{split}_LR_default_{scale}"
    if not (hr.exists() and lr.exists()):
        raise FileNotFoundError(f"HR/LR directories not found for split={split}, scale={scale} under {base}")
    return hr, lr


def _strip_lr_suffix(stem: str, scale: str) -> str:
    suf = scale.lower()
    if not suf.startswith("x"):
        suf = "x" + suf
    return re.sub(rf"([_-]?){re.escape(suf)}$", "", stem, flags=re.IGNORECASE)


class Shuffled2DPaired(Dataset):
    def __init__(self, root: str, split: str = "train", scale: str = "X2",
                 exts: Tuple[str, ...] = (".png", ".jpg", ".jpeg", ".tif", ".tiff"), transform_pair: Optional[Callable] = None):
        self.hr_dir, self.lr_dir = _dirs(root, split, scale)
        self.transform_pair = transform_pair
        hr_map = {p.stem: p for p in sorted(self.hr_dir.iterdir()) if p.suffix.lower() in exts}
        if not hr_map:
            raise RuntimeError(f"no HR files in {self.hr_dir}")
        self.pairs = []
        for p in sorted(self.lr_dir.iterdir()):
            if p.suffix.lower() in exts:
                hr = hr_map.get(_strip_lr_suffix(p.stem, scale))
                if hr is not None:
                    self.pairs.append((p, hr))
        if not self.pairs:
            raise RuntimeError("no LR/HR pairs with matching file stems")

    def __len__(self):
        return len(self.pairs)

    @staticmethod
    def _open(p: Path) -> Image.Image:
        with Image.open(p) as img:
            return img.copy()

    def __getitem__(self, idx: int):
        lr_path, hr_path = self.pairs[idx]
        lr, hr = self._open(lr_path), self._open(hr_path)
        if self.transform_pair is not None:
            lr, hr = self.transform_pair(lr, hr)
        return lr, hr


class Shuffled2DHR(Dataset):
    """The HR images of a split alone (`--synth_lr`): lists <root>/shuffled2D/shuffled2D_<split>_HR; no LR directory is required or
    read.  ``transform(hr_pil) -> tensor``; without one the PIL image is returned."""

    def __init__(self, root: str, split: str = "train", exts: Tuple[str, ...] = (".png", ".jpg", ".jpeg", ".tif", ".tiff"),
                 transform: Optional[Callable] = None):
        self.hr_dir = Path(root) / "shuffled2D" / f"shuffled2D_{split}_HR"
        if not self.hr_dir.exists():
            raise FileNotFoundError(f"HR directory not found for split={split} under {self.hr_dir.parent}")
        self.transform = transform
        self.files = [p for p in sorted(self.hr_dir.iterdir()) if p.suffix.lower() in exts]
        if not self.files:
            raise RuntimeError(f"no HR files in {self.hr_dir}")

    def __len__(self):
        return len(self.files)

    def __getitem__(self, idx: int):
        hr = Shuffled2DPaired._open(self.files[idx])
        return self.transform(hr) if self.transform is not None else hr


def hr_to_tensor3(hr_pil) -> torch.Tensor:
    """HR PIL image -> float32 [3,H,W] in [0,1]: the HR half of PairTransformValid."""
    return ensure_3ch(pil_to_tensor01(hr_pil))


# ---- minimal paired transforms of finetune_swinir.py:80-131 (augmentation: opt-in, augment.py) ------
def pil_to_tensor01(img: Image.Image) -> torch.Tensor:
    """uint8 PIL -> float32 [C,H,W] in [0,1] (torchvision ToImage + ToDtype(scale=True) for 8-bit inputs)."""
    a = np.asarray(img)
    if a.dtype == np.uint16:
        t = torch.from_numpy(a.astype(np.float32) / 65535.0)
    else:
        t = torch.from_numpy(np.ascontiguousarray(a).astype(np.float32) / 255.0)
    return t.unsqueeze(0) if t.ndim == 2 else t.permute(2, 0, 1).contiguous()


def ensure_3ch(t: torch.Tensor) -> torch.Tensor:
    if t.ndim != 3:
        raise ValueError(f"Expected [C,H,W], got {tuple(t.shape)}")
    if t.size(0) == 1:
        return t.repeat(3, 1, 1)
    if t.size(0) != 3:
        raise ValueError(f"Expected C=1 or C=3, got C={t.size(0)}")
    return t


def paired_random_crop(lr_t: torch.Tensor, hr_t: torch.Tensor, lr_patch: int, scale: int):
    """LR crop at (top, left), HR crop at (top*scale, left*scale)  (finetune_swinir.py:96-110)."""
    _, h, w = lr_t.shape
    if h < lr_patch or w < lr_patch:
        raise ValueError(f"LR image too small for patch {lr_patch}: lr_size=({h},{w})")
    top, left = random.randint(0, h - lr_patch), random.randint(0, w - lr_patch)
    hp = lr_patch * scale
    return (lr_t[:, top:top + lr_patch, left:left + lr_patch],
            hr_t[:, top * scale:top * scale + hp, left * scale:left * scale + hp])


class PairTransformTrain:
    """Paired random crop, then (augment 'flip' / 'd4') one D4 transform drawn after the crop corners and applied to both patches.
    'none' (the default) draws nothing and returns the crops as they are."""

    def __init__(self, lr_patch: int, scale: int, augment: str = "none"):
        if augment not in AUGMENT_MODES:
            raise ValueError(f"augment must be one of {AUGMENT_MODES} (got {augment!r})")
        self.lr_patch, self.scale, self.augment = lr_patch, scale, augment

    def __call__(self, lr_pil, hr_pil):
        lr, hr = ensure_3ch(pil_to_tensor01(lr_pil)), ensure_3ch(pil_to_tensor01(hr_pil))
        lr, hr = paired_random_crop(lr, hr, self.lr_patch, self.scale)
        k = draw_op(self.augment)
        return apply_op_host(lr, k), apply_op_host(hr, k)


class PairTransformValid:
    def __init__(self, scale: int):
        self.scale = scale

    def __call__(self, lr_pil, hr_pil):
        return ensure_3ch(pil_to_tensor01(lr_pil)), ensure_3ch(pil_to_tensor01(hr_pil))


# ---- device-resident training set (first slice) ---------------------------------------------------------
class _DeviceImagePool:
    """What the device pools share: groups of pre-decoded 8- / 16-bit images (a pair, or one HR image) packed back to
    back into one byte pool, optionally cut into pinned host shards of which two live on the device.  ``meta[i]`` = (shard, one
    (byte offset, H, W, C | wide << 8) per image of group i); ``_check_group(*entries)`` refuses a group the pool cannot sample.
    And the steps of every `sample`: `_draw_corners` (the global `random`), `_launch` (descriptor upload + one `srk_*crop*` entry),
    `_d4` (the dihedral tail)."""

    def _check_group(self, *entries) -> None:
        raise NotImplementedError

    def _configure(self, device, augment: str, quant_bits=None) -> None:
        """What every pool's constructor checks and keeps: the device, the D4 mode and (where LR values can be rounded) quant_bits."""
        if augment not in AUGMENT_MODES:
            raise ValueError(f"augment must be one of {AUGMENT_MODES} (got {augment!r})")
        if quant_bits is not None:
            self.quant_bits = _quant_bits(quant_bits, type(self).__name__)
        self.augment, self.device = augment, torch.device(device)

    def _pack(self, groups, shard_bytes: Optional[int]) -> None:
        name = type(self).__name__
        shards, chunks, self.meta, off = [], [], [], 0
        for group in groups:
            entry, pieces, size = [], [], 0
            for img in group:
                a = np.asarray(img)
                if a.dtype.byteorder == ">":
                    a = a.astype(a.dtype.newbyteorder("="))
                a = np.ascontiguousarray(a)
                if a.dtype not in (np.uint8, np.uint16):
                    raise ValueError(f"{name} holds 8-bit and 16-bit unsigned images, got {a.dtype}")
                if a.ndim == 2:
                    a = a[:, :, None]
                if a.ndim != 3 or a.shape[2] not in (1, 3):
                    raise ValueError(f"Expected C=1 or C=3, got shape {a.shape}")
                wide = int(a.dtype == np.uint16)
                size += size & 1 if wide else 0                   # uint16 samples start at an even byte
                entry.append([size, a.shape[0], a.shape[1], a.shape[2] | (wide << 8)])
                pieces.append((size, a.view(np.uint8).reshape(-1)))
                size += a.nbytes
            self._check_group(*entry)
            off += off & 1
            if shard_bytes and chunks and off + size > shard_bytes:
                shards.append((chunks, off))
                chunks, off = [], 0
            for e, (rel, flat) in zip(entry, pieces):
                e[0] = off + rel
            chunks.append((off, pieces))
            self.meta.append((len(shards),) + tuple(tuple(e) for e in entry))
            off += size
        if not self.meta:
            raise ValueError(f"{name}: no images")
        shards.append((chunks, off))
        self._host = []
        for sh_chunks, total in shards:
            buf = np.zeros(total, dtype=np.uint8)
            for base, pieces in sh_chunks:
                for rel, flat in pieces:
                    buf[base + rel:base + rel + flat.size] = flat
            t = torch.from_numpy(buf)
            self._host.append(t.pin_memory() if (self.device.type == "cuda" and len(shards) > 1) else t)
        self.num_shards = len(self._host)
        self._resident = {}                   # shard index -> (device tensor, ready event or None)
        self._side = torch.cuda.Stream(device=self.device) if (self.device.type == "cuda" and self.num_shards > 1) else None
        self.pool = self._host[0].to(self.device)          # single-shard pools: the whole set on the device (as before)
        self._resident[0] = (self.pool, None)
        self._current = 0

    def __len__(self):
        return len(self.meta)

    def shard_of(self, index: int) -> int:
        return self.meta[int(index)][0]

    def prefetch(self, shard: int) -> None:
        """Start the asynchronous host->device copy of a shard on the side stream (pinned source: a true async DMA)."""
        shard = int(shard) % self.num_shards
        if shard in self._resident or self._side is None:
            return
        for old in [k for k in self._resident if k != self._current]:      # keep at most two shards on the device
            del self._resident[old]
        with torch.cuda.stream(self._side):
            dev = self._host[shard].to(self.device, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(self._side)
        self._resident[shard] = (dev, ev)

    def _use(self, shard: int) -> torch.Tensor:
        if shard not in self._resident:
            self.prefetch(shard)
        dev, ev = self._resident[shard]
        if ev is not None:
            torch.cuda.current_stream(self.device).wait_event(ev)
            self._resident[shard] = (dev, None)
        if shard != self._current:
            self._current = shard
            self.prefetch(shard + 1)
        self.pool = dev
        return dev

    def _batch_pool(self, indices) -> torch.Tensor:
        """The device tensor of the one shard a batch comes from (switching to it, and prefetching the next, when needed)."""
        shard_ids = {self.meta[int(i)][0] for i in indices}
        if len(shard_ids) != 1:
            raise ValueError("a batch must come from one shard (order the epoch with shard_of())")
        return self._use(shard_ids.pop())

    def _draw_corners(self, indices, patch: int, step: int):
        """-> (six-slot descriptors, D4 codes) of a batch of one-image groups: per sample `random.randint` for the top, for the left, then
        `draw_op`, from the global `random` in DevicePairPool.sample's order; a corner is `step` times a draw in 0..extent // step - patch."""
        hd, codes = [], []
        for i in indices:
            _, (o, h, w, c) = self.meta[int(i)]
            top, left = random.randint(0, h // step - patch), random.randint(0, w // step - patch)
            hd.append((o, h, w, c, top * step, left * step))
            codes.append(draw_op(self.augment))
        return hd, codes

    def _launch(self, entry_name: str, pool: torch.Tensor, rows, outs, *ints, extra=()) -> None:
        """One launch of a `srk_*crop*` entry: `rows` go up as ONE int64 table -- ints[0] = B rows per descriptor argument, so the 2 B
        rows of srk_paired_crop_u8 are its two -- and the entry gets (pool, descriptors..., *extra, outs..., *ints, stream).  Raw
        `data_ptr()` on the pool's own device and stream: a pool may live on another device than the current one."""
        desc = torch.tensor(rows, dtype=torch.int64).to(self.device)
        row_bytes = 8 * desc.shape[1]
        check(getattr(lib(), entry_name)(pool.data_ptr(), *(desc.data_ptr() + i * row_bytes for i in range(0, len(rows), ints[0])), *extra,
                                         *(o.data_ptr() for o in outs), *ints, torch.cuda.current_stream(self.device).cuda_stream))

    def _empty(self, *shape) -> torch.Tensor:
        return torch.empty(shape, dtype=torch.float32, device=self.device)

    def _d4(self, codes, *tensors):
        """The batches under their samples' D4 codes: one `srk_dihedral_f32` launch each after one upload, none when every code is 0."""
        if not any(codes):
            return tensors
        ops = torch.tensor(codes, dtype=torch.int32).to(self.device)
        return tuple(dihedral(t, ops) for t in tensors)


class DevicePairPool(_DeviceImagePool):
    """Pre-decoded 8-bit LR/HR pairs in GPU memory + the paired train transform as one kernel pair per batch
    (`srk_paired_crop_u8`).  `sample(indices)` draws the crop corners with the same two `random.randint` calls per sample, in
    the same order, as `paired_random_crop` (finetune_swinir.py:96-110), so a host pipeline and this pool produce identical
    batches from the same `random` state.  8-bit and 16-bit (uint16 -> value / 65535, as pil_to_tensor01) images, mixed freely.

    ``shard_bytes``: when the decoded set is larger than this, it stays in PINNED host memory as shards and only two shards
    live on the device: ``prefetch(s)`` starts the asynchronous copy of shard s on a side stream, ``sample`` of an index in a
    shard that is not resident switches to it (joining its copy) and prefetches the next one -- the host->device transfer of
    shard s+1 overlaps the training steps on shard s.  ``shard_of(i)`` tells a sampler which shard an image
    lives in, so that epochs can be ordered shard by shard.

    ``augment`` ('none' | 'flip' | 'd4', augment.draw_op): `sample` draws one D4 code per sample right after its crop corners -- the
    order PairTransformTrain draws in, so the two paths still agree from the same `random` state -- and, when any code is non-zero,
    transforms the LR and the HR batch with one `srk_dihedral_f32` launch each (per-sample codes; patches are square)."""

    def __init__(self, pairs, lr_patch: int, scale: int, device="cuda", shard_bytes: Optional[int] = None, augment: str = "none"):
        """pairs: iterable of (lr, hr) PIL images or uint8 / uint16 arrays [H,W] / [H,W,1|3]."""
        self._configure(device, augment)
        self.lr_patch, self.scale = int(lr_patch), int(scale)
        self._pack(pairs, shard_bytes)

    def _check_group(self, lr, hr) -> None:
        (_, lh, lw, _), (_, hh, hw, _) = lr, hr
        if lh < self.lr_patch or lw < self.lr_patch:
            raise ValueError(f"LR image too small for patch {self.lr_patch}: lr_size=({lh},{lw})")
        if hh < lh * self.scale or hw < lw * self.scale:
            raise ValueError(f"HR image ({hh},{hw}) smaller than scale x LR ({lh},{lw})")

    def sample(self, indices):
        """-> (lr [B,3,P,P], hr [B,3,P*s,P*s]) fp32 on the device; advances the global `random` state like the host transform."""
        P, s = self.lr_patch, self.scale
        ld, hd, codes = [], [], []
        pool = self._batch_pool(indices)
        for i in indices:
            _, (lo, lh, lw, lc), (ho, hh, hw, hc) = self.meta[int(i)]
            top, left = random.randint(0, lh - P), random.randint(0, lw - P)
            ld.append((lo, lh, lw, lc, top, left))
            hd.append((ho, hh, hw, hc, top * s, left * s))
            codes.append(draw_op(self.augment))
        B = len(ld)
        lr, hr = self._empty(B, 3, P, P), self._empty(B, 3, P * s, P * s)
        self._launch("srk_paired_crop_u8", pool, ld + hd, (lr, hr), B, P, s)
        return self._d4(codes, lr, hr)


class DeviceHRPool(_DeviceImagePool):
    """Training pairs from HR images only (`--synth_lr`): the pool holds the decoded HR images -- half the device memory of a
    DevicePairPool at x2, no LR files to keep in sync -- and `sample` makes the HR patch AND its antialiased bicubic degradation
    (PIL's BICUBIC convention) in one launch (`srk_crop_degrade_u8`, csrc/resize.hip).  The LR patch is exactly the window of the
    (H // s, W // s) downscale of the image's top-left (H - H % s, W - W % s) region: the taps reach past the patch into the image.

    Same surface as DevicePairPool (shards, prefetch, augment), and `sample` draws `random.randint(0, H // s - P)`,
    `random.randint(0, W // s - P)` and the D4 code per sample -- DevicePairPool's order and ranges, so from one `random` state
    both pools cut the same HR patches.  ``quant_bits`` 8 (default): LR values are rounded to k / 255 as an 8-bit LR file would hold
    them; 0: the filtered fp32 values.

    ``degrade`` (a DegradeSpec; None = the clean downscale, today's launch): every sample is blurred and noised with parameters drawn
    from the spec's own generator (seed + ``rank``), in one `srk_crop_degrade_blind_u8` launch on ten-slot descriptors.  `draw`, and
    with it the global `random` state, the HR patches and the D4 codes, is the same with and without a spec.

    ``jpeg`` (a JpegSpec; None = no such stage, no further launch): the LR batch goes through `ops.jpeg_roundtrip` at one quality per
    sample from the spec's own generator, after the degrade launch and BEFORE the D4 transform, so the block grid is anchored to the
    patch as cut.  Needs ``quant_bits`` 8: JPEG codes 8-bit images.  `draw` and `draw_degrade` do not see it.

    ``psf`` (a PsfSpec; None = the axis-aligned Gaussian composed into the cubic tables, today's launch; needs ``degrade``): every
    sample is blurred with a 2-D table made from the sigmas of its `DegradeSpec.draw` and the PsfSpec's own generator, uploaded as one
    [B][ks][ks] block, in one `srk_crop_degrade_psf_u8` launch.  The DegradeSpec's draws, `draw` and the global `random` state are the
    same with and without it.

    ``tables`` "host" (default): the tables are evaluated in fp64 numpy and uploaded.  "device": `PsfSpec.draw` returns descriptors
    and `ops.kernel_tables` builds the block on the device (eight doubles per sample go up instead of ks^2 floats; a `file` bank is
    uploaded once, here); the draws are the same, the taps agree to one fp32 spacing."""

    def __init__(self, images, lr_patch: int, scale: int, device="cuda", shard_bytes: Optional[int] = None, augment: str = "none",
                 quant_bits: int = 8, degrade: Optional[DegradeSpec] = None, rank: int = 0, jpeg: Optional[JpegSpec] = None,
                 psf: Optional[PsfSpec] = None, tables: str = "host"):
        """images: iterable of HR PIL images or uint8 / uint16 arrays [H,W] / [H,W,1|3]."""
        self._configure(device, augment, quant_bits)
        if not 2 <= int(scale) <= 4:
            raise ValueError(f"DeviceHRPool degrades by an integer factor in 2..4 (got {scale!r})")
        if degrade is not None and not isinstance(degrade, DegradeSpec):
            raise ValueError(f"degrade must be a DegradeSpec or None (got {type(degrade).__name__})")
        if jpeg is not None and not isinstance(jpeg, JpegSpec):
            raise ValueError(f"jpeg must be a JpegSpec or None (got {type(jpeg).__name__})")
        if jpeg is not None and quant_bits != 8:
            raise ValueError(f"jpeg= codes 8-bit LR images: it needs quant_bits 8 (got {quant_bits!r})")
        self.degrade, self._degrade_rng = degrade, (degrade.rng(rank) if degrade is not None else None)
        self.jpeg, self._jpeg_rng = jpeg, (jpeg.rng(rank) if jpeg is not None else None)
        if psf is not None and not isinstance(psf, PsfSpec):
            raise ValueError(f"psf must be a PsfSpec or None (got {type(psf).__name__})")
        if psf is not None and degrade is None:
            raise ValueError("psf= shapes the blur of degrade=: it needs a DegradeSpec")
        self.psf, self._psf_rng, self._psf_buf = psf, (psf.rng(rank) if psf is not None else None), None
        if tables not in TABLE_MODES:
            raise ValueError(f"tables must be one of {TABLE_MODES} (got {tables!r})")
        self.tables = tables
        self.lr_patch, self.scale = int(lr_patch), int(scale)
        self._bank = None
        if tables == "device" and psf is not None and psf.tables is not None:
            self._bank = torch.from_numpy(psf.tables).to(self.device)
        self._pack(((img,) for img in images), shard_bytes)

    def _check_group(self, hr) -> None:
        _, hh, hw, _ = hr
        if hh // self.scale < self.lr_patch or hw // self.scale < self.lr_patch:
            raise ValueError(f"HR image ({hh},{hw}) too small for LR patch {self.lr_patch} at scale {self.scale}")

    def draw(self, indices):
        """-> (HR descriptors, D4 codes) of a batch; advances the global `random` state exactly as DevicePairPool.sample does."""
        return self._draw_corners(indices, self.lr_patch, self.scale)

    def draw_degrade(self, hd):
        """The ten-slot descriptors of a batch: `draw`'s six plus the packed parameters of one `DegradeSpec.draw` per sample, from the
        spec's generator alone (the global `random` state is not touched)."""
        return [tuple(d) + tuple(pack_degrade_params(*self.degrade.draw(self._degrade_rng, colour=(d[3] & 0xff) == 3))) for d in hd]

    def draw_psf(self, hd):
        """(ten-slot descriptors, fp32 numpy [B][ks][ks], ks) of a batch: `draw_degrade`'s draws, in its order, plus one `PsfSpec.draw`
        per sample on the sigmas of that sample; slot 6 keeps the sigmas, which the PSF entry ignores.  With tables = "device":
        (descriptors, the batch's `ops.DeviceTables`, ks), built by one `ops.kernel_tables` launch."""
        rows, tabs = [], []
        for d in hd:
            drawn = self.degrade.draw(self._degrade_rng, colour=(d[3] & 0xff) == 3)
            rows.append(tuple(d) + tuple(pack_degrade_params(*drawn)))
            tabs.append(self.psf.draw(self._psf_rng, drawn[0], as_desc=self.tables == "device"))
        if self.tables == "device":
            built = kernel_tables(tabs, bank=self._bank, signed=False, device=self.device)
            return rows, built, built.ks
        return (rows,) + pack_psf(tabs, len(tabs), checked=True)

    def _psf_upload(self, tabs) -> torch.Tensor:
        """The batch's tables in the pool's device buffer (grown when a batch is larger than any before): one copy."""
        n = tabs.size
        if self._psf_buf is None or self._psf_buf.numel() < n:
            self._psf_buf = torch.empty(max(n, 32 * 21 * 21), dtype=torch.float32, device=self.device)
        self._psf_buf[:n].copy_(torch.from_numpy(tabs).reshape(-1))
        return self._psf_buf

    def sample(self, indices):
        """-> (lr [B,3,P,P], hr [B,3,P*s,P*s]) fp32 on the device."""
        P, s = self.lr_patch, self.scale
        pool = self._batch_pool(indices)
        hd, codes = self.draw(indices)
        B = len(hd)
        lr, hr = self._empty(B, 3, P, P), self._empty(B, 3, P * s, P * s)
        if self.psf is not None:
            rows, tabs, ks = self.draw_psf(hd)
            k = tabs.tab if self.tables == "device" else self._psf_upload(tabs)
            self._launch("srk_crop_degrade_psf_u8", pool, rows, (lr, hr), B, P, s, self.quant_bits, extra=(k.data_ptr(), ks))
        elif self.degrade is not None:
            self._launch("srk_crop_degrade_blind_u8", pool, self.draw_degrade(hd), (lr, hr), B, P, s, self.quant_bits)
        else:
            self._launch("srk_crop_degrade_u8", pool, hd, (lr, hr), B, P, s, self.quant_bits)
        if self.jpeg is not None:
            lr = jpeg_roundtrip(lr, [self.jpeg.draw(self._jpeg_rng) for _ in range(B)], self.jpeg.subsample)
        return self._d4(codes, lr, hr)


def stage1_table(blur, as_desc: bool = False):
    """The stage-1 table of the second-order chain when no PsfSpec shapes it: the axis-aligned Gaussian of DegradeSpec's
    (sigma_y, sigma_x), R = min(ceil(3 sigma), 10), as a 2-D table (the chain filters with `ops.filter2d` only).  as_desc: its
    `blur_kernels.TableDesc`."""
    from . import blur_kernels as bk
    if as_desc:
        bk = bk.TableDesc
    sy, sx = (float(v) for v in blur)
    ks = 2 * min(math.ceil(3.0 * max(0.0, sy, sx)), 10) + 1
    return bk.gaussian(ks, max(sx, PSF_SIGMA_FLOOR), max(sy, PSF_SIGMA_FLOOR), 0.0)


def second_order_window(top: int, left: int, Hr: int, Wr: int, s: int, P: int, m: int):
    """The E x E window, E = s (P + 2 m), that the chain of an HR patch at (top, left) runs on, inside the image's Hr x Wr region: cut
    at the patch origin minus s m, then clamped into the region.  -> (window top, window left, LR row, LR column of the patch in it)."""
    E = s * (P + 2 * m)
    wt, wl = min(max(top - s * m, 0), Hr - E), min(max(left - s * m, 0), Wr - E)
    return wt, wl, (top - wt) // s, (left - wl) // s


class DeviceHR2Pool(DeviceHRPool):
    """Training pairs under the second-order degradation (`--degrade second_order`).  `draw` is DeviceHRPool's: from one
    `random` state both pools cut the same HR patches and D4 codes, and the HR patch is `srk_crop_u8`'s -- bit-identical to
    srk_paired_crop_u8's.  The chain changes sizes per sample and filters with a reflect border, so it cannot run on a window of the
    whole image bit for bit; it runs on an EXTENDED window of E = s (P + 2 m) HR pixels around the patch (`margin` m LR pixels, cut at
    the patch origin minus s m and clamped into the image's (H - H % s, W - W % s) region), and the LR patch is the P x P window of
    `ops.degrade_second_order`'s output at the patch's offset: the margin keeps the reflected border, the JPEG grid's edge and the
    resize's border taps away from the patch.  Noise is keyed on window coordinates.
    Stage 1 reuses ``degrade`` (a DegradeSpec: sigmas, noise, gray flag, noise id) and ``psf`` (a PsfSpec shaping the table; None =
    the axis-aligned Gaussian as a table); ``spec`` (a SecondOrderSpec) draws the rest from its own generator.  An image whose region
    is smaller than E is refused at construction.  The padded work buffers have the spec's largest sizes and are kept between calls:
    the launches and their shapes are the same every step.  ``tables`` "device": every stage's tables are built on the device from
    descriptors (DeviceHRPool's switch; three `ops.kernel_tables` launches per batch, no table evaluated or uploaded by the host).
    ``usm`` (a UsmSpec): the E x E window is unsharp-masked once, the chain runs on the sharpened window, and the HR patch is
    the P s window of the SHARPENED WINDOW at the patch's offset (not `srk_crop_u8`'s patch): a pixel of it depends on HR pixels up to
    2R away, so margin * scale >= 2R keeps the window's reflected edge out of the patch (13 at x4 for the default R = 25; the default
    margin of 8 does not).  None leaves `sample` as it was.  `spec.resize_mode_prob` draws the resize rules from a generator of its own."""

    def __init__(self, images, lr_patch: int, scale: int, spec: "SecondOrderSpec", degrade: Optional[DegradeSpec] = None, device="cuda",
                 shard_bytes: Optional[int] = None, augment: str = "none", rank: int = 0, psf: Optional[PsfSpec] = None, margin: int = 8,
                 subsample: bool = False, names=None, tables: str = "host", usm: Optional["UsmSpec"] = None):
        if not isinstance(spec, SecondOrderSpec):
            raise ValueError(f"spec must be a SecondOrderSpec (got {type(spec).__name__})")
        if usm is not None and not isinstance(usm, UsmSpec):
            raise ValueError(f"usm must be a UsmSpec (got {type(usm).__name__})")
        if isinstance(margin, bool) or int(margin) != margin or not 0 <= int(margin) <= 64:
            raise ValueError(f"margin must be an integer in 0..64 LR pixels (got {margin!r})")
        self.spec, self._spec_rng, self.margin, self.subsample = spec, spec.rng(rank), int(margin), bool(subsample)
        # at the default (0, 0, 1) every draw is the cubic whatever the variates: the generator is not consulted and `draw` costs what it did
        self._mode_rng = spec.mode_rng(rank) if spec.resize_mode_prob != (0.0, 0.0, 1.0) else None
        self.usm = usm
        self.extent = int(scale) * (int(lr_patch) + 2 * self.margin)
        if usm is not None and self.extent <= usm.ks // 2:
            raise ValueError(f"the {self.extent} x {self.extent} window of the second-order degradation is not larger than the R = "
                             f"{usm.ks // 2} of the unsharp mask (LR patch {lr_patch} + 2 x margin {margin}, scale {scale})")
        self._names = None if names is None else list(names)
        self._bufs: dict = {}
        super().__init__(images, lr_patch, scale, device, shard_bytes, augment, 8, degrade if degrade is not None else DegradeSpec(), rank, None, psf,
                         tables)
        rnd = lambda v: max(1, int(v + 0.5))          # noqa: E731
        E, s = self.extent, self.scale
        self.pads = ((rnd(E * spec.resize_range[1]),) * 2, (rnd(E / s * spec.resize2_range[1]),) * 2)

    def _check_group(self, hr) -> None:
        super()._check_group(hr)
        _, hh, hw, _ = hr
        s, E = self.scale, self.extent
        if hh - hh % s < E or hw - hw % s < E:
            i = len(self.meta)
            name = self._names[i] if self._names is not None and i < len(self._names) else f"image {i}"
            raise ValueError(f"{name}: its ({hh - hh % s},{hw - hw % s}) region is smaller than the {E} x {E} window of the second-order "
                             f"degradation (LR patch {self.lr_patch} + 2 x margin {self.margin}, scale {s})")

    def draw_second_order(self, hd):
        """-> (window descriptors, LR offsets of the patches in their windows, one ops.SecondOrder per sample): DegradeSpec's and
        PsfSpec's draws in DeviceHRPool's order, then SecondOrderSpec's; the global `random` state is not touched."""
        P, s, m = self.lr_patch, self.scale, self.margin
        wd, offs, params = [], [], []
        for ho, hh, hw, hc, top, left in hd:
            wt, wl, oy, ox = second_order_window(top, left, hh - hh % s, hw - hw % s, s, P, m)
            wd.append((ho, hh, hw, hc, wt, wl))
            offs.append((oy, ox))
            colour = (hc & 0xff) == 3
            blur, noise, nid, gray = self.degrade.draw(self._degrade_rng, colour=colour)
            dev = self.tables == "device"
            table1 = self.psf.draw(self._psf_rng, blur, dev) if self.psf is not None else stage1_table(blur, dev)
            params.append(self.spec.draw(self._spec_rng, table1, noise, nid, gray, colour, self.extent, s, dev, self._mode_rng))
        return wd, offs, params

    def _crop(self, pool, rows, patch: int) -> torch.Tensor:
        out = self._empty(len(rows), 3, patch, patch)
        self._launch("srk_crop_u8", pool, rows, (out,), len(rows), patch)
        return out

    def sample(self, indices):
        """-> (lr [B,3,P,P], hr [B,3,P*s,P*s]) fp32 on the device."""
        P, s = self.lr_patch, self.scale
        pool = self._batch_pool(indices)
        hd, codes = self.draw(indices)
        wd, offs, params = self.draw_second_order(hd)
        if self.usm is None:
            hr = self._crop(pool, hd, P * s)
            win = self._crop(pool, wd, self.extent)
        else:          # the target is a window of the sharpened WINDOW, and the chain runs on the sharpened window
            win = self.usm.sharpen(self._crop(pool, wd, self.extent))
        whole = degrade_second_order(win, s, params, self.subsample, self.pads, self._bufs, self._bank)
        if len(set(offs)) == 1:
            (oy, ox), = set(offs)
            lr = whole[:, :, oy:oy + P, ox:ox + P].contiguous()
            if self.usm is not None:
                hr = win[:, :, oy * s:(oy + P) * s, ox * s:(ox + P) * s].contiguous()
        else:
            lr = torch.stack([whole[b, :, oy:oy + P, ox:ox + P] for b, (oy, ox) in enumerate(offs)])
            if self.usm is not None:
                hr = torch.stack([win[b, :, oy * s:(oy + P) * s, ox * s:(ox + P) * s] for b, (oy, ox) in enumerate(offs)])
        return self._d4(codes, lr, hr)


def _equal_channels(x: torch.Tensor):
    """Per image of a [B,3,H,W] batch: are its three channels equal (a gray image held as RGB, which gets gray noise)?  -> B bools, the
    batch's one host read."""
    return ((x[:, 0] == x[:, 1]) & (x[:, 0] == x[:, 2])).flatten(1).all(dim=1).tolist()


class SynthLRBatches:
    """Wraps a loader of HR batches [B,3,H,W] into the (lr, hr) batches of `--synth_lr` validation / evaluation: each HR batch goes to
    the device, is cropped to a multiple of the factor and degraded there (ops.degrade_aa) -- the whole-image form of what
    DeviceHRPool's training patches are windows of.

    ``degrade`` (a FixedDegrade, or a DegradeSpec standing for its `fixed()` midpoints; None = the clean downscale): every image gets
    the SAME blur and noise amplitudes and the noise id = its index in the split (the loader must not shuffle), so every epoch and
    every run scores the same LR images (ops.degrade_blind).  An image whose three channels are equal gets gray noise.

    ``jpeg`` (a quality 1..100 with ``jpeg_subsample``, or a JpegSpec standing for its `fixed()` quality and its subsampling; None =
    no such stage): the whole degraded LR image goes through `ops.jpeg_roundtrip`, the same every epoch.  Needs ``quant_bits`` 8.

    ``psf`` (one ks x ks table, or a PsfSpec standing for its `fixed()` table -- table 0 of a PSF file, None otherwise; needs
    ``degrade``): the table replaces the Gaussian of ``degrade`` (ops.degrade_psf); the noise stays.

    ``second_order`` (a SecondOrderSpec standing for its `fixed()` chain; needs ``degrade`` and ``quant_bits`` 8, takes no ``jpeg``):
    the whole cropped image goes through `ops.degrade_second_order` with ``degrade`` / ``psf`` as its stage 1; the noise id is the
    image's index in the split, the same every epoch.  The fixed chain resizes with the cubic.

    ``usm`` (a UsmSpec; needs ``second_order``): the whole cropped image is unsharp-masked (ops.usm_sharpen), the chain runs on the
    sharpened image, and the yielded HR is the sharpened image -- the target `--gt_usm` trains against."""

    def __init__(self, loader, scale: int, quant_bits: int, device, degrade=None, jpeg=None, jpeg_subsample: bool = False, psf=None,
                 second_order=None, usm=None):
        self.loader, self.scale, self.quant_bits, self.device = loader, int(scale), int(quant_bits), torch.device(device)
        if usm is not None and (not isinstance(usm, UsmSpec) or second_order is None):
            raise ValueError("usm= takes a UsmSpec and sharpens the target of the second-order chain: it needs second_order=")
        self.usm = usm
        if second_order is not None:
            if not isinstance(second_order, SecondOrderSpec):
                raise ValueError(f"second_order must be a SecondOrderSpec (got {type(second_order).__name__})")
            if degrade is None or self.quant_bits != 8 or jpeg is not None:
                raise ValueError("second_order= needs degrade= (its stage 1), quant_bits 8, and takes its JPEG qualities from the spec (no jpeg=)")
        self.second_order = second_order
        if isinstance(psf, PsfSpec):
            psf = psf.fixed()
        if psf is not None:
            from .blur_kernels import check_table
            if degrade is None:
                raise ValueError("psf= shapes the blur of degrade=: it needs a FixedDegrade or a DegradeSpec")
            psf = check_table(psf)
        self.psf = psf
        if isinstance(jpeg, JpegSpec):
            jpeg, jpeg_subsample = jpeg.fixed(), jpeg.subsample
        if jpeg is not None:
            jpeg = check_jpeg_quality(jpeg)
            if self.quant_bits != 8:
                raise ValueError(f"jpeg= codes 8-bit LR images: it needs quant_bits 8 (got {quant_bits!r})")
        self.jpeg, self.jpeg_subsample = jpeg, bool(jpeg_subsample)
        self.degrade = degrade.fixed() if isinstance(degrade, DegradeSpec) else degrade
        if self.degrade is not None:
            pack_degrade_params(self.degrade.blur, self.degrade.noise, 0, self.degrade.gray_noise)          # the ranges, before any batch

    def __len__(self):
        return len(self.loader)

    def __iter__(self):
        for lr, hr in self._degraded():
            yield (lr if self.jpeg is None else jpeg_roundtrip(lr, self.jpeg, self.jpeg_subsample)), hr

    def _degraded(self):
        first = 0
        for hr in self.loader:
            hr = hr.to(self.device, dtype=torch.float32)
            if self.degrade is None:
                yield degrade_aa(hr, self.scale, self.quant_bits)
                continue
            B = hr.shape[0]
            gray = [True] * B
            if hr.shape[1] == 3 and not self.degrade.gray_noise:
                gray = _equal_channels(hr)
            if self.second_order is not None:
                H, W = hr.shape[-2:]
                hr = hr[..., :H - H % self.scale, :W - W % self.scale].contiguous()
                if self.usm is not None:
                    hr = self.usm.sharpen(hr)
                table1 = self.psf if self.psf is not None else stage1_table(self.degrade.blur)
                params = [self.second_order.fixed(table1, self.degrade.noise, gray[b], first + b) for b in range(B)]
                yield degrade_second_order(hr, self.scale, params, self.jpeg_subsample), hr
            elif self.psf is not None:
                yield degrade_psf(hr, self.scale, self.psf, self.degrade.noise, range(first, first + B), gray, self.quant_bits)
            else:
                yield degrade_blind(hr, self.scale, self.degrade.blur, self.degrade.noise, range(first, first + B), gray, self.quant_bits)
            first += B


# ---- scale-1 restoration: denoising and JPEG-artifact pairs ---------------------------------------------------------
class DeviceRestorePool(_DeviceImagePool):
    """Training pairs of the scale-1 tasks from clean images only (`--task dn | car`): `sample` cuts a P x P patch at ANY image pixel and
    makes the clean target and the degraded input in one launch (`srk_crop_restore_u8`, csrc/restore.hip).  The degraded patch is
    exactly the window of the whole-image degradation (ops.restore_degrade): noise keyed on image coordinates, JPEG blocks anchored
    at the image's (0, 0) -- so a batch sees 8 x 8 block edges at every phase relative to its patch, as crops of compressed files do.

    ``out_chans`` 3: RGB (a gray source is repeated); 1: gray (an RGB source becomes the integer luma of ops.to_gray).
    Same surface as DevicePairPool (shards, prefetch, augment): `draw` takes `random.randint(0, H - P)`, `random.randint(0, W - P)` and
    the D4 code per sample from the global `random`, in DevicePairPool's order, so from one `random` state a DevicePairPool at
    lr_patch P cuts the same LR windows.  The degradation parameters come from ``spec``'s own generator (seed + ``rank``).
    ``quant_bits`` 0 (default): the noised values are neither clipped nor rounded, as the published denoising recipe has it; 8: they
    are rounded to k / 255 (with a JPEG stage its 8-bit level step does that in either case)."""

    def __init__(self, images, patch: int, out_chans: int = 3, spec: Optional[RestoreSpec] = None, device="cuda",
                 shard_bytes: Optional[int] = None, augment: str = "none", quant_bits: int = 0, rank: int = 0):
        """images: iterable of clean PIL images or uint8 / uint16 arrays [H,W] / [H,W,1|3]."""
        self._configure(device, augment, quant_bits)
        if out_chans not in (1, 3):
            raise ValueError(f"out_chans must be 1 or 3 (got {out_chans!r})")
        if not isinstance(spec, RestoreSpec):
            raise ValueError(f"spec must be a RestoreSpec (got {type(spec).__name__})")
        if not 1 <= int(patch) <= 2048:
            raise ValueError(f"patch must be in 1..2048 (got {patch!r})")
        self.spec, self._spec_rng = spec, spec.rng(rank)
        self.patch, self.out_chans = int(patch), int(out_chans)
        self._pack(((img,) for img in images), shard_bytes)

    def _check_group(self, img) -> None:
        _, h, w, _ = img
        if h < self.patch or w < self.patch:
            raise ValueError(f"image ({h},{w}) too small for patch {self.patch}")

    def draw(self, indices):
        """-> (descriptors, D4 codes) of a batch; advances the global `random` state exactly as DevicePairPool.sample does."""
        return self._draw_corners(indices, self.patch, 1)

    def draw_restore(self, hd):
        """The ten-slot descriptors of a batch: `draw`'s six plus the packed parameters of one `RestoreSpec.draw` per sample, from the
        spec's generator alone (the global `random` state is not touched)."""
        rows = []
        for d in hd:
            sigma, q, nid, gray = self.spec.draw(self._spec_rng, colour=(d[3] & 0xff) == 3 and self.out_chans == 3)
            rows.append(tuple(d) + tuple(pack_restore_params(q, (sigma, 0.0), nid, gray)))
        return rows

    def sample(self, indices):
        """-> (degraded [B,out_chans,P,P], clean [B,out_chans,P,P]) fp32 on the device: one descriptor upload, one launch."""
        P, Co = self.patch, self.out_chans
        pool = self._batch_pool(indices)
        hd, codes = self.draw(indices)
        B = len(hd)
        clean, degraded = self._empty(B, Co, P, P), self._empty(B, Co, P, P)
        self._launch("srk_crop_restore_u8", pool, self.draw_restore(hd), (clean, degraded), B, P, Co, int(self.spec.subsample), self.quant_bits)
        return self._d4(codes, degraded, clean)


class RestoreBatches:
    """Wraps a loader of clean batches [B,out_chans,H,W] into the (degraded, clean) batches of `--task dn | car` validation /
    evaluation: each batch goes to the device and is degraded there as a whole image (ops.restore_degrade) -- what
    DeviceRestorePool's training patches are windows of.  ``spec_or_fixed``: a FixedRestore, or a RestoreSpec standing for its
    `fixed()` values.  Every image gets the SAME sigma and quality and the noise id = its index in the split (the loader must not
    shuffle), so every epoch and every run scores the same degraded images.  A colour image whose three channels are equal gets gray
    noise, as its gray file would."""

    def __init__(self, loader, out_chans: int, spec_or_fixed, quant_bits: int, device):
        if out_chans not in (1, 3):
            raise ValueError(f"out_chans must be 1 or 3 (got {out_chans!r})")
        _quant_bits(quant_bits, "RestoreBatches")
        fx = spec_or_fixed.fixed() if isinstance(spec_or_fixed, RestoreSpec) else spec_or_fixed
        if not isinstance(fx, FixedRestore):
            raise ValueError(f"spec_or_fixed must be a RestoreSpec or a FixedRestore (got {type(spec_or_fixed).__name__})")
        pack_restore_params(fx.jpeg_quality, (fx.sigma, 0.0), 0, fx.gray_noise)          # the ranges, before any batch
        self.loader, self.out_chans, self.fixed, self.quant_bits, self.device = loader, int(out_chans), fx, int(quant_bits), torch.device(device)

    def __len__(self):
        return len(self.loader)

    def __iter__(self):
        fx, first = self.fixed, 0
        for clean in self.loader:
            clean = clean.to(self.device, dtype=torch.float32).contiguous()
            if clean.dim() != 4 or clean.shape[1] != self.out_chans:
                raise ValueError(f"RestoreBatches(out_chans={self.out_chans}) got a batch of shape {tuple(clean.shape)}")
            B = clean.shape[0]
            gray = [True] * B
            if self.out_chans == 3 and not fx.gray_noise:
                gray = _equal_channels(clean)
            yield restore_degrade(clean, (fx.sigma, 0.0), range(first, first + B), gray, fx.jpeg_quality, fx.subsample, self.quant_bits), clean
            first += B


def clean_to_tensor(img, out_chans: int) -> torch.Tensor:
    """A clean PIL image as the fp32 [out_chans,H,W] tensor in [0, 1] that DeviceRestorePool cuts its targets from: three channels as
    `hr_to_tensor3`; one channel = the stored gray samples, or the integer luma (ops.to_gray) of an RGB image, over 255 / 65535."""
    if out_chans == 3:
        return hr_to_tensor3(img)
    a = np.asarray(img)
    if a.dtype.byteorder == ">":
        a = a.astype(a.dtype.newbyteorder("="))
    if a.dtype not in (np.uint8, np.uint16):
        raise ValueError(f"clean images are 8-bit or 16-bit (got {a.dtype})")
    if a.ndim == 3 and a.shape[2] == 3:
        a = to_gray(a)
    elif a.ndim == 3 and a.shape[2] == 1:
        a = a[:, :, 0]
    elif a.ndim != 2:
        raise ValueError(f"Expected C=1 or C=3, got shape {a.shape}")
    div = np.float32(255.0 if a.dtype == np.uint8 else 65535.0)
    return torch.from_numpy(np.ascontiguousarray(a).astype(np.float32) / div).unsqueeze(0)          # IEEE fp32 division, as pil_to_tensor01
