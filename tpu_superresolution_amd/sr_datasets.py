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
from dataclasses import dataclass
from pathlib import Path
from typing import Callable, NamedTuple, Optional, Tuple

import numpy as np
import torch
from PIL import Image
from torch.utils.data import Dataset

from .augment import AUGMENT_MODES, apply_op_host, draw_op


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
    """What DevicePairPool and DeviceHRPool share: groups of pre-decoded 8- / 16-bit images (a pair, or one HR image) packed back to
    back into one byte pool, optionally cut into pinned host shards of which two live on the device.  ``meta[i]`` = (shard, one
    (byte offset, H, W, C | wide << 8) per image of group i); ``_check_group(*entries)`` refuses a group the pool cannot sample."""

    def _check_group(self, *entries) -> None:
        raise NotImplementedError

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
        if augment not in AUGMENT_MODES:
            raise ValueError(f"augment must be one of {AUGMENT_MODES} (got {augment!r})")
        self.augment = augment
        self.lr_patch, self.scale, self.device = int(lr_patch), int(scale), torch.device(device)
        self._pack(pairs, shard_bytes)

    def _check_group(self, lr, hr) -> None:
        (_, lh, lw, _), (_, hh, hw, _) = lr, hr
        if lh < self.lr_patch or lw < self.lr_patch:
            raise ValueError(f"LR image too small for patch {self.lr_patch}: lr_size=({lh},{lw})")
        if hh < lh * self.scale or hw < lw * self.scale:
            raise ValueError(f"HR image ({hh},{hw}) smaller than scale x LR ({lh},{lw})")

    def sample(self, indices):
        """-> (lr [B,3,P,P], hr [B,3,P*s,P*s]) fp32 on the device; advances the global `random` state like the host transform."""
        from ._lib import check, lib
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
        desc = torch.tensor(ld + hd, dtype=torch.int64).to(self.device)
        lr = torch.empty(B, 3, P, P, dtype=torch.float32, device=self.device)
        hr = torch.empty(B, 3, P * s, P * s, dtype=torch.float32, device=self.device)
        st = torch.cuda.current_stream(self.device).cuda_stream
        check(lib().srk_paired_crop_u8(pool.data_ptr(), desc[:B].data_ptr(), desc[B:].data_ptr(), lr.data_ptr(), hr.data_ptr(),
                                       B, P, s, st))
        if any(codes):
            from .augment import dihedral
            ops = torch.tensor(codes, dtype=torch.int32).to(self.device)
            lr, hr = dihedral(lr, ops), dihedral(hr, ops)
        return lr, hr


class FixedDegrade(NamedTuple):
    """One fixed blind degradation (validation, evaluation): blur = (sigma_y, sigma_x) in HR pixels, noise = (sigma_n, gain) in [0, 1]
    units, gray_noise = one draw for the three channels of a colour image (a gray image always gets one)."""
    blur: Tuple[float, float]
    noise: Tuple[float, float]
    gray_noise: bool = False


def _check_range(name: str, r, hi: float) -> Tuple[float, float]:
    try:
        a, b = (float(v) for v in r)
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be two numbers LO HI (got {r!r})") from None
    if not 0.0 <= a <= b <= hi:          # also refuses NaN
        raise ValueError(f"{name} must satisfy 0 <= LO <= HI <= {hi:g} (got {a} {b})")
    return a, b


@dataclass(frozen=True)
class DegradeSpec:
    """The random first-order degradation of `--degrade blind`: per training sample a Gaussian blur with sigma_y uniform in
    `blur_sigma` HR pixels and, with probability `blur_aniso_p`, an independent sigma_x (else sigma_x = sigma_y); noise
    `sqrt(sigma_n^2 + gain v) z` with sigma_n uniform in `noise_sigma` and gain uniform in `noise_gain` (image units, [0, 1]); for a
    colour image one draw for all channels with probability `gray_noise_p`; a 64-bit noise id.  Everything comes from the spec's OWN
    generator `random.Random(seed + rank)`: the global `random` state, which places the crops, never sees it."""
    blur_sigma: Tuple[float, float] = (0.2, 2.0)
    blur_aniso_p: float = 0.5
    noise_sigma: Tuple[float, float] = (0.0, 10.0 / 255.0)
    noise_gain: Tuple[float, float] = (0.0, 0.0)
    gray_noise_p: float = 0.4
    seed: int = 0

    def __post_init__(self):
        from .ops import BLUR_SIGMA_MAX
        object.__setattr__(self, "blur_sigma", _check_range("blur_sigma", self.blur_sigma, BLUR_SIGMA_MAX))
        object.__setattr__(self, "noise_sigma", _check_range("noise_sigma", self.noise_sigma, 1.0))
        object.__setattr__(self, "noise_gain", _check_range("noise_gain", self.noise_gain, 1.0))
        for name in ("blur_aniso_p", "gray_noise_p"):
            if not 0.0 <= float(getattr(self, name)) <= 1.0:
                raise ValueError(f"{name} must be a probability (got {getattr(self, name)!r})")

    def rng(self, rank: int = 0) -> random.Random:
        return random.Random(int(self.seed) + int(rank))

    def draw(self, rng: random.Random, colour: bool):
        """-> (blur, noise, noise_id, gray_noise) of one sample; always the same seven variates, whatever they decide."""
        sy, sx = rng.uniform(*self.blur_sigma), rng.uniform(*self.blur_sigma)
        aniso = rng.random() < self.blur_aniso_p
        noise = (rng.uniform(*self.noise_sigma), rng.uniform(*self.noise_gain))
        gray = rng.random() < self.gray_noise_p
        return (sy, sx if aniso else sy), noise, rng.getrandbits(64), gray or not colour

    def fixed(self) -> FixedDegrade:
        """The midpoints of the ranges: what validation scores, every epoch and every run."""
        mid = lambda r: 0.5 * (r[0] + r[1])          # noqa: E731
        return FixedDegrade((mid(self.blur_sigma),) * 2, (mid(self.noise_sigma), mid(self.noise_gain)), self.gray_noise_p >= 0.5)


@dataclass(frozen=True)
class JpegSpec:
    """The JPEG stage of `--jpeg_quality`: per training sample, with probability `p`, a round trip through baseline JPEG at
    a quality uniform in the integers `quality` = (lo, hi), 1 <= lo <= hi <= 100; otherwise the sample passes through (quality 0).
    `subsample`: chroma at 4:2:0 instead of 4:4:4.  The qualities come from the spec's OWN generator
    `random.Random(f"jpeg:{seed + rank}")`: neither the global `random` state nor a DegradeSpec's generator sees it."""
    quality: Tuple[int, int] = (30, 95)
    p: float = 1.0
    subsample: bool = False
    seed: int = 0

    def __post_init__(self):
        from .ops import check_jpeg_quality
        try:
            lo, hi = self.quality
        except (TypeError, ValueError):
            raise ValueError(f"jpeg quality must be two integers LO HI (got {self.quality!r})") from None
        lo, hi = check_jpeg_quality(lo, "quality LO"), check_jpeg_quality(hi, "quality HI")
        if lo > hi:
            raise ValueError(f"jpeg quality must satisfy 1 <= LO <= HI <= 100 (got {lo} {hi})")
        if not 0.0 <= float(self.p) <= 1.0:          # also refuses NaN
            raise ValueError(f"jpeg p must be a probability (got {self.p!r})")
        object.__setattr__(self, "quality", (lo, hi))
        object.__setattr__(self, "subsample", bool(self.subsample))

    def rng(self, rank: int = 0) -> random.Random:
        return random.Random(f"jpeg:{int(self.seed) + int(rank)}")

    def draw(self, rng: random.Random) -> int:
        """-> the quality of one sample, 0 = pass-through; always the same two variates, whatever they decide."""
        lo, hi = self.quality
        take, q = rng.random() < self.p, min(lo + int(rng.random() * (hi - lo + 1)), hi)
        return q if take else 0

    def fixed(self) -> int:
        """The middle of the range: what validation scores, every epoch and every run."""
        return round((self.quality[0] + self.quality[1]) / 2)


PSF_MODES = ("rotated", "mixed", "file")
TABLE_MODES = ("host", "device")          # where a pool's blur / sinc tables are evaluated
PSF_SIGMA_FLOOR = 1e-3          # a sigma of 0 (no blur on that axis) as a Gaussian: every tap off the axis underflows to 0


@dataclass(frozen=True)
class PsfSpec:
    """The 2-D blur of `--blur_kernel rotated|mixed` / `--blur_psf FILE`: per training sample one ks x ks table
    (blur_kernels) in place of the axis-aligned Gaussian.  It takes the (sigma_y, sigma_x) that `DegradeSpec.draw` produced -- as
    (s2, s1): at theta = 0 the table is the separable path's Gaussian -- and draws the rest from its OWN generator
    `random.Random(f"psf:{seed + rank}")`, six variates per sample whatever they decide.
    `rotated`: a Gaussian, theta uniform in [-pi/2, pi/2), ks = 2 min(ceil(3 max(s1, s2)), 10) + 1.
    `mixed`: Real-ESRGAN's six kinds {iso, aniso, generalized iso / aniso, plateau iso / aniso} with probabilities `kernel_prob`
    (iso: s2 = s1), beta uniform in `beta_g` / `beta_p`, an odd ks uniform in `ksize`.
    `file`: one table, uniformly, of the .npy `file` ([k][k] or [n][k][k]), a measured point-spread function."""
    mode: str = "rotated"
    kernel_prob: Tuple[float, ...] = (0.45, 0.25, 0.12, 0.03, 0.12, 0.03)
    beta_g: Tuple[float, float] = (0.5, 4.0)
    beta_p: Tuple[float, float] = (1.0, 2.0)
    ksize: Tuple[int, int] = (7, 21)
    file: Optional[str] = None
    seed: int = 0

    def __post_init__(self):
        from . import blur_kernels as bk
        if self.mode not in PSF_MODES:
            raise ValueError(f"psf mode must be one of {PSF_MODES} (got {self.mode!r})")
        try:
            prob = tuple(float(v) for v in self.kernel_prob)
        except (TypeError, ValueError):
            raise ValueError(f"kernel_prob must be six numbers (got {self.kernel_prob!r})") from None
        if len(prob) != 6 or not all(0.0 <= v <= 1.0 for v in prob) or abs(sum(prob) - 1.0) > 1e-6:
            raise ValueError(f"kernel_prob must be six probabilities that sum to 1 (got {self.kernel_prob!r})")
        object.__setattr__(self, "kernel_prob", prob)
        for name in ("beta_g", "beta_p"):
            try:
                lo, hi = (float(v) for v in getattr(self, name))
            except (TypeError, ValueError):
                raise ValueError(f"{name} must be two numbers LO HI (got {getattr(self, name)!r})") from None
            if not 0.0 < lo <= hi <= 16.0:          # also refuses NaN
                raise ValueError(f"{name} must satisfy 0 < LO <= HI <= 16 (got {lo} {hi})")
            object.__setattr__(self, name, (lo, hi))
        try:
            lo, hi = self.ksize
            lo, hi = bk.check_ks(lo), bk.check_ks(hi)
        except (TypeError, ValueError):
            raise ValueError(f"ksize must be two odd integers LO HI in 1..{bk.KS_MAX} (got {self.ksize!r})") from None
        if lo > hi:
            raise ValueError(f"ksize must satisfy LO <= HI (got {lo} {hi})")
        object.__setattr__(self, "ksize", (lo, hi))
        if (self.mode == "file") != (self.file is not None):
            raise ValueError("psf mode 'file' needs file=, and the other modes take none")
        object.__setattr__(self, "_tables", bk.load_psf_file(self.file) if self.file is not None else None)

    def rng(self, rank: int = 0) -> random.Random:
        return random.Random(f"psf:{int(self.seed) + int(rank)}")

    @property
    def tables(self):
        """The checked tables of `file`, fp32 [n][k][k] (None in the other modes)."""
        return self._tables

    def draw(self, rng: random.Random, blur, as_desc: bool = False):
        """-> the fp32 table of one sample with blur = (sigma_y, sigma_x); always the same six variates, whatever they decide.
        as_desc: the `blur_kernels.TableDesc` of that table instead (`file`: a kind-5 descriptor into `tables`), for
        `ops.kernel_tables` to build on the device; same variates, same decisions."""
        from . import blur_kernels as bk
        if as_desc:
            bk = bk.TableDesc
        u_kind, u_theta, u_bg, u_bp, u_ks, u_idx = (rng.random() for _ in range(6))
        if self.mode == "file":
            idx = min(int(u_idx * len(self._tables)), len(self._tables) - 1)
            return bk.bank(idx, self._tables.shape[1]) if as_desc else self._tables[idx]
        s2, s1 = (max(float(v), PSF_SIGMA_FLOOR) for v in blur)
        theta = math.pi * (u_theta - 0.5)
        if self.mode == "rotated":
            return bk.gaussian(2 * min(math.ceil(3.0 * max(0.0, *(float(v) for v in blur))), 10) + 1, s1, s2, theta)          # sigma 0: R = 0
        kind, acc = 5, 0.0
        for i, pr in enumerate(self.kernel_prob):
            acc += pr
            if u_kind < acc:
                kind = i
                break
        lo, hi = self.ksize
        n = (hi - lo) // 2 + 1
        ks = lo + 2 * min(int(u_ks * n), n - 1)
        if kind % 2 == 0:          # the isotropic kinds
            s2 = s1
        if kind < 2:
            return bk.gaussian(ks, s1, s2, theta)
        if kind < 4:
            return bk.generalized(ks, s1, s2, theta, self.beta_g[0] + u_bg * (self.beta_g[1] - self.beta_g[0]))
        return bk.plateau(ks, s1, s2, theta, self.beta_p[0] + u_bp * (self.beta_p[1] - self.beta_p[0]))

    def fixed(self):
        """Table 0 of `file` (what validation scores); None in the other modes: validation keeps the isotropic midpoints, for which a
        rotation is moot."""
        return self._tables[0] if self._tables is not None else None


def _check_prob3(name: str, p, what: str = "UP DOWN KEEP") -> Tuple[float, float, float]:
    try:
        prob = tuple(float(v) for v in p)
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be three numbers {what} (got {p!r})") from None
    if len(prob) != 3 or not all(0.0 <= v <= 1.0 for v in prob) or abs(sum(prob) - 1.0) > 1e-6:
        raise ValueError(f"{name} must be three probabilities {what} that sum to 1 (got {p!r})")
    return prob


def _check_factors(name: str, r) -> Tuple[float, float]:
    try:
        lo, hi = (float(v) for v in r)
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be two numbers LO HI (got {r!r})") from None
    if not 0.125 <= lo <= 1.0 <= hi <= 2.0:          # also refuses NaN; below 1/8 the resize has more than 33 taps
        raise ValueError(f"{name} must satisfy 0.125 <= LO <= 1 <= HI <= 2 (got {lo} {hi})")
    return lo, hi


@dataclass(frozen=True)
class UsmSpec:
    """The unsharp mask of `--gt_usm` (Real-ESRGAN's `gt_usm`; `ops.usm_sharpen`): `radius` 1..51 (ks = radius + 1 if it is even),
    `sigma` (<= 0: OpenCV's rule from ks), `weight` of the residual, `threshold` of the mask in 8-bit levels."""
    radius: int = 50
    sigma: float = 0.0
    weight: float = 0.5
    threshold: float = 10.0

    def __post_init__(self):
        from .ops import usm_ks
        usm_ks(self.radius)
        for name, lo, hi in (("sigma", -math.inf, 100.0), ("weight", 0.0, 10.0), ("threshold", 0.0, 255.0)):
            try:
                v = float(getattr(self, name))
            except (TypeError, ValueError):
                raise ValueError(f"usm {name} must be a number (got {getattr(self, name)!r})") from None
            if not (lo <= v <= hi) or (name == "sigma" and not math.isfinite(v)):          # also refuses NaN
                raise ValueError(f"usm {name} must be in [{lo}, {hi}] (got {v!r})")
            object.__setattr__(self, name, v)
        object.__setattr__(self, "radius", int(self.radius))

    @property
    def ks(self) -> int:
        from .ops import usm_ks
        return usm_ks(self.radius)

    def sharpen(self, x: torch.Tensor) -> torch.Tensor:
        from .ops import usm_sharpen
        return usm_sharpen(x, self.radius, self.sigma, self.weight, self.threshold)


SECOND_ORDER_VARIATES = 23          # per SecondOrderSpec.draw, whatever they decide


@dataclass(frozen=True)
class SecondOrderSpec:
    """The random second-order degradation of `--degrade second_order` (Real-ESRGAN's chain and defaults): what one
    `ops.SecondOrder` is drawn from, on top of the first-order draws that stage 1 reuses -- the blur table of the 7n pool (PsfSpec on
    DegradeSpec's sigmas) and DegradeSpec's noise, gray flag and noise id.
    Stage 1: with probability `sinc_p` the table is a sinc filter instead; a resize by a factor that goes up / down / stays with
    probabilities `resize_prob`, uniform in [1, HI] / [LO, 1] of `resize_range`; JPEG at a quality uniform in `jpeg_quality`.
    Stage 2: with probability `blur2_p` a filter -- a sinc with probability `sinc_p`, else a rotated anisotropic Gaussian with sigmas
    uniform in `blur2_sigma` -- else none (a table that would not fit the size it filters, R >= an extent, is dropped at any stage);
    `resize2_prob` / `resize2_range` relative to the LR size; noise uniform in `noise2_sigma` / `noise2_gain`, gray with `gray_noise_p`;
    JPEG at `jpeg2_quality`, before or after the final resize and filter with equal probability.
    Final: with probability `final_sinc_p` a sinc filter.  A sinc table has an odd side uniform in `ksize` and a cutoff uniform in
    [pi/3, pi] for sides below 13, else [pi/5, pi].
    Everything comes from the spec's OWN generator `random.Random(f"degrade2:{seed + rank}")`, 23 variates per draw whatever they
    decide: the global `random` state and the other specs' generators never see it.
    `resize_mode_prob` = the probabilities AREA BILINEAR BICUBIC of the rule of each of the three resizes (`ops.resize_ragged`;
    Real-ESRGAN draws among the three), from a generator of their own, `random.Random(f"degrade2mode:{seed + rank}")`, three variates
    per draw: the 23 variates above and their generator are the same whatever it holds.  The default (0, 0, 1) is the antialiased
    cubic at every resize."""
    resize_prob: Tuple[float, float, float] = (0.2, 0.7, 0.1)
    resize_range: Tuple[float, float] = (0.15, 1.5)
    resize2_prob: Tuple[float, float, float] = (0.3, 0.4, 0.3)
    resize2_range: Tuple[float, float] = (0.3, 1.2)
    blur2_p: float = 0.8
    blur2_sigma: Tuple[float, float] = (0.2, 1.5)
    sinc_p: float = 0.1
    final_sinc_p: float = 0.8
    ksize: Tuple[int, int] = (7, 21)
    noise2_sigma: Tuple[float, float] = (1.0 / 255.0, 25.0 / 255.0)
    noise2_gain: Tuple[float, float] = (0.0, 0.0)
    gray_noise_p: float = 0.4
    jpeg_quality: Tuple[int, int] = (30, 95)
    jpeg2_quality: Tuple[int, int] = (30, 95)
    seed: int = 0
    resize_mode_prob: Tuple[float, float, float] = (0.0, 0.0, 1.0)

    def __post_init__(self):
        from . import blur_kernels as bk
        from .ops import check_jpeg_quality
        object.__setattr__(self, "resize_mode_prob", _check_prob3("resize_mode_prob", self.resize_mode_prob, "AREA BILINEAR BICUBIC"))
        object.__setattr__(self, "resize_prob", _check_prob3("resize_prob", self.resize_prob))
        object.__setattr__(self, "resize2_prob", _check_prob3("resize2_prob", self.resize2_prob))
        object.__setattr__(self, "resize_range", _check_factors("resize_range", self.resize_range))
        object.__setattr__(self, "resize2_range", _check_factors("resize2_range", self.resize2_range))
        for name in ("blur2_p", "sinc_p", "final_sinc_p", "gray_noise_p"):
            if not 0.0 <= float(getattr(self, name)) <= 1.0:          # also refuses NaN
                raise ValueError(f"{name} must be a probability (got {getattr(self, name)!r})")
        lo, hi = _check_range("blur2_sigma", self.blur2_sigma, 10.0)
        if lo <= 0.0:
            raise ValueError(f"blur2_sigma must be > 0 (got {lo} {hi})")
        object.__setattr__(self, "blur2_sigma", (lo, hi))
        object.__setattr__(self, "noise2_sigma", _check_range("noise2_sigma", self.noise2_sigma, 1.0))
        object.__setattr__(self, "noise2_gain", _check_range("noise2_gain", self.noise2_gain, 1.0))
        try:
            lo, hi = self.ksize
            lo, hi = bk.check_ks(lo), bk.check_ks(hi)
        except (TypeError, ValueError):
            raise ValueError(f"ksize must be two odd integers LO HI in 1..{bk.KS_MAX} (got {self.ksize!r})") from None
        if lo > hi:
            raise ValueError(f"ksize must satisfy LO <= HI (got {lo} {hi})")
        object.__setattr__(self, "ksize", (lo, hi))
        for name in ("jpeg_quality", "jpeg2_quality"):
            try:
                lo, hi = getattr(self, name)
            except (TypeError, ValueError):
                raise ValueError(f"{name} must be two integers LO HI (got {getattr(self, name)!r})") from None
            lo, hi = check_jpeg_quality(lo, f"{name} LO"), check_jpeg_quality(hi, f"{name} HI")
            if lo > hi:
                raise ValueError(f"{name} must satisfy 1 <= LO <= HI <= 100 (got {lo} {hi})")
            object.__setattr__(self, name, (lo, hi))

    def rng(self, rank: int = 0) -> random.Random:
        return random.Random(f"degrade2:{int(self.seed) + int(rank)}")

    def mode_rng(self, rank: int = 0) -> random.Random:
        return random.Random(f"degrade2mode:{int(self.seed) + int(rank)}")

    def draw_modes(self, mode_rng: Optional[random.Random]) -> Tuple[int, int, int]:
        """The `ops.SecondOrder.modes` of one sample: three variates of `mode_rng`, whatever they decide; None = the cubic."""
        if mode_rng is None:
            return (0, 0, 0)
        pa, pb, _ = self.resize_mode_prob
        pb += pa
        u0, u1, u2 = mode_rng.random(), mode_rng.random(), mode_rng.random()
        return (2 if u0 < pa else (1 if u0 < pb else 0), 2 if u1 < pa else (1 if u1 < pb else 0), 2 if u2 < pa else (1 if u2 < pb else 0))

    def _ks(self, u: float) -> int:
        lo, hi = self.ksize
        n = (hi - lo) // 2 + 1
        return lo + 2 * min(int(u * n), n - 1)

    @staticmethod
    def _cutoff(ks: int, u: float) -> float:
        lo = math.pi / 3.0 if ks < 13 else math.pi / 5.0
        return lo + u * (math.pi - lo)

    @staticmethod
    def _factor(prob, rng_, u_kind: float, u: float) -> float:
        lo, hi = rng_
        if u_kind < prob[0]:
            return 1.0 + u * (hi - 1.0)
        if u_kind < prob[0] + prob[1]:
            return lo + u * (1.0 - lo)
        return 1.0

    @staticmethod
    def _quality(q, u: float) -> int:
        return min(q[0] + int(u * (q[1] - q[0] + 1)), q[1])

    def draw(self, rng: random.Random, table1, noise1, noise_id: int, gray1: bool, colour: bool, extent: int, scale: int,
             as_desc: bool = False, mode_rng: Optional[random.Random] = None):
        """-> the `ops.SecondOrder` of one sample (as_desc: with `blur_kernels.TableDesc` descriptors for k1 / k2 / k3 -- table1 is then
        one too -- from the same variates and decisions).  table1, noise1, noise_id, gray1: the first-order draws (PsfSpec.draw or a Gaussian
        of DegradeSpec's sigmas; DegradeSpec.draw).  extent: the side of the square window the chain runs on at factor `scale`: it
        bounds filter 2, and factor 2 is raised where the second resize would shrink by more than the resampler's 8x (an upscale by
        1.5 followed by 0.3 / 4 is 20x; Real-ESRGAN's resize has no such limit because it does not antialias).  mode_rng: the
        generator of `mode_rng()`, which `draw_modes` reads; None leaves every resize the cubic."""
        from . import blur_kernels as bk
        from .ops import SecondOrder
        if as_desc:
            bk = bk.TableDesc
        u = [rng.random() for _ in range(SECOND_ORDER_VARIATES)]
        ks1 = self._ks(u[2])
        k1 = bk.sinc(self._cutoff(ks1, u[1]), ks1) if (u[0] < self.sinc_p and ks1 // 2 < extent) else table1
        r1 = self._factor(self.resize_prob, self.resize_range, u[3], u[4])
        ks2 = self._ks(u[9])
        if u[6] >= self.blur2_p or ks2 // 2 >= max(1, int(extent * r1 + 0.5)):
            k2 = bk.delta()
        elif u[7] < self.sinc_p:
            k2 = bk.sinc(self._cutoff(ks2, u[8]), ks2)
        else:
            lo, hi = self.blur2_sigma
            k2 = bk.gaussian(ks2, lo + u[10] * (hi - lo), lo + u[11] * (hi - lo), math.pi * (u[12] - 0.5))
        r2 = self._factor(self.resize2_prob, self.resize2_range, u[13], u[14])
        h1 = max(1, int(extent * r1 + 0.5))
        r2 = max(r2, (-(-h1 // 8) * int(scale) + 1e-6) / extent)
        noise2 = (self.noise2_sigma[0] + u[15] * (self.noise2_sigma[1] - self.noise2_sigma[0]),
                  self.noise2_gain[0] + u[16] * (self.noise2_gain[1] - self.noise2_gain[0]))
        ks3 = self._ks(u[22])
        k3 = bk.sinc(self._cutoff(ks3, u[21]), ks3) if (u[20] < self.final_sinc_p and ks3 // 2 < extent // int(scale)) else bk.delta()
        return SecondOrder(k1, r1, tuple(noise1), bool(gray1), self._quality(self.jpeg_quality, u[5]), k2, r2, noise2,
                           u[17] < self.gray_noise_p or not colour, self._quality(self.jpeg2_quality, u[18]), u[19] < 0.5, k3, int(noise_id),
                           self.draw_modes(mode_rng))

    def fixed(self, table1, noise1, gray1: bool = False, noise_id: int = 0):
        """What validation scores, every epoch and every run: no sinc at stages 1 and 2 (sinc_p < 0.5, else a sinc at the middle
        cutoff of a 13-tap table), the middle of the DOWN range at both resizes, an isotropic Gaussian at the middle `blur2_sigma`
        when blur2_p >= 0.5, the middle noise and qualities, order A (JPEG before the final resize), and when final_sinc_p >= 0.5 a
        13-tap final sinc at the middle of its cutoff range.  table1 / noise1 / gray1: the fixed first-order stage (FixedDegrade)."""
        from . import blur_kernels as bk
        from .ops import SecondOrder
        mid = lambda r: 0.5 * (r[0] + r[1])          # noqa: E731
        sinc13 = bk.sinc(self._cutoff(13, 0.5), 13)
        k2 = bk.delta() if self.blur2_p < 0.5 else (sinc13 if self.sinc_p >= 0.5 else bk.gaussian(13, mid(self.blur2_sigma), mid(self.blur2_sigma)))
        return SecondOrder(sinc13 if self.sinc_p >= 0.5 else table1, 0.5 * (self.resize_range[0] + 1.0), tuple(noise1), bool(gray1),
                           round(mid(self.jpeg_quality)), k2, 0.5 * (self.resize2_range[0] + 1.0),
                           (mid(self.noise2_sigma), mid(self.noise2_gain)), self.gray_noise_p >= 0.5, round(mid(self.jpeg2_quality)), False,
                           sinc13 if self.final_sinc_p >= 0.5 else bk.delta(), int(noise_id))


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
        if augment not in AUGMENT_MODES:
            raise ValueError(f"augment must be one of {AUGMENT_MODES} (got {augment!r})")
        if quant_bits not in (0, 8):
            raise ValueError(f"quant_bits must be 0 or 8 (got {quant_bits!r})")
        if not 2 <= int(scale) <= 4:
            raise ValueError(f"DeviceHRPool degrades by an integer factor in 2..4 (got {scale!r})")
        if degrade is not None and not isinstance(degrade, DegradeSpec):
            raise ValueError(f"degrade must be a DegradeSpec or None (got {type(degrade).__name__})")
        self.augment, self.quant_bits = augment, int(quant_bits)
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
        self.lr_patch, self.scale, self.device = int(lr_patch), int(scale), torch.device(device)
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
        P, s = self.lr_patch, self.scale
        hd, codes = [], []
        for i in indices:
            _, (ho, hh, hw, hc) = self.meta[int(i)]
            top, left = random.randint(0, hh // s - P), random.randint(0, hw // s - P)
            hd.append((ho, hh, hw, hc, top * s, left * s))
            codes.append(draw_op(self.augment))
        return hd, codes

    def draw_degrade(self, hd):
        """The ten-slot descriptors of a batch: `draw`'s six plus the packed parameters of one `DegradeSpec.draw` per sample, from the
        spec's generator alone (the global `random` state is not touched)."""
        from .ops import pack_degrade_params
        return [tuple(d) + tuple(pack_degrade_params(*self.degrade.draw(self._degrade_rng, colour=(d[3] & 0xff) == 3))) for d in hd]

    def draw_psf(self, hd):
        """(ten-slot descriptors, fp32 numpy [B][ks][ks], ks) of a batch: `draw_degrade`'s draws, in its order, plus one `PsfSpec.draw`
        per sample on the sigmas of that sample; slot 6 keeps the sigmas, which the PSF entry ignores.  With tables = "device":
        (descriptors, the batch's `ops.DeviceTables`, ks), built by one `ops.kernel_tables` launch."""
        from .ops import kernel_tables, pack_degrade_params, pack_psf
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
        from ._lib import check, lib
        P, s = self.lr_patch, self.scale
        pool = self._batch_pool(indices)
        hd, codes = self.draw(indices)
        B = len(hd)
        tabs = None
        if self.psf is not None:
            rows, tabs, ks = self.draw_psf(hd)
        else:
            rows = hd if self.degrade is None else self.draw_degrade(hd)
        desc = torch.tensor(rows, dtype=torch.int64).to(self.device)
        lr = torch.empty(B, 3, P, P, dtype=torch.float32, device=self.device)
        hr = torch.empty(B, 3, P * s, P * s, dtype=torch.float32, device=self.device)
        st = torch.cuda.current_stream(self.device).cuda_stream
        if tabs is not None:
            k = tabs.tab if self.tables == "device" else self._psf_upload(tabs)
            check(lib().srk_crop_degrade_psf_u8(pool.data_ptr(), desc.data_ptr(), k.data_ptr(), ks, lr.data_ptr(),
                                                hr.data_ptr(), B, P, s, self.quant_bits, st))
        else:
            entry = lib().srk_crop_degrade_u8 if self.degrade is None else lib().srk_crop_degrade_blind_u8
            check(entry(pool.data_ptr(), desc.data_ptr(), lr.data_ptr(), hr.data_ptr(), B, P, s, self.quant_bits, st))
        if self.jpeg is not None:
            from .ops import jpeg_roundtrip
            lr = jpeg_roundtrip(lr, [self.jpeg.draw(self._jpeg_rng) for _ in range(B)], self.jpeg.subsample)
        if any(codes):
            from .augment import dihedral
            ops = torch.tensor(codes, dtype=torch.int32).to(self.device)
            lr, hr = dihedral(lr, ops), dihedral(hr, ops)
        return lr, hr


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
        from ._lib import check, lib
        desc = torch.tensor(rows, dtype=torch.int64).to(self.device)
        out = torch.empty(len(rows), 3, patch, patch, dtype=torch.float32, device=self.device)
        check(lib().srk_crop_u8(pool.data_ptr(), desc.data_ptr(), out.data_ptr(), len(rows), patch, torch.cuda.current_stream(self.device).cuda_stream))
        return out

    def sample(self, indices):
        """-> (lr [B,3,P,P], hr [B,3,P*s,P*s]) fp32 on the device."""
        from .ops import degrade_second_order
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
        if any(codes):
            from .augment import dihedral
            ops = torch.tensor(codes, dtype=torch.int32).to(self.device)
            lr, hr = dihedral(lr, ops), dihedral(hr, ops)
        return lr, hr


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
            from .ops import check_jpeg_quality
            jpeg = check_jpeg_quality(jpeg)
            if self.quant_bits != 8:
                raise ValueError(f"jpeg= codes 8-bit LR images: it needs quant_bits 8 (got {quant_bits!r})")
        self.jpeg, self.jpeg_subsample = jpeg, bool(jpeg_subsample)
        self.degrade = degrade.fixed() if isinstance(degrade, DegradeSpec) else degrade
        if self.degrade is not None:
            from .ops import pack_degrade_params
            pack_degrade_params(self.degrade.blur, self.degrade.noise, 0, self.degrade.gray_noise)          # the ranges, before any batch

    def __len__(self):
        return len(self.loader)

    def __iter__(self):
        from .ops import jpeg_roundtrip
        for lr, hr in self._degraded():
            yield (lr if self.jpeg is None else jpeg_roundtrip(lr, self.jpeg, self.jpeg_subsample)), hr

    def _degraded(self):
        from .ops import degrade_aa, degrade_blind, degrade_psf
        first = 0
        for hr in self.loader:
            hr = hr.to(self.device, dtype=torch.float32)
            if self.degrade is None:
                yield degrade_aa(hr, self.scale, self.quant_bits)
                continue
            B = hr.shape[0]
            gray = [True] * B
            if hr.shape[1] == 3 and not self.degrade.gray_noise:
                gray = ((hr[:, 0] == hr[:, 1]) & (hr[:, 0] == hr[:, 2])).flatten(1).all(dim=1).tolist()
            if self.second_order is not None:
                from .ops import degrade_second_order
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
class FixedRestore(NamedTuple):
    """One fixed scale-1 degradation (validation, evaluation): the noise sigma in image units (0..1), the JPEG quality (0 = no JPEG
    stage), gray_noise = one draw for the three channels of a colour image, subsample = chroma at 4:2:0."""
    sigma: float
    jpeg_quality: int = 0
    gray_noise: bool = False
    subsample: bool = False


@dataclass(frozen=True)
class RestoreSpec:
    """The random degradation of `--task dn | car`: per training sample Gaussian noise with sigma uniform in `sigma`
    (image units, 0..1) and, with `jpeg_quality` = (lo, hi), a round trip through baseline JPEG at a quality uniform in the integers
    lo..hi (None = no JPEG stage); for a colour image one noise draw for all channels with probability `gray_noise_p`; `subsample`:
    chroma at 4:2:0; a 64-bit noise id.  Everything comes from the spec's OWN generator `random.Random(f"restore:{seed + rank}")`:
    neither the global `random` state, which places the crops, nor a DegradeSpec's or JpegSpec's generator sees it."""
    sigma: Tuple[float, float] = (0.0, 0.0)
    jpeg_quality: Optional[Tuple[int, int]] = None
    gray_noise_p: float = 0.0
    subsample: bool = False
    seed: int = 0

    def __post_init__(self):
        from .ops import check_jpeg_quality
        object.__setattr__(self, "sigma", _check_range("sigma", self.sigma, 1.0))
        if self.jpeg_quality is not None:
            try:
                lo, hi = self.jpeg_quality
            except (TypeError, ValueError):
                raise ValueError(f"jpeg quality must be two integers LO HI or None (got {self.jpeg_quality!r})") from None
            lo, hi = check_jpeg_quality(lo, "quality LO"), check_jpeg_quality(hi, "quality HI")
            if lo > hi:
                raise ValueError(f"jpeg quality must satisfy 1 <= LO <= HI <= 100 (got {lo} {hi})")
            object.__setattr__(self, "jpeg_quality", (lo, hi))
        if not 0.0 <= float(self.gray_noise_p) <= 1.0:          # also refuses NaN
            raise ValueError(f"gray_noise_p must be a probability (got {self.gray_noise_p!r})")
        object.__setattr__(self, "subsample", bool(self.subsample))

    def rng(self, rank: int = 0) -> random.Random:
        return random.Random(f"restore:{int(self.seed) + int(rank)}")

    def draw(self, rng: random.Random, colour: bool):
        """-> (sigma, quality, noise_id, gray_noise) of one sample, quality 0 = no JPEG stage; always the same four variates, whatever
        they decide."""
        sigma, u_q = rng.uniform(*self.sigma), rng.random()
        gray = rng.random() < self.gray_noise_p
        q = 0
        if self.jpeg_quality is not None:
            lo, hi = self.jpeg_quality
            q = min(lo + int(u_q * (hi - lo + 1)), hi)
        return sigma, q, rng.getrandbits(64), gray or not colour

    def fixed(self) -> FixedRestore:
        """The midpoint sigma and the middle quality: what validation scores, every epoch and every run."""
        q = 0 if self.jpeg_quality is None else round((self.jpeg_quality[0] + self.jpeg_quality[1]) / 2)
        return FixedRestore(0.5 * (self.sigma[0] + self.sigma[1]), q, self.gray_noise_p >= 0.5, self.subsample)


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
        if augment not in AUGMENT_MODES:
            raise ValueError(f"augment must be one of {AUGMENT_MODES} (got {augment!r})")
        if quant_bits not in (0, 8):
            raise ValueError(f"quant_bits must be 0 or 8 (got {quant_bits!r})")
        if out_chans not in (1, 3):
            raise ValueError(f"out_chans must be 1 or 3 (got {out_chans!r})")
        if not isinstance(spec, RestoreSpec):
            raise ValueError(f"spec must be a RestoreSpec (got {type(spec).__name__})")
        if not 1 <= int(patch) <= 2048:
            raise ValueError(f"patch must be in 1..2048 (got {patch!r})")
        self.augment, self.quant_bits, self.out_chans = augment, int(quant_bits), int(out_chans)
        self.spec, self._spec_rng = spec, spec.rng(rank)
        self.patch, self.device = int(patch), torch.device(device)
        self._pack(((img,) for img in images), shard_bytes)

    def _check_group(self, img) -> None:
        _, h, w, _ = img
        if h < self.patch or w < self.patch:
            raise ValueError(f"image ({h},{w}) too small for patch {self.patch}")

    def draw(self, indices):
        """-> (descriptors, D4 codes) of a batch; advances the global `random` state exactly as DevicePairPool.sample does."""
        P = self.patch
        hd, codes = [], []
        for i in indices:
            _, (o, h, w, c) = self.meta[int(i)]
            top, left = random.randint(0, h - P), random.randint(0, w - P)
            hd.append((o, h, w, c, top, left))
            codes.append(draw_op(self.augment))
        return hd, codes

    def draw_restore(self, hd):
        """The ten-slot descriptors of a batch: `draw`'s six plus the packed parameters of one `RestoreSpec.draw` per sample, from the
        spec's generator alone (the global `random` state is not touched)."""
        from .ops import pack_restore_params
        rows = []
        for d in hd:
            sigma, q, nid, gray = self.spec.draw(self._spec_rng, colour=(d[3] & 0xff) == 3 and self.out_chans == 3)
            rows.append(tuple(d) + tuple(pack_restore_params(q, (sigma, 0.0), nid, gray)))
        return rows

    def sample(self, indices):
        """-> (degraded [B,out_chans,P,P], clean [B,out_chans,P,P]) fp32 on the device: one descriptor upload, one launch."""
        from ._lib import check, lib
        P, Co = self.patch, self.out_chans
        pool = self._batch_pool(indices)
        hd, codes = self.draw(indices)
        B = len(hd)
        desc = torch.tensor(self.draw_restore(hd), dtype=torch.int64).to(self.device)
        clean = torch.empty(B, Co, P, P, dtype=torch.float32, device=self.device)
        degraded = torch.empty(B, Co, P, P, dtype=torch.float32, device=self.device)
        st = torch.cuda.current_stream(self.device).cuda_stream
        check(lib().srk_crop_restore_u8(pool.data_ptr(), desc.data_ptr(), clean.data_ptr(), degraded.data_ptr(), B, P, Co,
                                        int(self.spec.subsample), self.quant_bits, st))
        if any(codes):
            from .augment import dihedral
            ops = torch.tensor(codes, dtype=torch.int32).to(self.device)
            degraded, clean = dihedral(degraded, ops), dihedral(clean, ops)
        return degraded, clean


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
        if quant_bits not in (0, 8):
            raise ValueError(f"quant_bits must be 0 or 8 (got {quant_bits!r})")
        fx = spec_or_fixed.fixed() if isinstance(spec_or_fixed, RestoreSpec) else spec_or_fixed
        if not isinstance(fx, FixedRestore):
            raise ValueError(f"spec_or_fixed must be a RestoreSpec or a FixedRestore (got {type(spec_or_fixed).__name__})")
        from .ops import pack_restore_params
        pack_restore_params(fx.jpeg_quality, (fx.sigma, 0.0), 0, fx.gray_noise)          # the ranges, before any batch
        self.loader, self.out_chans, self.fixed, self.quant_bits, self.device = loader, int(out_chans), fx, int(quant_bits), torch.device(device)

    def __len__(self):
        return len(self.loader)

    def __iter__(self):
        from .ops import restore_degrade
        fx, first = self.fixed, 0
        for clean in self.loader:
            clean = clean.to(self.device, dtype=torch.float32).contiguous()
            if clean.dim() != 4 or clean.shape[1] != self.out_chans:
                raise ValueError(f"RestoreBatches(out_chans={self.out_chans}) got a batch of shape {tuple(clean.shape)}")
            B = clean.shape[0]
            gray = [True] * B
            if self.out_chans == 3 and not fx.gray_noise:
                gray = ((clean[:, 0] == clean[:, 1]) & (clean[:, 0] == clean[:, 2])).flatten(1).all(dim=1).tolist()
            yield restore_degrade(clean, (fx.sigma, 0.0), range(first, first + B), gray, fx.jpeg_quality, fx.subsample, self.quant_bits), clean
            first += B


def clean_to_tensor(img, out_chans: int) -> torch.Tensor:
    """A clean PIL image as the fp32 [out_chans,H,W] tensor in [0, 1] that DeviceRestorePool cuts its targets from: three channels as
    `hr_to_tensor3`; one channel = the stored gray samples, or the integer luma (ops.to_gray) of an RGB image, over 255 / 65535."""
    if out_chans == 3:
        return hr_to_tensor3(img)
    from .ops import to_gray
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
