"""The image-processing ops of the on-device data path: resizes, blurs and filters, noise, JPEG, unsharp mask, and the degradations
composed of them, and the conversion between decoded image files and fp32 batches (7v).  Thin torch wrappers over
libsrk.so like ops.py, which re-exports every public name here: `ops.<name>` stays the public spelling.

One shape for every op: `_batch` tests the tensor, one helper tests each further argument (`_quant_bits`, `_factor_crop`, `_padded_out`,
`_ids_and_grays`, `_qualities`, `_ragged`), the small tables go up in one `torch.tensor(...).to(device)` each, and ONE `check(lib()...)`
launches.  Nothing is read back from the device.
"""
from __future__ import annotations

import numbers
import struct
from typing import NamedTuple, Optional, Tuple

import numpy as np
import torch

from . import blur_kernels as bk
from ._lib import SrkUnsupported, _p, _stream, check, lib

__all__ = ["resize_aa", "degrade_aa", "BLUR_SIGMA_MAX", "pack_degrade_params", "degrade_blind", "pack_psf", "DeviceTables", "kernel_tables", "blur2d",
           "degrade_psf", "check_jpeg_quality", "jpeg_roundtrip", "pack_restore_params", "noise", "restore_degrade", "RaggedExt",
           "pack_filter_tables", "filter2d", "resize_aa_ragged", "RESIZE_MODES", "resize_ragged", "usm_ks", "usm_taps", "usm_sharpen",
           "jpeg_roundtrip_ragged", "SecondOrder", "second_order_sizes", "second_order_noise_ids", "degrade_second_order", "LUMA_COEF", "to_gray",
           "image_unpack", "image_pack"]


# ---- the argument checks every op shares ---------------------------------------------------------------------------------------------
def _batch(x: torch.Tensor, what: str, *, cuda: bool = True, fp32: bool = True, chans=None, nonempty: bool = False):
    """The one test of a batch argument -> its (B, C, H, W): a [B,C,H,W] tensor, on a CUDA device (cuda=False leaves that to `_p`, which
    raises RuntimeError), fp32 (fp32=False: the op converts), C in `chans`, no extent of 0 (nonempty)."""
    if x.dim() != 4 or (cuda and not x.is_cuda) or (fp32 and x.dtype != torch.float32) or (nonempty and min(x.shape) < 1) or \
            (chans is not None and x.shape[1] not in chans):
        kind = ("non-empty " if nonempty else "") + ("CUDA " if cuda else "") + ("fp32 " if fp32 else "")
        raise ValueError(f"{what} takes a {kind}[B,C,H,W] batch{' with C 1 or 3' if chans else ''} (got {x.dtype} {tuple(x.shape)} on {x.device})")
    return x.shape


def _quant_bits(v, what: str) -> int:
    if v not in (0, 8):
        raise ValueError(f"{what}: quant_bits must be 0 or 8 (got {v!r})")
    return int(v)


def _factor_crop(hr: torch.Tensor, scale, what: str, checked: bool = True):
    """-> (hr cropped to its top-left (H - H % s, W - W % s) region, fp32 and contiguous; s).  checked: a non-empty CUDA [B,C,H,W] batch of
    at least one output pixel and a factor in 2..4 (`degrade_aa` leaves the tests to `resize_aa`)."""
    s = int(scale)
    if checked:
        B, Cc, H, W = _batch(hr, what, fp32=False, nonempty=True)
        if not 2 <= s <= 4:
            raise ValueError(f"{what}: the factor must be in 2..4 (got {scale!r})")
        if H < s or W < s:
            raise ValueError(f"{what}: {tuple(hr.shape)} is smaller than one output pixel at factor {s}")
    H, W = hr.shape[-2:]
    return hr[..., :H - H % s, :W - W % s].float().contiguous(), s


def _padded_out(out: Optional[torch.Tensor], shape, like: torch.Tensor) -> torch.Tensor:
    if out is None:
        return torch.empty(shape, dtype=torch.float32, device=like.device)
    if tuple(out.shape) != tuple(shape) or out.dtype != torch.float32 or out.device != like.device or not out.is_contiguous():
        raise ValueError(f"out must be contiguous fp32 {tuple(shape)} on {like.device} (got {out.dtype} {tuple(out.shape)} on {out.device})")
    return out


def _per_sample(v, B: int, width: int, what: str):
    rows = [list(r) for r in v] if (len(v) and hasattr(v[0], "__len__")) else [list(v)] * B
    if len(rows) != B or any(len(r) != width for r in rows):
        raise ValueError(f"{what} must be {width} numbers or one such row per sample (B={B}; got {v!r})")
    return rows


def _ids_and_grays(noise_ids, gray_noise, B: int, what: str):
    ids = [int(v) for v in noise_ids]
    grays = [bool(gray_noise)] * B if isinstance(gray_noise, (bool, int)) else [bool(v) for v in gray_noise]
    if len(ids) != B or len(grays) != B:
        raise ValueError(f"{what}: one noise id and one gray flag per sample (B={B}; got {len(ids)} ids, {len(grays)} flags)")
    return ids, grays


def check_jpeg_quality(q, what: str = "quality") -> int:
    """A JPEG quality as an int in 1..100 (bools, floats with a fraction and anything else raise ValueError)."""
    if isinstance(q, bool) or not isinstance(q, numbers.Real) or q != q or int(q) != q or not 1 <= int(q) <= 100:          # q != q: NaN
        raise ValueError(f"jpeg {what} must be an integer in 1..100 (got {q!r})")
    return int(q)


def _quality(q) -> int:
    """One quality of a batch: 0 = that sample passes through, else 1..100."""
    return 0 if (not isinstance(q, bool) and q == 0) else check_jpeg_quality(q)


def _qualities(quality, B: int, what: str):
    qs = [quality] * B if isinstance(quality, numbers.Real) else list(quality)
    if len(qs) != B:
        raise ValueError(f"{what}: one quality or one per sample (B={B}; got {len(qs)})")
    return [_quality(q) for q in qs]


# ---- resize and the first-order degradations (csrc/resize.hip, csrc/degrade.hip) -----------------------------------------------------
def resize_aa(x: torch.Tensor, size, quant_bits: int = 0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Antialiased bicubic resize of a CUDA fp32 batch x [B,C,H,W] to size = (Ho, Wo), up or down (csrc/resize.hip,
    srk_resize_aa_f32): the Keys cubic with a = -0.5 in the convention of PIL's Image.BICUBIC and of
    F.interpolate(mode='bicubic', antialias=True, align_corners=False) -- fp64 weights rounded once to fp32, border taps dropped and
    renormalised, horizontal pass first.  quant_bits 8 rounds the result to k / 255 (what an 8-bit file of it would decode to);
    0 keeps the filtered values.  `out` must not alias `x`; it is allocated when absent.  One launch, no host read: capturable.
    An axis shrinking by more than 8x raises SrkUnsupported."""
    B, Cc, H, W = _batch(x, "resize_aa", cuda=False, nonempty=True)
    try:
        Ho, Wo = (int(v) for v in size)
    except (TypeError, ValueError):
        raise ValueError(f"resize_aa: size must be (Ho, Wo) (got {size!r})") from None
    if Ho < 1 or Wo < 1:
        raise ValueError(f"resize_aa: every extent must be >= 1 (got {tuple(x.shape)} -> {(Ho, Wo)})")
    q = _quant_bits(quant_bits, "resize_aa")
    if out is not None and not out.is_contiguous():          # `_p` has the same word for it
        raise RuntimeError("libsrk needs contiguous tensors")
    out = _padded_out(out, (B, Cc, Ho, Wo), x)
    check(lib().srk_resize_aa_f32(_p(x), _p(out), B, Cc, H, W, Ho, Wo, q, _stream()))
    return out


def degrade_aa(hr: torch.Tensor, scale: int, quant_bits: int = 8) -> Tuple[torch.Tensor, torch.Tensor]:
    """(lr, hr_cropped) of `--synth_lr` validation / evaluation: hr [B,C,H,W] cropped to its top-left (H - H % s, W - W % s) region and
    that region's (H // s, W // s) antialiased bicubic downscale -- what DeviceHRPool's training patches are windows of."""
    hr, s = _factor_crop(hr, scale, "degrade_aa", checked=False)
    return resize_aa(hr, (hr.shape[-2] // s, hr.shape[-1] // s), quant_bits), hr


BLUR_SIGMA_MAX = 2.5          # R = ceil(3 sigma) <= 8 taps on either side: what the 33-tap rows of csrc/resize.h hold at factors 2..4


def _f32_bits(v: float) -> int:
    return struct.unpack("<I", struct.pack("<f", v))[0]


def pack_degrade_params(blur, noise, noise_id: int, gray_noise: bool):
    """Slots 6..9 of a `srk_crop_degrade_blind_u8` descriptor / one row of `srk_degrade_blind_f32`'s table, as four signed 64-bit
    integers: fp32 bits of (sigma_y | sigma_x << 32), of (sigma_n | gain << 32), the noise id, the flags (bit 0 = gray noise).
    The one place that packs them; the ranges are checked here: sigmas in [0, 2.5] HR pixels, sigma_n and gain in [0, 1]."""
    (sy, sx), (sn, gain) = (float(v) for v in blur), (float(v) for v in noise)
    if not (0.0 <= sy <= BLUR_SIGMA_MAX and 0.0 <= sx <= BLUR_SIGMA_MAX):          # also refuses NaN
        raise ValueError(f"blur sigmas must be in [0, {BLUR_SIGMA_MAX}] HR pixels (got {(sy, sx)})")
    if not (0.0 <= sn <= 1.0 and 0.0 <= gain <= 1.0):
        raise ValueError(f"noise sigma and gain must be in [0, 1] (got {(sn, gain)})")
    noise_id = int(noise_id)
    if not -(1 << 63) <= noise_id < (1 << 64):
        raise ValueError(f"noise id must fit 64 bits (got {noise_id})")
    signed = lambda v: v - (1 << 64) if v >> 63 else v          # noqa: E731
    return [signed(_f32_bits(sy) | _f32_bits(sx) << 32), signed(_f32_bits(sn) | _f32_bits(gain) << 32),
            signed(noise_id & 0xFFFFFFFFFFFFFFFF), int(bool(gray_noise))]


def degrade_blind(hr: torch.Tensor, scale: int, blur, noise, noise_ids, gray_noise=False, quant_bits: int = 8) -> Tuple[torch.Tensor, torch.Tensor]:
    """(lr, hr_cropped) like `degrade_aa`, with a Gaussian blur (sigma_y, sigma_x) in HR pixels composed into the bicubic tables and
    noise `v + sqrt(sigma_n^2 + gain max(v, 0)) z` added before the rounding (csrc/degrade.hip, srk_degrade_blind_f32): what
    DeviceHRPool's blind training patches are windows of.  blur = (sigma_y, sigma_x) and noise = (sigma_n, gain): one pair or one per
    sample; noise_ids: B integers (the Philox key; the same id and coordinates give the same draw); gray_noise: a bool or B of them --
    one draw for all channels (always so for C == 1).  hr [B,C,H,W] is cropped to a multiple of the factor (2..4).  One launch after one
    small upload; sigmas and amplitudes out of range raise ValueError."""
    hr, s = _factor_crop(hr, scale, "degrade_blind")
    q = _quant_bits(quant_bits, "degrade_blind")
    B, Cc, H, W = hr.shape
    ids, grays = _ids_and_grays(noise_ids, gray_noise, B, "degrade_blind")
    rows = [pack_degrade_params(b, n, i, g) for b, n, i, g in
            zip(_per_sample(blur, B, 2, "degrade_blind: blur"), _per_sample(noise, B, 2, "degrade_blind: noise"), ids, grays)]
    par = torch.tensor(rows, dtype=torch.int64).to(hr.device)
    lr = torch.empty(B, Cc, H // s, W // s, dtype=torch.float32, device=hr.device)
    check(lib().srk_degrade_blind_f32(_p(hr), _p(lr), _p(par), B, Cc, H, W, s, q, _stream()))
    return lr, hr


# ---- 2-D tables: the host rule, the device builder, the blur (csrc/blur2d.hip, csrc/tables.hip) --------------------------------------
def _pack_tables(tab, B: int, rule, label: str, what: str):
    """tab: ONE 2-D numpy table for every sample, or a sequence of B tables of any odd sizes -> (fp32 numpy [B][ks][ks], ks, the B sizes
    before padding): each table checked by `rule` (blur_kernels.check_table / check_filter_table) and zero-padded, centred, to the
    largest ks -- which changes no bit of the result (include/srk.h "General 2-D blur")."""
    if isinstance(tab, np.ndarray) and tab.ndim == 2:
        tabs = [rule(tab)] * B
    else:
        tabs = [rule(t, f"{label}[{i}]") for i, t in enumerate(tab)]
    if len(tabs) != B:
        raise ValueError(f"{what}: one table or one per sample (B={B}; got {len(tabs)})")
    ks = max(t.shape[0] for t in tabs)
    return np.stack([bk.pad_to(t, ks) for t in tabs]), ks, [t.shape[0] for t in tabs]


def pack_psf(psf, B: int, checked: bool = False):
    """psf: one [ks][ks] table or B of them (a list of tables of different odd sizes, or an array [B][ks][ks]) -> (fp32 numpy
    [B][ks][ks], ks) by blur_kernels.check_table's rule (`_pack_tables`).  checked: a list of fp32 tables that blur_kernels made or
    checked already (sr_datasets.PsfSpec's draws) is only padded."""
    if checked:
        ks = max(t.shape[0] for t in psf)
        out = np.zeros((len(psf), ks, ks), dtype=np.float32)
        for i, t in enumerate(psf):
            p = (ks - t.shape[0]) // 2
            out[i, p:p + t.shape[0], p:p + t.shape[0]] = t
        if len(psf) != B:
            raise ValueError(f"psf: one table per sample (B={B}; got {len(psf)})")
        return out, ks
    if isinstance(psf, torch.Tensor):
        psf = psf.detach().cpu().numpy()
    try:
        psf = np.asarray(psf, dtype=np.float32)
    except (ValueError, TypeError):          # tables of different sizes
        pass
    return _pack_tables(psf, B, bk.check_table, "psf", "psf")[:2]


def pack_filter_tables(tab, B: int):
    """tab: one [ks][ks] table or B of them (mixed odd sizes allowed) -> (fp32 numpy [B][ks][ks], ks, the B sizes before padding), each
    checked by blur_kernels.check_filter_table -- finite, sum within 1e-3 of 1, any sign (`_pack_tables`)."""
    if isinstance(tab, torch.Tensor):
        tab = tab.detach().cpu().numpy()
    return _pack_tables(tab, B, bk.check_filter_table, "table", "filter tables")


class DeviceTables(NamedTuple):
    """Tables the device built (`kernel_tables`): `tab`, CUDA fp32 [n][ks][ks]; `ks`; `own`, the host list of the n sides before
    padding (what the radius-versus-extent checks run on: nothing is read back); `signed`: a sinc table is among them, so the batch
    goes through `filter2d` only."""
    tab: torch.Tensor
    ks: int
    own: Tuple[int, ...]
    signed: bool


def kernel_tables(descs, ks=None, bank=None, signed: bool = True, device=None) -> DeviceTables:
    """The tables of n `blur_kernels.TableDesc` built ON THE DEVICE (csrc/tables.hip, srk_kernel_tables_f32): one upload of n x 8
    doubles and one launch, in place of n fp64 numpy evaluations and an upload of n ks^2 floats.  ks: the side of the slots, by default
    the largest own side (smaller tables are centred in +0, `blur_kernels.pad_to`).  bank: the CUDA fp32 [n_bank][kb][kb] tables that
    kind-5 descriptors index (a numpy array is checked by `blur_kernels.check_table` and uploaded; keep the tensor to upload once).
    signed=False refuses sinc descriptors: what `blur2d` / `degrade_psf` need, whose mass rule has no negative taps.  Each tap is
    within one fp32 spacing of `TableDesc.table()`'s (tests/tables_ref.py derives the bound)."""
    ds = list(descs)
    if not ds or not all(isinstance(d, bk.TableDesc) for d in ds):
        raise ValueError(f"kernel_tables takes a non-empty list of blur_kernels.TableDesc (got {len(ds)} entries)")
    rows = [d.row() for d in ds]                                     # refuses what the table functions refuse
    for d in ds:                                                     # a NamedTuple built by hand gets the constructors' checks
        if d.kind == bk.KIND_SINC:
            bk.TableDesc.sinc(d.cutoff, d.ks)
        elif d.kind in (bk.KIND_GENERALIZED, bk.KIND_PLATEAU):
            bk._beta(d.beta)
    if not signed and any(d.kind == bk.KIND_SINC for d in ds):
        raise ValueError("kernel_tables(signed=False): a sinc table has negative taps (ops.filter2d takes it, ops.blur2d cannot)")
    own = tuple(d.ks for d in ds)
    ks = max(own) if ks is None else bk.check_ks(ks)
    if max(own) > ks:
        raise ValueError(f"kernel_tables: a table of side {max(own)} does not fit ks = {ks}")
    n_bank = kb = 0
    if bank is not None and isinstance(bank, torch.Tensor) and not any(d.kind == bk.KIND_BANK for d in ds):
        device, bank = bank.device, None                             # nothing indexes it: its side need not fit ks
    if bank is not None and not isinstance(bank, torch.Tensor):
        arr = np.asarray(bank)
        if arr.ndim != 3:
            raise ValueError(f"kernel_tables: a bank is [n][kb][kb] (got shape {arr.shape})")
        bank = torch.from_numpy(np.stack([bk.check_table(t, f"bank[{i}]") for i, t in enumerate(arr)])).to(_default_device(device))
    if bank is not None:
        if bank.dim() != 3 or not bank.is_cuda or bank.dtype != torch.float32 or bank.shape[1] != bank.shape[2] or bank.shape[0] < 1 or \
                not bank.is_contiguous():
            raise ValueError(f"kernel_tables: a bank is a contiguous CUDA fp32 [n][kb][kb] tensor (got {bank.dtype} {tuple(bank.shape)} on {bank.device})")
        n_bank, kb = int(bank.shape[0]), bk.check_ks(int(bank.shape[1]))
        if kb > ks:
            raise ValueError(f"kernel_tables: the bank's tables of side {kb} do not fit ks = {ks}")
    for i, d in enumerate(ds):
        if d.kind == bk.KIND_BANK and (bank is None or d.ks != kb or not 0 <= d.bank_index < n_bank):
            raise ValueError(f"kernel_tables: descriptor {i} names table {d.bank_index} of side {d.ks}, which the bank "
                             f"({n_bank} tables of side {kb}) does not hold")
    dev = bank.device if bank is not None else _default_device(device)
    desc = torch.tensor(rows, dtype=torch.float64).to(dev)
    tab = torch.empty(len(ds), ks, ks, dtype=torch.float32, device=dev)
    check(lib().srk_kernel_tables_f32(_p(desc), _p(bank), n_bank, kb, _p(tab), len(ds), ks, _stream()))
    return DeviceTables(tab, ks, own, any(d.kind == bk.KIND_SINC for d in ds))


def _default_device(device):
    return torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)


def _device_tables(t: DeviceTables, B: int, x: torch.Tensor, what: str) -> DeviceTables:
    if t.tab.dim() != 3 or t.tab.shape[0] != B or tuple(t.tab.shape[1:]) != (t.ks, t.ks) or len(t.own) != B or t.tab.device != x.device or \
            t.tab.dtype != torch.float32 or not t.tab.is_contiguous():
        raise ValueError(f"{what}: DeviceTables of one fp32 table per sample on {x.device} are needed (B={B}; got {tuple(t.tab.shape)} on {t.tab.device})")
    return t


def blur2d(x: torch.Tensor, psf, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x CUDA fp32 [B,C,H,W] blurred with one ks x ks table or one per sample (csrc/blur2d.hip, srk_blur2d_f32): a correlation (no flip,
    cv2.filter2D's convention) in which taps outside the image are dropped and the rest renormalised per pixel.  Tables: odd ks <= 21,
    taps finite and >= 0, centre > 0, sum within 1e-3 of 1 (ValueError otherwise); mixed sizes are zero-padded to the largest.  One
    launch after one small upload.  psf may be `DeviceTables` made with signed=False (one per sample): nothing is checked, packed or
    uploaded then."""
    B, Cc, H, W = _batch(x, "blur2d", nonempty=True)
    x = x.contiguous()
    if isinstance(psf, DeviceTables):
        if psf.signed:
            raise ValueError("blur2d: these DeviceTables hold a sinc table (negative taps); build them with kernel_tables(signed=False)")
        tabs, ks = None, _device_tables(psf, B, x, "blur2d").ks
    else:
        tabs, ks = pack_psf(psf, B)
    out = _padded_out(out, x.shape, x)
    k = psf.tab if tabs is None else torch.from_numpy(tabs).to(x.device)
    check(lib().srk_blur2d_f32(_p(x), _p(k), _p(out), B, Cc, H, W, ks, _stream()))
    return out


def degrade_psf(hr: torch.Tensor, scale: int, psf, noise=(0.0, 0.0), noise_ids=None, gray_noise=False, quant_bits: int = 8) -> Tuple[torch.Tensor, torch.Tensor]:
    """(lr, hr_cropped) like `degrade_blind` with a general 2-D blur: LR = noise(resize_aa(blur2d(HR))), i.e. `blur2d` on the region
    cropped to a multiple of the factor, then `degrade_blind` with sigma (0, 0) -- the plain bicubic tables on the blurred values, the
    same noise and rounding.  What DeviceHRPool(psf=)'s training patches are windows of, bit for bit.  The HR target is not blurred."""
    hr, s = _factor_crop(hr, scale, "degrade_psf")
    ids = list(range(hr.shape[0])) if noise_ids is None else noise_ids
    return degrade_blind(blur2d(hr, psf), s, (0.0, 0.0), noise, ids, gray_noise, quant_bits)[0], hr


# ---- JPEG, noise and the scale-1 restoration pairs (csrc/jpeg.hip, csrc/restore.hip) ----------------------------------
def jpeg_roundtrip(x: torch.Tensor, quality, subsample: bool = False, return_coef: bool = False):
    """What a baseline JPEG file of the 8-bit image of x at `quality` decodes to (csrc/jpeg.hip, srk_jpeg_roundtrip_f32): x CUDA fp32
    [B,C,H,W] with C = 1 or 3 is levelled to 8 bits, converted to JFIF YCbCr, transformed in 8 x 8 blocks anchored at (0, 0),
    quantised with libjpeg's scaling of the Annex K tables, and decoded again; chroma at 4:2:0 (`subsample`, C == 3 only) is averaged
    over 2 x 2 cells and upsampled by replication.  quality: an int or one per sample, each in 1..100, or 0 = that sample passes through
    bit for bit.  return_coef: also the quantised coefficients, int16 [B,C,Hm,Wm] (a test port; the part of a subsampled chroma plane
    outside its top-left [Hm/2,Wm/2] is zero).  One launch after one small upload."""
    B, Cc, H, W = _batch(x, "jpeg_roundtrip", chans=(1, 3), nonempty=True)
    qs = _qualities(quality, B, "jpeg_roundtrip")
    x = x.contiguous()
    qd = torch.tensor(qs, dtype=torch.int32).to(x.device)
    out = torch.empty_like(x)
    coef = None
    if return_coef:
        m = 16 if (subsample and Cc == 3) else 8
        coef = torch.zeros(B, Cc, -(-H // m) * m, -(-W // m) * m, dtype=torch.int16, device=x.device)
    check(lib().srk_jpeg_roundtrip_f32(_p(x), _p(out), _p(qd), B, Cc, H, W, int(bool(subsample)), _p(coef), _stream()))
    return (out, coef) if return_coef else out


def pack_restore_params(jpeg_quality, noise, noise_id: int, gray_noise: bool):
    """Slots 6..9 of a `srk_crop_restore_u8` descriptor / one row of `srk_noise_f32`'s table: `pack_degrade_params` with the JPEG
    quality (0 = no JPEG stage, else 1..100) as the low word of slot 6 in place of the blur sigmas."""
    return [_quality(jpeg_quality)] + pack_degrade_params((0.0, 0.0), noise, noise_id, gray_noise)[1:]


def noise(x: torch.Tensor, noise, noise_ids, gray_noise=False, quant_bits: int = 0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The noise stage of `degrade_blind` at scale 1 (csrc/restore.hip, srk_noise_f32): x CUDA fp32 [B,C,H,W], C = 1 or 3, gets
    `v + sqrt(sigma_n^2 + gain max(v, 0)) z` per element, z from Philox on the counter (x, y, ch | 0 with gray noise) under the key
    noise_id.  noise = (sigma_n, gain): one pair or one per sample, image units in [0, 1]; noise_ids: B integers; gray_noise: a bool or
    B of them (always so for C == 1).  Zero amplitudes pass the bits through; quant_bits 8 rounds to k / 255.  One launch after one small
    upload.  `out`: a buffer to write into.  On a padded batch the counter is (x, y, ch) only, so inside a sample's extents the bits
    are those of the dense call on that sample; what lands in the padding is never read."""
    B, Cc, H, W = _batch(x, "noise", chans=(1, 3), nonempty=True)
    q = _quant_bits(quant_bits, "noise")
    ids, grays = _ids_and_grays(noise_ids, gray_noise, B, "noise")
    rows = [pack_restore_params(0, n, i, g) for n, i, g in zip(_per_sample(noise, B, 2, "noise: noise"), ids, grays)]
    x = x.contiguous()
    par = torch.tensor(rows, dtype=torch.int64).to(x.device)
    out = _padded_out(out, x.shape, x)
    check(lib().srk_noise_f32(_p(x), _p(out), _p(par), B, Cc, H, W, q, _stream()))
    return out


_noise_stage = noise          # `restore_degrade` names its amplitude pair `noise`, as `degrade_blind` does


def restore_degrade(x: torch.Tensor, noise, noise_ids, gray_noise=False, jpeg_quality=0, subsample: bool = False,
                    quant_bits: int = 0) -> torch.Tensor:
    """The whole-image degradation of the scale-1 tasks: `noise`, then `jpeg_roundtrip` where the quality (an int or one per sample,
    0 = no JPEG stage) is > 0.  What DeviceRestorePool's training patches are windows of, bit for bit.  It is the composition of the
    two entries, no kernel of its own."""
    y = _noise_stage(x, noise, noise_ids, gray_noise, quant_bits)
    qs = _qualities(jpeg_quality, x.shape[0], "restore_degrade")
    return jpeg_roundtrip(y, qs, subsample) if any(qs) else y


# ---- second-order degradation: signed tables and ragged batches (csrc/filter2d.hip, csrc/ragged.hip) -----------------
class RaggedExt:
    """The extents of a ragged batch (include/srk.h "Ragged batches"): `host`, a list of B (h, w), and `dev`, the int32 [B][2] copy the
    kernels read.  The host copy is what the checks run on: nothing is read back from the device."""

    def __init__(self, ext, device):
        try:
            self.host = [(int(h), int(w)) for h, w in ext]
        except (TypeError, ValueError):
            raise ValueError(f"extents must be B pairs (h, w) (got {ext!r})") from None
        if not self.host or any(h < 1 or w < 1 for h, w in self.host):
            raise ValueError(f"every extent must be >= 1 (got {self.host})")
        self.dev = torch.tensor(self.host, dtype=torch.int32).to(device)

    def pad(self) -> Tuple[int, int]:
        return max(h for h, _ in self.host), max(w for _, w in self.host)


def _ragged(ext, B: int, Hp: int, Wp: int, device, what: str) -> Optional[RaggedExt]:
    """ext (None = dense, a list of pairs, or a RaggedExt) checked against a padded [B][.][Hp][Wp] buffer."""
    if ext is None:
        return None
    if not isinstance(ext, RaggedExt):
        ext = RaggedExt(ext, device)
    if len(ext.host) != B or any(h > Hp or w > Wp for h, w in ext.host):
        raise ValueError(f"{what}: {B} extents inside the padded {Hp} x {Wp} are needed (got {ext.host})")
    return ext


def _ext_ptr(ext: Optional[RaggedExt]):
    return None if ext is None else _p(ext.dev)


def filter2d(x: torch.Tensor, tab, ext=None, quant_bits: int = 0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x CUDA fp32 [B,C,Hp,Wp] filtered with one signed ks x ks table or one per sample (csrc/filter2d.hip, srk_filter2d_f32): a
    correlation with a reflect-101 border and no normalisation, cv2.filter2D's default and Real-ESRGAN's filter2D -- the rule sinc
    tables need, and the one every 2-D filter of the second-order chain takes.  ext: None (dense) or the (h, w) of every sample in the
    padded batch; each must exceed the R = ks // 2 of its sample's OWN table (zero-padding a table to the batch's largest ks adds taps
    that multiply in-extent pixels by 0: no bit changes).  A delta table passes its sample through bit for bit.  quant_bits 8 rounds to
    k / 255.  One launch after one small upload.  tab may be `DeviceTables` (one per sample): nothing is checked, packed or uploaded
    then, and the extent check runs on their host list of own sizes."""
    B, Cc, Hp, Wp = _batch(x, "filter2d", nonempty=True)
    q = _quant_bits(quant_bits, "filter2d")
    x = x.contiguous()
    if isinstance(tab, DeviceTables):
        tabs, ks, own = None, tab.ks, _device_tables(tab, B, x, "filter2d").own
    else:
        tabs, ks, own = pack_filter_tables(tab, B)
    e = _ragged(ext, B, Hp, Wp, x.device, "filter2d")
    for b, (h, w) in enumerate([(Hp, Wp)] * B if e is None else e.host):
        if min(h, w) <= own[b] // 2:
            raise ValueError(f"filter2d: sample {b} of {h} x {w} does not exceed the R = {own[b] // 2} of its table")
    out = _padded_out(out, x.shape, x)
    k = tab.tab if tabs is None else torch.from_numpy(tabs).to(x.device)
    check(lib().srk_filter2d_f32(_p(x), _p(k), _p(out), _ext_ptr(e), B, Cc, Hp, Wp, ks, q, _stream()))
    return out


RESIZE_MODES = ("cubic", "bilinear", "area")          # the mode words of srk_resize_ragged_mode_f32


def resize_ragged(x: torch.Tensor, ext_in, ext_out, modes, pad_out=None, quant_bits: int = 0, out: Optional[torch.Tensor] = None, *,
                  what: str = "resize_ragged") -> torch.Tensor:
    """`resize_aa` with a size and a resize rule per sample: sample b of the padded x [B,C,Hp,Wp] is resized from ext_in[b] to ext_out[b]
    into the top-left of out [B,C,Hop,Wop]; the rest of out keeps its bits.  ext_in / ext_out: None (dense) or B pairs; pad_out =
    (Hop, Wop), by default the largest output extents.  modes = None or B words: 0 the antialiased cubic (bit-identical to `resize_aa`
    on that sample alone), 1 bilinear without antialiasing (F.interpolate, align_corners=False), 2 area (adaptive average pooling).
    None or all zeros is ONE launch of csrc/ragged.hip's srk_resize_aa_ragged_f32 and no upload of modes; anything else one launch of
    csrc/resize_modes.hip's srk_resize_ragged_mode_f32 after one small upload.  The 8x limit of `resize_aa` holds for every mode and
    is checked here, on the host copies of the extents (SrkUnsupported).  what: the name the messages carry."""
    ms = None
    if modes is not None:
        try:
            ms = [int(m) for m in modes]
        except (TypeError, ValueError):
            raise ValueError(f"{what}: modes must be None or one word in 0..2 per sample (got {modes!r})") from None
        if any(m not in (0, 1, 2) or isinstance(v, bool) for m, v in zip(ms, modes)):
            raise ValueError(f"{what}: a mode is 0 (cubic), 1 (bilinear) or 2 (area) (got {ms})")
        if x.dim() != 4 or len(ms) != x.shape[0]:
            raise ValueError(f"{what}: one mode per sample of a [B,C,H,W] batch (got {len(ms)} for {tuple(x.shape)})")
    B, Cc, Hp, Wp = _batch(x, what, nonempty=True)
    q = _quant_bits(quant_bits, what)
    x = x.contiguous()
    ei = _ragged(ext_in, B, Hp, Wp, x.device, f"{what}: ext_in")
    if ext_out is None and pad_out is None:
        raise ValueError(f"{what}: a dense output needs pad_out = (Hop, Wop)")
    if ext_out is not None and not isinstance(ext_out, RaggedExt):
        ext_out = RaggedExt(ext_out, x.device)
    try:
        Hop, Wop = ext_out.pad() if pad_out is None else (int(v) for v in pad_out)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: pad_out must be (Hop, Wop) (got {pad_out!r})") from None
    if Hop < 1 or Wop < 1:
        raise ValueError(f"{what}: pad_out must be >= 1 (got {(Hop, Wop)})")
    eo = _ragged(ext_out, B, Hop, Wop, x.device, f"{what}: ext_out")
    for (h, w), (ho, wo) in zip([(Hp, Wp)] * B if ei is None else ei.host, [(Hop, Wop)] * B if eo is None else eo.host):
        if h > 8 * ho or w > 8 * wo:
            raise SrkUnsupported(f"{what}: {h} x {w} -> {ho} x {wo} shrinks an axis by more than 8x (more than 33 taps; the tile staging covers 8x)")
    out = _padded_out(out, (B, Cc, Hop, Wop), x)
    if ms is None or not any(ms):
        check(lib().srk_resize_aa_ragged_f32(_p(x), _ext_ptr(ei), _p(out), _ext_ptr(eo), B, Cc, Hp, Wp, Hop, Wop, q, _stream()))
    else:
        md = torch.tensor(ms, dtype=torch.int32).to(x.device)
        check(lib().srk_resize_ragged_mode_f32(_p(x), _ext_ptr(ei), _p(out), _ext_ptr(eo), _p(md), B, Cc, Hp, Wp, Hop, Wop, q, _stream()))
    return out


def resize_aa_ragged(x: torch.Tensor, ext_in, ext_out, pad_out=None, quant_bits: int = 0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """`resize_ragged` with the antialiased cubic for every sample (modes = None): bit-identical to `resize_aa` per sample.  One launch."""
    return resize_ragged(x, ext_in, ext_out, None, pad_out, quant_bits, out, what="resize_aa_ragged")


_USM_TAPS: dict = {}


def usm_ks(radius: int) -> int:
    """The tap count of `usm_sharpen` for Real-ESRGAN's `radius`: radius + 1 if it is even, else radius."""
    if isinstance(radius, bool) or not isinstance(radius, numbers.Integral) or not 1 <= radius <= 51:
        raise ValueError(f"usm: radius must be an integer in 1..51 (got {radius!r})")
    return int(radius) + 1 if radius % 2 == 0 else int(radius)


def usm_taps(ks: int, sigma: float, device) -> torch.Tensor:
    """The fp32 taps `blur_kernels.gaussian1d(ks, sigma)` on `device`: uploaded once per (device, ks, sigma) and kept."""
    device = torch.device(device)
    key = (device.type, device.index if device.index is not None else torch.cuda.current_device(), int(ks), float(sigma))
    t = _USM_TAPS.get(key)
    if t is None:
        t = _USM_TAPS[key] = torch.from_numpy(bk.gaussian1d(ks, sigma)).to(device)
    return t


def usm_sharpen(x: torch.Tensor, radius: int = 50, sigma: float = 0.0, weight: float = 0.5, threshold: float = 10.0,
                out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Real-ESRGAN's USMSharp on x CUDA fp32 [B,C,H,W] in [0, 1], C 1 or 3 (csrc/usm.hip, srk_usm_sharpen_f32; include/srk.h states the
    arithmetic): blur = G(x), res = x - blur, mask = |res| 255 > threshold, soft = G(mask), out = soft clamp(x + weight res, 0, 1) +
    (1 - soft) x, G the separable Gaussian of ks = radius + 1 (radius even) or radius taps under a reflect-101 border.  sigma <= 0 takes
    OpenCV's rule 0.3 ((ks - 1) / 2 - 1) + 0.8: the defaults are 51 taps at sigma 8.  H and W must exceed (ks - 1) / 2.  Two launches;
    one work buffer of x's size is allocated per call by torch."""
    B, Cc, H, W = _batch(x, "usm_sharpen", chans=(1, 3), nonempty=True)
    ks = usm_ks(radius)
    sigma = float(sigma)
    if not sigma == sigma or sigma == float("inf"):
        raise ValueError(f"usm_sharpen: sigma must be finite (got {sigma!r})")
    if sigma <= 0.0:
        sigma = 0.3 * ((ks - 1) / 2 - 1) + 0.8
    weight, threshold = float(weight), float(threshold)
    if not (weight == weight and threshold == threshold) or abs(weight) == float("inf"):
        raise ValueError(f"usm_sharpen: weight and threshold must be numbers (got {weight!r}, {threshold!r})")
    x = x.contiguous()
    if min(H, W) <= ks // 2:
        raise SrkUnsupported(f"usm_sharpen: a {H} x {W} image is not larger than R = {ks // 2} (radius {radius})")
    out = _padded_out(out, x.shape, x)
    work = torch.empty_like(x)
    check(lib().srk_usm_sharpen_f32(_p(x), _p(usm_taps(ks, sigma, x.device)), _p(out), _p(work), B, Cc, H, W, ks, weight, threshold, _stream()))
    return out


def jpeg_roundtrip_ragged(x: torch.Tensor, quality, ext=None, subsample: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """`jpeg_roundtrip` with a size per sample (csrc/ragged.hip, srk_jpeg_roundtrip_ragged_f32): the block grid and the edge replication
    of sample b are those of its own extents ext[b], so it is bit-identical to `jpeg_roundtrip` on that sample alone; quality 0 copies
    the in-extent words.  The padding of out keeps its bits.  One launch after one small upload."""
    B, Cc, Hp, Wp = _batch(x, "jpeg_roundtrip_ragged", chans=(1, 3), nonempty=True)
    qs = _qualities(quality, B, "jpeg_roundtrip_ragged")
    x = x.contiguous()
    e = _ragged(ext, B, Hp, Wp, x.device, "jpeg_roundtrip_ragged")
    out = _padded_out(out, x.shape, x)
    qd = torch.tensor(qs, dtype=torch.int32).to(x.device)
    check(lib().srk_jpeg_roundtrip_ragged_f32(_p(x), _p(out), _p(qd), _ext_ptr(e), B, Cc, Hp, Wp, int(bool(subsample)), _stream()))
    return out


class SecondOrder(NamedTuple):
    """The second-order degradation of ONE sample (Real-ESRGAN's chain; sr_datasets.SecondOrderSpec draws it): tables k1 / k2 / k3 for
    the three filters (blur_kernels; a delta = no filter; or `blur_kernels.TableDesc` descriptors, which the device turns into tables), resize factors r1 / r2 of the two intermediate sizes, noise1 / noise2 =
    (sigma_n, gain) with their gray flags, JPEG qualities q1 (stage 1) and q2 (stage 2), `jpeg_last`: False = order A (JPEG 2, final
    resize, final filter), True = order B (final resize, final filter, JPEG 2); the Philox key of noise 1 (noise 2 takes its
    complement).  modes: the rule of resize 1, resize 2 and the final resize (`resize_ragged`: 0 antialiased cubic, 1 bilinear,
    2 area); the default is the cubic of every earlier release."""
    k1: object
    r1: float
    noise1: Tuple[float, float]
    gray1: bool
    q1: int
    k2: object
    r2: float
    noise2: Tuple[float, float]
    gray2: bool
    q2: int
    jpeg_last: bool
    k3: object
    noise_id: int
    modes: Tuple[int, int, int] = (0, 0, 0)


def second_order_sizes(H: int, W: int, scale: int, p: SecondOrder):
    """((h1, w1), (h2, w2), (ho, wo)) of one sample: round-half-up of H r1, of (H / scale) r2, and the dense output H / scale."""
    rnd = lambda v: max(1, int(v + 0.5))          # noqa: E731
    s = int(scale)
    return (rnd(H * p.r1), rnd(W * p.r1)), (rnd(H / s * p.r2), rnd(W / s * p.r2)), (H // s, W // s)


def second_order_noise_ids(p: SecondOrder) -> Tuple[int, int]:
    i = int(p.noise_id) & 0xFFFFFFFFFFFFFFFF
    return i, i ^ 0xFFFFFFFFFFFFFFFF


def _stage_tables(ks_list, bank, device, what: str):
    """One stage's tables of `degrade_second_order`: arrays as they are (filter2d checks, packs and uploads them), descriptors built by
    ONE `kernel_tables` launch."""
    n = sum(isinstance(k, bk.TableDesc) for k in ks_list)
    if n == 0:
        return ks_list
    if n != len(ks_list):
        raise ValueError(f"degrade_second_order: {what} mixes tables and TableDesc descriptors in one batch ({n} of {len(ks_list)} are descriptors)")
    return kernel_tables(ks_list, bank=bank, device=device)


def _stage_modes(ps):
    """The mode lists of the three resizes of `degrade_second_order`; None for a stage whose samples all take the cubic (the launch of
    `resize_aa_ragged`, and no upload)."""
    if all(p.modes == (0, 0, 0) for p in ps):          # the chain of every earlier release: nothing to check, build or upload
        return None, None, None
    for p in ps:
        if len(p.modes) != 3 or any(isinstance(m, bool) or m not in (0, 1, 2) for m in p.modes):
            raise ValueError(f"degrade_second_order: modes must be three words in 0..2 (got {p.modes!r})")
    return tuple(([p.modes[k] for p in ps] if any(p.modes[k] for p in ps) else None) for k in range(3))


def degrade_second_order(x: torch.Tensor, scale: int, params, subsample: bool = False, pads=None, bufs: Optional[dict] = None,
                         bank=None) -> torch.Tensor:
    """The second-order blind degradation on a batch x CUDA fp32 [B,C,H,W] (C = 1 or 3; H, W multiples of `scale` in 1..4), one
    `SecondOrder` per sample -> the LR batch [B,C,H/scale,W/scale] in 8-bit levels:
        filter k1 -> resize to (H, W) r1 -> noise 1 -> JPEG q1 -> filter k2 -> resize to (H, W) / scale r2 -> noise 2
        -> [order A: JPEG q2] -> resize to (H, W) / scale -> filter k3, rounded to 8 bits -> [order B: JPEG q2]
    Every filter is `filter2d` (reflect border), every intermediate is a ragged batch in a padded buffer, so every sample has its own
    sizes and every stage is ONE launch: eleven launches and their small uploads, no host read, no intermediate copy.  Each sample is
    bit-identical to the composition of the dense ops on that sample alone.  pads = ((Hp1, Wp1), (Hp2, Wp2)) fixes the padded sizes
    (default: the batch's largest); bufs: a dict that keeps the work buffers between calls.
    k1 / k2 / k3 may be `blur_kernels.TableDesc` descriptors in place of tables -- per stage all or none of the batch -- and the
    stage's tables are then built on the device by one `kernel_tables` launch (three more tiny launches, three fewer table uploads);
    bank: the CUDA tensor that kind-5 descriptors index.
    `SecondOrder.modes` picks the rule of each of the three resizes per sample (`resize_ragged`); a stage whose samples all take mode 0
    is the launch of `resize_aa_ragged`, so the default is the chain of every earlier release."""
    B, Cc, H, W = _batch(x, "degrade_second_order", chans=(1, 3), nonempty=True)
    s = int(scale)
    if not 1 <= s <= 4 or H % s or W % s:
        raise ValueError(f"degrade_second_order: scale in 1..4 dividing H and W (got scale {scale!r}, {tuple(x.shape)})")
    ps = list(params)
    if len(ps) != B or not all(isinstance(p, SecondOrder) for p in ps):
        raise ValueError(f"degrade_second_order: one SecondOrder per sample (B={B}; got {len(ps)})")
    sizes = [second_order_sizes(H, W, s, p) for p in ps]
    e1, e2 = RaggedExt([z[0] for z in sizes], x.device), RaggedExt([z[1] for z in sizes], x.device)
    (Hp1, Wp1), (Hp2, Wp2) = (e1.pad(), e2.pad()) if pads is None else pads
    Ho, Wo = H // s, W // s
    bufs = {} if bufs is None else bufs

    def buf(name, *shape):
        t = bufs.get(name)
        if t is None or tuple(t.shape) != shape or t.device != x.device:
            t = bufs[name] = torch.empty(shape, dtype=torch.float32, device=x.device)
        return t

    ids = [second_order_noise_ids(p) for p in ps]
    qa = [0 if p.jpeg_last else p.q2 for p in ps]
    qb = [p.q2 if p.jpeg_last else 0 for p in ps]
    x = x.contiguous()
    t1, t2, t3 = (_stage_tables([getattr(p, k) for p in ps], bank, x.device, k) for k in ("k1", "k2", "k3"))
    a = filter2d(x, t1, out=buf("f1", B, Cc, H, W))
    m1, m2, m3 = _stage_modes(ps)
    a = resize_ragged(a, None, e1, m1, (Hp1, Wp1), out=buf("a1", B, Cc, Hp1, Wp1))
    a = noise(a, [p.noise1 for p in ps], [i[0] for i in ids], [p.gray1 for p in ps], out=buf("b1", B, Cc, Hp1, Wp1))
    a = jpeg_roundtrip_ragged(a, [p.q1 for p in ps], e1, subsample, out=buf("a1", B, Cc, Hp1, Wp1))
    a = filter2d(a, t2, e1, out=buf("b1", B, Cc, Hp1, Wp1))
    a = resize_ragged(a, e1, e2, m2, (Hp2, Wp2), out=buf("a2", B, Cc, Hp2, Wp2))
    a = noise(a, [p.noise2 for p in ps], [i[1] for i in ids], [p.gray2 for p in ps], out=buf("b2", B, Cc, Hp2, Wp2))
    a = jpeg_roundtrip_ragged(a, qa, e2, subsample, out=buf("a2", B, Cc, Hp2, Wp2))
    a = resize_ragged(a, e2, None, m3, (Ho, Wo), out=buf("lr0", B, Cc, Ho, Wo))
    a = filter2d(a, t3, quant_bits=8, out=buf("lr1", B, Cc, Ho, Wo))
    return jpeg_roundtrip(a, qb, subsample)


LUMA_COEF = (4899, 9617, 1868)          # /16384: full-range BT.601 in 14-bit fixed point, the sum is 16384


def to_gray(x):
    """The integer luma `(4899 R + 9617 G + 1868 B + 8192) >> 14` of stored samples, on the CPU: x uint8 / uint16, a numpy array or a
    CPU tensor, [..., H, W, 3] -> [..., H, W] of the same type and dtype.  What srk_crop_restore_u8 makes of an RGB source at
    out_chans 1, so a validation loader can form the same one-channel HR images."""
    is_t = isinstance(x, torch.Tensor)
    a = x.detach().cpu().numpy() if is_t else np.asarray(x)
    if a.dtype not in (np.uint8, np.uint16):
        raise ValueError(f"to_gray takes uint8 or uint16 samples (got {a.dtype})")
    if a.ndim < 3 or a.shape[-1] != 3:
        raise ValueError(f"to_gray takes [..., H, W, 3] samples (got shape {tuple(a.shape)})")
    v = a.astype(np.uint32)          # 16384 * 65535 + 8192 < 2^32
    y = ((LUMA_COEF[0] * v[..., 0] + LUMA_COEF[1] * v[..., 1] + LUMA_COEF[2] * v[..., 2] + 8192) >> 14).astype(a.dtype)
    return torch.from_numpy(y) if is_t else y


# ---- image files to and from the device (csrc/image_io.hip) -----------------------------------------------------------------
_SAMPLE_MAX = {torch.uint8: 255, torch.uint16: 65535}


def _samples_i32(a: torch.Tensor) -> torch.Tensor:
    """Stored samples as int32 (torch has little arithmetic on uint16: its bits are read as int16 and the sign is undone)."""
    return a.to(torch.int32) if a.dtype == torch.uint8 else a.view(torch.int16).to(torch.int32) & 0xFFFF


def _luma_i32(r, g, b):
    """`to_gray` on int32 samples: 16384 * 65535 + 8192 needs 31 bits, so the sum is formed in int64."""
    y = (LUMA_COEF[0] * r.to(torch.int64) + LUMA_COEF[1] * g.to(torch.int64) + LUMA_COEF[2] * b.to(torch.int64) + 8192) >> 14
    return y.to(torch.int32)


def image_unpack(a: torch.Tensor, out_chans: int, want_alpha: bool = False):
    """Decoded image samples -> (x, alpha | None): a uint8 / uint16 [B,H,W,ch], [H,W,ch] or [H,W] (ch 1..4: gray, gray + alpha, RGB,
    RGB + alpha; a 3-D tensor is one image) -> x fp32 [B,out_chans,H,W] in [0, 1] (B = 1 for one image), out_chans 1 | 3.
    Value = sample / 255 or / 65535 as an IEEE fp32 division -- the bits of `pil_to_tensor01`; gray is repeated into three channels
    (`ensure_3ch`), RGB becomes one channel by the integer luma of the stored samples (`to_gray`, as `clean_to_tensor`).  want_alpha: the
    last sample of ch 2 | 4 as fp32 [B,1,H,W] (None for ch 1 | 3, and when not asked for).  A CUDA tensor is one launch
    (srk_image_unpack), capturable; a CPU tensor runs the same arithmetic in torch."""
    if not isinstance(a, torch.Tensor) or a.dtype not in _SAMPLE_MAX:
        raise ValueError(f"image_unpack takes a uint8 or uint16 tensor (got {getattr(a, 'dtype', type(a))})")
    if out_chans not in (1, 3):
        raise ValueError(f"image_unpack: out_chans must be 1 or 3 (got {out_chans!r})")
    if a.dim() == 2:
        a = a[None, :, :, None]
    elif a.dim() == 3:
        a = a[None]
    if a.dim() != 4 or not 1 <= a.shape[3] <= 4 or min(a.shape) < 1:
        raise ValueError(f"image_unpack takes non-empty [B,H,W,ch], [H,W,ch] or [H,W] samples with ch in 1..4 (got {tuple(a.shape)})")
    B, H, W, ch = a.shape
    has_alpha = bool(want_alpha) and ch in (2, 4)
    if a.is_cuda:
        a = a.contiguous()
        x = torch.empty((B, out_chans, H, W), dtype=torch.float32, device=a.device)
        alpha = torch.empty((B, 1, H, W), dtype=torch.float32, device=a.device) if has_alpha else None
        check(lib().srk_image_unpack(_p(a), _p(x), _p(alpha), B, H, W, ch, 8 * a.element_size(), out_chans, _stream()))
        return x, alpha
    s = _samples_i32(a)
    mx = float(_SAMPLE_MAX[a.dtype])
    if ch <= 2:
        planes = [s[..., 0]] * out_chans
    elif out_chans == 3:
        planes = [s[..., 0], s[..., 1], s[..., 2]]
    else:
        planes = [_luma_i32(s[..., 0], s[..., 1], s[..., 2])]
    x = torch.stack(planes, 1).to(torch.float32) / mx
    alpha = (s[..., ch - 1].to(torch.float32) / mx).unsqueeze(1) if has_alpha else None
    return x.contiguous(), alpha


def _quantise_i32(v: torch.Tensor, mx: int) -> torch.Tensor:
    """q(v): NaN -> 0, v <= 0 -> 0, v >= 1 -> max, else round-half-to-even of the fp32 product v * max."""
    q = torch.round(v * float(mx))                                          # NaN stays NaN here and fails `v > 0` below
    q = torch.where(v >= 1.0, torch.full_like(q, float(mx)), q)
    return torch.where(v > 0.0, q, torch.zeros_like(q)).to(torch.int32)


def image_pack(y: torch.Tensor, alpha: Optional[torch.Tensor] = None, out_chans: Optional[int] = None, bits: int = 8,
               counters: Optional[torch.Tensor] = None) -> torch.Tensor:
    """A prediction as file samples: y fp32 [B,C,H,W] (or [C,H,W]: one image), C 1 | 3, + alpha fp32 [B,1,H,W] -> uint8 (bits 8) or
    uint16 (bits 16) [B,H,W,out_chans] ([H,W,out_chans] for one image).  out_chans 1 gray, 2 gray + alpha, 3 RGB, 4 RGB + alpha (default: C,
    plus 1 with an alpha).  Samples are q(v) = rint(v * max) of the clamped value (NaN -> 0): the `(x * 255).round()` of the public test
    scripts, not the truncation of `evaluate.save_tensor_as_png`; RGB -> gray is the integer luma (`to_gray`) of the QUANTISED samples,
    gray -> RGB repeats the sample.  counters: an int32 [2] tensor on y's device that the call ADDS to -- [0] the non-finite input values,
    [1] the finite ones outside [0, 1] (y, and alpha where it is written).  A CUDA tensor is one launch (srk_image_pack), capturable;
    a CPU tensor runs the same arithmetic in torch."""
    if not isinstance(y, torch.Tensor) or y.dtype != torch.float32 or y.dim() not in (3, 4):
        raise ValueError(f"image_pack takes an fp32 [B,C,H,W] or [C,H,W] tensor (got {getattr(y, 'dtype', type(y))} "
                         f"{tuple(getattr(y, 'shape', ()))})")
    single = y.dim() == 3
    if single:
        y = y[None]
        alpha = alpha[None] if (alpha is not None and alpha.dim() == 3) else alpha
    B, C, H, W = y.shape
    if C not in (1, 3) or min(B, H, W) < 1:
        raise ValueError(f"image_pack takes a non-empty batch with C 1 or 3 (got {tuple(y.shape)})")
    if out_chans is None:
        out_chans = C + (alpha is not None)
    if out_chans not in (1, 2, 3, 4):
        raise ValueError(f"image_pack: out_chans must be in 1..4 (got {out_chans!r})")
    if bits not in (8, 16):
        raise ValueError(f"image_pack: bits must be 8 or 16 (got {bits!r})")
    with_alpha = out_chans in (2, 4)
    if with_alpha and alpha is None:
        raise ValueError(f"image_pack: out_chans {out_chans} needs an alpha plane")
    if alpha is not None and (alpha.dtype != torch.float32 or tuple(alpha.shape) != (B, 1, H, W) or alpha.device != y.device):
        raise ValueError(f"image_pack: alpha must be fp32 {(B, 1, H, W)} on {y.device} (got {alpha.dtype} {tuple(alpha.shape)} on {alpha.device})")
    if counters is not None and (counters.dtype != torch.int32 or tuple(counters.shape) != (2,) or counters.device != y.device or
                                 not counters.is_contiguous()):
        raise ValueError(f"image_pack: counters must be a contiguous int32 [2] tensor on {y.device}")
    dtype = torch.uint8 if bits == 8 else torch.uint16
    if y.is_cuda:
        y = y.contiguous()
        a = alpha.contiguous() if with_alpha else None
        out = torch.empty((B, H, W, out_chans), dtype=dtype, device=y.device)
        check(lib().srk_image_pack(_p(y), _p(a), _p(out), _p(counters), B, H, W, C, out_chans, bits, _stream()))
        return out[0] if single else out
    mx = _SAMPLE_MAX[dtype]
    vals = [y] + ([alpha] if with_alpha else [])
    if counters is not None:
        fin = [torch.isfinite(v) for v in vals]
        counters += torch.tensor([sum(int((~f).sum()) for f in fin), sum(int((f & ((v < 0) | (v > 1))).sum()) for f, v in zip(fin, vals))],
                                 dtype=torch.int32)
    q = _quantise_i32(y, mx)
    if out_chans <= 2:
        chans = [_luma_i32(q[:, 0], q[:, 1], q[:, 2]) if C == 3 else q[:, 0]]
    else:
        chans = [q[:, c if C == 3 else 0] for c in range(3)]
    if with_alpha:
        chans.append(_quantise_i32(alpha, mx)[:, 0])
    s = torch.stack(chans, -1)
    out = s.to(torch.uint8) if bits == 8 else (s - ((s >= 32768).to(torch.int32) << 16)).to(torch.int16).view(torch.uint16)
    out = out.contiguous()
    return out[0] if single else out
