"""Upscale image files that have no ground truth: the `--folder_lq` mode of the SwinIR test script, the HAT / DAT test configs without
`dataroot_gt`, Real-ESRGAN's inference script.

    python -m tpu_superresolution_amd.predict --input FILE|DIR --output DIR --arch swinir|hat|dat --scale X1|X2|X3|X4|X8 --ckpt F
    python -m tpu_superresolution_amd.predict --input FILE|DIR --output DIR --arch auto --scale auto --ckpt F

--arch auto: the checkpoint is the specification.  checkpoint_arch.build_from_state reads the family and the constructor
keywords from the state_dict's key names and shapes, prints them on `[arch]` lines with the conventions it applied (img_range, HAT's
conv_scale), and refuses what the HIP path does not cover with the package's own reason before anything runs.  --scale auto takes the
file's scale; an explicit --scale must equal it.  --window_size, --task, --channels and --upsampler are refused (the file decides them);
--img_range R overrides the img_range convention.  An explicit --arch builds one configuration per family, as before.

Files: --input is one file or a directory (not recursive, sorted by name, only what PIL opens; anything else prints a `[skip]` line).
Outputs are `<stem><--suffix, default _sr>.png` under --output; an output that would overwrite its input is refused.  Modes L, LA, RGB,
RGBA and I;16 (16-bit gray) are kept as they are; P, 1, CMYK and the rest are converted to RGB (RGBA with transparency) with a `[convert]`
line.  The output has the input's mode and bit depth (--out_bits 8 | 16 overrides the depth): gray in gives gray out, alpha is kept.

Model: --param_key, --window_size, --task sr|dn|car and --channels 1|3 as in evaluate (finetune_swinir.build_sr_model /
build_restoration_model, evaluate._load_state); `--upsampler nearest+conv` (--arch swinir, window 8) builds the M-size real-SR SwinIR of
the SwinIR authors' real_sr task.  --tile / --tile_overlap / --tile_batch / --tile_blend / --self_ensemble as in evaluate (the ensemble
outside, the tiles inside).  --batch_size N: up to N consecutive files of equal (H, W, mode, depth) form one model call.  --outscale S
(default: the model's scale): the fp32 prediction is resized to (max(1, int(H S + 0.5)), max(1, int(W S + 0.5))) with ops.resize_aa before
it is quantised.  Alpha does not go through the model: the alpha plane is resized to the output size with ops.resize_aa.

Per group of files, on the device: one upload of the raw samples, one unpack launch (ops.image_unpack), the model path, the
optional resize, one pack launch (ops.image_pack: clamp, x max, round-half-to-even -- the `(x * 255).round()` of the public scripts),
one download of the packed samples and one read of the two counters.  A non-finite value in a prediction raises before anything of its
group is written; the count of clipped values is printed.  `upscale()` is the function under the command line: it takes any callable as
the model and any device; `main(argv)` is callable and returns a dict.

--niqe F.npz [--niqe_crop_border N]: every output is scored with NIQE (niqe.py) against the parameter file, on the device,
from the fp32 prediction after the optional resize and before the download -- the score of the 8-bit quantisation of what is written, also
with --out_bits 16.  `[niqe] <name> <score>` lines, the mean in `[done]`, and 'niqe' in the result dict; without the flag nothing changes.
The file is checked (keys, shapes, finite, symmetric covariance) while the arguments are parsed, before the checkpoint is read.
"""
from __future__ import annotations

import argparse
import math
import time
from functools import partial
from pathlib import Path
from typing import Callable, List, Optional, Sequence

import numpy as np
import torch
from PIL import Image

from . import ops
from .data_cli import SCALES, default_window_size, flag, shared_flags
from .evaluate import PARAM_KEYS, _load_state

PREDICT_SCALES = dict(sorted({**SCALES, "X3": 3, "X8": 8}.items()))          # predict's own table: x3 for the three families, x8 for SwinIR (data_cli.SCALES is the training parsers')
KEPT_MODES = ("L", "LA", "RGB", "RGBA", "I;16")          # kept as they are; every other mode is converted
_CHANNELS = {"L": 1, "LA": 2, "RGB": 3, "RGBA": 4, "I;16": 1}
_OUT_MODE = {1: "L", 2: "LA", 3: "RGB", 4: "RGBA"}


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="Upscale image files without ground truth (SwinIR / HAT / DAT on the MI355X HIP path)")
    ap.add_argument("--input", type=str, required=True, help="an image file, or a directory of them (not recursive, sorted by name)")
    ap.add_argument("--output", type=str, required=True, help="directory of the <stem><suffix>.png outputs (created)")
    ap.add_argument("--suffix", type=str, default="_sr", help="appended to the input's stem")
    ap.add_argument("--arch", type=str, choices=["swinir", "hat", "dat", "auto"], required=True,
                    help="auto: the constructor keywords are read from the checkpoint (checkpoint_arch.infer_arch)")
    ap.add_argument("--scale", type=str, choices=[*PREDICT_SCALES, "auto"], required=True,
                    help="the model's scale; X1 with --task dn | car; X8 with --arch swinir; auto (with --arch auto): the checkpoint's")
    ap.add_argument("--img_range", type=float, default=None, metavar="R",
                    help="with --arch auto: SwinIR(img_range=R) instead of the convention (255 for the scale-1 head at window 7, else 1.0)")
    ap.add_argument("--ckpt", type=str, required=True)
    ap.add_argument("--param_key", type=str, choices=["auto", *PARAM_KEYS], default="auto",
                    help="which envelope of the checkpoint to load (auto: model, then params, then params_ema)")
    ap.add_argument("--device", type=str, default=None, help="force 'cpu' / 'cuda' (default: cuda if available)")
    ap.add_argument("--window_size", type=int, default=None, help="--arch swinir: SwinIR(window_size=N), N in 2..8 (default: 8, or 7 with --task car)")
    flag(ap, "task", str, "sr", choices=["sr", "dn", "car"],
         text="--arch swinir: dn = denoising, car = JPEG compression-artifact reduction (finetune_swinir.build_restoration_model); they need --scale X1")
    shared_flags(ap, "channels")
    ap.add_argument("--upsampler", type=str, choices=["pixelshuffle", "nearest+conv"], default="pixelshuffle",
                    help="--arch swinir --task sr, window 8: nearest+conv = the M-size real-SR SwinIR of the SwinIR authors' real_sr task")
    ap.add_argument("--self_ensemble", action="store_true", help="predict with the x8 self-ensemble (augment.self_ensemble)")
    ap.add_argument("--tile", type=int, default=0, help="predict on overlapping tiles of N x N input pixels (tiling.tiled_forward; 0 = off)")
    ap.add_argument("--tile_overlap", type=int, default=32, help="with --tile: input pixels two neighbouring tiles share")
    ap.add_argument("--tile_batch", type=int, default=1, help="with --tile: tiles per model call")
    ap.add_argument("--tile_blend", type=str, choices=["mean", "center"], default="mean", help="with --tile: as in evaluate")
    ap.add_argument("--batch_size", type=int, default=1, help="consecutive files of equal (H, W, mode, depth), up to N, form one model call")
    ap.add_argument("--outscale", type=float, default=None, metavar="S",
                    help="final size = input size x S (default: the model's scale): the fp32 prediction is resized with ops.resize_aa before it is quantised")
    ap.add_argument("--out_bits", type=str, choices=["auto", "8", "16"], default="auto", help="bit depth of the outputs (auto: the input's)")
    ap.add_argument("--niqe", type=str, default=None, metavar="F.npz",
                    help="score every output with NIQE against this parameter file (niqe_pris_params.npz format; `python -m tpu_superresolution_amd.niqe fit` "
                         "writes one): on the device, from the fp32 prediction quantised to 8 bits -- also with --out_bits 16, where the score is that of the "
                         "8-bit quantisation of what is written")
    ap.add_argument("--niqe_crop_border", type=int, default=0, metavar="N", help="with --niqe: pixels cropped on every side before the score")
    args = ap.parse_args(argv)
    args.niqe_params = None
    if args.niqe is not None:          # the file is read and checked here, before the checkpoint is opened
        from .niqe import load_niqe_params
        try:
            args.niqe_params = load_niqe_params(args.niqe)
        except ValueError as e:
            ap.error(f"--niqe {e}")
    if args.niqe_crop_border < 0 or (args.niqe_crop_border and args.niqe is None):
        ap.error(f"--niqe_crop_border is an option of --niqe and must be >= 0 (got {args.niqe_crop_border})")
    if args.img_range is not None and not (math.isfinite(args.img_range) and args.img_range > 0):
        ap.error(f"--img_range must be a positive number (got {args.img_range})")
    if args.arch == "auto":          # the file decides the model: its flags are refused off their defaults
        given = [f"--{n} {getattr(args, n)}" for n, dflt in (("window_size", None), ("task", "sr"), ("channels", 3), ("upsampler", "pixelshuffle"))
                 if getattr(args, n) != dflt]
        if given:
            ap.error(f"{', '.join(given)}: with --arch auto the checkpoint decides window_size, task, channels and upsampler")
        args.window_size = default_window_size(args.task)
    else:
        if args.scale == "auto":
            ap.error(f"--scale auto goes with --arch auto (--arch {args.arch} builds one configuration per scale: name it)")
        if args.img_range is not None:
            ap.error(f"--img_range is an option of --arch auto (--arch {args.arch} builds its configuration's own)")
        if args.scale.upper() == "X8" and args.arch != "swinir":
            ap.error(f"--scale X8 is an option of --arch swinir and --arch auto (got --arch {args.arch})")
        if args.upsampler == "nearest+conv" and args.scale.upper() not in ("X2", "X4"):
            ap.error(f"--upsampler nearest+conv upsamples by 2 or 4 (got --scale {args.scale})")
    if args.window_size is None:
        args.window_size = default_window_size(args.task)
    restore = args.task != "sr"
    if args.arch != "auto" and restore != (args.scale.upper() == "X1"):
        ap.error(f"--task dn | car and --scale X1 go together (got --task {args.task} --scale {args.scale})")
    if restore and args.arch != "swinir":
        ap.error(f"--task {args.task} is an option of --arch swinir (got --arch {args.arch})")
    if args.channels != 3 and not restore:
        ap.error("--channels 1 is an option of --task dn | car (the super-resolution models take three channels)")
    if args.tile < 0 or args.tile_batch < 1 or args.tile_overlap < 0 or (args.tile and args.tile_overlap >= args.tile):
        ap.error(f"--tile must be >= 0, --tile_batch >= 1 and 0 <= --tile_overlap < --tile (got --tile {args.tile} "
                 f"--tile_overlap {args.tile_overlap} --tile_batch {args.tile_batch})")
    if not 2 <= args.window_size <= 8 or (args.window_size != 8 and args.arch != "swinir"):
        ap.error(f"--window_size must be in 2..8 and is an option of --arch swinir (got {args.window_size} with --arch {args.arch})")
    if args.upsampler != "pixelshuffle" and (args.arch != "swinir" or restore or args.window_size != 8):
        ap.error(f"--upsampler {args.upsampler} is an option of --arch swinir --task sr at window 8")
    if args.batch_size < 1:
        ap.error(f"--batch_size must be >= 1 (got {args.batch_size})")
    if args.outscale is not None and not (math.isfinite(args.outscale) and args.outscale > 0):
        ap.error(f"--outscale must be a positive number (got {args.outscale})")
    if "/" in args.suffix or "\\" in args.suffix:
        ap.error(f"--suffix is a part of a file name (got {args.suffix!r})")
    return args


# ---- files -----------------------------------------------------------------------------------------------------------------------------
def discover(inp, log: Callable = print) -> List[Path]:
    """The image files of --input: the file itself, or the directory's entries sorted by name (not recursive); whatever PIL cannot
    open is left out with a `[skip]` line."""
    inp = Path(inp)
    if not inp.exists():
        raise FileNotFoundError(f"--input {inp} does not exist")
    files = []
    for p in ([inp] if inp.is_file() else sorted(inp.iterdir(), key=lambda q: q.name)):
        if not p.is_file():
            log(f"[skip] {p.name}: not a file")
            continue
        try:
            with Image.open(p) as im:
                im.verify()
        except Exception as e:          # PIL raises UnidentifiedImageError, OSError, SyntaxError, ... by format
            log(f"[skip] {p.name}: PIL cannot open it ({type(e).__name__})")
            continue
        files.append(p)
    return files


def load_image(path, log: Callable = print):
    """-> (samples uint8 / uint16 [H,W] or [H,W,ch] in host byte order, mode).  L, LA, RGB, RGBA and I;16 are kept; I;16B / I;16L become
    I;16 silently (the same samples); every other mode is converted to RGB, or RGBA when the image has transparency, with a `[convert]` line."""
    with Image.open(path) as im:
        im.load()
        mode = im.mode
        if mode in ("I;16B", "I;16L", "I;16N"):
            mode = "I;16"
        if mode not in KEPT_MODES:
            to = "RGBA" if (im.mode in ("PA", "La", "RGBa") or "transparency" in im.info) else "RGB"
            log(f"[convert] {Path(path).name}: mode {im.mode} -> {to}")
            im = im.convert(to)
            mode = to
        a = np.asarray(im)
    if a.dtype.byteorder == ">":
        a = a.astype(a.dtype.newbyteorder("="))
    if a.dtype not in (np.uint8, np.uint16):
        raise ValueError(f"{path}: mode {mode} decoded to {a.dtype} samples (8- or 16-bit expected)")
    return np.ascontiguousarray(a), mode


def output_path(src, out_dir, suffix: str = "_sr") -> Path:
    """<out_dir>/<stem><suffix>.png; an output that is its own input is refused."""
    src, dst = Path(src), Path(out_dir) / f"{Path(src).stem}{suffix}.png"
    if dst.resolve() == src.resolve():
        raise ValueError(f"the output {dst} would overwrite its input (choose another --output or --suffix)")
    return dst


def save_image(a: np.ndarray, path) -> None:
    """Packed samples [H,W,ch] -> PNG: uint8 ch 1..4 as L / LA / RGB / RGBA, uint16 ch 1 as I;16."""
    ch = a.shape[2]
    if a.dtype == np.uint16:
        if ch != 1:
            raise ValueError(f"16-bit PNG output is gray only (got {ch} channels: PIL has no 16-bit {_OUT_MODE[ch]})")
        img = Image.frombytes("I;16", (a.shape[1], a.shape[0]), np.ascontiguousarray(a[:, :, 0]).astype("<u2").tobytes())
    else:
        img = Image.fromarray(a[:, :, 0] if ch == 1 else a, mode=_OUT_MODE[ch])
    img.save(str(path), format="PNG")


# ---- the prediction ---------------------------------------------------------------------------------------------------------------------
def _to_device(stack: np.ndarray, device) -> torch.Tensor:
    """One upload of the raw samples (torch reads uint16 through its int16 view)."""
    t = torch.from_numpy(stack.view(np.int16)).view(torch.uint16) if stack.dtype == np.uint16 else torch.from_numpy(stack)
    return t.to(device)


def _to_host(t: torch.Tensor) -> np.ndarray:
    t = t.cpu()
    return t.view(torch.int16).numpy().view(np.uint16) if t.dtype == torch.uint16 else t.numpy()


def _resize(x: torch.Tensor, size) -> torch.Tensor:
    """ops.resize_aa on the device; a CPU tensor takes torch's antialiased bicubic, the convention resize_aa restates."""
    if x.is_cuda:
        return ops.resize_aa(x.contiguous(), size)
    return torch.nn.functional.interpolate(x, size=tuple(size), mode="bicubic", antialias=True, align_corners=False)


def out_size(H: int, W: int, outscale: float):
    return max(1, int(H * outscale + 0.5)), max(1, int(W * outscale + 0.5))


def make_predict(model, *, tile: int = 0, tile_overlap: int = 32, tile_batch: int = 1, tile_blend: str = "mean", self_ensemble: bool = False,
                 log: Callable = print):
    """The model path of evaluate: the tiles inside, the self-ensemble outside."""
    predict = model
    if tile:
        from .tiling import tiled_forward
        predict = partial(tiled_forward, model, tile=tile, overlap=tile_overlap, tile_batch=tile_batch, blend=tile_blend)
        log(f"[tile] {tile} overlap {tile_overlap} batch {tile_batch} blend {tile_blend}")
    if self_ensemble:
        from .augment import self_ensemble as ensemble
        predict = partial(ensemble, predict)
        log("[self_ensemble] x8")
    return predict


def _key(a: np.ndarray):
    return a.shape, a.dtype


def _mode_label(ch: int, bits: int) -> str:
    """The PIL mode an array of `ch` samples of `bits` stands for: I;16 for 16-bit gray; PIL has no name for the other 16-bit layouts."""
    if bits == 8:
        return _OUT_MODE[ch]
    return "I;16" if ch == 1 else f"{_OUT_MODE[ch]};16"


def upscale(model, arrays: Sequence[np.ndarray], *, scale: int, device, channels: int = 3, outscale: Optional[float] = None,
            out_bits="auto", batch_size: int = 1, names: Optional[Sequence[str]] = None, modes: Optional[Sequence[str]] = None,
            sink: Optional[Callable] = None, log: Callable = print, niqe_params: Optional[dict] = None, niqe_crop_border: int = 0) -> dict:
    """Runs `model` (any callable [B,channels,H,W] fp32 in [0, 1] -> [B,channels,H scale,W scale]) on decoded images.

    arrays: uint8 / uint16 [H,W] or [H,W,ch], ch 1..4 (gray, gray + alpha, RGB, RGB + alpha).  Consecutive arrays of equal shape and dtype,
    up to batch_size, form one group = one model call.  Per group: one upload, ops.image_unpack, the model, the optional ops.resize_aa to
    out_size(H, W, outscale), ops.image_pack with the counters, one download, one read of the counters.  The output of an image has its
    channel count, and its depth unless out_bits is 8 or 16.  sink(index, samples [Ho,Wo,ch]) receives every output after its group's
    guard has passed (default: they are collected in the result's 'outputs').  A non-finite value raises RuntimeError before the sink sees
    any image of the group.  niqe_params (niqe.load_niqe_params' dict): every prediction is scored with niqe.niqe after the resize and before
    the download -- the 8-bit quantisation of the fp32 prediction, whatever the output depth; `[niqe]` lines, and the result gains 'niqe'
    {index: score} (an image with fewer than 2 blocks is left out with a `skipped` line)."""
    if channels not in (1, 3):
        raise ValueError(f"channels must be 1 or 3 (got {channels!r})")
    if str(out_bits) not in ("auto", "8", "16"):
        raise ValueError(f"out_bits must be 'auto', 8 or 16 (got {out_bits!r})")
    if int(batch_size) < 1:
        raise ValueError(f"batch_size must be >= 1 (got {batch_size!r})")
    S = float(scale if outscale is None else outscale)
    if not (math.isfinite(S) and S > 0):
        raise ValueError(f"outscale must be a positive number (got {outscale!r})")
    device = torch.device(device)
    names = [f"#{i}" for i in range(len(arrays))] if names is None else list(names)
    outputs = {} if sink is None else None
    clipped_total, groups, pixels, scores = 0, [], 0, {}
    i = 0
    while i < len(arrays):
        j = i + 1
        while j < len(arrays) and j - i < int(batch_size) and _key(arrays[j]) == _key(arrays[i]):
            j += 1
        group = [np.asarray(a) for a in arrays[i:j]]
        t0 = time.time()
        stack = np.stack([a[:, :, None] if a.ndim == 2 else a for a in group])
        if stack.ndim != 4 or stack.dtype not in (np.uint8, np.uint16):
            raise ValueError(f"{names[i]}: images are uint8 / uint16 [H,W] or [H,W,ch] arrays (got {stack.dtype} {group[0].shape})")
        n, H, W, ch = stack.shape
        in_bits = 8 * stack.dtype.itemsize
        bits = in_bits if str(out_bits) == "auto" else int(out_bits)
        Ho, Wo = out_size(H, W, S)
        with torch.no_grad():
            raw = _to_device(stack, device)
            x, alpha = ops.image_unpack(raw, channels, want_alpha=True)
            pred = model(x)
            if pred.dim() != 4 or pred.shape[0] != n or pred.shape[1] != channels:
                raise ValueError(f"the model returned {tuple(pred.shape)} for a batch of {tuple(x.shape)}")
            pred = pred.float()
            if tuple(pred.shape[-2:]) != (Ho, Wo):
                pred = _resize(pred, (Ho, Wo))
            if alpha is not None and tuple(alpha.shape[-2:]) != (Ho, Wo):
                alpha = _resize(alpha, (Ho, Wo))
            group_scores = _niqe_group(pred, niqe_params, niqe_crop_border) if niqe_params is not None else None
            counters = torch.zeros(2, dtype=torch.int32, device=device)
            packed = ops.image_pack(pred.contiguous(), alpha, out_chans=ch, bits=bits, counters=counters)
            host = _to_host(packed)
            bad, clipped = (int(v) for v in counters.tolist())
        ms = (time.time() - t0) * 1e3
        if bad:
            raise RuntimeError(f"Pred has non-finite values: count={bad} in {', '.join(names[i:j])}")
        clipped_total += clipped
        groups.append(n)
        for k in range(n):
            mode = modes[i + k] if modes is not None else _mode_label(ch, in_bits)
            log(f"[predict] {names[i + k]} {H}x{W} {mode} {in_bits} -> {Ho}x{Wo} | {ms / n:.1f} ms")
            pixels += Ho * Wo
            if group_scores is not None:
                if isinstance(group_scores[k], float):
                    scores[i + k] = group_scores[k]
                    log(f"[niqe] {names[i + k]} {group_scores[k]:.4f}")
                else:
                    log(f"[niqe] {names[i + k]}: skipped ({group_scores[k]})")
            if sink is None:
                outputs[i + k] = host[k]
            else:
                sink(i + k, host[k])
        if clipped:
            log(f"[clipped] {clipped} values outside [0, 1] in {', '.join(names[i:j])}")
        i = j
    result = {"outputs": None if outputs is None else [outputs[k] for k in range(len(arrays))], "groups": groups, "clipped": clipped_total,
              "pixels": pixels}
    if niqe_params is not None:
        result["niqe"] = scores
    return result


def _niqe_group(pred: torch.Tensor, params: dict, crop_border: int) -> list:
    """NIQE of every prediction of a group -> per image the score (float) or the reason it has none (str)."""
    from .niqe import NIQE_BLOCK, niqe_distance, niqe_moments, niqe_plane_shape, niqe_rows
    n = pred.shape[0]
    try:
        _, _, nbh, nbw = niqe_plane_shape(pred.shape, crop_border)
        if nbh * nbw < 2:
            raise ValueError(f"{pred.shape[2]} x {pred.shape[3]} with a border of {crop_border} holds {nbh * nbw} block of {NIQE_BLOCK} x {NIQE_BLOCK}; "
                             "the score needs at least 2")
    except ValueError as e:
        return [str(e)] * n
    mom1, mom2, _ = niqe_moments(pred.contiguous(), crop_border, NIQE_BLOCK, params["window"])
    rows = niqe_rows(mom1, mom2)
    out = []
    for b in range(n):
        try:
            out.append(niqe_distance(rows[b], params["mu"], params["cov"]))
        except ValueError as e:
            out.append(str(e))
    return out


# ---- the model --------------------------------------------------------------------------------------------------------------------------
def build_real_sr_model(scale_int: int):
    """The M-size real-SR SwinIR of the SwinIR authors' real_sr task: finetune_swinir.build_model's keywords with the 'nearest+conv' head."""
    from .network_swinir import SwinIR
    return SwinIR(upscale=scale_int, in_chans=3, img_size=64, window_size=8, img_range=1.0, depths=[6] * 6, embed_dim=180, num_heads=[6] * 6,
                  mlp_ratio=2, upsampler="nearest+conv", resi_connection="1conv", drop_path_rate=0.0)


def build_model(args, scale_int: int):
    from .finetune_swinir import build_restoration_model, build_sr_model
    if args.task != "sr":
        return build_restoration_model(args.task, args.channels, 0.0, args.window_size)
    if args.upsampler == "nearest+conv":
        return build_real_sr_model(scale_int)
    return build_sr_model(args.arch, scale_int, drop_path_rate=0.0, window_size=args.window_size)


def main(argv=None):
    args = parse_args(argv)
    device = torch.device(args.device) if args.device else torch.device("cuda" if torch.cuda.is_available() else "cpu")
    print("[device]", device, torch.cuda.get_device_name(0) if device.type == "cuda" else "-")
    if device.type != "cuda":
        raise SystemExit(f"--arch {args.arch} runs on the MI355X HIP path only (no CPU fallback)")
    if args.arch == "auto":
        model, scale_int = build_auto_model(args)
    else:
        scale_int = PREDICT_SCALES[args.scale.upper()]
        model = build_model(args, scale_int)
        state, msg = _load_state(args.ckpt, args.param_key)
        model.load_state_dict(state, strict=True)
        print(msg)
    model = model.to(device).eval()
    return run(model, args, scale_int, device)


def build_auto_model(args, log: Callable = print):
    """--arch auto: the model of checkpoint_arch.build_from_state on the state evaluate._load_state returns -> (model, scale).  Sets
    args.channels to the file's in_chans (a scale-1 file thereby takes upscale()'s restoration path); an explicit --scale must be the file's.
    Raises (SrkUnsupported, ValueError, SystemExit) before anything touches the GPU or the output directory."""
    from .checkpoint_arch import build_from_state, format_call, infer_arch
    state, msg = _load_state(args.ckpt, args.param_key)
    log(msg)
    file_scale = int(infer_arch(state).kwargs["upscale"])
    if args.scale != "auto" and PREDICT_SCALES[args.scale.upper()] != file_scale:
        raise SystemExit(f"--scale {args.scale} does not match the checkpoint: {args.ckpt} is a x{file_scale} model (name --scale X{file_scale} or --scale auto)")
    model, spec = build_from_state(state, drop_path_rate=0.0, img_range=getattr(args, "img_range", None))
    log(f"[arch] {spec.arch}: {format_call(spec)}")
    for note in spec.notes:
        log(f"[arch] note: {note}")
    args.channels = int(spec.kwargs["in_chans"])
    return model, file_scale


def run(model, args, scale_int: int, device) -> dict:
    """main() behind the model: files -> upscale -> files."""
    files = discover(args.input)
    if not files:          # a run that processes nothing is an error, not '[done] 0 images' with exit status 0
        raise SystemExit(f"--input {args.input}: no image that PIL can open (see the [skip] lines)")
    out_dir = Path(args.output)
    targets = [output_path(p, out_dir, args.suffix) for p in files]          # every refusal before any work
    if len(set(targets)) != len(targets):
        dup = sorted({str(t) for t in targets if targets.count(t) > 1})
        raise ValueError(f"several inputs share one output name: {dup}")
    out_dir.mkdir(parents=True, exist_ok=True)
    predict = make_predict(model, tile=args.tile, tile_overlap=args.tile_overlap, tile_batch=args.tile_batch, tile_blend=args.tile_blend,
                           self_ensemble=args.self_ensemble)
    t0 = time.time()
    written, clipped, pixels, groups, scores = [], 0, 0, [], {}
    niqe_params = getattr(args, "niqe_params", None)
    # decode and predict one run of equal files at a time: a group is complete before its files are written, a directory is never held whole
    i, ahead = 0, None          # ahead: the decoded file that ended the previous run
    while i < len(files):
        arrays, modes = [], []
        while i + len(arrays) < len(files) and len(arrays) < args.batch_size:
            a, mode = ahead if ahead is not None else load_image(files[i + len(arrays)])
            ahead = None
            if arrays and (_key(a) != _key(arrays[0]) or mode != modes[0]):
                ahead = (a, mode)
                break
            if args.out_bits == "16" and a.ndim == 3 and a.shape[2] != 1:
                raise ValueError(f"{files[i + len(arrays)].name}: --out_bits 16 writes gray files only (PNG through PIL has no 16-bit {mode})")
            arrays.append(a)
            modes.append(mode)
        names = [p.name for p in files[i:i + len(arrays)]]
        base = i

        def sink(k, samples, base=base):
            save_image(samples, targets[base + k])
            written.append(str(targets[base + k]))

        r = upscale(predict, arrays, scale=scale_int, device=device, channels=args.channels, outscale=args.outscale, out_bits=args.out_bits,
                    batch_size=args.batch_size, names=names, modes=modes, sink=sink,
                    **({} if niqe_params is None else {"niqe_params": niqe_params, "niqe_crop_border": args.niqe_crop_border}))
        scores.update({names[k]: v for k, v in r.get("niqe", {}).items()})
        clipped += r["clipped"]
        pixels += r["pixels"]
        groups += r["groups"]
        i += len(arrays)
    dt = time.time() - t0
    result = {"n": len(written), "written": written, "groups": groups, "clipped": clipped, "seconds": dt, "output_mp": pixels / 1e6}
    tail = ""
    if niqe_params is not None:
        mean = float(np.mean(list(scores.values()))) if scores else float("nan")
        result["niqe"] = {"scores": scores, "mean": mean}
        tail = f" | niqe mean {mean:.4f} over {len(scores)}"
    print(f"[done] {len(written)} images | {dt:.1f} s | {pixels / 1e6 / max(dt, 1e-9):.2f} output MP/s{tail}")
    return result


if __name__ == "__main__":
    main()
