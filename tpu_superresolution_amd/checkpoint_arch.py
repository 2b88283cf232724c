"""The checkpoint as the specification: constructor keywords of this package's SwinIR / HAT / DAT read from a state_dict.

    spec = infer_arch(state_dict)                 # ArchSpec(arch, kwargs, notes)
    model, spec = build_from_state(state_dict)    # constructed from spec.kwargs, loaded with strict=True

Only key names and shapes are read, with one exception: DAT's ``split_size`` comes from the CONTENTS of a ``rpe_biases`` buffer (its
coordinate ranges), because (2 s0 - 1)(2 s1 - 1) rows do not say which side is which.  A uniform ``module.`` prefix is stripped first.
Two things are not in a file and follow a stated convention, recorded in ``ArchSpec.notes``:

    img_range     255 for SwinIR's scale-1 head at window 7 (the published JPEG-artifact files, data_cli.RESTORATION_TASKS['car']),
                  1.0 otherwise; build_from_state(img_range=R) overrides it
    conv_scale    HAT's 0.01, the value of every published HAT file

``build_from_state`` asks the constructed module for its own ``_unsupported_reason()`` (for SwinIR at a window other than 8: the
host-run path's) and raises SrkUnsupported with that reason before anything touches the GPU.  A state_dict of none of the three
families, or one whose shapes contradict each other, raises ValueError naming the keys involved.
"""
from __future__ import annotations

import math
import re
from collections import namedtuple
from typing import Dict, List, Optional, Tuple

import torch

from ._lib import SrkUnsupported

ArchSpec = namedtuple("ArchSpec", ["arch", "kwargs", "notes"])

MARKERS = {"hat": ("relative_position_index_SA",), "dat": ("before_RG.1.weight",),
           "swinir": ("patch_embed.norm.weight", "layers.0.residual_group.blocks.0.attn.relative_position_index")}
HAT_CONV_SCALE = 0.01
NUM_FEAT = 64          # width of the upsampling heads: a constant of the three constructors


def strip_module_prefix(state: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """Keys without a uniform ``module.`` prefix (DataParallel files); a prefix on only some of the keys is left alone."""
    if state and all(k.startswith("module.") for k in state):
        return {k[len("module."):]: v for k, v in state.items()}
    return dict(state)


def _shape(sd, key) -> Tuple[int, ...]:
    if key not in sd:
        raise ValueError(f"the state_dict has no key {key!r}, which the inference reads")
    return tuple(sd[key].shape)


def _isqrt_exact(n: int, what: str) -> int:
    r = math.isqrt(int(n))
    if n <= 0 or r * r != n:
        raise ValueError(f"{what}: {n} is not a square")
    return r


def _block_counts(sd, fmt=r"layers\.(\d+)\.residual_group\.blocks\.(\d+)\.") -> List[int]:
    """blocks per group, from the key names; groups and blocks must be numbered 0..n-1 without gaps"""
    seen: Dict[int, set] = {}
    rx = re.compile(fmt)
    for k in sd:
        m = rx.match(k)
        if m:
            seen.setdefault(int(m.group(1)), set()).add(int(m.group(2)))
    if not seen or sorted(seen) != list(range(len(seen))):
        raise ValueError(f"layers.N.*: the groups are not numbered 0..n-1 (found {sorted(seen)})")
    counts = []
    for g in range(len(seen)):
        if sorted(seen[g]) != list(range(len(seen[g]))):
            raise ValueError(f"layers.{g}.residual_group.blocks.N.*: the blocks are not numbered 0..n-1 (found {sorted(seen[g])})")
        counts.append(len(seen[g]))
    return counts


def _same(values: List, keys: str):
    """the one value every stage agrees on"""
    if len(set(values)) != 1:
        raise ValueError(f"{keys}: the stages disagree ({sorted(set(values))})")
    return values[0]


def _ratio(n: int, C: int) -> float:
    """hidden / C as the constructors take it: int(C * ratio) must give n back"""
    r = n / C
    r = int(r) if r == int(r) else r
    if int(C * r) != n:
        raise ValueError(f"hidden width {n} is not int(embed_dim * ratio) for embed_dim {C}")
    return r


def _divisor(C: int, n: int, key: str) -> int:
    """r with C // r == n (compress_ratio, squeeze_factor)"""
    if n <= 0 or C // n <= 0 or C // (C // n) != n:
        raise ValueError(f"{key}: {n} output channels are not embed_dim // r for embed_dim {C}")
    return C // n


def _resi(sd, prefix="layers.0.conv") -> Optional[str]:
    if f"{prefix}.weight" in sd:
        return "1conv"
    if f"{prefix}.0.weight" in sd and f"{prefix}.4.weight" in sd:
        return "3conv"
    return None


def _head(sd, C: int, in_chans: int, notes: List[str]) -> Tuple[str, int]:
    """(upsampler, upscale) from the head's key set"""
    if "conv_up1.weight" in sd:
        return "nearest+conv", 4 if "conv_up2.weight" in sd else 2
    if "conv_before_upsample.0.weight" in sd and "upsample.0.weight" in sd:
        stages = sorted(int(m.group(1)) for m in (re.fullmatch(r"upsample\.(\d+)\.weight", k) for k in sd) if m)
        scale = 1
        for k in stages:
            co, ci = _shape(sd, f"upsample.{k}.weight")[:2]
            if ci != NUM_FEAT or co % NUM_FEAT:
                raise ValueError(f"upsample.{k}.weight {_shape(sd, f'upsample.{k}.weight')}: a stage of the 'pixelshuffle' head maps {NUM_FEAT} to r^2 * {NUM_FEAT} channels")
            scale *= _isqrt_exact(co // NUM_FEAT, f"upsample.{k}.weight: r^2 = {co} / {NUM_FEAT}")
        if stages != list(range(0, 2 * len(stages), 2)):
            raise ValueError(f"upsample.N.weight: the stages of the 'pixelshuffle' head sit at 0, 2, 4, ... (found {stages})")
        return "pixelshuffle", scale
    if "upsample.0.weight" in sd and "conv_last.weight" not in sd:
        co, ci = _shape(sd, "upsample.0.weight")[:2]
        if ci != C or co % in_chans:
            raise ValueError(f"upsample.0.weight {_shape(sd, 'upsample.0.weight')}: the 'pixelshuffledirect' head maps embed_dim = {C} to upscale^2 * in_chans "
                             f"channels (in_chans = {in_chans} by conv_first.weight)")
        return "pixelshuffledirect", _isqrt_exact(co // in_chans, f"upsample.0.weight: upscale^2 = {co} / {in_chans}")
    if "conv_last.weight" in sd and _shape(sd, "conv_last.weight")[:2] == (in_chans, C):
        return "", 1
    raise ValueError("the head is none of 'nearest+conv' (conv_up1), 'pixelshuffle' (conv_before_upsample.0 + upsample.*), 'pixelshuffledirect' "
                     "(upsample.0 without conv_last) and '' (conv_last reading embed_dim channels)")


def _stem(sd) -> Tuple[int, int]:
    s = _shape(sd, "conv_first.weight")
    if len(s) != 4 or s[2:] != (3, 3):
        raise ValueError(f"conv_first.weight {s}: a 3 x 3 convolution [embed_dim][in_chans][3][3] is expected")
    return s[1], s[0]


def _window_body(sd, C: int, rpi_key: Optional[str], table_fmt: str, notes: List[str]):
    """depths, num_heads, window_size, mlp_ratio of a SwinIR / HAT body"""
    depths = _block_counts(sd)
    heads = []
    for g in range(len(depths)):
        hs = []
        for j in range(depths[g]):
            key = table_fmt.format(g=g, j=j)
            t = _shape(sd, key)
            if len(t) != 2:
                raise ValueError(f"{key} {t}: a table [(2 ws - 1)^2][num_heads] is expected")
            hs.append(t[1])
        h = _same(hs, f"layers.{g}.*.relative_position_bias_table")
        if h <= 0 or C % h:
            raise ValueError(f"layers.{g}.*.relative_position_bias_table: {h} heads do not divide embed_dim = {C} (conv_first.weight)")
        heads.append(h)
    if rpi_key is None:
        rpi_key = "layers.0.residual_group.blocks.0.attn.relative_position_index"
    r = _shape(sd, rpi_key)
    if len(r) != 2 or r[0] != r[1]:
        raise ValueError(f"{rpi_key} {r}: a square table ws^2 x ws^2 is expected")
    ws = _isqrt_exact(r[0], f"{rpi_key}: ws^2")
    t0 = _shape(sd, table_fmt.format(g=0, j=0))
    if t0[0] != (2 * ws - 1) ** 2:
        raise ValueError(f"{table_fmt.format(g=0, j=0)} has {t0[0]} rows, {rpi_key} says window {ws}: (2 ws - 1)^2 = {(2 * ws - 1) ** 2}")
    hid = [_shape(sd, f"layers.{g}.residual_group.blocks.{j}.mlp.fc1.weight") for g in range(len(depths)) for j in range(depths[g])]
    if any(len(h) != 2 or h[1] != C for h in hid):
        raise ValueError(f"layers.*.mlp.fc1.weight: the input width is not embed_dim = {C} (conv_first.weight)")
    mlp_ratio = _ratio(_same([h[0] for h in hid], "layers.*.mlp.fc1.weight"), C)
    return depths, heads, ws, mlp_ratio


def _img_size_from_mask(sd, ws: int) -> Optional[int]:
    sizes = []
    for k, v in sd.items():
        if k.endswith(".attn_mask") and v is not None:
            s = tuple(v.shape)
            if len(s) != 3 or s[1] != ws * ws or s[2] != ws * ws:
                raise ValueError(f"{k} {s}: a mask [nW][ws^2][ws^2] with ws = {ws} (relative_position_index) is expected")
            sizes.append(ws * _isqrt_exact(s[0], f"{k}: nW"))
    return _same(sizes, "layers.*.attn_mask") if sizes else None


def _infer_swinir(sd, notes) -> dict:
    in_chans, C = _stem(sd)
    depths, heads, ws, mlp_ratio = _window_body(sd, C, None, "layers.{g}.residual_group.blocks.{j}.attn.relative_position_bias_table", notes)
    resi = _resi(sd)
    if resi is None:
        raise ValueError("layers.0.conv: neither layers.0.conv.weight ('1conv') nor layers.0.conv.0.weight + layers.0.conv.4.weight ('3conv')")
    upsampler, upscale = _head(sd, C, in_chans, notes)
    img_size = _img_size_from_mask(sd, ws)
    ape = "absolute_pos_embed" in sd
    if ape:
        n = _shape(sd, "absolute_pos_embed")[1]
        side = _isqrt_exact(n, "absolute_pos_embed: img_size^2")
        if img_size is not None and side != img_size:
            raise ValueError(f"absolute_pos_embed has {n} rows, the attn_mask buffers say img_size {img_size}")
        img_size = side
    if img_size is None:
        img_size = 64
        notes.append("img_size=64: the file has no attn_mask buffer (img_size only sizes those buffers)")
    if upscale == 1 and upsampler == "" and ws == 7:
        img_range = 255.0
        notes.append("img_range=255: convention for the scale-1 head at window 7 (the published JPEG-artifact files); not in a state_dict")
    else:
        img_range = 1.0
        notes.append("img_range=1.0: convention (255 only for the scale-1 head at window 7); not in a state_dict")
    return dict(img_size=img_size, in_chans=in_chans, embed_dim=C, depths=depths, num_heads=heads, window_size=ws, mlp_ratio=mlp_ratio, ape=ape,
                upscale=upscale, img_range=img_range, upsampler=upsampler, resi_connection=resi)


def _infer_hat(sd, notes) -> dict:
    in_chans, C = _stem(sd)
    depths, heads, ws, mlp_ratio = _window_body(sd, C, "relative_position_index_SA", "layers.{g}.residual_group.blocks.{j}.attn.relative_position_bias_table", notes)
    ratios = []
    for g in range(len(depths)):
        key = f"layers.{g}.residual_group.overlap_attn.relative_position_bias_table"
        t = _shape(sd, key)
        side = _isqrt_exact(t[0], f"{key}: (ws + ows - 1)^2")
        extra = side + 1 - 2 * ws          # int(ratio * ws)
        if extra < 0 or t[1] != heads[g]:
            raise ValueError(f"{key} {t}: (ws + ows - 1)^2 rows with ows >= ws = {ws} and {heads[g]} heads are expected")
        ratios.append(extra)
    extra = _same(ratios, "layers.*.overlap_attn.relative_position_bias_table")
    overlap_ratio = extra / ws
    if "relative_position_index_OCA" in sd and _shape(sd, "relative_position_index_OCA") != (ws * ws, (ws + extra) ** 2):
        raise ValueError(f"relative_position_index_OCA {_shape(sd, 'relative_position_index_OCA')} contradicts the overlap tables: ({ws * ws}, {(ws + extra) ** 2}) expected")
    cab = "layers.{g}.residual_group.blocks.{j}.conv_block.cab."
    blocks = [(g, j) for g in range(len(depths)) for j in range(depths[g])]
    compress = _divisor(C, _same([_shape(sd, cab.format(g=g, j=j) + "0.weight")[0] for g, j in blocks], "layers.*.conv_block.cab.0.weight"),
                        "layers.*.conv_block.cab.0.weight")
    squeeze = _divisor(C, _same([_shape(sd, cab.format(g=g, j=j) + "3.attention.1.weight")[0] for g, j in blocks], "layers.*.conv_block.cab.3.attention.1.weight"),
                       "layers.*.conv_block.cab.3.attention.1.weight")
    if "layers.0.conv.weight" not in sd or "conv_after_body.weight" not in sd:
        raise ValueError("layers.0.conv.weight / conv_after_body.weight: HAT files have the '1conv' residual connection")
    if "conv_before_upsample.0.weight" in sd:
        upsampler, upscale = _head(sd, C, in_chans, notes)
        if upsampler != "pixelshuffle":
            raise ValueError(f"the head's keys say {upsampler!r}; HAT has the 'pixelshuffle' head only")
    else:
        upsampler, upscale = "", 1
    ape = "absolute_pos_embed" in sd
    img_size = _isqrt_exact(_shape(sd, "absolute_pos_embed")[1], "absolute_pos_embed: img_size^2") if ape else 64
    if not ape:
        notes.append("img_size=64: HAT files carry no buffer that depends on it")
    notes.append(f"conv_scale={HAT_CONV_SCALE}: the published value; not in a state_dict")
    notes.append("img_range=1.0: convention; not in a state_dict")
    return dict(img_size=img_size, in_chans=in_chans, embed_dim=C, depths=depths, num_heads=heads, window_size=ws, compress_ratio=compress,
                squeeze_factor=squeeze, conv_scale=HAT_CONV_SCALE, overlap_ratio=overlap_ratio, mlp_ratio=mlp_ratio, ape=ape, upscale=upscale,
                img_range=1.0, upsampler=upsampler, resi_connection="1conv")


def _infer_dat(sd, notes) -> dict:
    in_chans, C = _stem(sd)
    depth = _block_counts(sd, r"layers\.(\d+)\.blocks\.(\d+)\.")
    heads = []
    for g, d in enumerate(depth):
        if d < 2:
            raise ValueError(f"layers.{g}.blocks: num_heads is read from attn.temperature of a channel-attention block (an odd block); the group has {d} block")
        h = _same([_shape(sd, f"layers.{g}.blocks.{j}.attn.temperature")[0] for j in range(1, d, 2)], f"layers.{g}.blocks.*.attn.temperature")
        if h <= 0 or C % h:
            raise ValueError(f"layers.{g}.blocks.1.attn.temperature: {h} heads do not divide embed_dim = {C} (conv_first.weight)")
        heads.append(h)
    key = "layers.0.blocks.0.attn.attns.0.rpe_biases"
    if key not in sd:
        raise ValueError(f"the state_dict has no key {key!r}, which split_size is read from")
    rpe = sd[key]
    if rpe.dim() != 2 or rpe.shape[1] != 2:
        raise ValueError(f"{key} {tuple(rpe.shape)}: a coordinate table [(2 s0 - 1)(2 s1 - 1)][2] is expected")
    s0, s1 = int(rpe[:, 0].max().item()) + 1, int(rpe[:, 1].max().item()) + 1
    if (2 * s0 - 1) * (2 * s1 - 1) != rpe.shape[0] or int(rpe[:, 0].min().item()) != 1 - s0 or int(rpe[:, 1].min().item()) != 1 - s1:
        raise ValueError(f"{key}: coordinates span {s0} x {s1}, which needs {(2 * s0 - 1) * (2 * s1 - 1)} rows; the table has {rpe.shape[0]}")
    k1 = "layers.0.blocks.0.attn.attns.1.rpe_biases"
    if k1 in sd and (int(sd[k1][:, 0].max().item()) + 1, int(sd[k1][:, 1].max().item()) + 1) != (s1, s0):
        raise ValueError(f"{key} says split_size [{s0}, {s1}]; {k1} is not its transpose")
    hid = [_shape(sd, f"layers.{g}.blocks.{j}.ffn.fc1.weight") for g, d in enumerate(depth) for j in range(d)]
    if any(len(h) != 2 or h[1] != C for h in hid):
        raise ValueError(f"layers.*.ffn.fc1.weight: the input width is not embed_dim = {C} (conv_first.weight)")
    expansion = _ratio(_same([h[0] for h in hid], "layers.*.ffn.fc1.weight"), C)
    resi = _resi(sd)
    if resi is None:
        raise ValueError("layers.0.conv: neither layers.0.conv.weight ('1conv') nor layers.0.conv.0.weight + layers.0.conv.4.weight ('3conv')")
    upsampler, upscale = _head(sd, C, in_chans, notes)
    if upsampler not in ("pixelshuffle", "pixelshuffledirect"):
        raise ValueError(f"the head's keys say {upsampler!r}; DAT has the 'pixelshuffle' and 'pixelshuffledirect' heads")
    sizes = []
    for k, v in sd.items():
        if k.endswith(".attn_mask_0") and v is not None:
            s = tuple(v.shape)
            if len(s) != 3 or s[1] != s0 * s1:
                raise ValueError(f"{k} {s}: a mask [nW][{s0 * s1}][{s0 * s1}] is expected for split_size [{s0}, {s1}]")
            sizes.append(_isqrt_exact(s[0] * s0 * s1, f"{k}: nW * s0 * s1 = img_size^2"))
    if sizes:
        img_size = _same(sizes, "layers.*.attn.attn_mask_0")
    else:
        img_size = 64
        notes.append("img_size=64: the file has no shift-mask buffer")
    notes.append("img_range=1.0: convention; not in a state_dict")
    return dict(img_size=img_size, in_chans=in_chans, embed_dim=C, split_size=[s0, s1], depth=depth, num_heads=heads, expansion_factor=expansion,
                upscale=upscale, img_range=1.0, resi_connection=resi, upsampler=upsampler)


def family(sd) -> str:
    if all(k in sd for k in MARKERS["hat"]):
        return "hat"
    if all(k in sd for k in MARKERS["dat"]):
        return "dat"
    if all(k in sd for k in MARKERS["swinir"]):
        return "swinir"
    looked = "; ".join(f"{a}: {' + '.join(ks)}" for a, ks in MARKERS.items())
    raise ValueError(f"the state_dict is none of SwinIR, HAT and DAT: no marker key found (looked for {looked}); it has {len(sd)} keys"
                     + (f", the first is {next(iter(sd))!r}" if sd else ""))


def infer_arch(state_dict) -> ArchSpec:
    sd = strip_module_prefix(state_dict)
    arch = family(sd)
    notes: List[str] = []
    kwargs = {"swinir": _infer_swinir, "hat": _infer_hat, "dat": _infer_dat}[arch](sd, notes)
    return ArchSpec(arch, kwargs, notes)


def constructor(arch: str):
    if arch == "swinir":
        from .network_swinir import SwinIR
        return SwinIR
    if arch == "hat":
        from .hat_arch import HAT
        return HAT
    if arch == "dat":
        from .dat_arch import DAT
        return DAT
    raise ValueError(f"arch must be 'swinir', 'hat' or 'dat' (got {arch!r})")


def unsupported_reason(arch: str, model) -> Optional[str]:
    """What the HIP path does not cover of this model, as the package's own checks state it, or None."""
    why = model._unsupported_reason()
    if not why and arch == "swinir" and model.window_size != 8:          # windows 2..7 and 16 run on the host-orchestrated path
        from . import swinir_w16
        why = swinir_w16.unsupported_reason(model)
    if not why and arch == "swinir" and model.window_size == 8:          # the engine's own limits (srk_swinir_plan_create)
        if model.upsampler == "pixelshuffledirect" and model.upscale ** 2 * model.in_chans > 64:
            why = "pixelshuffledirect with upscale^2 * in_chans > 64"
        elif model.embed_dim > 256 or len(model.depths) > 16 or any(model.embed_dim // h > 32 for h in model.heads):
            why = "embed_dim > 256, more than 16 groups or head_dim > 32"
    return why or None


def format_call(spec: ArchSpec) -> str:
    """The inferred constructor call as one line."""
    name = {"swinir": "SwinIR", "hat": "HAT", "dat": "DAT"}[spec.arch]
    return f"{name}({', '.join(f'{k}={v!r}' for k, v in spec.kwargs.items())})"


def build_from_state(state_dict, drop_path_rate: float = 0.0, img_range: Optional[float] = None):
    """-> (model, spec): the model of the inferred keywords with the state loaded strictly.  img_range overrides the convention.
    Raises SrkUnsupported with the package's own reason when the HIP path does not cover the model, before anything touches the GPU."""
    sd = strip_module_prefix(state_dict)
    spec = infer_arch(sd)
    if img_range is not None:
        if not (math.isfinite(float(img_range)) and float(img_range) > 0):
            raise ValueError(f"img_range must be a positive number (got {img_range!r})")
        kwargs = dict(spec.kwargs, img_range=float(img_range))
        notes = [n for n in spec.notes if not n.startswith("img_range=")] + [f"img_range={float(img_range)}: given by the caller"]
        spec = ArchSpec(spec.arch, kwargs, notes)
    model = constructor(spec.arch)(drop_path_rate=drop_path_rate, **spec.kwargs)
    why = unsupported_reason(spec.arch, model)
    if why:
        raise SrkUnsupported(f"{format_call(spec)}: the MI355X HIP path does not cover {why}; no fallback path exists in this package")
    model.load_state_dict(sd, strict=True)
    return model, spec
