"""SwinIR with window_size 16 on the HIP path (inference): the 256-token window attention of the HAT path applied to SwinIR's blocks.

The C++ executor (csrc/swinir.hip) is built around 64-token windows (window_size 8, every configuration the reference's scripts
use).  ``SwinIR(window_size=16)`` -- network_swinir.py builds any window size (:640-760) -- runs here instead, as a host-side
sequence of C-ABI calls in the manner of ``hat_arch._hat_forward``: a Swin block with 16 x 16 windows is HAT's HAB without its conv
branch (hat_arch.py:281-325 vs network_swinir.py:240-279), so the kernels are the same:

    check_image_size + normalise (:783-788, :807-809)     srk_img_prep (reflect padding to a multiple of 16)
    conv_first, patch_embed.norm                          srk_stem_conv, srk_layernorm_fwd
    norm1 -> qkv -> (S)W-MSA -> proj + shortcut -> norm2   srk_gemm_ex, srk_win256_attention_fwd (roll / partition / reverse in the addresses,
                                                          arithmetic shift mask, the 961-row bias table indexed in the kernel), next norm fused
    Mlp + shortcut                                        srk_mlp_fused_fwd (width 180) or fc1 + GELU / fc2 + residual GEMMs
    RSTB conv + skip, conv_after_body, head               implicit-GEMM 3x3 convs with residual / LeakyReLU / PixelShuffle / image epilogues

Inference only ('pixelshuffle' and 'pixelshuffledirect' heads, resi_connection '1conv', no ape); a grad-enabled training forward raises.

The same sequence runs ``SwinIR(window_size=2..7)`` (7 is the constructor's default; the SwinIR JPEG-artifact models use it): only the
attention launch differs -- srk_win_small_attention_fwd (csrc/attn_small.hip: windows of <= 49 tokens padded to 32 / 64 with the padded
keys excluded, bias table indexed in the kernel, arithmetic shift mask with shift = ws // 2) -- and the denoising / JPEG head ''
(x + conv_last(res), network_swinir.py:832-836) is covered too.  Token counts are then not always multiples of 64: the token-row buffers
are padded to a multiple of 64 rows, so that the persistent GEMMs and the fused MLP cover every row-wise step.
"""
from __future__ import annotations

from typing import Dict

import torch

from . import _lib, host_pass as hp, ops
from ._lib import SrkUnsupported, check, lib
from .host_pass import _gemm
from .packing import _pack_conv, _pack_vec, _rup, cached_pack, pack_attn, pack_mlp


def unsupported_reason(m) -> str:
    ws = m.window_size
    heads = ("pixelshuffle", "pixelshuffledirect") + (("",) if ws < 8 else ())
    if m.upsampler not in heads:
        return f"window_size={ws} with upsampler={m.upsampler!r}"
    if m.resi_connection != "1conv" or m.ape or not m.patch_norm or not m.qkv_bias or m.patch_size != 1 or m.drop_rate or m.attn_drop_rate:
        return f"window_size={ws} with resi_connection != '1conv', ape, patch_norm=False, qkv_bias=False, patch_size != 1 or dropout"
    if m.embed_dim > 256 or any(m.embed_dim % h or m.embed_dim // h > 32 for h in m.heads):
        return "embed_dim > 256 or head_dim > 32"
    if m.upsampler == "" and m.upscale != 1:
        return "upsampler='' with upscale != 1"
    if m.upsampler == "pixelshuffledirect" and m.upscale ** 2 * m.in_chans > 16:
        return "pixelshuffledirect with upscale^2 * in_chans > 16"
    if any(blk.window_size != ws for layer in m.layers for blk in layer.residual_group.blocks) or (ws < 8 and min(m.patches_resolution) <= ws):
        return f"window_size={ws} with img_size <= {ws} (the blocks fall back to one window of the image size)"
    return ""


def pack(m, device) -> Dict[str, torch.Tensor]:
    return cached_pack(m, "w16", device, lambda P: _fill_pack(P, m, device))


def _fill_pack(P: dict, m, device) -> None:
    C_, CP = m.embed_dim, _rup(m.embed_dim, 64)
    HP = _rup(int(C_ * m.mlp_ratio), 64)
    for li, layer in enumerate(m.layers):
        nH = m.heads[li]
        for bi, blk in enumerate(layer.residual_group.blocks):
            pre = f"{li}.{bi}."
            pack_attn(P, pre, blk.attn.qkv, blk.attn.proj, nH, C_ // nH, CP, device)
            pack_mlp(P, pre, blk.mlp.fc1, blk.mlp.fc2, HP, CP)
        P[f"{li}.Wconv"] = _pack_conv(layer.conv.weight, CP, CP)
        P[f"{li}.bconv"] = _pack_vec(layer.conv.bias, CP)
    hp.pack_tail(P, m, CP, device)


def forward(m, x: torch.Tensor) -> torch.Tensor:
    why = unsupported_reason(m)
    if why:
        raise SrkUnsupported(f"the MI355X HIP path does not cover {why}; no fallback path exists in this package")
    p0 = next(m.parameters())
    if p0.device != x.device:
        raise RuntimeError(f"input is on {x.device} but the model is on {p0.device}")
    _lib.claim_device(x.device.index if x.device.index is not None else torch.cuda.current_device())
    with torch.no_grad(), torch.cuda.device(x.device):
        return _forward(m, x.contiguous().float(), pack(m, x.device))


def _forward(m, x: torch.Tensor, P: Dict[str, torch.Tensor]) -> torch.Tensor:
    dev = x.device
    st = torch.cuda.current_stream(dev).cuda_stream
    B, Cin, H0, W0 = x.shape
    ws = m.window_size
    H, W = _rup(H0, ws), _rup(W0, ws)
    if (H - H0 >= H0) or (W - W0 >= W0):
        raise RuntimeError(f"reflect padding {H0}x{W0} -> {H}x{W} needs pad < size (as torch 'reflect')")
    T, HW = B * H * W, H * W
    C_, CP = m.embed_dim, _rup(m.embed_dim, 64)
    HP = _rup(int(C_ * m.mlp_ratio), 64)
    f32, b16 = dict(dtype=torch.float32, device=dev), dict(dtype=torch.bfloat16, device=dev)
    L = lib()
    # token rows: the persistent GEMMs and the fused MLP cover multiples of 64 rows.  Windows of 8 x 8 / 16 x 16 tokens make T one; with
    # smaller windows (8 x 63 x 63 = 31752 tokens) the row buffers get TR = T rounded up to 64 rows and every row-wise kernel runs on all
    # TR: the padding rows are never read by the attention or the 3x3 convs (their geometry is B x H x W) and never reach the output
    TR = _rup(T, 64)
    img4, f0, cur = hp.head_forward(m, x, m.patch_embed.norm, st, H, W, TR=TR)

    CAmax = max(h * 32 for h in m.heads)
    qkv, ao = torch.empty(TR, 3 * CAmax, **b16), torch.empty(TR, CAmax, **b16)
    if TR > T:
        ao[T:].zero_()
    xn2, hh, xb = torch.empty(TR, CP, **b16), torch.empty(TR, HP, **b16), torch.empty(TR, CP, **b16)
    stat_a, stat_b = torch.empty(TR, **f32), torch.empty(TR, **f32)
    xn_a, xn_b = torch.empty(TR, CP, **b16), torch.empty(TR, CP, **b16)
    mlp = hp.mlp_inference(st, P, TR, CP, HP, hh, fused=hp.fused_mlp_ok(dev, CP, HP, TR))
    ln_fusable = CP in (64, 128, 192)

    def next_norm(norm, dst):
        return dict(out=dst, mean=stat_a, rstd=stat_b, gamma=norm.weight, beta=norm.bias, C=C_) if ln_fusable else None

    xn1 = None
    for li, layer in enumerate(m.layers):
        nH = m.heads[li]
        CA = nH * 32
        scale = float(m.qk_scale or (C_ // nH) ** -0.5)
        layer_in = cur
        blocks = list(layer.residual_group.blocks)
        for bi, blk in enumerate(blocks):
            pre = f"{li}.{bi}."
            if xn1 is None:
                xn1, _, _, _ = ops.layernorm_fwd(cur, blk.norm1.weight, blk.norm1.bias, C_)
            _gemm(st, _lib.LD_ROWS, _lib.EP_BF16, xn1, P[pre + "Wqkv"], TR, 3 * CA, CP, lda=CP, bias=P[pre + "bqkv"], outb=qkv, ldo=3 * CA)
            tab = blk.attn.relative_position_bias_table
            sh = blk.shift_size
            if ws == 16:
                check(L.srk_win256_attention_fwd(qkv.data_ptr(), 3 * CA, CA, tab.data_ptr(), tab.shape[0], ao.data_ptr(), CA, B, H, W, ws, ws, sh,
                                                 sh, nH, scale, 0, st))
            else:
                check(L.srk_win_small_attention_fwd(qkv.data_ptr(), 3 * CA, CA, tab.data_ptr(), ao.data_ptr(), CA, B, H, W, ws, sh, nH, scale, st))
            x1 = torch.empty(TR, CP, **f32)
            _gemm(st, _lib.LD_ROWS, _lib.EP_RES, ao, P[pre + "Wproj"], TR, CP, CA, lda=CA, bias=P[pre + "bproj"], res=cur, outf=x1,
                  xn=dict(out=xn2, mean=stat_a, rstd=stat_b, gamma=blk.norm2.weight, beta=blk.norm2.bias, C=C_))
            nxt = torch.empty(TR, CP, **f32)
            last = bi == len(blocks) - 1
            dst = xn_a if xn1 is not xn_a else xn_b
            nn_ = None if last else next_norm(blocks[bi + 1].norm1, dst)
            mlp(pre, xn2, x1, nxt, out_b=xb if last else None, nn_=nn_)
            cur = nxt
            xn1 = dst if nn_ is not None else None
        nxt = torch.empty(TR, CP, **f32)
        if TR > T:
            nxt[T:].zero_()
        following = m.layers[li + 1].residual_group.blocks[0].norm1 if li + 1 < len(m.layers) else m.norm
        nn_ = next_norm(following, xn_a)
        _gemm(st, _lib.LD_CONV3, _lib.EP_RES, xb, P[f"{li}.Wconv"], T, CP, 9 * CP, conv=(B, H, W, CP), bias=P[f"{li}.bconv"], res=layer_in, outf=nxt,
              xn=nn_)
        cur = nxt
        xn1 = xn_a if nn_ is not None else None

    xnf = xn1 if xn1 is not None else ops.layernorm_fwd(cur, m.norm.weight, m.norm.bias, C_)[0]
    return hp.tail_forward(m, P, st, xnf, f0, img4, B, Cin, H0, W0, H, W)
