"""SwinIR training at window sizes 2..7 on MI355X: ``swinir_w16._forward`` with the activations kept, and the backward pass, both as
host-side sequences of C-ABI calls (include/srk.h) -- written after ``hat_train.py``: a Swin block with small windows is HAT's HAB
without its conv branch (network_swinir.py:240-279 vs hat_arch.py:281-325).

    tail      'pixelshuffle': HAT's tail (conv_last, conv + PixelShuffle stages, conv_before_upsample + LeakyReLU');
              'pixelshuffledirect' / '': srk_img_grad_prep (r = upscale / 1) and the small-conv gradients on CP input channels (for ''
              the added input image takes no gradient); then conv_after_body and the final LayerNorm
    RSTB      conv dgrad / wgrad, skip add at the layer input
    block     fc2 dgrad * GELU'(u) -> fc1 dgrad -> norm2 backward (one kernel where srk_mlp_fused_bwd applies) ; proj dgrad ->
              srk_win_small_attention_bwd (csrc/attn_small_bwd.hip: the ONLY window-specific launch) -> one launch for the four weight
              gradients -> qkv dgrad with the norm1 backward in its epilogue
    head      patch_embed.norm backward + long skip, conv_first weight gradient

Token rows.  T = B H W is usually not a multiple of 64 (8 * 49^2 = 19208): the row buffers have TR = round_up(T, 64) rows and the
row-wise kernels (GEMMs, fused MLP, LayerNorm, weight gradients) run over all TR.  In the forward the padding rows hold
LayerNorm(0) = beta and what follows from it; nothing reads them but the same rows of the next row-wise kernel.  In the backward every
operand of a weight / bias / gamma / beta reduction has EXACTLY ZERO padding rows: the kernels that address tokens through B x H x W
(conv dgrads, attention backward) never write rows >= T, so the host zeroes those rows of their outputs, and zero rows stay zero
through the bias-free dgrads and the LayerNorm backward.  The per-sample DropPath factors are indexed row / (H W), which is B on a
padding row: the factor rows carry a (B + 1)-th entry equal to 0.
"""
from __future__ import annotations

import ctypes as C
import math
import os
from typing import Dict, Optional

import torch
import torch.nn as nn

from . import _lib, ops, swinir_w16
from ._lib import SrkUnsupported, check, lib
from .hat_arch import _gemm, _head_map, _pack_conv_T, _pack_linear, _ps_map, _ptr, _qkv_rows, _rup, batched_pack
from .hat_train import _unpack_conv, _unpack_linear

_POISON = os.environ.get("SRK_DBG_POISON") == "1"


def unsupported_reason(m) -> str:
    """why ``enable_small_window_training`` refuses this model ('' = covered)"""
    ws = m.window_size
    if not 2 <= ws <= 7:
        return f"window_size={ws}: small-window training covers window sizes 2..7 (window 8 trains through the engine as it is)"
    if m.use_checkpoint:
        return f"window_size={ws} with use_checkpoint=True"
    return swinir_w16.unsupported_reason(m)


def is_enabled(model) -> bool:
    return bool(getattr(model, "_small_window_training", False))


# ---- packed operands of the backward pass (transposed copies for the dgrads) ---------------------------------------------------
def pack_transposed(m, device) -> Dict[str, torch.Tensor]:
    ver = sum(p._version for p in m.parameters())
    if getattr(m, "_wsT_packed", None) is not None and m._wsT_version == ver and m._wsT_device == device:
        return m._wsT_packed
    C_, CP = m.embed_dim, _rup(m.embed_dim, 64)
    HP = _rup(int(C_ * m.mlp_ratio), 64)
    P: Dict[str, torch.Tensor] = {}
    with torch.no_grad(), batched_pack() as pk:
        for li, layer in enumerate(m.layers):
            nH = m.heads[li]
            dh, CA = C_ // nH, nH * 32
            hm = _head_map(nH, dh, device)
            qkv_rows = _qkv_rows(nH, dh, device)
            for bi, blk in enumerate(layer.residual_group.blocks):
                pre = f"{li}.{bi}."
                P[pre + "WqkvT"] = _pack_linear(blk.attn.qkv.weight.t(), CP, 3 * CA, col_map=qkv_rows)        # [c][3 CA]
                P[pre + "WprojT"] = _pack_linear(blk.attn.proj.weight.t(), CA, CP, row_map=hm)                # [ca][c]
                P[pre + "W1T"] = _pack_linear(blk.mlp.fc1.weight.t(), CP, HP)
                P[pre + "W2T"] = _pack_linear(blk.mlp.fc2.weight.t(), HP, CP)
            P[f"{li}.WconvT"] = _pack_conv_T(layer.conv.weight, CP, CP)
        P["WcabT"] = _pack_conv_T(m.conv_after_body.weight, CP, CP)
        if m.upsampler == "pixelshuffle":
            P["WbeforeT"] = _pack_conv_T(m.conv_before_upsample[0].weight, CP, 64)
            k = 0
            for mod in m.upsample:
                if isinstance(mod, nn.Conv2d):
                    r = int(round(math.sqrt(mod.weight.shape[0] // 64)))
                    pm = _ps_map(mod.weight.shape[0], r, 64, device)
                    P[f"WupT{k}"] = _pack_conv_T(mod.weight, 64, mod.weight.shape[0], col_map=pm)
                    k += 1
        pk.resolve(P)
    m._wsT_packed, m._wsT_version, m._wsT_device = P, ver, device
    return P


def _rows(TR: int, T: int, cols: int, kw: dict) -> torch.Tensor:
    """[TR][cols] buffer whose rows < T a kernel writes in full (NaN-filled first under SRK_DBG_POISON) and whose padding rows are 0"""
    t = torch.empty(TR, cols, **kw) if not _POISON else torch.full((TR, cols), float("nan"), **kw)
    if TR > T:
        t[T:].zero_()
    return t


def _full(shape, kw: dict) -> torch.Tensor:
    """buffer that one kernel writes in full"""
    return torch.empty(shape, **kw) if not _POISON else torch.full(tuple(shape) if not isinstance(shape, int) else (shape,), float("nan"), **kw)


# ---- forward, keeping activations ---------------------------------------------------------------------------------------------
def forward_train(m, x: torch.Tensor, P: Dict[str, torch.Tensor], drop: Optional[torch.Tensor]) -> (torch.Tensor, dict):
    """drop: None or fp32 [n_blocks][2][B] DropPath factors (0 or 1 / keep_prob; [.][0] the attention branch, [.][1] the MLP branch)"""
    dev = x.device
    st = torch.cuda.current_stream(dev).cuda_stream
    B, Cin, H0, W0 = x.shape
    ws, s = m.window_size, m.upscale
    H, W = _rup(H0, ws), _rup(W0, ws)
    if (H - H0 >= H0) or (W - W0 >= W0):
        raise RuntimeError(f"reflect padding {H0}x{W0} -> {H}x{W} needs pad < size (as torch 'reflect')")
    T, HW = B * H * W, H * W
    TR = _rup(T, 64)
    C_, CP = m.embed_dim, _rup(m.embed_dim, 64)
    HP = _rup(int(C_ * m.mlp_ratio), 64)
    f32, b16 = dict(dtype=torch.float32, device=dev), dict(dtype=torch.bfloat16, device=dev)
    L = lib()
    if drop is not None:          # a (B + 1)-th factor, 0, for the padding rows (row / HW == B)
        drop = torch.cat([drop.to(torch.float32), torch.zeros(drop.shape[0], 2, 1, **f32)], dim=2).contiguous()
    S: dict = dict(B=B, Cin=Cin, H0=H0, W0=W0, H=H, W=W, T=T, TR=TR, blocks=[], layers=[], drop=drop)

    mean3 = (C.c_float * 3)(*(m.mean.flatten().tolist() if m.in_chans == 3 else [0.0, 0.0, 0.0]))
    img4 = _full((T, 4), f32)
    check(L.srk_img_prep(x.data_ptr(), img4.data_ptr(), B, Cin, H0, W0, H, W, float(m.img_range), C.byref(mean3), st))
    f0 = _rows(TR, T, CP, f32)
    check(L.srk_stem_conv(img4.data_ptr(), m.conv_first.weight.data_ptr(), m.conv_first.bias.data_ptr(), f0.data_ptr(), B, H, W, Cin, C_, CP, st))
    _, cur, mean_pe, rstd_pe = ops.layernorm_fwd(f0, m.patch_embed.norm.weight, m.patch_embed.norm.bias, C_, out_bf16=False, out_f32=True)
    S.update(img4=img4, f0=f0, mean_pe=mean_pe, rstd_pe=rstd_pe)
    fused_mlp_ok = (CP == 192 and HP == 384 and TR >= 64 * torch.cuda.get_device_properties(dev).multi_processor_count)

    def rs(bidx, which):
        return None if drop is None else drop[bidx, which]

    def mlp(pre, xn_in, x_res, rowscale):
        """-> (out fp32, out bf16, u, h): out = x_res + f * fc2(gelu(fc1(xn_in)))"""
        out, out_b = _full((TR, CP), f32), _full((TR, CP), b16)
        u, h = _full((TR, HP), b16), _full((TR, HP), b16)
        if fused_mlp_ok and (rowscale is None or HW % 64 == 0):      # with a DropPath factor, a 64-row tile must lie inside one sample
            check(L.srk_mlp_fused_fwd_train(xn_in.data_ptr(), P[pre + "W1"].data_ptr(), P[pre + "b1"].data_ptr(), P[pre + "W2"].data_ptr(),
                                            P[pre + "b2"].data_ptr(), x_res.data_ptr(), out.data_ptr(), out_b.data_ptr(), u.data_ptr(),
                                            h.data_ptr(), None, None, None, None, None, 0, _ptr(rowscale), HW, TR, st))
        else:
            _gemm(st, _lib.LD_ROWS, _lib.EP_GELU, xn_in, P[pre + "W1"], TR, HP, CP, lda=CP, bias=P[pre + "b1"], outb=u, outb2=h)
            _gemm(st, _lib.LD_ROWS, _lib.EP_RES, h, P[pre + "W2"], TR, CP, HP, lda=HP, bias=P[pre + "b2"], res=x_res, outf=out, outb=out_b,
                  rowscale=rowscale, rows_per_sample=HW)
        return out, out_b, u, h

    bidx = 0
    for li, layer in enumerate(m.layers):
        nH = m.heads[li]
        CA = nH * 32
        scale = float(m.qk_scale or (C_ // nH) ** -0.5)
        layer_in = cur
        xb = None
        for bi, blk in enumerate(layer.residual_group.blocks):
            pre = f"{li}.{bi}."
            xn1, _, mean1, rstd1 = ops.layernorm_fwd(cur, blk.norm1.weight, blk.norm1.bias, C_)
            qkv = _full((TR, 3 * CA), b16)
            _gemm(st, _lib.LD_ROWS, _lib.EP_BF16, xn1, P[pre + "Wqkv"], TR, 3 * CA, CP, lda=CP, bias=P[pre + "bqkv"], outb=qkv, ldo=3 * CA)
            tab = blk.attn.relative_position_bias_table
            sh = blk.shift_size
            ao = _rows(TR, T, CA, b16)
            check(L.srk_win_small_attention_fwd(qkv.data_ptr(), 3 * CA, CA, tab.data_ptr(), ao.data_ptr(), CA, B, H, W, ws, sh, nH, scale, st))
            x1 = _full((TR, CP), f32)
            _gemm(st, _lib.LD_ROWS, _lib.EP_RES, ao, P[pre + "Wproj"], TR, CP, CA, lda=CA, bias=P[pre + "bproj"], res=cur, outf=x1,
                  rowscale=rs(bidx, 0), rows_per_sample=HW)
            xn2, _, mean2, rstd2 = ops.layernorm_fwd(x1, blk.norm2.weight, blk.norm2.bias, C_)
            nxt, xb, u, h = mlp(pre, xn2, x1, rs(bidx, 1))
            S["blocks"].append(dict(li=li, bi=bi, pre=pre, blk=blk, nH=nH, CA=CA, scale=scale, shift=sh, x_in=cur, xn1=xn1, mean1=mean1,
                                    rstd1=rstd1, qkv=qkv, ao=ao, x1=x1, xn2=xn2, mean2=mean2, rstd2=rstd2, u=u, h=h, bidx=bidx))
            cur = nxt
            bidx += 1
        nxt = _rows(TR, T, CP, f32)
        _gemm(st, _lib.LD_CONV3, _lib.EP_RES, xb, P[f"{li}.Wconv"], T, CP, 9 * CP, conv=(B, H, W, CP), bias=P[f"{li}.bconv"], res=layer_in, outf=nxt)
        S["layers"].append(dict(li=li, xb=xb, n_blocks=len(layer.residual_group.blocks)))
        cur = nxt

    xnf, _, meanf, rstdf = ops.layernorm_fwd(cur, m.norm.weight, m.norm.bias, C_)
    fb = _full((T, CP), b16)
    _gemm(st, _lib.LD_CONV3, _lib.EP_RES_BF16, xnf, P["Wcab"], T, CP, 9 * CP, conv=(B, H, W, CP), bias=P["bcab"], res=f0, outb=fb)
    S.update(x_last=cur, xnf=xnf, meanf=meanf, rstdf=rstdf, fb=fb, ups=[])
    y = _full((B, Cin, H0 * s, W0 * s), f32)
    mean4 = (m.mean.flatten().tolist() if m.in_chans == 3 else [0.0, 0.0, 0.0]) + [0.0]
    img = dict(inv_range=1.0 / float(m.img_range), Cimg=Cin, Hc=H0 * s, Wc=W0 * s, mean=mean4)
    if m.upsampler == "pixelshuffle":
        t1 = _full((T, 64), b16)
        _gemm(st, _lib.LD_CONV3, _lib.EP_LRELU, fb, P["Wbefore"], T, 64, 9 * CP, conv=(B, H, W, CP), bias=P["bbefore"], outb=t1, scale=0.01)
        S["t1"] = t1
        src, h_, w_, k = t1, H, W, 0
        while f"Wup{k}" in P:
            r = int(P[f"rup{k}"])
            N = P[f"Wup{k}"].shape[0]
            up = _full((B * h_ * r * w_ * r, 64), b16)
            _gemm(st, _lib.LD_CONV3, _lib.EP_PS, src, P[f"Wup{k}"], B * h_ * w_, N, 9 * 64, conv=(B, h_, w_, 64), bias=P[f"bup{k}"], outb=up, r=r, Cs=64,
                  ldo=N)
            S["ups"].append(dict(src=src, out=up, h=h_, w=w_, r=r, N=N))
            src, h_, w_, k = up, h_ * r, w_ * r, k + 1
        _gemm(st, _lib.LD_CONV3, _lib.EP_IMG, src, P["Wlast"], B * h_ * w_, 16, 9 * 64, conv=(B, h_, w_, 64), bias=P["blast"], outf=y, img=img)
        S.update(hr_h=h_, hr_w=w_)
    else:       # UpsampleOneStep (:594-615), or '' with upscale 1: x + conv_last(res), x = the normalised, padded input (:832-836)
        _gemm(st, _lib.LD_CONV3, _lib.EP_PS_IMG, fb, P["Wdirect"], T, 16, 9 * CP, conv=(B, H, W, CP), bias=P["bdirect"], outf=y, img=dict(img), r=s,
              res=img4 if m.upsampler == "" else None)
    return y, S


# ---- backward -----------------------------------------------------------------------------------------------------------------------
def backward(m, S: dict, dy: torch.Tensor, hook=None) -> Dict[str, torch.Tensor]:
    """-> {parameter name: gradient} for every parameter of the model.  hook (distributed.ListGradSynchronizer or None): gets the
    gradient tensors of each finished segment (tail, every RSTB, head) so that their all-reduce overlaps the next segment."""
    dev = dy.device
    P = swinir_w16.pack(m, dev)
    PT = pack_transposed(m, dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    B, Cin, H0, W0, H, W, T, TR = S["B"], S["Cin"], S["H0"], S["W0"], S["H"], S["W"], S["T"], S["TR"]
    HW = H * W
    ws, s = m.window_size, m.upscale
    C_, CP = m.embed_dim, _rup(m.embed_dim, 64)
    HP = _rup(int(C_ * m.mlp_ratio), 64)
    f32, b16 = dict(dtype=torch.float32, device=dev), dict(dtype=torch.bfloat16, device=dev)
    L = lib()
    drop = S["drop"]          # [n_blocks][2][B + 1], the last factor 0
    G: Dict[str, torch.Tensor] = {}
    names = {id(p): n for n, p in m.named_parameters()}
    handed = set()

    def segment_done():
        if hook is not None:
            fresh = [k for k in G if k not in handed]
            handed.update(fresh)
            hook.segment_done([G[k] for k in fresh])

    def pname(p):
        return names[id(p)]

    pending = []          # the block's linear weight gradients: queued, then ONE launch for all four (flush_wgrads)

    def lin_wgrad(y, x, lin, row_map=None, col_map=None):
        pending.append((y, x, lin, row_map, col_map))

    def flush_wgrads():
        if not pending:
            return
        for (y, x, lin, row_map, col_map), (dw, db) in zip(pending, ops.linear_wgrad_multi_bf16([(q[0], q[1]) for q in pending])):
            N, K = lin.weight.shape
            G[pname(lin.weight)] = _unpack_linear(dw, N, K, row_map, col_map)
            if lin.bias is not None:
                G[pname(lin.bias)] = (db[:N] if row_map is None else db[row_map]).contiguous()
        pending.clear()

    def conv_wgrad(dyb, xb, conv, Bc, Hc, Wc, CinP, NP, r=1, row_map=None):
        dw = ops.zeros_f32((NP, 9 * CinP), dev)
        db = ops.zeros_f32((NP,), dev)
        ops._bind_wgrad_workspace(dev)
        if r == 1:
            check(L.srk_conv3x3_wgrad_bf16(dyb.data_ptr(), xb.data_ptr(), dw.data_ptr(), db.data_ptr(), Bc, Hc, Wc, CinP, NP, st))
        else:
            check(L.srk_conv3x3_wgrad_ps_bf16(dyb.data_ptr(), xb.data_ptr(), dw.data_ptr(), db.data_ptr(), Bc, Hc, Wc, CinP, NP, r, 64, st))
        Cout, Cin_ = conv.weight.shape[:2]
        G[pname(conv.weight)] = _unpack_conv(dw, Cout, Cin_, CinP, row_map)
        G[pname(conv.bias)] = (db[:Cout] if row_map is None else db[row_map]).contiguous()

    def ln_bwd(dyb, x, mean, rstd, norm, gx, gxb, accumulate):
        dg, dbt = ops.zeros_f32((C_,), dev), ops.zeros_f32((C_,), dev)
        check(L.srk_layernorm_bwd(dyb.data_ptr(), x.data_ptr(), mean.data_ptr(), rstd.data_ptr(), norm.weight.data_ptr(), gx.data_ptr(),
                                  _ptr(gxb), dg.data_ptr(), dbt.data_ptr(), TR, C_, CP, 1 if accumulate else 0, st))
        G[pname(norm.weight)], G[pname(norm.bias)] = dg, dbt

    def scaled(gb, bidx, which):
        """bf16 gradient copy entering a branch whose output was scaled by a DropPath factor (padding rows: factor 0)"""
        if drop is None:
            return gb
        out = _full((TR, CP), b16)
        check(L.srk_rowscale_bf16(gb.data_ptr(), out.data_ptr(), drop[bidx, which].data_ptr(), TR, HW, CP, st))
        return out

    # ---------------- reconstruction tail: -> gfb, the gradient of conv_after_body's output + long skip (bf16 [T][CP]) ----------------
    if m.upsampler == "pixelshuffle":
        hs, wsz = S["hr_h"], S["hr_w"]
        gyimg = _full((B * hs * wsz, 4), f32)
        check(L.srk_img_grad_prep(dy.data_ptr(), gyimg.data_ptr(), B, Cin, H0 * s, W0 * s, hs, wsz, 1, 4, 1.0 / float(m.img_range), st))
        last_in = S["ups"][-1]["out"] if S["ups"] else S["t1"]
        dwl, dbl = ops.zeros_f32(m.conv_last.weight.shape, dev), ops.zeros_f32(m.conv_last.bias.shape, dev)
        check(L.srk_smallconv_wgrad(last_in.data_ptr(), gyimg.data_ptr(), dwl.data_ptr(), dbl.data_ptr(), B, hs, wsz, 64, 64, Cin, 4, st))
        G[pname(m.conv_last.weight)], G[pname(m.conv_last.bias)] = dwl, dbl
        gcur = _full((B * hs * wsz, 64), b16)
        check(L.srk_smallconv_dgrad(gyimg.data_ptr(), m.conv_last.weight.data_ptr(), gcur.data_ptr(), B, hs, wsz, 64, 64, Cin, 4, st))
        up_convs = [mod for mod in m.upsample if isinstance(mod, nn.Conv2d)]
        for k in range(len(S["ups"]) - 1, -1, -1):
            u = S["ups"][k]
            r, N, h_, w_ = u["r"], u["N"], u["h"], u["w"]
            pm = _ps_map(N, r, 64, dev)
            conv_wgrad(gcur, u["src"], up_convs[k], B, h_, w_, 64, N, r=r, row_map=pm)
            gprev = _full((B * h_ * w_, 64), b16)
            if k == 0:     # through the LeakyReLU(0.01) of conv_before_upsample
                _gemm(st, _lib.LD_CONV3_PS, _lib.EP_DLRELU, gcur, PT[f"WupT{k}"], B * h_ * w_, 64, 9 * N, conv=(B, h_, w_, N), r=r, Cs=64, outb=gprev,
                      aux=S["t1"], scale=0.01, ldo=64)
            else:
                _gemm(st, _lib.LD_CONV3_PS, _lib.EP_BF16, gcur, PT[f"WupT{k}"], B * h_ * w_, 64, 9 * N, conv=(B, h_, w_, N), r=r, Cs=64, outb=gprev, ldo=64)
            gcur = gprev
        gt1 = gcur
        conv_wgrad(gt1, S["fb"], m.conv_before_upsample[0], B, H, W, CP, 64)
        gfb = _full((T, CP), b16)
        _gemm(st, _lib.LD_CONV3, _lib.EP_BF16, gt1, PT["WbeforeT"], T, CP, 9 * 64, conv=(B, H, W, 64), outb=gfb)
    else:
        # UpsampleOneStep's conv (+ PixelShuffle) or conv_last of the '' head: embed_dim -> Co = in_chans * r^2 channels, fp32 parameters
        direct = m.upsample[0] if m.upsampler == "pixelshuffledirect" else m.conv_last
        r = s if m.upsampler == "pixelshuffledirect" else 1
        Co = Cin * r * r
        CoP = 4 if Co <= 4 else 16
        gyimg = _full((T, CoP), f32)
        check(L.srk_img_grad_prep(dy.data_ptr(), gyimg.data_ptr(), B, Cin, H0 * s, W0 * s, H, W, r, CoP, 1.0 / float(m.img_range), st))
        dwl, dbl = ops.zeros_f32(direct.weight.shape, dev), ops.zeros_f32(direct.bias.shape, dev)
        check(L.srk_smallconv_wgrad(S["fb"].data_ptr(), gyimg.data_ptr(), dwl.data_ptr(), dbl.data_ptr(), B, H, W, C_, CP, Co, CoP, st))
        G[pname(direct.weight)], G[pname(direct.bias)] = dwl, dbl
        gfb = _full((T, CP), b16)
        check(L.srk_smallconv_dgrad(gyimg.data_ptr(), direct.weight.data_ptr(), gfb.data_ptr(), B, H, W, C_, CP, Co, CoP, st))
    conv_wgrad(gfb, S["xnf"], m.conv_after_body, B, H, W, CP, CP)
    dxn = _rows(TR, T, CP, b16)
    _gemm(st, _lib.LD_CONV3, _lib.EP_BF16, gfb, PT["WcabT"], T, CP, 9 * CP, conv=(B, H, W, CP), outb=dxn)
    gx = _full((TR, CP), f32)        # gradient of the current layer's OUTPUT (later: of its input); padding rows 0
    gxb = _full((TR, CP), b16)
    ln_bwd(dxn, S["x_last"], S["meanf"], S["rstdf"], m.norm, gx, gxb, accumulate=False)
    segment_done()

    opt = C.c_int()
    check(L.srk_get_option(b"mlp_bwd_fused", C.byref(opt)))
    fused_mlp_bwd_ok = (opt.value != 0 and CP == 192 and HP == 384 and T % 64 == 0 and HW % 64 == 0 and
                        T >= 64 * torch.cuda.get_device_properties(dev).multi_processor_count)
    # ---------------- layers, last to first ----------------
    blocks = S["blocks"]
    pos = len(blocks)
    attn_scratch = None
    for lay in reversed(S["layers"]):
        li = lay["li"]
        layer = m.layers[li]
        conv_wgrad(gxb, lay["xb"], layer.conv, B, H, W, CP, CP)
        gx2 = _rows(TR, T, CP, f32)       # gradient stream through the layer's body
        gxb2 = _rows(TR, T, CP, b16)
        _gemm(st, _lib.LD_CONV3, _lib.EP_F32_BF16, gxb, PT[f"{li}.WconvT"], T, CP, 9 * CP, conv=(B, H, W, CP), outf=gx2, outb=gxb2)
        for _ in range(lay["n_blocks"]):
            pos -= 1
            bk = blocks[pos]
            pre, blk, nH, CA = bk["pre"], bk["blk"], bk["nH"], bk["CA"]
            hm = _head_map(nH, C_ // nH, dev)
            qkv_rows = _qkv_rows(nH, C_ // nH, dev)
            # ---- MLP half: x2 = x1 + f_mlp * fc2(gelu(fc1(norm2(x1)))) ----
            g_mlp = scaled(gxb2, bk["bidx"], 1)
            du = _full((TR, HP), b16)
            g1b = _full((TR, CP), b16)
            g1b_scaled = False
            if fused_mlp_bwd_ok:
                dg, dbt = ops.zeros_f32((C_,), dev), ops.zeros_f32((C_,), dev)
                rsc = drop[bk["bidx"], 0] if drop is not None else None
                check(L.srk_mlp_fused_bwd(g_mlp.data_ptr(), PT[pre + "W2T"].data_ptr(), bk["u"].data_ptr(), du.data_ptr(), PT[pre + "W1T"].data_ptr(),
                                          bk["x1"].data_ptr(), bk["mean2"].data_ptr(), bk["rstd2"].data_ptr(), blk.norm2.weight.data_ptr(),
                                          gx2.data_ptr(), g1b.data_ptr(), _ptr(rsc), HW, dg.data_ptr(), dbt.data_ptr(), C_, TR, st))
                G[pname(blk.norm2.weight)], G[pname(blk.norm2.bias)] = dg, dbt
                g1b_scaled = True
            else:
                _gemm(st, _lib.LD_ROWS, _lib.EP_DGELU, g_mlp, PT[pre + "W2T"], TR, HP, CP, lda=CP, aux=bk["u"], outb=du, ldo=HP)
            lin_wgrad(g_mlp, bk["h"], blk.mlp.fc2)
            lin_wgrad(du, bk["xn2"], blk.mlp.fc1)
            if not fused_mlp_bwd_ok:
                dxn2 = _full((TR, CP), b16)
                _gemm(st, _lib.LD_ROWS, _lib.EP_BF16, du, PT[pre + "W1T"], TR, CP, HP, lda=HP, outb=dxn2)
                ln_bwd(dxn2, bk["x1"], bk["mean2"], bk["rstd2"], blk.norm2, gx2, g1b, accumulate=True)      # gx2 = d x1 (fp32), g1b its bf16 copy
            # ---- attention half: x1 = x + f_attn * proj(attention(qkv(norm1(x)))) ----
            g_att = scaled(g1b, bk["bidx"], 0) if not g1b_scaled else g1b
            dao = _full((TR, CA), b16)
            _gemm(st, _lib.LD_ROWS, _lib.EP_BF16, g_att, PT[pre + "WprojT"], TR, CA, CP, lda=CP, outb=dao, ldo=CA)
            lin_wgrad(g_att, bk["ao"], blk.attn.proj, col_map=hm)
            tab = blk.attn.relative_position_bias_table
            # the attention backward: the only window-specific launch of the pass
            need = int(L.srk_win_small_attention_bwd_scratch(B, H, W, ws, nH))
            if attn_scratch is None or attn_scratch.numel() < need:
                attn_scratch = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
            dqkv = _rows(TR, T, 3 * CA, b16)      # rows < T: every element is written by the attention backward
            dtab = ops.zeros_f32(tab.shape, dev)
            check(L.srk_win_small_attention_bwd(bk["qkv"].data_ptr(), 3 * CA, CA, tab.data_ptr(), dao.data_ptr(), CA, dqkv.data_ptr(),
                                                dtab.data_ptr(), attn_scratch.data_ptr(), B, H, W, ws, bk["shift"], nH, bk["scale"], st))
            G[pname(tab)] = dtab
            lin_wgrad(dqkv, bk["xn1"], blk.attn.qkv, row_map=qkv_rows)
            flush_wgrads()            # before the kernel below overwrites gxb2 (the fc2 gradient's operand when no DropPath copy was made)
            if CP in (64, 128, 192):      # qkv dgrad with the norm1 backward in its epilogue
                dg, dbt = ops.zeros_f32((C_,), dev), ops.zeros_f32((C_,), dev)
                _gemm(st, _lib.LD_ROWS, _lib.EP_LNBWD, dqkv, PT[pre + "WqkvT"], TR, CP, 3 * CA, lda=3 * CA, outf=gx2, outb=gxb2, ldo=CP,
                      ln=dict(x=bk["x_in"], mean=bk["mean1"], rstd=bk["rstd1"], gamma=blk.norm1.weight, dgamma=dg, dbeta=dbt, C=C_))
                G[pname(blk.norm1.weight)], G[pname(blk.norm1.bias)] = dg, dbt
            else:
                dxn1 = _full((TR, CP), b16)
                _gemm(st, _lib.LD_ROWS, _lib.EP_BF16, dqkv, PT[pre + "WqkvT"], TR, CP, 3 * CA, lda=3 * CA, outb=dxn1)
                ln_bwd(dxn1, bk["x_in"], bk["mean1"], bk["rstd1"], blk.norm1, gx2, gxb2, accumulate=True)
        # layer skip: d(layer input) = d(body input) + d(layer output)
        check(L.srk_add_f32_bf16(gx.data_ptr(), gx2.data_ptr(), gxb.data_ptr(), TR * CP, st))
        segment_done()

    # ---------------- head: patch_embed.norm, long skip, conv_first ----------------
    gf = _full((TR, CP), f32)
    ln_bwd(gxb, S["f0"], S["mean_pe"], S["rstd_pe"], m.patch_embed.norm, gf, None, accumulate=False)
    check(L.srk_add_bf16_into_f32(gf.data_ptr(), gfb.data_ptr(), T * CP, st))
    dwf, dbf = ops.zeros_f32(m.conv_first.weight.shape, dev), ops.zeros_f32(m.conv_first.bias.shape, dev)
    check(L.srk_stem_wgrad(S["img4"].data_ptr(), gf.data_ptr(), dwf.data_ptr(), dbf.data_ptr(), B, H, W, Cin, C_, CP, st))
    G[pname(m.conv_first.weight)], G[pname(m.conv_first.bias)] = dwf, dbf
    segment_done()
    if hook is not None:
        hook.finish()
    return G


class SwinIRSmallFunction(torch.autograd.Function):
    """One autograd node for the whole model (as HATFunction): forward keeps the activations, backward returns every parameter's
    gradient.  The input image gets no gradient."""

    @staticmethod
    def forward(ctx, model, x, drop, *params):
        with torch.cuda.device(x.device):
            y, saved = forward_train(model, x.contiguous().float(), swinir_w16.pack(model, x.device), drop)
        ctx.model, ctx.saved = model, saved
        return y

    @staticmethod
    def backward(ctx, dy):
        model = ctx.model
        arena = model.__dict__.setdefault("_zero_arena", ops.ZeroArena())      # the pass's zeroed accumulators: one buffer, one fill
        with torch.cuda.device(dy.device), ops.arena_scope(arena, dy.device):
            G = backward(model, ctx.saved, dy.contiguous().float(), hook=getattr(model, "grad_sync", None))
        ctx.saved = None
        grads = []
        for n, p in model.named_parameters():
            g = G.get(n)
            grads.append(None if g is None else g.reshape(p.shape).to(p.dtype))
        return (None, None, None, *grads)


def train_forward(model, x: torch.Tensor) -> torch.Tensor:
    """the grad-enabled, train-mode forward of an enabled model (SwinIR.forward dispatches here)"""
    why = unsupported_reason(model)
    if why:
        raise SrkUnsupported(f"the MI355X HIP path does not cover {why}; no fallback path exists in this package")
    p0 = next(model.parameters())
    if p0.device != x.device:
        raise RuntimeError(f"input is on {x.device} but the model is on {p0.device}")
    _lib.claim_device(x.device.index if x.device.index is not None else torch.cuda.current_device())
    drop = getattr(model, "_drop_override", None)          # training.GraphedTrainStep draws the factors outside its graph
    if drop is None:
        drop = model.draw_drop_path(x.shape[0], x.device)
    return SwinIRSmallFunction.apply(model, x, drop, *[p for _, p in model.named_parameters()])
