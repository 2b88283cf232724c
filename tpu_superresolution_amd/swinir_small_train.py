"""SwinIR training at window sizes 2..7 on MI355X: ``swinir_w16._forward`` with the activations kept, and the backward pass, both as
host-side sequences of C-ABI calls (include/srk.h).  A Swin block with small windows is HAT's HAB without its conv branch
(network_swinir.py:240-279 vs hat_arch.py:281-325); head, reconstruction tail, the MLP, the gradient sink and the autograd node are the
shared ones of ``host_pass.py``, this file holds the block and RSTB bodies.

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

from typing import Dict, Optional

import torch

from . import _lib, host_pass as hp, ops, swinir_w16
from ._lib import SrkUnsupported, check, lib
from .host_pass import GradSink, _full, _gemm, _rows
from .packing import _head_map, _pack_conv_T, _qkv_rows, _rup, cached_pack, pack_attn_T, pack_mlp_T


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
    return cached_pack(m, "wsT", device, lambda P: _fill_transposed(P, m, device))


def _fill_transposed(P: dict, m, device) -> None:
    C_, CP = m.embed_dim, _rup(m.embed_dim, 64)
    HP = _rup(int(C_ * m.mlp_ratio), 64)
    for li, layer in enumerate(m.layers):
        nH = m.heads[li]
        for bi, blk in enumerate(layer.residual_group.blocks):
            pre = f"{li}.{bi}."
            pack_attn_T(P, pre, blk.attn.qkv, blk.attn.proj, nH, C_ // nH, CP, device)
            pack_mlp_T(P, pre, blk.mlp.fc1, blk.mlp.fc2, HP, CP)
        P[f"{li}.WconvT"] = _pack_conv_T(layer.conv.weight, CP, CP)
    hp.pack_tail_T(P, m, CP, device)


# ---- forward, keeping activations ---------------------------------------------------------------------------------------------
def forward_train(m, x: torch.Tensor, P: Dict[str, torch.Tensor], drop: Optional[torch.Tensor]) -> (torch.Tensor, dict):
    """drop: None or fp32 [n_blocks][2][B] DropPath factors (0 or 1 / keep_prob; [.][0] the attention branch, [.][1] the MLP branch)"""
    dev = x.device
    st = torch.cuda.current_stream(dev).cuda_stream
    B, Cin, H0, W0 = x.shape
    ws = m.window_size
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

    _, _, cur = hp.head_forward(m, x, m.patch_embed.norm, st, H, W, TR=TR, keep=S)
    # with a DropPath factor, a 64-row tile of the one-kernel MLP must lie inside one sample
    mlp = hp.mlp_training(st, P, dev, TR, HW, CP, HP, fused=hp.fused_mlp_ok(dev, CP, HP, TR) and (drop is None or HW % 64 == 0))

    def rs(bidx, which):
        return None if drop is None else drop[bidx, which]

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
    S.update(x_last=cur, xnf=xnf, meanf=meanf, rstdf=rstdf)
    return hp.tail_forward(m, P, st, xnf, S["f0"], S["img4"], B, Cin, H0, W0, H, W, keep=S), S


# ---- backward -----------------------------------------------------------------------------------------------------------------------
def backward(m, S: dict, dy: torch.Tensor, hook=None) -> Dict[str, torch.Tensor]:
    """-> {parameter name: gradient} for every parameter of the model.  hook (distributed.ListGradSynchronizer or None): gets the
    gradient tensors of each finished segment (tail, every RSTB, head) so that their all-reduce overlaps the next segment."""
    dev = dy.device
    PT = pack_transposed(m, dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    B, Cin, H0, W0, H, W, T, TR = S["B"], S["Cin"], S["H0"], S["W0"], S["H"], S["W"], S["T"], S["TR"]
    HW = H * W
    ws = m.window_size
    C_, CP = m.embed_dim, _rup(m.embed_dim, 64)
    HP = _rup(int(C_ * m.mlp_ratio), 64)
    f32, b16 = dict(dtype=torch.float32, device=dev), dict(dtype=torch.bfloat16, device=dev)
    L = lib()
    drop = S["drop"]          # [n_blocks][2][B + 1], the last factor 0
    sink = GradSink(m, hook, st, dev, TR, C_, CP, HW, drop)
    conv_wgrad, ln_bwd, put = sink.conv_wgrad, sink.ln_bwd, sink.put
    gfb, gx, gxb = hp.tail_backward(sink, m, S, PT, dy, B, Cin, H0, W0, H, W)
    fused_mlp_bwd_ok = hp.fused_mlp_bwd_ok(dev, CP, HP, T, HW)
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
            g1b, g1b_scaled = hp.mlp_backward(sink, PT, bk, HP, gx2, gxb2, bk["bidx"], fused_mlp_bwd_ok)
            # ---- attention half: x1 = x + f_attn * proj(attention(qkv(norm1(x)))) ----
            g_att = sink.scaled(g1b, bk["bidx"], 0) if not g1b_scaled else g1b
            dao = _full((TR, CA), b16)
            _gemm(st, _lib.LD_ROWS, _lib.EP_BF16, g_att, PT[pre + "WprojT"], TR, CA, CP, lda=CP, outb=dao, ldo=CA)
            sink.lin_wgrad(g_att, bk["ao"], blk.attn.proj, col_map=hm)
            tab = blk.attn.relative_position_bias_table
            # the attention backward: the only window-specific launch of the pass
            need = int(L.srk_win_small_attention_bwd_scratch(B, H, W, ws, nH))
            if attn_scratch is None or attn_scratch.numel() < need:
                attn_scratch = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
            dqkv = _rows(TR, T, 3 * CA, b16)      # rows < T: every element is written by the attention backward
            dtab = ops.zeros_f32(tab.shape, dev)
            check(L.srk_win_small_attention_bwd(bk["qkv"].data_ptr(), 3 * CA, CA, tab.data_ptr(), dao.data_ptr(), CA, dqkv.data_ptr(),
                                                dtab.data_ptr(), attn_scratch.data_ptr(), B, H, W, ws, bk["shift"], nH, bk["scale"], st))
            put(tab, dtab)
            sink.lin_wgrad(dqkv, bk["xn1"], blk.attn.qkv, row_map=qkv_rows)
            sink.flush_wgrads()            # before the kernel below overwrites gxb2 (the fc2 gradient's operand when no DropPath copy was made)
            if CP in (64, 128, 192):      # qkv dgrad with the norm1 backward in its epilogue
                dg, dbt = ops.zeros_f32((C_,), dev), ops.zeros_f32((C_,), dev)
                _gemm(st, _lib.LD_ROWS, _lib.EP_LNBWD, dqkv, PT[pre + "WqkvT"], TR, CP, 3 * CA, lda=3 * CA, outf=gx2, outb=gxb2, ldo=CP,
                      ln=dict(x=bk["x_in"], mean=bk["mean1"], rstd=bk["rstd1"], gamma=blk.norm1.weight, dgamma=dg, dbeta=dbt, C=C_))
                put(blk.norm1.weight, dg), put(blk.norm1.bias, dbt)
            else:
                dxn1 = _full((TR, CP), b16)
                _gemm(st, _lib.LD_ROWS, _lib.EP_BF16, dqkv, PT[pre + "WqkvT"], TR, CP, 3 * CA, lda=3 * CA, outb=dxn1)
                ln_bwd(dxn1, bk["x_in"], bk["mean1"], bk["rstd1"], blk.norm1, gx2, gxb2, accumulate=True)
        # layer skip: d(layer input) = d(body input) + d(layer output)
        check(L.srk_add_f32_bf16(gx.data_ptr(), gx2.data_ptr(), gxb.data_ptr(), TR * CP, st))
        sink.segment_done()

    # ---------------- head: patch_embed.norm, long skip, conv_first ----------------
    hp.head_backward(sink, m, S, m.patch_embed.norm, gxb, gfb)
    return sink.G


class SwinIRSmallFunction(hp.WholeModelFunction):
    """SwinIR at window 2..7 as one autograd node (as HATFunction)"""
    forward_train = staticmethod(lambda m, x, drop: forward_train(m, x, swinir_w16.pack(m, x.device), drop))
    backward_pass = staticmethod(backward)


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
