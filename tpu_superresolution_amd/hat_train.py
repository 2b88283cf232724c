"""HAT training on MI355X: the forward that keeps what the backward needs, and the backward pass, both as host-side sequences of
C-ABI calls (include/srk.h) -- the training-mode counterpart of ``hat_arch._hat_forward``.  Head, reconstruction tail, the Swin MLP, the
gradient sink and the autograd node are the shared ones of ``host_pass.py``; this file holds the HAB / OCAB / RHAG bodies.

Reference: hat_arch.py:281-325 (HAB.forward), :403-439 (OCAB.forward), :600-620 (RHAG), :943-987 (HAT.forward); autograd of those
is what ``hat_backward`` restates by hand, block by block in reverse:

    tail      conv_last (fp32 small-conv gradients), conv + PixelShuffle stages (weight gradient on the shuffled gradient, dgrad
              through the pixel-shuffled loader), conv_before_upsample (+ LeakyReLU'), conv_after_body, final LayerNorm
    RHAG      conv dgrad / wgrad, RSTB-style skip add at the layer input
    OCAB/HAB  fc2 dgrad * GELU'(u) -> fc1 dgrad -> LayerNorm backward (adds into the fp32 gradient stream) ; CAB: channel gate,
              both 3x3 convs ; proj dgrad -> 256-query window attention backward (csrc/attn256_bwd.hip) -> qkv dgrad (+ the conv
              branch's gradient) -> LayerNorm backward
    head      patch_embed.norm backward + long skip, conv_first weight gradient

DropPath (drop_path_rate > 0 in train mode, hat_arch.py:258 / :321-325) is data: per-block, per-sample factors 0 or 1 / keep
that scale the attention and MLP branch in the forward epilogues and the bf16 gradient copies that enter those branches.
The weight gradients come out of the kernels in the packed (padded / permuted) layouts and are scattered back into the
parameters' shapes with index maps (host plumbing on parameter-sized tensors).
"""
from __future__ import annotations

from typing import Dict, Optional

import torch

from . import _lib, host_pass as hp, ops
from ._lib import check, lib
from .host_pass import GradSink, _full, _gemm
from .packing import _head_map, _pack_conv_T, _qkv_rows, _rup, cached_pack, pack_attn_T, pack_mlp_T


# ---- packed operands of the backward pass (transposed copies for the dgrads) ---------------------------------------------------
def pack_transposed(m, device) -> Dict[str, torch.Tensor]:
    return cached_pack(m, "T", device, lambda P: _fill_transposed(P, m, device))


def _fill_transposed(P: dict, m, device) -> None:
    C_, CP = m.embed_dim, _rup(m.embed_dim, 64)
    HP = _rup(int(C_ * m.mlp_ratio), 64)
    for li, layer in enumerate(m.layers):
        nH = m.heads[li]
        dh = C_ // nH
        for bi, blk in enumerate(layer.residual_group.blocks):
            pre = f"{li}.{bi}."
            pack_attn_T(P, pre, blk.attn.qkv, blk.attn.proj, nH, dh, CP, device)
            pack_mlp_T(P, pre, blk.mlp.fc1, blk.mlp.fc2, HP, CP)
            cab = blk.conv_block.cab
            P[pre + "Wc0T"] = _pack_conv_T(cab[0].weight, CP, 64)
            P[pre + "Wc2T"] = _pack_conv_T(cab[2].weight, 64, CP)
        oc = layer.residual_group.overlap_attn
        pack_attn_T(P, f"{li}.oca.", oc.qkv, oc.proj, nH, dh, CP, device)
        pack_mlp_T(P, f"{li}.oca.", oc.mlp.fc1, oc.mlp.fc2, HP, CP)
        P[f"{li}.WconvT"] = _pack_conv_T(layer.conv.weight, CP, CP)
    hp.pack_tail_T(P, m, CP, device)


# ---- forward, keeping activations ---------------------------------------------------------------------------------------------
def hat_forward_train(m, x: torch.Tensor, P: Dict[str, torch.Tensor], drop: Optional[torch.Tensor]) -> (torch.Tensor, dict):
    """drop: None or fp32 [n_blocks][B] DropPath factors (0 or 1 / keep_prob) shared by a HAB's attention and MLP branch
    (hat_arch.py:321-325 draws them independently; here each branch gets its own row: [n_blocks][2][B])."""
    dev = x.device
    st = torch.cuda.current_stream(dev).cuda_stream
    B, Cin, H0, W0 = x.shape
    ws = m.window_size
    H, W = _rup(H0, ws), _rup(W0, ws)
    if (H - H0 >= H0) or (W - W0 >= W0):
        raise RuntimeError(f"reflect padding {H0}x{W0} -> {H}x{W} needs pad < size (as torch 'reflect')")
    T, HW = B * H * W, H * W
    C_, CP = m.embed_dim, _rup(m.embed_dim, 64)
    hid = int(C_ * m.mlp_ratio)
    HP = _rup(hid, 64)
    f32 = dict(dtype=torch.float32, device=dev)
    b16 = dict(dtype=torch.bfloat16, device=dev)
    L = lib()
    S: dict = dict(B=B, Cin=Cin, H0=H0, W0=W0, H=H, W=W, T=T, blocks=[], layers=[], drop=drop)

    _, _, cur = hp.head_forward(m, x, m.patch_embed.norm, st, H, W, keep=S)

    gate_ws = torch.empty(max(1, int(L.srk_channel_gate_workspace(B, HW, CP))), dtype=torch.uint8, device=dev)
    mlp = hp.mlp_training(st, P, dev, T, HW, CP, HP, fused=hp.fused_mlp_ok(dev, CP, HP, T) and T % 64 == 0)

    def rs(bidx, which):
        return None if drop is None else drop[bidx, which]

    bidx = 0
    for li, layer in enumerate(m.layers):
        nH = m.heads[li]
        CA = nH * 32
        scale = float(m.qk_scale or (C_ // nH) ** -0.5)
        layer_in = cur
        oc = layer.residual_group.overlap_attn
        for bi, blk in enumerate(layer.residual_group.blocks):
            pre = f"{li}.{bi}."
            xn1, _, mean1, rstd1 = ops.layernorm_fwd(cur, blk.norm1.weight, blk.norm1.bias, C_)
            qkv = torch.empty(T, 3 * CA, **b16)
            _gemm(st, _lib.LD_ROWS, _lib.EP_BF16, xn1, P[pre + "Wqkv"], T, 3 * CA, CP, lda=CP, bias=P[pre + "bqkv"], outb=qkv, ldo=3 * CA)
            tab = blk.attn.relative_position_bias_table
            sh = blk.shift_size
            ao = torch.empty(T, CA, **b16)
            check(L.srk_win256_attention_fwd(qkv.data_ptr(), 3 * CA, CA, tab.data_ptr(), tab.shape[0], ao.data_ptr(), CA, B, H, W, ws, ws,
                                             sh, sh, nH, scale, 0, st))
            x1 = torch.empty(T, CP, **f32)
            _gemm(st, _lib.LD_ROWS, _lib.EP_RES, ao, P[pre + "Wproj"], T, CP, CA, lda=CA, bias=P[pre + "bproj"], res=cur, outf=x1,
                  rowscale=rs(bidx, 0), rows_per_sample=HW)
            u1, c1 = torch.empty(T, 64, **b16), torch.empty(T, 64, **b16)
            _gemm(st, _lib.LD_CONV3, _lib.EP_GELU, xn1, P[pre + "Wc0"], T, 64, 9 * CP, conv=(B, H, W, CP), bias=P[pre + "bc0"], outb=u1, outb2=c1)
            c2 = torch.empty(T, CP, **b16)
            _gemm(st, _lib.LD_CONV3, _lib.EP_BF16, c1, P[pre + "Wc2"], T, CP, 9 * 64, conv=(B, H, W, 64), bias=P[pre + "bc2"], outb=c2)
            gate = torch.empty(B, CP, **f32)
            Sq = P[pre + "ca_w1"].shape[0]
            check(L.srk_channel_gate(c2.data_ptr(), gate_ws.data_ptr(), P[pre + "ca_w1"].data_ptr(), P[pre + "ca_b1"].data_ptr(),
                                     P[pre + "ca_w2"].data_ptr(), P[pre + "ca_b2"].data_ptr(), float(blk.conv_scale), gate.data_ptr(), B, HW,
                                     C_, CP, Sq, st))
            check(L.srk_cab_add_ln(x1.data_ptr(), c2.data_ptr(), gate.data_ptr(), None, None, None, T, HW, C_, CP, st))     # x1 += conv * gate
            xn2, _, mean2, rstd2 = ops.layernorm_fwd(x1, blk.norm2.weight, blk.norm2.bias, C_)
            nxt, _, u, h = mlp(pre, xn2, x1, rs(bidx, 1))
            S["blocks"].append(dict(kind="hab", li=li, bi=bi, pre=pre, blk=blk, nH=nH, CA=CA, scale=scale, shift=sh, x_in=cur, xn1=xn1,
                                    mean1=mean1, rstd1=rstd1, qkv=qkv, ao=ao, x1=x1, u1=u1, c1=c1, c2=c2, gate=gate, xn2=xn2, mean2=mean2,
                                    rstd2=rstd2, u=u, h=h, bidx=bidx))
            cur = nxt
            bidx += 1
        pre = f"{li}.oca."
        xn1, _, mean1, rstd1 = ops.layernorm_fwd(cur, oc.norm1.weight, oc.norm1.bias, C_)
        qkv = torch.empty(T, 3 * CA, **b16)
        _gemm(st, _lib.LD_ROWS, _lib.EP_BF16, xn1, P[pre + "Wqkv"], T, 3 * CA, CP, lda=CP, bias=P[pre + "bqkv"], outb=qkv, ldo=3 * CA)
        tab = oc.relative_position_bias_table
        ao = torch.empty(T, CA, **b16)
        check(L.srk_win256_attention_fwd(qkv.data_ptr(), 3 * CA, CA, tab.data_ptr(), tab.shape[0], ao.data_ptr(), CA, B, H, W, ws, ws, 0, 0, nH,
                                         scale, oc.overlap_win_size - ws, st))
        x1 = torch.empty(T, CP, **f32)
        _gemm(st, _lib.LD_ROWS, _lib.EP_RES, ao, P[pre + "Wproj"], T, CP, CA, lda=CA, bias=P[pre + "bproj"], res=cur, outf=x1)
        xn2, _, mean2, rstd2 = ops.layernorm_fwd(x1, oc.norm2.weight, oc.norm2.bias, C_)
        x2, xb, u, h = mlp(pre, xn2, x1, None)
        S["blocks"].append(dict(kind="ocab", li=li, pre=pre, blk=oc, nH=nH, CA=CA, scale=scale, x_in=cur, xn1=xn1, mean1=mean1, rstd1=rstd1,
                                qkv=qkv, ao=ao, x1=x1, xn2=xn2, mean2=mean2, rstd2=rstd2, u=u, h=h))
        nxt = torch.empty(T, CP, **f32)
        _gemm(st, _lib.LD_CONV3, _lib.EP_RES, xb, P[f"{li}.Wconv"], T, CP, 9 * CP, conv=(B, H, W, CP), bias=P[f"{li}.bconv"], res=layer_in, outf=nxt)
        S["layers"].append(dict(li=li, xb=xb, n_blocks=len(layer.residual_group.blocks) + 1))
        cur = nxt

    xnf, _, meanf, rstdf = ops.layernorm_fwd(cur, m.norm.weight, m.norm.bias, C_)
    S.update(x_last=cur, xnf=xnf, meanf=meanf, rstdf=rstdf)
    return hp.tail_forward(m, P, st, xnf, S["f0"], S["img4"], B, Cin, H0, W0, H, W, keep=S), S


# ---- backward -----------------------------------------------------------------------------------------------------------------------
def hat_backward(m, S: dict, dy: torch.Tensor, hook=None) -> Dict[str, torch.Tensor]:
    """-> {parameter name: gradient} for every parameter of the model.  hook (distributed.ListGradSynchronizer or None): gets the
    gradient tensors of each finished segment (tail, every RHAG, head) so that their all-reduce overlaps the next segment."""
    P = m._pack(dy.device)
    PT = pack_transposed(m, dy.device)
    dev = dy.device
    st = torch.cuda.current_stream(dev).cuda_stream
    B, Cin, H0, W0, H, W, T = S["B"], S["Cin"], S["H0"], S["W0"], S["H"], S["W"], S["T"]
    HW = H * W
    C_, CP = m.embed_dim, _rup(m.embed_dim, 64)
    hid = int(C_ * m.mlp_ratio)
    HP = _rup(hid, 64)
    f32 = dict(dtype=torch.float32, device=dev)
    b16 = dict(dtype=torch.bfloat16, device=dev)
    L = lib()
    drop = S["drop"]
    sink = GradSink(m, hook, st, dev, T, C_, CP, HW, drop)
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
        gx2 = torch.empty(T, CP, **f32)       # gradient stream through the layer's body
        gxb2 = torch.empty(T, CP, **b16)
        _gemm(st, _lib.LD_CONV3, _lib.EP_F32_BF16, gxb, PT[f"{li}.WconvT"], T, CP, 9 * CP, conv=(B, H, W, CP), outf=gx2, outb=gxb2)
        for _ in range(lay["n_blocks"]):
            pos -= 1
            bk = blocks[pos]
            pre, blk, nH, CA = bk["pre"], bk["blk"], bk["nH"], bk["CA"]
            hab = bk["kind"] == "hab"
            hm = _head_map(nH, C_ // nH, dev)
            qkv_rows = _qkv_rows(nH, C_ // nH, dev)
            bidx = bk["bidx"] if hab else None          # the OCAB has no DropPath
            g1b, g1b_scaled = hp.mlp_backward(sink, PT, bk, HP, gx2, gxb2, bidx, fused_mlp_bwd_ok)
            dxc = None
            if hab:
                # ---- CAB: x1 += conv2(gelu(conv1(xn1))) * gate ----
                cab = blk.conv_block.cab
                att = cab[3].attention
                Sq = att[1].weight.shape[0]
                dw1, db1 = ops.zeros_f32((Sq, C_), dev), ops.zeros_f32((Sq,), dev)
                dw2, db2 = ops.zeros_f32((C_, Sq), dev), ops.zeros_f32((C_,), dev)
                dmean = torch.empty(B, CP, **f32)
                dc2 = torch.empty(T, CP, **b16)
                wsb = torch.empty(max(1, int(L.srk_cab_bwd_workspace(B, HW, CP))), dtype=torch.uint8, device=dev)
                check(L.srk_cab_bwd(bk["c2"].data_ptr(), gx2.data_ptr(), bk["gate"].data_ptr(), wsb.data_ptr(), P[pre + "ca_w1"].data_ptr(),
                                    P[pre + "ca_b1"].data_ptr(), P[pre + "ca_w2"].data_ptr(), P[pre + "ca_b2"].data_ptr(), float(blk.conv_scale),
                                    dw1.data_ptr(), db1.data_ptr(), dw2.data_ptr(), db2.data_ptr(), dmean.data_ptr(), dc2.data_ptr(), B, HW, C_,
                                    CP, Sq, st))
                put(att[1].weight, dw1.view_as(att[1].weight)), put(att[1].bias, db1)
                put(att[3].weight, dw2.view_as(att[3].weight)), put(att[3].bias, db2)
                conv_wgrad(dc2, bk["c1"], cab[2], B, H, W, 64, CP)
                du1 = torch.empty(T, 64, **b16)
                _gemm(st, _lib.LD_CONV3, _lib.EP_DGELU, dc2, PT[pre + "Wc2T"], T, 64, 9 * CP, conv=(B, H, W, CP), aux=bk["u1"], outb=du1, ldo=64)
                conv_wgrad(du1, bk["xn1"], cab[0], B, H, W, CP, 64)
                dxc = torch.empty(T, CP, **f32)
                _gemm(st, _lib.LD_CONV3, _lib.EP_F32_BF16, du1, PT[pre + "Wc0T"], T, CP, 9 * 64, conv=(B, H, W, 64), outf=dxc)
            # ---- attention half: x1 = x + f_attn * proj(attention(qkv(norm1(x)))) ----
            attn_mod = blk.attn if hab else blk
            g_att = sink.scaled(g1b, bidx, 0) if (hab and not g1b_scaled) else g1b
            dao = torch.empty(T, CA, **b16)
            _gemm(st, _lib.LD_ROWS, _lib.EP_BF16, g_att, PT[pre + "WprojT"], T, CA, CP, lda=CP, outb=dao, ldo=CA)
            sink.lin_wgrad(g_att, bk["ao"], attn_mod.proj, col_map=hm)
            tab = attn_mod.relative_position_bias_table
            overlap = 0 if hab else blk.overlap_win_size - m.window_size
            sh = bk["shift"] if hab else 0
            need = int(L.srk_win256_attention_bwd_scratch(B, H, W, nH, CA, tab.shape[0], overlap))
            if attn_scratch is None or attn_scratch.numel() < need:
                attn_scratch = torch.empty(need, dtype=torch.uint8, device=dev)
            dqkv = _full((T, 3 * CA), b16)      # every element is written by the attention backward
            dtab = ops.zeros_f32(tab.shape, dev)
            check(L.srk_win256_attention_bwd(bk["qkv"].data_ptr(), 3 * CA, CA, tab.data_ptr(), tab.shape[0], dao.data_ptr(), CA, dqkv.data_ptr(),
                                             dtab.data_ptr(), attn_scratch.data_ptr(), B, H, W, sh, sh, nH, bk["scale"], overlap, st))
            put(tab, dtab)
            sink.lin_wgrad(dqkv, bk["xn1"], attn_mod.qkv, row_map=qkv_rows)
            sink.flush_wgrads()            # before the kernel below overwrites gxb2 (the fc2 gradient's operand when no DropPath copy was made)
            dxn1 = torch.empty(T, CP, **b16)
            if dxc is not None:
                _gemm(st, _lib.LD_ROWS, _lib.EP_RES_BF16, dqkv, PT[pre + "WqkvT"], T, CP, 3 * CA, lda=3 * CA, res=dxc, outb=dxn1)
                ln_bwd(dxn1, bk["x_in"], bk["mean1"], bk["rstd1"], blk.norm1, gx2, gxb2, accumulate=True)
            elif CP in (64, 128, 192):      # OCAB: qkv dgrad with the norm1 backward in its epilogue
                dg, dbt = ops.zeros_f32((C_,), dev), ops.zeros_f32((C_,), dev)
                _gemm(st, _lib.LD_ROWS, _lib.EP_LNBWD, dqkv, PT[pre + "WqkvT"], T, CP, 3 * CA, lda=3 * CA, outf=gx2, outb=gxb2, ldo=CP,
                      ln=dict(x=bk["x_in"], mean=bk["mean1"], rstd=bk["rstd1"], gamma=blk.norm1.weight, dgamma=dg, dbeta=dbt, C=C_))
                put(blk.norm1.weight, dg), put(blk.norm1.bias, dbt)
            else:
                _gemm(st, _lib.LD_ROWS, _lib.EP_BF16, dqkv, PT[pre + "WqkvT"], T, CP, 3 * CA, lda=3 * CA, outb=dxn1)
                ln_bwd(dxn1, bk["x_in"], bk["mean1"], bk["rstd1"], blk.norm1, gx2, gxb2, accumulate=True)
        # layer skip: d(layer input) = d(body input) + d(layer output)
        check(L.srk_add_f32_bf16(gx.data_ptr(), gx2.data_ptr(), gxb.data_ptr(), T * CP, st))
        sink.segment_done()

    # ---------------- head: patch_embed.norm, long skip, conv_first ----------------
    hp.head_backward(sink, m, S, m.patch_embed.norm, gxb, gfb)
    return sink.G


class HATFunction(hp.WholeModelFunction):
    """HAT as one autograd node (as the SwinIR engine)"""
    forward_train = staticmethod(lambda m, x, drop: hat_forward_train(m, x, m._pack(x.device), drop))
    backward_pass = staticmethod(hat_backward)
