"""What the host-run passes of HAT, DAT and SwinIR (window 2..7 / 16) have in common, each sequence of C-ABI calls (include/srk.h) once:

    head      srk_img_prep -> srk_stem_conv -> first LayerNorm (head_forward); its backward + long skip + conv_first gradient (head_backward)
    tail      conv_after_body + long skip, then conv_before_upsample + LeakyReLU -> conv + PixelShuffle stages -> conv_last -> image
              ('pixelshuffle') or ONE conv to the image ('pixelshuffledirect'; '' adds the input image): pack_tail / pack_tail_T,
              tail_forward, tail_backward
    Swin MLP  fc1 -> GELU -> fc2 + residual as one kernel at width 180 or as two GEMMs: mlp_inference, mlp_training, mlp_backward
    GradSink  where a backward pass puts its gradients: name map, queued linear weight gradients (ONE launch per block), conv / LayerNorm
              gradients, DropPath-scaled gradient copies, hand-over of each finished segment to the all-reduce hook
    WholeModelFunction     the autograd node of a whole model; a subclass binds its (forward keeping activations, backward) pair

The architecture files keep what is theirs: the blocks between head and tail.

Token rows.  ``rows`` is the row count of the token buffers: T = B H W, or (small windows) TR = T rounded up to 64 with the padding rows
of every reduction operand exactly zero (swinir_small_train.py).  Buffers come from ``_full`` / ``_rows``: torch.empty, or NaN-filled
under SRK_DBG_POISON=1 so that a kernel that leaves part of its output unwritten shows.
"""
from __future__ import annotations

import ctypes as C
import math
import os
from typing import Dict, Optional

import torch
import torch.nn as nn

from . import _lib, ops
from ._lib import GemmArgs, check, lib
from .packing import _pack_conv, _pack_conv_T, _pack_vec, _ps_map, _rup

_POISON = os.environ.get("SRK_DBG_POISON") == "1"


# ---- buffers ---------------------------------------------------------------------------------------------------------------------------
def _full(shape, kw: dict) -> torch.Tensor:
    """buffer that one kernel writes in full (NaN-filled first under SRK_DBG_POISON)"""
    if _POISON:
        return torch.full(tuple(shape) if not isinstance(shape, int) else (shape,), float("nan"), **kw)
    return torch.empty(shape, **kw)


def _rows(TR: int, T: int, cols: int, kw: dict) -> torch.Tensor:
    """[TR][cols] buffer whose rows < T a kernel writes in full and whose padding rows are 0"""
    t = _full((TR, cols), kw)
    if TR > T:
        t[T:].zero_()
    return t


def _kw(dev):
    return dict(dtype=torch.float32, device=dev), dict(dtype=torch.bfloat16, device=dev)


# ---- launch helpers ----------------------------------------------------------------------------------------------------------------------
def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def _gemm(st, loader, ep, A, W, M, N, K, *, lda=0, conv=None, bias=None, outf=None, outb=None, outb2=None, res=None, ldo=0, scale=0.0,
          r=0, Cs=0, img=None, xn=None, aux=None, rowscale=None, rows_per_sample=0, ln=None):
    a = GemmArgs()
    a.loader, a.epilogue = loader, ep
    a.A, a.lda, a.W, a.M, a.N, a.K = _ptr(A), lda, _ptr(W), M, N, K
    if conv is not None:
        a.B, a.H, a.Wd, a.CinP = conv
    a.r, a.Cs = r, Cs
    a.bias, a.outf, a.outb, a.outb2, a.res = _ptr(bias), _ptr(outf), _ptr(outb), _ptr(outb2), _ptr(res)
    a.aux, a.rowscale, a.rows_per_sample = _ptr(aux), _ptr(rowscale), (rows_per_sample if rowscale is not None else 0)
    a.ldo, a.scale = ldo or N, scale
    if img is not None:
        a.inv_range, a.Cimg, a.Hc, a.Wc = img["inv_range"], img["Cimg"], img["Hc"], img["Wc"]
        for i in range(4):
            a.mean[i] = img["mean"][i]
    if xn is not None:
        a.xn_out, a.xn_mean, a.xn_rstd, a.xn_gamma, a.xn_beta, a.xn_C = (_ptr(xn["out"]), _ptr(xn["mean"]), _ptr(xn["rstd"]),
                                                                       _ptr(xn["gamma"]), _ptr(xn["beta"]), xn["C"])
    if ln is not None:      # EP_LNBWD: LayerNorm backward fused into the dgrad's epilogue
        a.ln_x, a.ln_mean, a.ln_rstd, a.ln_gamma = _ptr(ln["x"]), _ptr(ln["mean"]), _ptr(ln["rstd"]), _ptr(ln["gamma"])
        a.ln_dgamma, a.ln_dbeta, a.ln_C = _ptr(ln["dgamma"]), _ptr(ln["dbeta"]), ln["C"]
    check(lib().srk_gemm_ex(C.byref(a), st))


# ---- packed gradients back into the parameters' shapes ------------------------------------------------------------------------------------
_ARANGE: Dict[tuple, torch.Tensor] = {}


def _arange(n: int, device) -> torch.Tensor:
    key = (n, str(device))
    t = _ARANGE.get(key)
    if t is None:
        t = _ARANGE[key] = torch.arange(n, device=device)
    return t


def _unpack_linear(dw: torch.Tensor, N: int, K: int, row_map=None, col_map=None) -> torch.Tensor:
    if row_map is None and col_map is None:
        return dw[:N, :K].contiguous()
    rows = row_map if row_map is not None else _arange(N, dw.device)
    cols = col_map if col_map is not None else _arange(K, dw.device)
    return dw[rows[:, None], cols[None, :]].contiguous()


def _unpack_conv(dw: torch.Tensor, Cout: int, Cin: int, CinP: int, row_map=None) -> torch.Tensor:
    v = dw.view(dw.shape[0], 9, CinP)
    v = v[:Cout] if row_map is None else v[row_map]
    return v[:, :, :Cin].reshape(Cout, 3, 3, Cin).permute(0, 3, 1, 2).contiguous()


# ---- gradient sink ------------------------------------------------------------------------------------------------------------------------
class GradSink:
    """{parameter name: gradient} of one backward pass.  hook (distributed.ListGradSynchronizer or None) gets the gradient tensors of each
    finished segment (tail, every residual group, head), every gradient exactly once and in the order it was made, so that their
    all-reduce overlaps the next segment."""

    def __init__(self, m, hook, st, dev, rows: int, C_: int, CP: int, HW: int, drop: Optional[torch.Tensor]):
        self.G: Dict[str, torch.Tensor] = {}
        self.names = {id(p): n for n, p in m.named_parameters()}
        self.handed = set()
        self.pending = []          # the block's linear weight gradients: queued, then ONE launch for all four (flush_wgrads)
        self.hook, self.st, self.dev, self.rows, self.C_, self.CP, self.HW, self.drop = hook, st, dev, rows, C_, CP, HW, drop
        self.L = lib()
        self.f32, self.b16 = _kw(dev)

    def put(self, p, g: torch.Tensor) -> None:
        self.G[self.names[id(p)]] = g

    def lin_wgrad(self, y, x, lin, row_map=None, col_map=None) -> None:
        """dW = y^T x, db = colsum(y) in the packed layout -> the nn.Linear's gradient, computed at the next flush_wgrads: y and x must stay
        untouched until then"""
        self.pending.append((y, x, lin, row_map, col_map))

    def flush_wgrads(self) -> None:
        pending = self.pending
        if not pending:
            return
        G, names = self.G, self.names
        for (y, x, lin, row_map, col_map), (dw, db) in zip(pending, ops.linear_wgrad_multi_bf16([(q[0], q[1]) for q in pending])):
            N, K = lin.weight.shape
            G[names[id(lin.weight)]] = _unpack_linear(dw, N, K, row_map, col_map)
            if lin.bias is not None:
                G[names[id(lin.bias)]] = (db[:N] if row_map is None else db[row_map]).contiguous()
        pending.clear()

    def conv_wgrad(self, dyb, xb, conv, Bc, Hc, Wc, CinP, NP, r=1, row_map=None) -> None:
        dev, st, L = self.dev, self.st, self.L
        dw = ops.zeros_f32((NP, 9 * CinP), dev)
        db = ops.zeros_f32((NP,), dev)
        ops._bind_wgrad_workspace(dev)
        if r == 1:
            check(L.srk_conv3x3_wgrad_bf16(dyb.data_ptr(), xb.data_ptr(), dw.data_ptr(), db.data_ptr(), Bc, Hc, Wc, CinP, NP, st))
        else:
            check(L.srk_conv3x3_wgrad_ps_bf16(dyb.data_ptr(), xb.data_ptr(), dw.data_ptr(), db.data_ptr(), Bc, Hc, Wc, CinP, NP, r, 64, st))
        Cout, Cin_ = conv.weight.shape[:2]
        G, names = self.G, self.names
        G[names[id(conv.weight)]] = _unpack_conv(dw, Cout, Cin_, CinP, row_map)
        G[names[id(conv.bias)]] = (db[:Cout] if row_map is None else db[row_map]).contiguous()

    def ln_bwd(self, dyb, x, mean, rstd, norm, gx, gxb, accumulate: bool) -> None:
        C_, dev = self.C_, self.dev
        dg, dbt = ops.zeros_f32((C_,), dev), ops.zeros_f32((C_,), dev)
        check(self.L.srk_layernorm_bwd(dyb.data_ptr(), x.data_ptr(), mean.data_ptr(), rstd.data_ptr(), norm.weight.data_ptr(), gx.data_ptr(),
                                       _ptr(gxb), dg.data_ptr(), dbt.data_ptr(), self.rows, C_, self.CP, 1 if accumulate else 0, self.st))
        names = self.names
        self.G[names[id(norm.weight)]], self.G[names[id(norm.bias)]] = dg, dbt

    def scaled(self, gb, bidx, which):
        """bf16 gradient copy entering a branch whose output was scaled by a DropPath factor (padding rows: factor 0)"""
        if self.drop is None:
            return gb
        out = _full((self.rows, self.CP), self.b16)
        check(self.L.srk_rowscale_bf16(gb.data_ptr(), out.data_ptr(), self.drop[bidx, which].data_ptr(), self.rows, self.HW, self.CP, self.st))
        return out

    def segment_done(self) -> None:
        if self.hook is not None:
            G, handed = self.G, self.handed
            fresh = [k for k in G if k not in handed]
            handed.update(fresh)
            self.hook.segment_done([G[k] for k in fresh])

    def finish(self) -> None:
        if self.hook is not None:
            self.hook.finish()


# ---- head ---------------------------------------------------------------------------------------------------------------------------------
def _mean3(m):
    return m.mean.flatten().tolist() if m.in_chans == 3 else [0.0, 0.0, 0.0]


def head_forward(m, x: torch.Tensor, norm, st, H: int, W: int, TR: Optional[int] = None, keep: Optional[dict] = None):
    """check_image_size + normalise, conv_first, the first LayerNorm -> (img4 fp32 [T][4], f0 fp32 [TR][CP], the normalised fp32 stream).
    x [B][Cin][H0][W0] is reflect-padded to H x W.  TR > T: the padding rows of f0 are 0.  keep: also gets img4, f0 and the norm's mean / rstd."""
    B, Cin, H0, W0 = x.shape
    T = B * H * W
    C_, CP = m.embed_dim, _rup(m.embed_dim, 64)
    f32, _ = _kw(x.device)
    L = lib()
    mean3 = (C.c_float * 3)(*_mean3(m))
    img4 = _full((T, 4), f32)
    check(L.srk_img_prep(x.data_ptr(), img4.data_ptr(), B, Cin, H0, W0, H, W, float(m.img_range), C.byref(mean3), st))
    f0 = _rows(TR or T, T, CP, f32)
    check(L.srk_stem_conv(img4.data_ptr(), m.conv_first.weight.data_ptr(), m.conv_first.bias.data_ptr(), f0.data_ptr(), B, H, W, Cin, C_, CP, st))
    _, cur, mean_pe, rstd_pe = ops.layernorm_fwd(f0, norm.weight, norm.bias, C_, out_bf16=False, out_f32=True)
    if keep is not None:
        keep.update(img4=img4, f0=f0, mean_pe=mean_pe, rstd_pe=rstd_pe)
    return img4, f0, cur


def head_backward(sink: GradSink, m, S: dict, norm, gxb, gfb) -> None:
    """the first LayerNorm's backward, the long skip (gfb: the gradient that conv_after_body's skip carries), conv_first's gradient; hands
    the last segment over and closes the hook"""
    B, Cin, H, W = S["B"], S["Cin"], S["H"], S["W"]
    T, CP, dev, st, L = B * H * W, sink.CP, sink.dev, sink.st, sink.L
    gf = _full((sink.rows, CP), sink.f32)
    sink.ln_bwd(gxb, S["f0"], S["mean_pe"], S["rstd_pe"], norm, gf, None, accumulate=False)
    check(L.srk_add_bf16_into_f32(gf.data_ptr(), gfb.data_ptr(), T * CP, st))
    dwf, dbf = ops.zeros_f32(m.conv_first.weight.shape, dev), ops.zeros_f32(m.conv_first.bias.shape, dev)
    check(L.srk_stem_wgrad(S["img4"].data_ptr(), gf.data_ptr(), dwf.data_ptr(), dbf.data_ptr(), B, H, W, Cin, sink.C_, CP, st))
    sink.put(m.conv_first.weight, dwf)
    sink.put(m.conv_first.bias, dbf)
    sink.segment_done()
    sink.finish()


# ---- reconstruction tail --------------------------------------------------------------------------------------------------------------------
def _up_convs(m):
    return [mod for mod in m.upsample if isinstance(mod, nn.Conv2d)]


def _direct_conv(m):
    """UpsampleOneStep's conv ('pixelshuffledirect') or conv_last of the '' head: embed_dim -> in_chans * r^2 channels"""
    return m.upsample[0] if m.upsampler == "pixelshuffledirect" else m.conv_last


def pack_tail(P: dict, m, CP: int, device) -> None:
    """the tail's forward operands; called inside the caller's batched_pack() block"""
    P["Wcab"] = _pack_conv(m.conv_after_body.weight, CP, CP)
    P["bcab"] = _pack_vec(m.conv_after_body.bias, CP)
    if m.upsampler == "pixelshuffle":
        P["Wbefore"] = _pack_conv(m.conv_before_upsample[0].weight, 64, CP)
        P["bbefore"] = _pack_vec(m.conv_before_upsample[0].bias, 64)
        for k, mod in enumerate(_up_convs(m)):
            N = mod.weight.shape[0]
            r = int(round(math.sqrt(N // 64)))
            pm = _ps_map(N, r, 64, device)
            P[f"Wup{k}"] = _pack_conv(mod.weight, N, 64, row_map=pm)
            P[f"bup{k}"] = _pack_vec(mod.bias, N, row_map=pm)
            P[f"rup{k}"] = torch.tensor(r)
        P["Wlast"] = _pack_conv(m.conv_last.weight, 16, 64)
        P["blast"] = _pack_vec(m.conv_last.bias, 16)
    else:
        direct = _direct_conv(m)
        P["Wdirect"] = _pack_conv(direct.weight, 16, CP)
        P["bdirect"] = _pack_vec(direct.bias, 16)


def pack_tail_T(P: dict, m, CP: int, device) -> None:
    """the transposed copies for the tail's dgrads; called inside the caller's batched_pack() block"""
    P["WcabT"] = _pack_conv_T(m.conv_after_body.weight, CP, CP)
    if m.upsampler == "pixelshuffle":
        P["WbeforeT"] = _pack_conv_T(m.conv_before_upsample[0].weight, CP, 64)
        for k, mod in enumerate(_up_convs(m)):
            N = mod.weight.shape[0]
            r = int(round(math.sqrt(N // 64)))
            P[f"WupT{k}"] = _pack_conv_T(mod.weight, 64, N, col_map=_ps_map(N, r, 64, device))


def tail_forward(m, P: dict, st, xnf, f0, img4, B: int, Cin: int, H0: int, W0: int, H: int, W: int, keep: Optional[dict] = None) -> torch.Tensor:
    """xnf: the final LayerNorm's bf16 output -> the image y fp32 [B][Cin][H0 s][W0 s].  keep: gets fb, ups (and t1, hr_h, hr_w)"""
    T, s = B * H * W, m.upscale
    CP = _rup(m.embed_dim, 64)
    f32, b16 = _kw(xnf.device)
    fb = _full((T, CP), b16)
    _gemm(st, _lib.LD_CONV3, _lib.EP_RES_BF16, xnf, P["Wcab"], T, CP, 9 * CP, conv=(B, H, W, CP), bias=P["bcab"], res=f0, outb=fb)
    y = _full((B, Cin, H0 * s, W0 * s), f32)
    img = dict(inv_range=1.0 / float(m.img_range), Cimg=Cin, Hc=H0 * s, Wc=W0 * s, mean=_mean3(m) + [0.0])
    if m.upsampler == "pixelshuffle":
        t1 = _full((T, 64), b16)
        _gemm(st, _lib.LD_CONV3, _lib.EP_LRELU, fb, P["Wbefore"], T, 64, 9 * CP, conv=(B, H, W, CP), bias=P["bbefore"], outb=t1, scale=0.01)
        ups = []
        src, h_, w_, k = t1, H, W, 0
        while f"Wup{k}" in P:
            r = int(P[f"rup{k}"])
            N = P[f"Wup{k}"].shape[0]
            up = _full((B * h_ * r * w_ * r, 64), b16)
            _gemm(st, _lib.LD_CONV3, _lib.EP_PS, src, P[f"Wup{k}"], B * h_ * w_, N, 9 * 64, conv=(B, h_, w_, 64), bias=P[f"bup{k}"], outb=up, r=r, Cs=64,
                  ldo=N)
            ups.append(dict(src=src, out=up, h=h_, w=w_, r=r, N=N))
            src, h_, w_, k = up, h_ * r, w_ * r, k + 1
        _gemm(st, _lib.LD_CONV3, _lib.EP_IMG, src, P["Wlast"], B * h_ * w_, 16, 9 * 64, conv=(B, h_, w_, 64), bias=P["blast"], outf=y, img=img)
        if keep is not None:
            keep.update(fb=fb, t1=t1, ups=ups, hr_h=h_, hr_w=w_)
    else:       # UpsampleOneStep, or '' with upscale 1: x + conv_last(res), x = the normalised, padded input
        _gemm(st, _lib.LD_CONV3, _lib.EP_PS_IMG, fb, P["Wdirect"], T, 16, 9 * CP, conv=(B, H, W, CP), bias=P["bdirect"], outf=y, img=img, r=s,
              res=img4 if m.upsampler == "" else None)
        if keep is not None:
            keep.update(fb=fb, ups=[])
    return y


def tail_backward(sink: GradSink, m, S: dict, PT: dict, dy, B: int, Cin: int, H0: int, W0: int, H: int, W: int, direct_CoP: Optional[int] = None):
    """dy -> (gfb, gx, gxb): gfb bf16 [T][CP] the gradient of conv_after_body's output + long skip; gx fp32 / gxb bf16 [rows][CP] the
    gradient of the last residual group's output.  Hands the tail's gradients over as the first segment."""
    dev, st, L, TR, C_, CP, f32, b16 = sink.dev, sink.st, sink.L, sink.rows, sink.C_, sink.CP, sink.f32, sink.b16
    T, s = B * H * W, m.upscale
    inv_range = 1.0 / float(m.img_range)
    if m.upsampler == "pixelshuffle":
        hs, wsz = S["hr_h"], S["hr_w"]
        gyimg = _full((B * hs * wsz, 4), f32)
        check(L.srk_img_grad_prep(dy.data_ptr(), gyimg.data_ptr(), B, Cin, H0 * s, W0 * s, hs, wsz, 1, 4, inv_range, st))
        last_in = S["ups"][-1]["out"] if S["ups"] else S["t1"]
        dwl, dbl = ops.zeros_f32(m.conv_last.weight.shape, dev), ops.zeros_f32(m.conv_last.bias.shape, dev)
        check(L.srk_smallconv_wgrad(last_in.data_ptr(), gyimg.data_ptr(), dwl.data_ptr(), dbl.data_ptr(), B, hs, wsz, 64, 64, Cin, 4, st))
        sink.put(m.conv_last.weight, dwl)
        sink.put(m.conv_last.bias, dbl)
        gcur = _full((B * hs * wsz, 64), b16)
        check(L.srk_smallconv_dgrad(gyimg.data_ptr(), m.conv_last.weight.data_ptr(), gcur.data_ptr(), B, hs, wsz, 64, 64, Cin, 4, st))
        up_convs = _up_convs(m)
        for k in range(len(S["ups"]) - 1, -1, -1):
            u = S["ups"][k]
            r, N, h_, w_ = u["r"], u["N"], u["h"], u["w"]
            sink.conv_wgrad(gcur, u["src"], up_convs[k], B, h_, w_, 64, N, r=r, row_map=_ps_map(N, r, 64, dev))
            gprev = _full((B * h_ * w_, 64), b16)
            if k == 0:     # through the LeakyReLU(0.01) of conv_before_upsample
                _gemm(st, _lib.LD_CONV3_PS, _lib.EP_DLRELU, gcur, PT[f"WupT{k}"], B * h_ * w_, 64, 9 * N, conv=(B, h_, w_, N), r=r, Cs=64, outb=gprev,
                      aux=S["t1"], scale=0.01, ldo=64)
            else:
                _gemm(st, _lib.LD_CONV3_PS, _lib.EP_BF16, gcur, PT[f"WupT{k}"], B * h_ * w_, 64, 9 * N, conv=(B, h_, w_, N), r=r, Cs=64, outb=gprev, ldo=64)
            gcur = gprev
        sink.conv_wgrad(gcur, S["fb"], m.conv_before_upsample[0], B, H, W, CP, 64)
        gfb = _full((T, CP), b16)
        _gemm(st, _lib.LD_CONV3, _lib.EP_BF16, gcur, PT["WbeforeT"], T, CP, 9 * 64, conv=(B, H, W, 64), outb=gfb)
    else:       # fp32 small-conv gradients on CP input channels; for '' the added input image takes no gradient
        direct = _direct_conv(m)
        r = s if m.upsampler == "pixelshuffledirect" else 1
        Co = Cin * r * r
        CoP = direct_CoP or (4 if Co <= 4 else 16)
        gyimg = _full((T, CoP), f32)
        check(L.srk_img_grad_prep(dy.data_ptr(), gyimg.data_ptr(), B, Cin, H0 * s, W0 * s, H, W, r, CoP, inv_range, st))
        dwl, dbl = ops.zeros_f32(direct.weight.shape, dev), ops.zeros_f32(direct.bias.shape, dev)
        check(L.srk_smallconv_wgrad(S["fb"].data_ptr(), gyimg.data_ptr(), dwl.data_ptr(), dbl.data_ptr(), B, H, W, C_, CP, Co, CoP, st))
        sink.put(direct.weight, dwl)
        sink.put(direct.bias, dbl)
        gfb = _full((T, CP), b16)
        check(L.srk_smallconv_dgrad(gyimg.data_ptr(), direct.weight.data_ptr(), gfb.data_ptr(), B, H, W, C_, CP, Co, CoP, st))
    sink.conv_wgrad(gfb, S["xnf"], m.conv_after_body, B, H, W, CP, CP)
    dxn = _rows(TR, T, CP, b16)
    _gemm(st, _lib.LD_CONV3, _lib.EP_BF16, gfb, PT["WcabT"], T, CP, 9 * CP, conv=(B, H, W, CP), outb=dxn)
    gx = _full((TR, CP), f32)        # gradient of the current layer's OUTPUT (later: of its input); padding rows 0
    gxb = _full((TR, CP), b16)
    sink.ln_bwd(dxn, S["x_last"], S["meanf"], S["rstdf"], m.norm, gx, gxb, accumulate=False)
    sink.segment_done()
    return gfb, gx, gxb


# ---- Swin MLP -----------------------------------------------------------------------------------------------------------------------------
def fused_mlp_ok(dev, CP: int, HP: int, rows: int) -> bool:
    """the one-kernel MLP forward covers width 180 / hidden 360 once every CU gets a 64-row tile (callers add their own row conditions)"""
    return CP == 192 and HP == 384 and rows >= 64 * torch.cuda.get_device_properties(dev).multi_processor_count


def fused_mlp_bwd_ok(dev, CP: int, HP: int, T: int, HW: int) -> bool:
    opt = C.c_int()
    check(lib().srk_get_option(b"mlp_bwd_fused", C.byref(opt)))
    return opt.value != 0 and T % 64 == 0 and HW % 64 == 0 and fused_mlp_ok(dev, CP, HP, T)


def mlp_inference(st, P: dict, rows: int, CP: int, HP: int, hh, fused: bool):
    """-> mlp(pre, xn_in, x_res, out, out_b=None, nn_=None): out = x_res + fc2(gelu(fc1(xn_in))) [+ the next LayerNorm of the new rows];
    hh bf16 [rows][HP] is the hidden activation's scratch"""
    L = lib()

    def mlp(pre, xn_in, x_res, out, out_b=None, nn_=None):
        if fused:
            args = (None, None, None, None, None, 0) if nn_ is None else (nn_["out"].data_ptr(), nn_["mean"].data_ptr(), nn_["rstd"].data_ptr(),
                                                                       nn_["gamma"].data_ptr(), nn_["beta"].data_ptr(), nn_["C"])
            check(L.srk_mlp_fused_fwd(xn_in.data_ptr(), P[pre + "W1"].data_ptr(), P[pre + "b1"].data_ptr(), P[pre + "W2"].data_ptr(),
                                      P[pre + "b2"].data_ptr(), x_res.data_ptr(), out.data_ptr(), _ptr(out_b), *args, rows, st))
        else:
            _gemm(st, _lib.LD_ROWS, _lib.EP_GELU, xn_in, P[pre + "W1"], rows, HP, CP, lda=CP, bias=P[pre + "b1"], outb2=hh)
            _gemm(st, _lib.LD_ROWS, _lib.EP_RES, hh, P[pre + "W2"], rows, CP, HP, lda=HP, bias=P[pre + "b2"], res=x_res, outf=out, outb=out_b, xn=nn_)
    return mlp


def mlp_training(st, P: dict, dev, rows: int, HW: int, CP: int, HP: int, fused: bool):
    """-> mlp(pre, xn_in, x_res, rowscale) -> (out fp32, out bf16, u, h): out = x_res + f * fc2(gelu(fc1(xn_in))), f the per-sample
    DropPath factor (rowscale) or 1; u = fc1's output and h = gelu(u) are kept for the backward"""
    L = lib()
    f32, b16 = _kw(dev)

    def mlp(pre, xn_in, x_res, rowscale):
        out, out_b = _full((rows, CP), f32), _full((rows, CP), b16)
        u, h = _full((rows, HP), b16), _full((rows, HP), b16)
        if fused:
            check(L.srk_mlp_fused_fwd_train(xn_in.data_ptr(), P[pre + "W1"].data_ptr(), P[pre + "b1"].data_ptr(), P[pre + "W2"].data_ptr(),
                                            P[pre + "b2"].data_ptr(), x_res.data_ptr(), out.data_ptr(), out_b.data_ptr(), u.data_ptr(),
                                            h.data_ptr(), None, None, None, None, None, 0, _ptr(rowscale), HW, rows, st))
        else:
            _gemm(st, _lib.LD_ROWS, _lib.EP_GELU, xn_in, P[pre + "W1"], rows, HP, CP, lda=CP, bias=P[pre + "b1"], outb=u, outb2=h)
            _gemm(st, _lib.LD_ROWS, _lib.EP_RES, h, P[pre + "W2"], rows, CP, HP, lda=HP, bias=P[pre + "b2"], res=x_res, outf=out, outb=out_b,
                  rowscale=rowscale, rows_per_sample=HW)
        return out, out_b, u, h
    return mlp


def mlp_backward(sink: GradSink, PT: dict, bk: dict, HP: int, gx2, gxb2, bidx: Optional[int], fused: bool):
    """The MLP half of a Swin block's backward, x2 = x1 + f_mlp * fc2(gelu(fc1(norm2(x1)))): fc2 dgrad * GELU'(u) -> fc1 dgrad -> norm2
    backward into gx2 (then d x1), one kernel when ``fused``; queues the two weight gradients.  bidx: the block's row of DropPath factors
    (None: a block without DropPath).  -> (g1b, scaled): the bf16 copy of d x1, and whether the attention branch's factor is already on it."""
    st, rows, C_, CP, dev, b16 = sink.st, sink.rows, sink.C_, sink.CP, sink.dev, sink.b16
    pre, blk = bk["pre"], bk["blk"]
    g_mlp = sink.scaled(gxb2, bidx, 1) if bidx is not None else gxb2
    du = _full((rows, HP), b16)
    g1b = _full((rows, CP), b16)
    if fused:      # the bf16 copy comes out already scaled by the attention branch's DropPath factor
        dg, dbt = ops.zeros_f32((C_,), dev), ops.zeros_f32((C_,), dev)
        rsc = sink.drop[bidx, 0] if (bidx is not None and sink.drop is not None) else None
        check(sink.L.srk_mlp_fused_bwd(g_mlp.data_ptr(), PT[pre + "W2T"].data_ptr(), bk["u"].data_ptr(), du.data_ptr(), PT[pre + "W1T"].data_ptr(),
                                       bk["x1"].data_ptr(), bk["mean2"].data_ptr(), bk["rstd2"].data_ptr(), blk.norm2.weight.data_ptr(),
                                       gx2.data_ptr(), g1b.data_ptr(), _ptr(rsc), sink.HW, dg.data_ptr(), dbt.data_ptr(), C_, rows, st))
        sink.put(blk.norm2.weight, dg)
        sink.put(blk.norm2.bias, dbt)
    else:
        _gemm(st, _lib.LD_ROWS, _lib.EP_DGELU, g_mlp, PT[pre + "W2T"], rows, HP, CP, lda=CP, aux=bk["u"], outb=du, ldo=HP)
    sink.lin_wgrad(g_mlp, bk["h"], blk.mlp.fc2)
    sink.lin_wgrad(du, bk["xn2"], blk.mlp.fc1)
    if not fused:
        dxn2 = _full((rows, CP), b16)
        _gemm(st, _lib.LD_ROWS, _lib.EP_BF16, du, PT[pre + "W1T"], rows, CP, HP, lda=HP, outb=dxn2)
        sink.ln_bwd(dxn2, bk["x1"], bk["mean2"], bk["rstd2"], blk.norm2, gx2, g1b, accumulate=True)      # gx2 = d x1 (fp32), g1b its bf16 copy
    return g1b, fused


# ---- the autograd node ------------------------------------------------------------------------------------------------------------------------
class WholeModelFunction(torch.autograd.Function):
    """One autograd node for a whole model: forward keeps the activations, backward returns every parameter's gradient (model.grad_sync,
    when set, is the hook that gets each finished segment).  The input image gets no gradient.  A subclass binds its pair:
    ``forward_train(model, x, drop) -> (y, saved)`` and ``backward_pass(model, saved, dy, hook=) -> {parameter name: gradient}``."""
    forward_train = backward_pass = None

    @staticmethod
    def forward(ctx, model, x, drop, *params):
        with torch.cuda.device(x.device):
            y, saved = ctx._forward_cls.forward_train(model, x.contiguous().float(), drop)
        ctx.model, ctx.saved = model, saved
        return y

    @staticmethod
    def backward(ctx, dy):
        model = ctx.model
        arena = model.__dict__.setdefault("_zero_arena", ops.ZeroArena())      # the pass's zeroed accumulators: one buffer, one fill
        with torch.cuda.device(dy.device), ops.arena_scope(arena, dy.device):
            G = ctx._forward_cls.backward_pass(model, ctx.saved, dy.contiguous().float(), hook=getattr(model, "grad_sync", None))
        ctx.saved = None
        grads = []
        for n, p in model.named_parameters():
            g = G.get(n)
            grads.append(None if g is None else g.reshape(p.shape).to(p.dtype))
        return (None, None, None, *grads)
