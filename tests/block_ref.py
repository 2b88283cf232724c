"""fp64 restatements of the fused per-block Swin kernels as the SwinIR executor launches them, their derived tolerances and the case
matrix of tests/test_gpu_block_fused.py.  Plain torch on the CPU; pinned in tests/test_block_ref.py.

  entry point (include/srk.h)        production kernel (csrc/)                                     restatement
  srk_mlp_fused_fwd_ex               gemm_stream.hip  mlp_fused_fwd_kernel<u_dgelu>                mlp_fwd_stage1 / mlp_fwd_stage2
  srk_mlp_fused_bwd_ex               gemm_stream.hip  mlp_fused_bwd_kernel<u_is_dgelu>             mlp_bwd_stage1 / mlp_bwd_stage2
  srk_qkv_window_attention_fwd       attn_fused.hip   qkv_attn_fwd3_kernel / qkv_attn_fwd_kernel   attn_qkv / attn_out
  srk_proj_residual_fwd              gemm_stream_split_kernel<EP_PROJ_RES> / tile kernel           proj_residual (+ gemm_ex_ref.ln_fwd)
  srk_qkv_dgrad_lnbwd                gemm_stream_kernel<EP_LNBWD, 9> / tile kernel                 qkv_dgrad_lnbwd

Layouts (C = 180 in CP = 192, hidden 360 in HP = 384, 6 heads x 30 in 32; every pad row / column of a weight, bias, gamma, beta and of
a row operand is zero, as the executor's packed buffers are):
  token order   row t = (b * H + y) * W + x
  window order  row m = (b * nW + wy * nWw + wx) * 64 + py * 8 + px  holds token  win_to_token(...)[m]  (roll(-shift) + window_partition)
"""
from __future__ import annotations

import math
from dataclasses import dataclass, replace
from typing import Dict, List, Optional, Tuple

import torch

from gemm_ex_ref import BF16_REL, BF16_TINY, GELU_LIP, LN_EPS, U, Out, Tol, compare, dgelu, gelu, ln_bwd, ln_fwd, round_as  # noqa: F401

C, CP, HID, HP, NH, D, DP = 180, 192, 360, 384, 6, 30, 32
CA = NH * DP
DGELU_LIP = 0.8            # max |gelu''| = 2 phi(0) = 0.7979 (gelu''(x) = phi(x) (2 - x^2))
KEEP = float(torch.tensor(1.0 / 0.85, dtype=torch.float32))     # DropPath factor of a kept sample (drop_path 0.15), as the fp32 the device reads


# ---- window maps, written from network_swinir.py's roll + window_partition ---------------------------------------------------------
@dataclass(frozen=True)
class Variant:
    """Negative controls: each flag makes a restatement compute a deliberately WRONG result."""
    shift_sign: bool = False        # roll(+shift) instead of roll(-shift)
    swap_hw: bool = False           # H and W exchanged in the row map
    shift_rowscale: bool = False    # DropPath factor of the neighbouring sample
    ln_over_cp: bool = False        # LayerNorm statistics over 192 columns instead of 180
    dgelu_of_rounded: bool = False  # gelu'(bf16(u)) where the kernel takes gelu'(u)
    no_mask: bool = False
    bias_transposed: bool = False   # relative-position table read at (dx, dy)
    scale_after_round: bool = False  # q = bf16(bf16(acc + b) * scale)
    skip_into_outf: bool = False    # ln_skip form: the sum stored to outf as well


OK = Variant()


def win_to_token(B: int, H: int, W: int, shift: int, v: Variant = OK) -> torch.Tensor:
    """[B*H*W] int64: the token that window-order row m holds (network_swinir.py:249-256: torch.roll(x, (-shift, -shift), (1, 2)), then
    window_partition: view(B, H/8, 8, W/8, 8, C).permute(0, 1, 3, 2, 4, 5))."""
    if v.swap_hw:
        H, W = W, H
    t = torch.arange(B * H * W).view(B, H, W, 1)
    s = shift if v.shift_sign else -shift
    if shift:
        t = torch.roll(t, shifts=(s, s), dims=(1, 2))
    return t.view(B, H // 8, 8, W // 8, 8, 1).permute(0, 1, 3, 2, 4, 5).reshape(-1)


def token_to_win(B: int, H: int, W: int, shift: int, v: Variant = OK) -> torch.Tensor:
    """The inverse map: window-order row of token t (window_reverse + roll(+shift), :265-272)."""
    tok = win_to_token(B, H, W, shift, v)
    inv = torch.empty_like(tok)
    inv[tok] = torch.arange(tok.numel())
    return inv


def region_labels(H: int, W: int, v: Variant = OK) -> torch.Tensor:
    """[nW][64] region id of every window position in the shifted frame (network_swinir.py:219-230, window 8, shift 4): the img_mask
    built with the slices (0, -8), (-8, -4), (-4, None), then window_partition."""
    if v.swap_hw:
        H, W = W, H
    img = torch.zeros(1, H, W, 1)
    cnt = 0
    for hs in (slice(0, -8), slice(-8, -4), slice(-4, None)):
        for ws in (slice(0, -8), slice(-8, -4), slice(-4, None)):
            img[:, hs, ws, :] = cnt
            cnt += 1
    return img.view(1, H // 8, 8, W // 8, 8, 1).permute(0, 1, 3, 2, 4, 5).reshape(-1, 64).long()


def shift_mask(H: int, W: int, v: Variant = OK) -> torch.Tensor:
    """[nW][64][64] fp64 in {0, -100} (:231-235)."""
    lab = region_labels(H, W, v)
    d = lab[:, None, :] - lab[:, :, None]
    return torch.where(d != 0, -100.0, 0.0).double()


def rel_pos_index(v: Variant = OK) -> torch.Tensor:
    """[64][64] index into the 225-entry table (:89-103)."""
    p = torch.arange(64)
    y, x = p // 8, p % 8
    dy, dx = y[:, None] - y[None, :] + 7, x[:, None] - x[None, :] + 7
    return (dx * 15 + dy) if v.bias_transposed else (dy * 15 + dx)


def dense_bias(table: torch.Tensor, v: Variant = OK) -> torch.Tensor:
    """table [225][6] -> [6][64][64] = table[relative_position_index] (:127-129)."""
    return table[rel_pos_index(v).reshape(-1)].reshape(64, 64, -1).permute(2, 0, 1).contiguous()


# ---- cases --------------------------------------------------------------------------------------------------------------------------
ROW_HW = ((64, 64, 0), (32, 40, 0), (24, 24, 4), (128, 136, 0))     # (H, W, samples beyond the smallest B with B*H*W >= 64 n)
ROWSCALES = ("none", "mix", "ones")
KINDS = ("mlp_fwd", "mlp_bwd", "proj", "lnbwd")


@dataclass(frozen=True)
class BCase:
    kind: str                 # mlp_fwd | mlp_bwd | proj | lnbwd | attn
    B: int
    H: int
    W: int
    shift: int = 0
    rs: str = "none"          # row-scale variant: none | mix (1/0.85 and exact 0.0 samples) | ones
    dg: int = 0               # fused MLP: the u buffer holds gelu'(u)
    skip: bool = False        # lnbwd: ln_skip form
    lda: int = CP             # attn
    small: bool = False       # below the streaming kernels' M >= 64 n: tile kernel only (proj / lnbwd)

    @property
    def M(self) -> int:
        return self.B * self.H * self.W

    @property
    def B_(self) -> int:
        return self.M // 64

    @property
    def rps(self) -> int:
        """Rows per DropPath sample: H*W as in the model; with fewer than 3 images one window row of tokens (8 W, a multiple of 64), so
        that a boundary and a dropped sample lie inside the case.  For the window-ordered entry points that is a tile-kernel case: the
        streaming kernel serves rows_per_sample == H*W only (stream_path)."""
        return self.H * self.W if self.B >= 3 else 8 * self.W

    @property
    def id(self) -> str:
        s = f"{self.kind}-{self.B}x{self.H}x{self.W}-s{self.shift}"
        if self.kind == "attn":
            return s + f"-lda{self.lda}"
        s += f"-rs_{self.rs}"
        if self.kind.startswith("mlp"):
            s += f"-dg{self.dg}"
        if self.skip:
            s += "-skip"
        return s + ("-small" if self.small else "")

    @property
    def shape_key(self) -> Tuple:
        return (self.kind, self.B, self.H, self.W) + ((self.lda,) if self.kind == "attn" else ())


def row_shapes(n: int) -> List[Tuple[int, int, int]]:
    """The (B, H, W) of the four row-stream kernels for a device with n CUs (they use n & ~7): the even tile list, a non-power-of-two
    H*W and W (inexact reciprocal division, uneven lists), many samples, one tall sample.  n = 256: (4,64,64) (13,32,40) (33,24,24) (1,128,136)."""
    need = 64 * (n & ~7)
    return [(-(-need // (H * W)) + extra, H, W) for H, W, extra in ROW_HW]


def row_cases(n: int = 256) -> List[BCase]:
    cs: List[BCase] = []
    for kind in KINDS:
        for B, H, W in row_shapes(n):
            for shift in (0, 4):
                for rs in ROWSCALES:
                    if kind.startswith("mlp"):
                        cs += [BCase(kind, B, H, W, shift, rs, dg=dg) for dg in (0, 1)]
                    elif kind == "lnbwd":
                        cs.append(BCase(kind, B, H, W, shift, rs, skip=(rs != "mix") == bool(shift)))
                    else:
                        cs.append(BCase(kind, B, H, W, shift, rs))
        if kind in ("proj", "lnbwd"):      # M = 64 * 5: tile kernel only
            cs += [BCase(kind, 5, 8, 8, 4, "mix", small=True), BCase(kind, 1, 40, 8, 4, "none", small=True, skip=kind == "lnbwd")]
    return cs


def attn_shapes(n: int) -> List[Tuple[int, int, int]]:
    """Windows B_ = n, n + 1, n + 4, about 2 n and >= 3 n + 5; n = 256: (4,64,64) -> 256, (257,8,8) -> 257 (the image is one window),
    (13,32,40) -> 260, (7,64,72) -> 504, (11,64,72) -> 792.  Both kernels walk the windows with a stride of n (one 8-wave workgroup per
    CU; n / 8 groups of 8 windows for the 4-wave kernel), so up to 2 n windows a workgroup sees at most two: a first iteration that
    prefetches into a slot that never held anything and a last one that prefetches nothing.  Only the last shape has the STEADY-STATE
    iteration (a predecessor and a successor: the prefetch of window t + 1 into the ring slot that held window t - 1's ao tile): every
    workgroup gets at least 3 windows, a few get 4."""
    return [(-(-n // 64), 64, 64), (n + 1, 8, 8), (-(-(n + 4) // 20), 32, 40), (max(1, round(2 * n / 72)), 64, 72), (-(-(3 * n + 5) // 72), 64, 72)]


def attn_cases(n: int = 256) -> List[BCase]:
    return [BCase("attn", B, H, W, shift, lda=lda) for B, H, W in attn_shapes(n) for shift in (0, 4) for lda in (CP, CP + 8)]


def stream_path(c: BCase, n_cus: int, stream_on: bool) -> str:
    """Which implementation srk_launch_gemm picks for proj / lnbwd (csrc/gemm_stream.hip: srk_launch_gemm_stream)."""
    cus = n_cus & ~7
    if not stream_on or cus < 8 or c.M % 64 or c.M < 64 * cus or c.M >= 1 << 24:
        return "tile"
    if c.rs != "none" and (c.rps % 64 or c.rps != c.H * c.W):      # window-ordered rows: the streaming kernel's sample is the image
        return "tile"
    return "stream"


# ---- inputs -------------------------------------------------------------------------------------------------------------------------
def rowscale(c: BCase) -> Optional[torch.Tensor]:
    ns = c.M // c.rps
    if c.rs == "none":
        return None
    if c.rs == "ones":
        return torch.ones(ns)
    f = torch.full((ns,), KEEP)
    f[1::3] = 0.0
    return f


def row_factor(c: BCase, rows: torch.Tensor, v: Variant = OK) -> torch.Tensor:
    """[len(rows)][1] fp64 DropPath factor of the given TOKEN rows."""
    f = rowscale(c)
    if f is None:
        return torch.ones(rows.numel(), 1, dtype=torch.float64)
    idx = rows // c.rps
    if v.shift_rowscale:
        idx = (idx + 1) % f.numel()
    return f.double()[idx][:, None]


def _padded(g, rows, cols, rcap, ccap, std):
    t = torch.zeros(rows, cols)
    t[:rcap, :ccap] = torch.randn(rcap, ccap, generator=g) * std
    return t


def _heads(t: torch.Tensor) -> torch.Tensor:
    """Zero the pad channels (30, 31 of every 32) of a [..][k * 32] tensor."""
    t = t.clone()
    t.view(*t.shape[:-1], -1, DP)[..., D:] = 0.0
    return t


def _ln_operands(g, M):
    x = _padded(g, M, CP, M, C, 1.5) + 0.3
    x[:, C:] = 0.0
    mean = x[:, :C].double().mean(1)
    var = ((x[:, :C].double() - mean[:, None]) ** 2).mean(1)
    gam = torch.zeros(CP)
    gam[:C] = 1.0 + 0.5 * torch.randn(C, generator=g)
    gx0 = _padded(g, M, CP, M, C, 1.0)
    return dict(ln_x=x, ln_mean=mean.float(), ln_rstd=(var + LN_EPS).rsqrt().float(), ln_gamma=gam, gx0=gx0,
                dgamma0=torch.randn(C, generator=g), dbeta0=torch.randn(C, generator=g))


def _bias(g, n, cap):
    b = torch.zeros(n)
    v = 0.5 * torch.randn(cap, generator=g)
    v[v.abs() < 0.05] = 0.25
    b[:cap] = v
    return b


def make_inputs(c: BCase) -> Dict[str, torch.Tensor]:
    """Seeded operands of a SHAPE (kind, B, H, W[, lda]) in the device's dtypes; shift / rowscale / dg / skip do not change them."""
    g = torch.Generator().manual_seed(4321 + 7 * c.B + c.H + 3 * c.W + 1000 * (KINDS + ("attn",)).index(c.kind))
    bf = torch.bfloat16
    M = c.M
    inp: Dict[str, torch.Tensor] = {}
    if c.kind == "mlp_fwd":
        inp["xn"] = _padded(g, M, CP, M, C, 1.0).to(bf)
        inp["w1"], inp["b1"] = _padded(g, HP, CP, HID, C, C ** -0.5).to(bf), _bias(g, HP, HID)
        inp["w2"], inp["b2"] = _padded(g, CP, HP, C, HID, HID ** -0.5).to(bf), _bias(g, CP, C)
        inp["res"] = _padded(g, M, CP, M, C, 1.0)
        inp["gamma"] = torch.zeros(CP)
        inp["gamma"][:C] = 1.0 + 0.5 * torch.randn(C, generator=g)
        inp["beta"] = _padded(g, 1, CP, 1, C, 0.3)[0]
    elif c.kind == "mlp_bwd":
        inp["g"] = _padded(g, M, CP, M, C, 0.5).to(bf)
        inp["w2t"] = _padded(g, HP, CP, HID, C, HID ** -0.5).to(bf)          # [hidden j][channel c] = fc2.weight^T
        inp["w1t"] = _padded(g, CP, HP, C, HID, C ** -0.5).to(bf)            # [channel c][hidden j] = fc1.weight^T
        u = 1.5 * _padded(g, M, HP, M, HID, 1.0)
        pick = torch.rand(M, HP, generator=g) < 0.03
        u[pick] = (12.0 * torch.rand(M, HP, generator=g) - 6.0)[pick]      # |u| up to 6
        u[:, HID:] = 0.0
        inp["u"] = u.to(bf)
        inp["udg"] = dgelu(u.double()).to(bf)                               # what mlp_fused_fwd_kernel<true> leaves (pads: gelu'(0) = 0.5)
        inp.update(_ln_operands(g, M))
    elif c.kind == "attn":
        xn = torch.full((M, c.lda), 1000.0)                                 # beyond column 192: never read
        xn[:, :CP] = _padded(g, M, CP, M, C, 1.0)
        inp["xn"] = xn.to(bf)
        inp["wqkv"] = _heads(_padded(g, CP, 3 * CA, C, 3 * CA, 0.08)).t().contiguous().to(bf)     # [576 (which, head, d)][192]
        inp["bqkv"] = _heads(0.2 * torch.randn(1, 3 * CA, generator=g))[0].contiguous()
        inp["table"] = 0.5 * torch.randn(225, NH, generator=g)
    elif c.kind == "proj":
        inp["ao"] = _heads(torch.randn(M, CA, generator=g)).to(bf)
        inp["w"] = _heads(_padded(g, CP, CA, C, CA, C ** -0.5)).to(bf)      # [channel][attention channel (head, d)]
        inp["b"] = _bias(g, CP, C)
        inp["res"] = _padded(g, M, CP, M, C, 1.0)
        inp["gamma"] = torch.zeros(CP)
        inp["gamma"][:C] = 1.0 + 0.5 * torch.randn(C, generator=g)
        inp["beta"] = _padded(g, 1, CP, 1, C, 0.3)[0]
    elif c.kind == "lnbwd":
        inp["dqkv"] = _heads(0.5 * torch.randn(M, 3 * CA, generator=g)).to(bf)
        inp["wt"] = _heads(_padded(g, CP, 3 * CA, C, 3 * CA, (3 * C) ** -0.5)).to(bf)     # [channel][576] = qkv.weight^T
        inp.update(_ln_operands(g, M))
        inp["skip0"] = _padded(g, M, CP, M, C, 1.0)
    else:
        raise ValueError(c.kind)
    return inp


# ---- tolerances -----------------------------------------------------------------------------------------------------------------------
class BTol(Tol):
    """Tolerances of the fused-block tests, derived from the number formats in the manner of gemm_ex_ref.Tol (whose f32 / bf16 / dgelu /
    ln_fwd / lnbwd / scaled_bf16 are used unchanged; delta = 2 K u S is its accumulation bound).  Every multi-stage kernel is checked
    STAGE BY STAGE: an exposed intermediate (u / h, d u, q / k / v, the fp32 residual row) is compared with the fp64 value from the
    bf16 operands; the stage behind it with the fp64 evaluation from the DEVICE's own intermediate, so that a half-ulp flip of one h
    does not widen the bound of out.

      dgelu_store(ref, delta)   u_out = bf16(gelu'(u)) of the unrounded u = acc + b: 2^-8 |ref| + 0.8 delta + 8u + tiny -- 0.8 >= max |gelu''|
                                = 2 phi(0); 8u (absolute: |gelu'| <= 1.13) is the project's convention for the device erf / exp
      mul_bf16(ref, delta, a)   bf16(acc * a) with an exact bf16 factor a: 2^-8 |ref| + |a| delta + 2u |ref| + tiny
      q (scaled)                bf16((acc + b) * scale): Tol.bf16 with delta * |scale| + 2u |ref| for the extra product
      attn(...)                 o = sum_j bf16(e_j) v_j / sum_j e_j, e_j = exp2(s_j log2e - max log2e), from the DEVICE's q / k / v (exact
                                bf16 values, products exact in fp32).  Scores: ds_j = 2 * 32 u sum_d |q k| + 2u (|bias_j| + 100) for the
                                MFMA accumulation and the bias / mask additions.  The device exponential gets 8u.  To first order
                                |d p_j| / p_j <= (ds_j + 8u) + max_j (ds_j + 8u) (numerator and denominator), so with A = sum_j p_j |v_j|
                                and As = sum_j p_j |v_j| ds_j:
                                  2^-8 |o|              the stored bf16
                                  + 2 * 2^-8 A          the numerators are rounded to bf16 as the MFMA operand; the factor 2 covers a
                                                        denominator formed from rounded or unrounded numerators
                                  + As + (max_j ds_j + 16u) A        propagated score and exp errors
                                  + 64u A               64 fp32 additions of the P V product, the row sum, the reciprocal, the scaling
                                  + tiny

    Measured on MI355X (256 CUs; max err / tol over all cases; no factor had to be replaced):
      fused MLP forward    u (or gelu'(u)) 0.982, h 0.979 -- the bound is the bf16 rounding itself; out 0.004 (2 K u S is a worst case, the
                           errors add like a random walk); xn_next 0.995, mean 0.034, rstd 0.317
      fused MLP backward   d u 0.979, gx 0.003, gxb 0.984, d gamma / d beta < 0.001 (their bound is the M u sum of an atomic sum in ANY order)
      attention            q / k / v 0.978, ao 0.484 with the issue's own score bound (both kernels, bit-equal to each other); the steady-state
                           shape (11, 64, 72) -> 792 windows alone: q / k / v 0.978, ao 0.411
      proj_residual        out 0.006, xn 0.995, mean 0.032, rstd 0.361 (streaming and tile kernel)
      qkv_dgrad_lnbwd      gx / ln_skip 0.001, gxb 0.962, d gamma / d beta < 0.001
    (the d gamma / d beta bound weighs about one 16-row tile at these M; tests/test_gpu_block_fused.py therefore also asserts d beta of
    integer operands, which is exact in any summation order, with equality).  The one finding of the first run was not a value: with
    rows_per_sample != H*W the streaming kernel took the DropPath sample of a window-ordered tile from its image while the tile kernel
    takes it from the token; srk_launch_gemm_stream now leaves that case to the tile kernel (csrc/gemm_stream.hip)."""

    @staticmethod
    def dgelu_store(ref, delta):
        return BF16_REL * ref.abs() + DGELU_LIP * delta + 8 * U + BF16_TINY

    @staticmethod
    def mul_bf16(ref, delta, a):
        return BF16_REL * ref.abs() + a.abs() * delta + 2 * U * ref.abs() + BF16_TINY

    @staticmethod
    def attn(o, A, As, ds_max):
        return BF16_REL * o.abs() + 2 * BF16_REL * A + As + (ds_max + 16 * U) * A + 64 * U * A + BF16_TINY


def _exact_where_dropped(ref_t: torch.Tensor, tol: torch.Tensor, f: torch.Tensor):
    """Rows whose DropPath factor is exactly 0: the output IS the other operand, bit for bit (tolerance 0)."""
    tol = tol.clone()
    tol[(f == 0).expand_as(tol)] = 0.0
    return tol


# ---- fused MLP forward ------------------------------------------------------------------------------------------------------------------
def mlp_fwd_core(inp):
    xn, w1 = inp["xn"].double(), inp["w1"].double()
    return xn @ w1.t(), xn.abs() @ w1.abs().t()


def mlp_fwd_stage1(c: BCase, inp, core=None, v: Variant = OK) -> Dict[str, Out]:
    """u = xn W1^T + b1 (fp32); u_out = bf16(u) or bf16(gelu'(u)) of the UNROUNDED u; h_out = bf16(gelu(u))."""
    acc, S = core if core is not None else mlp_fwd_core(inp)
    b1 = inp["b1"].double()
    u = acc + b1
    d = Tol.delta(CP, S + b1.abs())
    out = {"h": Out(gelu(u), Tol.bf16(gelu(u), d, GELU_LIP), "bf16")}
    if c.dg:
        ud = dgelu(round_as(u, "bf16") if v.dgelu_of_rounded else u)
        out["u"] = Out(ud, BTol.dgelu_store(dgelu(u), d), "bf16")
    else:
        out["u"] = Out(u, Tol.bf16(u, d), "bf16")
    return out


def mlp_fwd_stage2(c: BCase, inp, h_dev: torch.Tensor, v: Variant = OK) -> Dict[str, Out]:
    """out = res + f (h W2^T + b2) from the given (device's own) bf16 h."""
    h, w2, b2, res = h_dev.double(), inp["w2"].double(), inp["b2"].double(), inp["res"].double()
    f = row_factor(c, torch.arange(c.M), v)
    acc, S = h @ w2.t(), h.abs() @ w2.abs().t()
    y = res + f * (acc + b2)
    tol = Tol.f32(y, Tol.delta(HP, f.abs() * (S + b2.abs()) + res.abs()))
    return {"out": Out(y, _exact_where_dropped(y, tol, row_factor(c, torch.arange(c.M))), "f32")}


def ln_rows(c: BCase, inp, out_dev: torch.Tensor, window: bool, v: Variant = OK) -> Dict[str, Out]:
    """The fused LayerNorm of the freshly written fp32 rows (the device's own), in token order or in window order of (H, W, shift)."""
    Cn = CP if v.ln_over_cp else C
    x, gam, bet = out_dev.double(), inp["gamma"].double(), inp["beta"].double()
    xn, mean, rstd = ln_fwd(x, gam, bet, Cn)
    t, t_mean, t_rstd = Tol.ln_fwd(xn, x, rstd, gam, bet, C)
    o = {"xn_out": (xn, t, "bf16"), "xn_mean": (mean[:, None], t_mean, "f32"), "xn_rstd": (rstd[:, None], t_rstd, "f32")}
    if window:
        tok = win_to_token(c.B, c.H, c.W, c.shift, v)
        tok_ok = win_to_token(c.B, c.H, c.W, c.shift)
        return {k: Out(r[tok], tl[tok_ok], kind) for k, (r, tl, kind) in o.items()}
    return {k: Out(r, tl, kind) for k, (r, tl, kind) in o.items()}


# ---- fused MLP backward -----------------------------------------------------------------------------------------------------------------
def mlp_bwd_core(inp):
    g, w = inp["g"].double(), inp["w2t"].double()
    return g @ w.t(), g.abs() @ w.abs().t()


def mlp_bwd_stage1(c: BCase, inp, core=None, v: Variant = OK) -> Dict[str, Out]:
    """d u = bf16((g W2) * gelu'(u)), or * u_stored when the buffer holds gelu'(u)."""
    acc, S = core if core is not None else mlp_bwd_core(inp)
    d = Tol.delta(CP, S)
    if c.dg:
        a = inp["udg"].double()
        return {"du": Out(acc * a, BTol.mul_bf16(acc * a, d, a), "bf16")}
    y = acc * dgelu(inp["u"].double())
    return {"du": Out(y, Tol.dgelu(y, d, acc), "bf16")}


def _lnbwd_outputs(c, acc, S, K, x, mean, rstd, gam, old, f, dg0, db0, v, old_abs=None):
    """Rows in ANY common order: (y = old + dx, its tolerance, the bf16 copy's Out, dgamma Out, dbeta Out).  old_abs: the sum of the
    absolute terms that make up `old` (the ln_skip form adds two streams)."""
    Cn = CP if v.ln_over_cp else C
    dx, dg, db = ln_bwd(acc, x, mean, rstd, gam, Cn)
    dx[:, C:] = 0.0
    y = old + dx
    xh = (x[:, :C] - mean[:, None]) * rstd[:, None]
    t_dx, t_dg, t_db = Tol.lnbwd(Tol.delta(K, S)[:, :C], acc[:, :C], xh, gam[:C], rstd, (old if old_abs is None else old_abs)[:, :C])
    t = torch.zeros_like(y)
    t[:, :C] = t_dx
    yb = y * f
    return y, t, Out(yb, Tol.scaled_bf16(yb, f, t), "bf16"), Out((dg0 + dg[:C])[None], t_dg[None], "f32"), Out((db0 + db[:C])[None], t_db[None], "f32")


def mlp_bwd_stage2(c: BCase, inp, du_dev: torch.Tensor, v: Variant = OK, old=None, dg0=None, db0=None) -> Dict[str, Out]:
    """d xn = d u W1 from the given (device's own) d u; norm2's backward in token order: gx += d x, gxb[window row of t or t] =
    bf16(gx[t] f[t]), d gamma / d beta accumulated."""
    du, w = du_dev.double(), inp["w1t"].double()
    acc, S = du @ w.t(), du.abs() @ w.abs().t()
    rows = torch.arange(c.M)
    f = row_factor(c, rows, v)
    old = inp["gx0"].double() if old is None else old
    dg0 = inp["dgamma0"].double() if dg0 is None else dg0
    db0 = inp["dbeta0"].double() if db0 is None else db0
    y, t, gxb, dgo, dbo = _lnbwd_outputs(c, acc, S, HP, inp["ln_x"].double(), inp["ln_mean"].double(), inp["ln_rstd"].double(),
                                         inp["ln_gamma"].double(), old, f, dg0, db0, v)
    tok, tok_ok = win_to_token(c.B, c.H, c.W, c.shift, v), win_to_token(c.B, c.H, c.W, c.shift)
    return {"gx": Out(y, t, "f32"), "gxb": Out(gxb.ref[tok], gxb.tol[tok_ok], "bf16"), "dgamma": dgo, "dbeta": dbo}


# ---- qkv projection + window attention forward ----------------------------------------------------------------------------------------------
def attn_core(inp):
    xn, w = inp["xn"].double()[:, :CP], inp["wqkv"].double()
    return xn @ w.t(), xn.abs() @ w.abs().t()


def _to_heads(t: torch.Tensor, B_: int) -> torch.Tensor:
    """[B_*64][576] columns (which, head, d) -> the device's qkv layout [3][B_][6][64][32]."""
    return t.view(B_, 64, 3, NH, DP).permute(2, 0, 3, 1, 4).contiguous()


def attn_qkv(c: BCase, inp, scale: float, core=None, v: Variant = OK) -> Out:
    """q = bf16((acc + b) * scale), k, v = bf16(acc + b), as [3][B_][6][64][32] flattened to [3 B_ 6 64][32]."""
    acc, S = core if core is not None else attn_core(inp)
    b = inp["bqkv"].double()
    u, d = acc + b, Tol.delta(CP, S + b.abs())
    sc = torch.ones(3 * CA, dtype=torch.float64)
    sc[:CA] = scale
    ref = round_as(u, "bf16") * sc if v.scale_after_round else u * sc
    tol = Tol.bf16(u * sc, d * sc) + 2 * U * (u * sc).abs()
    return Out(_to_heads(ref, c.B_).reshape(-1, DP), _to_heads(tol, c.B_).reshape(-1, DP), "bf16")


def attn_out(c: BCase, inp, qkv_dev: torch.Tensor, v: Variant = OK) -> Out:
    """ao [B_*64][192] = softmax(q k^T + table[rpi] + mask) v from the given (device's own) q / k / v [3][B_][6][64][32]."""
    q, k, vv = qkv_dev.double().view(3, c.B_, NH, 64, DP)
    bias = dense_bias(inp["table"].double(), v)[None]
    s = q @ k.transpose(-1, -2) + bias
    sabs = q.abs() @ k.abs().transpose(-1, -2)
    ds = 2 * DP * U * sabs + 2 * U * (bias.abs() + 100.0)
    if c.shift and not v.no_mask:
        m = shift_mask(c.H, c.W, v)
        nW = m.shape[0]
        s = (s.view(c.B_ // nW, nW, NH, 64, 64) + m[None, :, None]).view(c.B_, NH, 64, 64)
    p = torch.softmax(s, -1)
    o = p @ vv
    A, As = p @ vv.abs(), (p * ds) @ vv.abs()
    tol = BTol.attn(o, A, As, ds.amax(-1, keepdim=True))
    tol[..., D:] = 0.0                                       # pad channels: exactly 0
    flat = lambda t: t.permute(0, 2, 1, 3).reshape(c.M, CA)
    return Out(flat(o), flat(tol), "bf16")


# ---- proj + window reverse + un-roll + residual (+ norm2) --------------------------------------------------------------------------------
def proj_core(inp):
    a, w = inp["ao"].double(), inp["w"].double()
    return a @ w.t(), a.abs() @ w.abs().t()


def proj_residual(c: BCase, inp, core=None, v: Variant = OK) -> Dict[str, Out]:
    """EP_PROJ_RES (csrc/gemm.h): t = token(m): out[t] = res[t] + f[t / rows_per_sample] (ao[m] . W^T + b)."""
    acc, S = core if core is not None else proj_core(inp)
    b, res = inp["b"].double(), inp["res"].double()
    tok = win_to_token(c.B, c.H, c.W, c.shift, v)
    inv_ok = token_to_win(c.B, c.H, c.W, c.shift)
    rows = torch.arange(c.M)
    y = res.clone()
    y[tok] = res[tok] + row_factor(c, tok, v) * (acc + b)
    f_ok = row_factor(c, rows)
    tol = Tol.f32(y, Tol.delta(CA, f_ok.abs() * (S + b.abs())[inv_ok] + res.abs()))
    return {"out": Out(y, _exact_where_dropped(y, tol, f_ok), "f32")}


# ---- qkv dgrad + norm1 backward + window reverse + un-roll (+ RSTB skip fold) -----------------------------------------------------------------
def lnbwd_core(inp):
    a, w = inp["dqkv"].double(), inp["wt"].double()
    return a @ w.t(), a.abs() @ w.abs().t()


def qkv_dgrad_lnbwd(c: BCase, inp, core=None, v: Variant = OK, old=None, dg0=None, db0=None, skip0=None) -> Dict[str, Out]:
    """EP_LNBWD as the executor runs it (csrc/gemm.h): row m in window order, statistics at m, t = token(m): gx[t] += dx, gxb[t] =
    bf16(gx[t] f[t]); ln_skip form: ln_skip[t] = gx[t] + dx + ln_skip[t], gx untouched, gxb its scaled bf16 copy."""
    acc, S = core if core is not None else lnbwd_core(inp)
    tok, tok_ok = win_to_token(c.B, c.H, c.W, c.shift, v), win_to_token(c.B, c.H, c.W, c.shift)
    inv_ok = token_to_win(c.B, c.H, c.W, c.shift)
    old = inp["gx0"].double() if old is None else old
    dg0 = inp["dgamma0"].double() if dg0 is None else dg0
    db0 = inp["dbeta0"].double() if db0 is None else db0
    skip = (inp["skip0"].double() if skip0 is None else skip0) if c.skip else None
    base = old + skip if c.skip else old
    # everything in window order (the order of the GEMM rows), then scattered to token order
    y_w, t_w, gxb_w, dgo, dbo = _lnbwd_outputs(c, acc, S, 3 * CA, inp["ln_x"].double()[tok], inp["ln_mean"].double(), inp["ln_rstd"].double(),
                                               inp["ln_gamma"].double(), base[tok], row_factor(c, tok, v), dg0, db0, v,
                                               (old.abs() + skip.abs())[tok_ok] if c.skip else None)
    y, gb = torch.empty_like(y_w), torch.empty_like(y_w)
    y[tok], gb[tok] = y_w, gxb_w.ref
    t, tb = t_w[inv_ok], gxb_w.tol[inv_ok]
    out = {"gxb": Out(gb, tb, "bf16"), "dgamma": dgo, "dbeta": dbo}
    if c.skip:
        out["skip"] = Out(y, t, "f32")
        out["gx"] = Out(y if v.skip_into_outf else old, torch.zeros_like(t), "f32")       # untouched, bit for bit
    else:
        out["gx"] = Out(y, t, "f32")
    return out


# ---- negative controls ----------------------------------------------------------------------------------------------------------------------
def controls_for(c: BCase) -> Dict[str, Variant]:
    """The negative controls that apply to a case."""
    out: Dict[str, Variant] = {}
    k = c.kind
    window_rows = k in ("proj", "lnbwd") or k in ("mlp_fwd", "mlp_bwd")      # the MLP pair: the window-ordered xn_next / gxb
    if window_rows and c.shift and ((2 * c.shift) % c.H or (2 * c.shift) % c.W):      # an 8 x 8 image rolled by +4 is rolled by -4
        out["shift applied with the wrong sign"] = Variant(shift_sign=True)
    if (window_rows or (k == "attn" and c.shift)) and c.H != c.W:
        out["H and W swapped in the row map"] = Variant(swap_hw=True)
    if k != "attn" and c.rs == "mix" and c.M > c.rps:
        out["rowscale of the neighbouring sample"] = Variant(shift_rowscale=True)
    if k != "attn":
        out["LayerNorm over 192 instead of 180"] = Variant(ln_over_cp=True)
    if k == "mlp_fwd" and c.dg:
        out["gelu' of the rounded u"] = Variant(dgelu_of_rounded=True)
    if k == "attn":
        if c.shift:
            out["mask dropped"] = Variant(no_mask=True)
        out["bias table transposed"] = Variant(bias_transposed=True)
        out["q scale applied after the rounding"] = Variant(scale_after_round=True)
    if k == "lnbwd" and c.skip:
        out["ln_skip added into outf"] = Variant(skip_into_outf=True)
    return out


CORES = {"mlp_fwd": mlp_fwd_core, "mlp_bwd": mlp_bwd_core, "attn": attn_core, "proj": proj_core, "lnbwd": lnbwd_core}
SCALE = float(torch.tensor(D ** -0.5, dtype=torch.float32))      # the ABI passes the q scale as a float


_memo: Dict = {}


def _memoised(c: BCase, key, fn):
    """Stage results are shared between the cases of one shape (shift / rowscale / dg / control only change some stages)."""
    if _memo.get("shape") != c.shape_key:
        _memo.clear()
        _memo["shape"] = c.shape_key
    if key not in _memo:
        _memo[key] = fn()
    return _memo[key]


def host_outputs(c: BCase, inp, core, v: Variant = OK) -> Dict[str, Out]:
    """Every output of one call with the intermediates taken from the fp64 reference ROUNDED as the device rounds them (what a correct
    kernel would hand to its next stage): the CPU tests and the negative controls run on this; the GPU test substitutes the device's own
    intermediates stage by stage.  `inp` / `core` must be those of c's shape (make_inputs is deterministic per shape)."""
    k = c.kind
    geo = (c.shift, v.shift_sign, v.swap_hw)
    if k == "mlp_fwd":
        o = dict(_memoised(c, ("s1", c.dg, v.dgelu_of_rounded), lambda: mlp_fwd_stage1(c, inp, core, v)))
        h = _memoised(c, "h", lambda: mlp_fwd_stage1(with_(c, dg=0), inp, core)["h"].rounded().to(torch.bfloat16))
        o.update(_memoised(c, ("s2", c.rs, v.shift_rowscale), lambda: mlp_fwd_stage2(c, inp, h, v)))
        good = _memoised(c, ("s2", c.rs, False), lambda: mlp_fwd_stage2(c, inp, h))["out"].rounded().float()
        o.update(_memoised(c, ("ln", c.rs, geo, v.ln_over_cp), lambda: ln_rows(c, inp, good, True, v)))
        return o
    if k == "mlp_bwd":
        o = dict(_memoised(c, ("s1", c.dg), lambda: mlp_bwd_stage1(c, inp, core)))
        o.update(mlp_bwd_stage2(c, inp, o["du"].rounded().to(torch.bfloat16), v))
        return o
    if k == "attn":
        qkv = _memoised(c, ("qkv", v.scale_after_round), lambda: attn_qkv(c, inp, SCALE, core, v))
        good = _memoised(c, ("qkv", False), lambda: attn_qkv(c, inp, SCALE, core)).rounded().to(torch.bfloat16)
        return {"qkv": qkv, "ao": attn_out(c, inp, good, v)}
    if k == "proj":
        o = dict(proj_residual(c, inp, core, v))
        good = _memoised(c, ("out", c.rs, c.shift), lambda: proj_residual(c, inp, core))["out"].rounded().float()
        o.update(ln_rows(c, inp, good, False, v))
        return o
    return qkv_dgrad_lnbwd(c, inp, core, v)


def all_cases(n: int = 256) -> List[BCase]:
    return row_cases(n) + attn_cases(n)


def for_device(c: BCase, n: int) -> BCase:
    """The case of a device with n CUs that corresponds to a case of the 256-CU matrix (the test ids are those of the 256-CU matrix; the
    shapes follow the device)."""
    if n == 256 or c.small:
        return c
    ref, dev = (attn_shapes(256), attn_shapes(n)) if c.kind == "attn" else (row_shapes(256), row_shapes(n))
    B, H, W = dev[ref.index((c.B, c.H, c.W))]
    return replace(c, B=B, H=H, W=W)


def with_(c: BCase, **kw) -> BCase:
    return replace(c, **kw)
