"""fp64 restatements, case lists and derived tolerances of DAT's token passes and token reductions (include/srk.h: srk_rowln_bf16,
srk_rowln_bwd_bf16, srk_chan_stats, srk_sum_rows_f32, srk_bn_train_coeffs, srk_bn_train_bwd_coeffs, srk_affine_act_bf16,
srk_dgelu_affine_bf16, srk_lincomb2_bf16, srk_mul_bwd_bf16, srk_dual_gate_combine, srk_dual_gate_bwd, srk_dwconv3x3, srk_dwconv3x3_wgrad,
srk_chan_gram, srk_chan_apply_mat, srk_channel_attention_fwd, srk_spatial_gate_train; csrc/dat_train.hip and the non-attention half of
csrc/dat.hip).

Plain torch on the CPU, no GPU import.  tests/test_dat_ref.py pins the restatements against torch.nn.functional / autograd and exercises
their negative controls; tests/test_gpu_dat_direct.py compares the kernels with them through the C ABI.

Tolerances.  u = 2^-24 (fp32), 2^-8 the unit roundoff of bf16 (gemm_ex_ref.BF16_REL, the figure tests/attn_ref.py settled on).  An fp32
sum of L terms in ANY order is off by at most Tol.delta(L, S) = 2 L u S, S = the sum of the absolute terms.  The operands are exact
bf16 values, so a product of two of them is exact in fp32.  No figure below is fitted to what the kernels return.

  bf16 output     t_bf16(ref, t32) = t32 + 2^-8 |ref| + tiny: the fp32 bound of the value plus its one rounding.
  bit equality    where the kernel is a fixed sequence of IEEE operations the expectation is the same sequence in fp32 on the CPU, with
                  torch's round-to-nearest-even store: mul_bwd (one product, exact in fp32, one rounding), the d_chan / d_tok products of
                  dual_gate_bwd (bf16 x fp32, one fp32 rounding, one bf16 rounding), the forms of lincomb2 that come down to ONE operation
                  (copy: 0 + p; A p: 0 + A p; old + p; old + C -- the unused terms of  old + A p + B q + C  are 1 * 0 or + 0 and change
                  nothing, whether or not the compiler contracts them; a -0 operand comes out +0 because 0 + -0 = +0).
  contraction     device code is built with the compiler's default contraction, so  x * s + t  of affine_act (act 0) is ONE fused
                  multiply-add: expected fma(x, s, t), evaluated exactly (a bf16 x fp32 product has 32 significant bits and its sum with
                  an fp32 value is formed in fp64) and rounded once.  dual_gate_combine's  a * g1 + b * g2  may contract around either
                  product; the three evaluations (none, around the first, around the second) are all within its bound
                  Tol.delta(2, |a g1| + |b g2|), and the GPU test requires the output to be bit-equal to ONE of them throughout.
  GELU, GELU'     the device functions are gelu_f / dgelu_shared_exp of the GEMM epilogues: GELU_LIP times the bound of the argument plus
                  the 8u |v| device-function term of Tol.dgelu (erf by Abramowitz-Stegun 7.1.26, |err| <= 1.5e-7 = 2.5u, one hardware
                  reciprocal, one hardware exp), v the factor that multiplies the function (the argument itself for gelu = v Phi(v)).
  reductions      chan_stats, sum_rows, the dwconv weight gradient, dcg_partial, dsmap, chan_gram: Tol.delta(L, S), L the number of terms.
  chan_apply_mat  Tol.delta(34, sum |M src| + |diag src2| + |old|) (32 multiply-adds and two additions), then bf16.
  channel attention, spatial_gate_train: chains of the above; the derivations stand in the docstrings of channel_attention_ref and
                  spatial_gate_train_ref.
  one-pass stats  bn_train_coeffs / bn_train_bwd_coeffs form their statistics from sums BY DESIGN; the reference reads the same fp32
                  partial rows in fp64, so only the kernel's own arithmetic is bounded:
                    s1, s2   Tol.delta(R, sum |rows|)
                    mean     t_s1 / n + u |mean|
                    var      t_s2 / n + 2 |mean| t_mean + u (s2 / n + mean^2) + u |var|     the cancellation term: two roundings of the size
                             of the operands, not of the difference
                    rstd     the exact image of [var - t_var, var + t_var] (clamped at 0) under (. + eps)^-1/2, plus 4u rstd for the
                             hardware reciprocal square root -- not a first-order figure: at a constant channel t_var is not small
                             against eps
                    scale    |gamma| t_rstd + u |scale|;   shift  |scale| t_mean + |mean| t_scale + u (|mean scale| + |shift|)
                    running  momentum times the bound of mean / var n / (n - 1), plus 4u of the absolute terms
                    dgamma = rstd (S2 - mean S1):  rstd (t_S2 + |mean| t_S1 + u (|S2| + 2 |mean S1|)) + u |dgamma| -- the same cancellation
                    B = -scale rstd dgamma / n, C = scale / n (mean rstd dgamma - S1): first order in t_dgamma, t_S1, plus 4u of the terms
  row LayerNorm   rowln_bf16 and rowln_bwd_bf16 are bounded for a TWO-PASS evaluation of the row statistics (mean, then the variance from
                  x - mean), as glue_ref bounds srk_layernorm_fwd, with two refinements that the offset rows (|mean| >> std) need:
                    * the sums run down a tree of depth <= ROWLN_DEPTH = 38 (a lane adds at most 8 x 4 values in sequence, then at most six
                      butterfly levels): Tol.delta(38, .), not the any-order figure with L = C;
                    * the row sum of bf16 values is EXACT where they share a quantum and stay below 2^24 quanta (_row_sum_bound: the offset
                      rows, whose values are 196 .. 204 in steps of 1 or 30 .. 34 in steps of 1/4), so there
                      t_mean = 2u |mean| (the reciprocal of C and the product), else Tol.delta(38, sum |x|) / C + 2u |mean|;
                    * a wrong mean m + e shifts every deviation by the same e, and sum_i (d_i - e)^2 = sum d_i^2 + C e^2 exactly because
                      sum d_i = 0: the variance of a two-pass evaluation moves by e^2, not by 2 |d| e:
                        t_var = t_mean^2 + (3u sum (|d| + t_mean)^2 + Tol.delta(38, sum (|d| + t_mean)^2)) / C + 2u var
                        t_rstd = the exact image of var +- t_var as above + 4u rstd
                    forward   y = d rstd gamma + beta:  |gamma| (rstd t_d + |d| t_rstd) + 8u (|d rstd gamma| + |beta|), then bf16
                    backward  dx = rstd (g - s1 - xh s2), g = dy gamma, s1 = mean(g), s2 = mean(g xh): first-order propagation of
                              t_xh = rstd t_d + |d| t_rstd + 2u |xh| through the formula, Tol.delta(38, .) / C for the two means, then bf16;
                              partials: sum over the block's rows of |dy| t_xh + Tol.delta(rows of the block, sum |dy xh|)
                  A ONE-PASS variance E[x^2] - mean^2 in fp32 is NOT within this bound on the offset rows (relative rstd error up to 3e-3
                  at mean 200 / std 1); the mutant 'one_pass_f32' is that evaluation and must be rejected.

Cases.  Operands are bf16 slices at a non-zero 8-element column offset inside wider rows (ld > width): `embed` builds them; everything
outside a slice is NaN.  The grid-stride wrap of the row-walking element-wise kernel (affine_act, lincomb2) needs more than
65535 x lanes x 4 > 10^6 rows and is not reachable at test size; it is not tested.

Negative controls: every restatement takes mut = <name>; *_MUTANTS lists them per family, *_identity names the (mutant, case) pairs on
which a mutant IS the reference by construction and *_exercises those on which a case reaches the mutated code at all."""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import torch
import torch.nn.functional as F

import gemm_ex_ref as G
from gemm_ex_ref import BF16_REL, BF16_TINY, GELU_LIP, LN_EPS, U, Tol
from glue_ref import Out, accepts, bits, same_bits  # noqa: F401  (re-exported for the tests)

BF = torch.bfloat16
ROWLN_DEPTH = 38


def t_bf16(ref: torch.Tensor, t32) -> torch.Tensor:
    return t32 + BF16_REL * ref.abs() + BF16_TINY


def fma32(a: torch.Tensor, b: torch.Tensor, c: torch.Tensor) -> torch.Tensor:
    """fp32 fused multiply-add of a bf16-valued a (or b) with fp32 operands: the product has at most 32 significant bits, so it and its sum
    with c are formed in fp64 and rounded once to fp32."""
    return (a.double() * b.double() + c.double()).float()


def embed(t: torch.Tensor, ld: int, off: int, fill: float = float("nan")) -> torch.Tensor:
    """[rows][width] -> [rows][ld] with the slice at column `off`, `fill` elsewhere."""
    out = torch.full((t.shape[0], ld), fill, dtype=t.dtype)
    out[:, off:off + t.shape[1]] = t
    return out


def _gen(*key: int) -> torch.Generator:
    s = 0
    for k in key:
        s = (s * 1000003 + int(k) + 17) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(s)


def _image_of_rsqrt(var: torch.Tensor, t_var: torch.Tensor, eps: float) -> torch.Tensor:
    r = (var + eps).rsqrt()
    lo, hi = (var + t_var + eps).rsqrt(), ((var - t_var).clamp_min(0.0) + eps).rsqrt()
    return torch.maximum(hi - r, r - lo) + 4 * U * r


# ---- row LayerNorm on bf16 rows: srk_rowln_bf16, srk_rowln_bwd_bf16 ---------------------------------------------------------------------
ROWLN_C_CP = ((5, 8), (90, 128), (180, 192), (360, 384), (500, 512))
ROWLN_ROWS = (1, 15, 17, 300)
ROWLN_BWD_CAP = 1024                       # srk_rowln_bwd_blocks: min(1024, ceil(rows / 16))
ROWLN_FAMILIES = ("mean200", "constant", "zero_mean", "mean32")       # row r belongs to family r % 4: a single row is an offset row


@dataclass(frozen=True)
class RowlnCase:
    C: int
    CP: int
    rows: int

    @property
    def id(self) -> str:
        return f"C{self.C}of{self.CP}-rows{self.rows}"


ROWLN_FWD_CASES = [RowlnCase(C, CP, r) for C, CP in ROWLN_C_CP for r in ROWLN_ROWS]
ROWLN_BWD_CASES = ROWLN_FWD_CASES + [RowlnCase(180, 192, ROWLN_BWD_CAP * 16 + 16)]


def rowln_bwd_K(CP: int) -> int:
    return 1 if CP <= 128 else 3 if CP <= 384 else 4


def rowln_fwd_LPR(CP: int) -> int:
    return 16 if CP <= 128 else 32 if CP <= 256 else 64


def rowln_bwd_blocks(rows: int) -> int:
    return max(1, min(ROWLN_BWD_CAP, -(-rows // 16)))


def rowln_coverage(cases: List[RowlnCase]) -> Dict[str, object]:
    return dict(K=sorted({rowln_bwd_K(c.CP) for c in cases}), LPR=sorted({rowln_fwd_LPR(c.CP) for c in cases}),
                straddle=any(c.C % 8 for c in cases), dead_pieces=any(c.CP - c.C >= 8 for c in cases),
                partial_group=any(c.rows % 16 for c in cases), single_row=any(c.rows == 1 for c in cases),
                capped=any(-(-c.rows // 16) > ROWLN_BWD_CAP for c in cases), families=min(c.rows for c in cases if c.rows >= 4) >= 4)


def rowln_inputs(c: RowlnCase) -> Dict[str, torch.Tensor]:
    """x, dy bf16 [rows][C]; gamma, beta fp32 [C].  Row families by r % 4: mean 200 / std 1, a constant row (5.0), zero mean with std 4e-3
    (variance ~ eps), mean 32 / std 0.5."""
    g = _gen(1, c.C, c.CP, c.rows)
    n = torch.randn(c.rows, c.C, generator=g)
    fam = torch.arange(c.rows) % 4
    mean = torch.tensor([200.0, 5.0, 0.0, 32.0])[fam][:, None]
    std = torch.tensor([1.0, 0.0, 4e-3, 0.5])[fam][:, None]
    x = (n * std + mean).to(BF)
    dy = torch.randn(c.rows, c.C, generator=g).to(BF)
    return dict(x=x, dy=dy, gamma=torch.rand(c.C, generator=g) + 0.5, beta=torch.randn(c.C, generator=g) * 0.1)


def _row_sum_bound(xd: torch.Tensor) -> torch.Tensor:
    """Bound of the fp32 sum of each row of bf16 values: every value is an integer multiple of the row's quantum 2^(e_min - 8) (8
    significant bits, e_min the smallest exponent of a non-zero entry), and so is every partial sum; where sum |x| < 2^24 quanta all of
    them are representable and the sum is EXACT in any order.  Otherwise the tree bound Tol.delta(ROWLN_DEPTH, sum |x|)."""
    _, e = torch.frexp(xd)
    e = torch.where(xd == 0, torch.full_like(e, 1 << 20), e).amin(1)
    S = xd.abs().sum(1)
    quantum = torch.where(e < (1 << 20), torch.ldexp(torch.ones_like(S), (e - 8).clamp(-1000, 1000)), torch.ones_like(S))
    return torch.where(S < quantum * 2.0 ** 24, torch.zeros_like(S), Tol.delta(ROWLN_DEPTH, S))


def _rowln_stats(x: torch.Tensor, C: int):
    """exact statistics and the two-pass bounds (see the module docstring) -> mean, rstd, d, t_d, t_rstd"""
    xd = x.double()
    mean = xd.sum(1) / C
    d = xd - mean[:, None]
    var = (d * d).sum(1) / C
    rstd = (var + LN_EPS).rsqrt()
    t_mean = _row_sum_bound(xd) / C + 2 * U * mean.abs()
    sq = ((d.abs() + t_mean[:, None]) ** 2).sum(1)
    t_var = t_mean ** 2 + (3 * U * sq + Tol.delta(ROWLN_DEPTH, sq)) / C + 2 * U * var
    t_rstd = _image_of_rsqrt(var, t_var, LN_EPS)
    return mean, rstd, d, t_mean[:, None] + U * d.abs(), t_rstd


def _one_pass_f32(x: torch.Tensor, C: int):
    """the one-pass evaluation in fp32: mean = sum x / C, var = max(sum x^2 / C - mean^2, 0)"""
    xf = x.float()
    invC = torch.tensor(1.0 / C, dtype=torch.float32)
    mean = xf.sum(1) * invC
    var = ((xf * xf).sum(1) * invC - mean * mean).clamp_min(0.0)
    return mean.double(), (var + torch.tensor(LN_EPS, dtype=torch.float32)).rsqrt().double()


def rowln_fwd_ref(x, gamma, beta, CP: int, mut: Optional[str] = None) -> Dict[str, Out]:
    """out bf16 [rows][CP], columns C.. +0.  mut: 'div_cp', 'no_beta', 'no_eps'."""
    rows, C = x.shape
    mean, rstd, d, t_d, t_rstd = _rowln_stats(x, C)
    ga, be = gamma.double(), beta.double()
    exact = d * rstd[:, None] * ga + be
    t = ga.abs() * (rstd[:, None] * t_d + d.abs() * t_rstd[:, None]) + 8 * U * ((d * rstd[:, None] * ga).abs() + be.abs())
    if mut is not None:
        n = CP if mut == "div_cp" else C
        xd = x.double()
        m = xd.sum(1) / n
        dd = xd - m[:, None]
        r = ((dd * dd).sum(1) / n + (0.0 if mut == "no_eps" else LN_EPS)).rsqrt()
        val = dd * r[:, None] * ga + (0.0 if mut == "no_beta" else be)
    else:
        val = exact
    ref, tol = torch.zeros(rows, CP, dtype=torch.float64), torch.zeros(rows, CP, dtype=torch.float64)
    ref[:, :C], tol[:, :C] = val, t_bf16(exact, t)
    return dict(out=Out(ref, tol))


def rowln_bwd_ref(dy, x, gamma, CP: int, mut: Optional[str] = None) -> Dict[str, Out]:
    """dx bf16 [rows][CP] (columns C.. +0) and partial fp32 [blocks][2][C] (row m belongs to block (m / 16) % blocks).
    mut: 'div_cp', 'no_xhat_term', 'dgamma_no_xhat', 'one_pass_f32', 'tail_dropped' (the rows after the last full group of 16 are missing
    from the partials)."""
    rows, C = x.shape
    mean, rstd, d, t_d, t_rstd = _rowln_stats(x, C)
    ga, dyd = gamma.double(), dy.double()
    r_ = rstd[:, None]
    xh = d * r_
    g = dyd * ga
    s1, s2 = g.sum(1, keepdim=True) / C, (g * xh).sum(1, keepdim=True) / C
    inner = g - s1 - xh * s2
    dx = r_ * inner
    # bounds
    t_xh = r_ * t_d + d.abs() * t_rstd[:, None] + 2 * U * xh.abs()
    t_s1 = (Tol.delta(ROWLN_DEPTH, g.abs().sum(1, keepdim=True)) + U * g.abs().sum(1, keepdim=True)) / C + 2 * U * s1.abs()
    t_s2 = ((g.abs() * t_xh + 2 * U * (g * xh).abs()).sum(1, keepdim=True) + Tol.delta(ROWLN_DEPTH, (g * xh).abs().sum(1, keepdim=True))) / C \
        + 2 * U * s2.abs()
    t_inner = U * g.abs() + t_s1 + t_xh * s2.abs() + xh.abs() * t_s2 + 3 * U * (g.abs() + s1.abs() + (xh * s2).abs())
    t_dx = r_ * t_inner + t_rstd[:, None] * inner.abs() + U * dx.abs()
    nb = rowln_bwd_blocks(rows)
    blk = (torch.arange(rows) // 16) % nb
    per_blk = torch.bincount(blk, minlength=nb).double()[:, None]

    def blocks(v):
        return torch.zeros(nb, C, dtype=torch.float64).index_add_(0, blk, v)

    t_dg = blocks(dyd.abs() * t_xh + U * (dyd * xh).abs()) + Tol.delta(per_blk + 16, blocks((dyd * xh).abs()))
    t_db = Tol.delta(per_blk + 16, blocks(dyd.abs()))
    if mut is not None:
        n = CP if mut == "div_cp" else C
        m_, rs_ = mean, rstd
        if mut == "one_pass_f32":
            m_, rs_ = _one_pass_f32(x, C)
        if mut == "div_cp":
            m_ = x.double().sum(1) / n
            dd = x.double() - m_[:, None]
            rs_ = ((dd * dd).sum(1) / n + LN_EPS).rsqrt()
        xh = (x.double() - m_[:, None]) * rs_[:, None]
        s2m = 0.0 if mut == "no_xhat_term" else xh * ((g * xh).sum(1, keepdim=True) / n)
        dx = rs_[:, None] * (g - g.sum(1, keepdim=True) / n - s2m)
    keep = (torch.arange(rows) < rows // 16 * 16).double()[:, None] if mut == "tail_dropped" else 1.0
    dg = blocks(dyd * (1.0 if mut == "dgamma_no_xhat" else xh) * keep)
    db = blocks(dyd * keep)
    ref, tol = torch.zeros(rows, CP, dtype=torch.float64), torch.zeros(rows, CP, dtype=torch.float64)
    ref[:, :C], tol[:, :C] = dx, t_bf16(r_ * inner, t_dx)
    return dict(dx=Out(ref, tol), partial=Out(torch.stack([dg, db], 1), torch.stack([t_dg, t_db], 1)))


ROWLN_FWD_MUTANTS = ("div_cp", "no_beta", "no_eps")
ROWLN_BWD_MUTANTS = ("div_cp", "no_xhat_term", "dgamma_no_xhat", "one_pass_f32", "tail_dropped")


def rowln_identity(mut: str, c: RowlnCase) -> bool:
    return mut == "tail_dropped" and c.rows % 16 == 0


def rowln_exercises(mut: str, c: RowlnCase) -> bool:
    """no_eps needs a row whose variance is not far above eps (the constant row: rows >= 2).  Every case has an offset row (row 0), so the
    one-pass variance is exercised everywhere, C = 5 included."""
    return c.rows >= 2 if mut == "no_eps" else True


# ---- srk_chan_stats ---------------------------------------------------------------------------------------------------------------------
ST_ROWS = 256


@dataclass(frozen=True)
class StatsCase:
    C8: int
    rps: int
    samples: int

    @property
    def id(self) -> str:
        return f"C8_{self.C8}-rps{self.rps}-s{self.samples}"


STATS_CASES = [StatsCase(1, 1, 1), StatsCase(5, 7, 3), StatsCase(32, 256, 1), StatsCase(33, 257, 3), StatsCase(64, 513, 1), StatsCase(5, 513, 3),
               StatsCase(33, 7, 1), StatsCase(64, 1, 3), StatsCase(1, 257, 1), StatsCase(32, 513, 1), StatsCase(64, 256, 3)]


def stats_coverage(cases: List[StatsCase]) -> Dict[str, object]:
    return dict(second_pass=any(c.C8 > 32 for c in cases), exactly_32=any(c.C8 == 32 for c in cases),
                ragged_second_pass=any(32 < c.C8 < 64 for c in cases), chunks=sorted({-(-c.rps // ST_ROWS) for c in cases}),
                chunk_tail=any(c.rps % ST_ROWS not in (0,) and c.rps > ST_ROWS for c in cases), partial_rowgroup=any(c.rps % 8 for c in cases),
                samples=sorted({c.samples for c in cases}))


def stats_inputs(c: StatsCase, integers: bool = False):
    g = _gen(2, c.C8, c.rps, c.samples)
    T, C = c.samples * c.rps, 8 * c.C8
    if integers:
        return torch.randint(-8, 9, (T, C), generator=g).float().to(BF), torch.randint(-8, 9, (T, C), generator=g).float().to(BF)
    return (torch.randn(T, C, generator=g) + 0.5).to(BF), (torch.randn(T, C, generator=g) * 2).to(BF)


def chan_stats_ref(p, q, c: StatsCase, mut: Optional[str] = None) -> Dict[str, Out]:
    """partial fp32 [samples][chunks][2][C].  mut: 'q_is_p', 'swap_rows', 'tail_dropped' (rows after the last full group of 8 of a sample),
    'sample_off_by_one' (sample s starts one row late; the last row read twice)."""
    C = p.shape[1]
    nck = -(-c.rps // ST_ROWS)
    pd, qd = p.double().view(c.samples, c.rps, C), (p if mut == "q_is_p" else q).double().view(c.samples, c.rps, C)
    terms = torch.stack([pd, pd * qd], 2)                               # [s][r][2][C]
    src = terms
    if mut == "sample_off_by_one":
        flat = terms.reshape(-1, 2, C)
        idx = (torch.arange(c.samples * c.rps) + torch.arange(c.samples).repeat_interleave(c.rps).clamp_max(1)).clamp_max(len(flat) - 1)
        src = flat[idx].view_as(terms)
    if mut == "tail_dropped":
        src = terms * (torch.arange(c.rps) < c.rps // 8 * 8).double()[None, :, None, None]
    if mut == "swap_rows":
        src = terms.flip(2)
    pad = nck * ST_ROWS - c.rps
    chunked = lambda v: F.pad(v, (0, 0, 0, 0, 0, pad)).view(c.samples, nck, ST_ROWS, 2, C).sum(2)
    n_in = torch.tensor([min(ST_ROWS, c.rps - k * ST_ROWS) for k in range(nck)], dtype=torch.float64)[None, :, None, None]
    return dict(partial=Out(chunked(src), Tol.delta(n_in, chunked(terms.abs()))))


STATS_MUTANTS = ("q_is_p", "swap_rows", "tail_dropped", "sample_off_by_one")


def stats_identity(mut: str, c: StatsCase) -> bool:
    return (mut == "tail_dropped" and c.rps % 8 == 0) or (mut == "sample_off_by_one" and c.samples == 1)


# ---- srk_sum_rows_f32, srk_bn_train_coeffs, srk_bn_train_bwd_coeffs ------------------------------------------------------------------------
BN_R = (1, 3, 28, 29, 32, 33, 37, 64)
BN_N = (1, 63, 64, 65, 130)


@dataclass(frozen=True)
class BnCase:
    R: int
    C: int               # n of sum_rows
    outer: int = 1

    @property
    def id(self) -> str:
        return f"R{self.R}-C{self.C}-o{self.outer}"

    @property
    def ld(self) -> int:
        return (self.C + 7) // 8 * 8 + 8

    @property
    def row_stride(self) -> int:
        return 2 * self.ld + 24


BN_CASES = [BnCase(R, C, 1 + (i + j) % 2) for i, R in enumerate(BN_R) for j, C in enumerate(BN_N) if (i + 2 * j) % 3 != 2 or R in (29, 33) or C == 130]


def bn_coverage(cases: List[BnCase]) -> Dict[str, object]:
    """the eight-deep loop runs while r + 28 < R for the row group that starts at r in 0..3: never (R <= 28), for some row groups only
    (29 <= R <= 31), for all of them (R >= 32), with a tail behind it (R % 32 != 0), twice (R >= 64)"""
    return dict(never=any(c.R <= 28 for c in cases), some_groups=any(29 <= c.R <= 31 for c in cases), all_groups=any(c.R >= 32 for c in cases),
                tail_after=any(c.R > 32 and c.R % 32 for c in cases), twice=any(c.R >= 64 for c in cases),
                blocks=sorted({-(-c.C // 64) for c in cases}), ragged_block=any(c.C % 64 for c in cases), outer=sorted({c.outer for c in cases}))


def sum_rows_inputs(c: BnCase) -> torch.Tensor:
    g = _gen(3, c.R, c.C, c.outer)
    return torch.randn(c.outer, c.R, c.C, generator=g) * 10.0 ** torch.randint(-2, 3, (c.outer, c.R, c.C), generator=g).float()


def sum_rows_ref(inp, mut: Optional[str] = None) -> Dict[str, Out]:
    """[outer][R][n] -> [outer][n].  mut: 'drop_last_row', 'outer_stride' (sample o starts at row o (R - 1))."""
    outer, R, n = inp.shape
    d = inp.double()
    src = d
    if mut == "drop_last_row":
        src = d[:, :R - 1]
    if mut == "outer_stride":
        flat = d.reshape(-1, n)
        src = torch.stack([flat[o * (R - 1):o * (R - 1) + R] for o in range(outer)])
    return dict(sum=Out(src.sum(1), Tol.delta(R, d.abs().sum(1))))


SUM_ROWS_MUTANTS = ("drop_last_row", "outer_stride")


def sum_rows_identity(mut: str, c: BnCase) -> bool:
    return mut == "outer_stride" and c.outer == 1


BN_EPS, BN_MOMENTUM, BN_PER_ROW = 1e-5, 0.1, 64


def bn_inputs(c: BnCase) -> Dict[str, torch.Tensor]:
    """partial fp32 [R][row_stride]: sums of x at + 0, of x^2 (resp. dz x) at + ld over 64 values per row; everything else NaN.  Where C > 1, channel 0
    has |mean| >> std (mean 100, std 0.1) and channel 1 is constant (3.0: the clamp at 0 applies), the rest mixed.  real_of
    maps every third channel to -1 (padding) and the others to consecutive indices of the un-padded buffers."""
    g = _gen(4, c.R, c.C)
    C, R, k = c.C, c.R, BN_PER_ROW
    mean = torch.randn(C, generator=g) * 2
    std = torch.rand(C, generator=g) + 0.2
    if C > 1:
        mean[0], std[0] = 100.0, 0.1
        mean[1], std[1] = 3.0, 0.0
    x = (torch.randn(R, k, C, generator=g) * std + mean).to(BF).double()
    dz = torch.randn(R, k, C, generator=g).to(BF).double()
    nan = float("nan")
    part = torch.full((R, c.row_stride), nan)
    part[:, :C], part[:, c.ld:c.ld + C] = x.sum(1).float(), (x * x).sum(1).float()
    bpart = torch.full((R, c.row_stride), nan)
    bpart[:, :C], bpart[:, c.ld:c.ld + C] = dz.sum(1).float(), (dz * x).sum(1).float()
    real_of = torch.full((c.ld,), -1, dtype=torch.int32)
    real = [i for i in range(C) if i % 3 != 2]
    real_of[real] = torch.arange(len(real), dtype=torch.int32)
    return dict(partial=part, bwd_partial=bpart, n=float(R * k), gamma=torch.rand(C, generator=g) + 0.5, beta=torch.randn(C, generator=g) * 0.1,
                real_of=real_of, n_real=len(real), rm0=torch.randn(len(real), generator=g), rv0=torch.rand(len(real), generator=g) + 0.5)


def _bn_sums(part, c: BnCase, mut: Optional[str]):
    d = part.double()
    a, b = d[:, :c.C], d[:, c.ld:c.ld + c.C]
    t1, t2 = Tol.delta(c.R, a.abs().sum(0)), Tol.delta(c.R, b.abs().sum(0))
    if mut == "drop_last_row":
        a, b = a[:c.R - 1], b[:c.R - 1]
    return a.sum(0), b.sum(0), t1, t2


def bn_train_coeffs_ref(i: Dict[str, torch.Tensor], c: BnCase, use_real_of: bool = True, mut: Optional[str] = None) -> Dict[str, Out]:
    """coef [4][C] (scale, shift, mean, rstd), running_mean / running_var [n_real] (or [C] without real_of: rm0 / rv0 must then have C
    entries).  mut: 'drop_last_row', 'biased_running_var', 'momentum_swapped', 'real_of_ignored'."""
    n = i["n"]
    ga, be = i["gamma"].double(), i["beta"].double()
    s1e, s2e, t_s1, t_s2 = _bn_sums(i["partial"], c, None)
    s1, s2, _, _ = _bn_sums(i["partial"], c, mut)

    def stats(s1, s2):
        mean = s1 / n
        var = (s2 / n - mean * mean).clamp_min(0.0)
        rstd = (var + BN_EPS).rsqrt()
        sc = ga * rstd
        return mean, var, rstd, sc, be - mean * sc

    mean, var, rstd, sc, sh = stats(s1e, s2e)
    t_mean = t_s1 / n + U * mean.abs()
    t_var = t_s2 / n + 2 * mean.abs() * t_mean + U * (s2e / n + mean * mean) + U * var
    t_rstd = _image_of_rsqrt(var, t_var, BN_EPS)
    t_sc = ga.abs() * t_rstd + U * sc.abs()
    t_sh = sc.abs() * t_mean + mean.abs() * t_sc + U * ((mean * sc).abs() + sh.abs())
    m = BN_MOMENTUM
    unb = n / max(n - 1.0, 1.0)
    rm0, rv0 = i["rm0"].double(), i["rv0"].double()
    idx = i["real_of"][:c.C].long() if use_real_of else torch.arange(c.C)
    live = idx >= 0
    tgt = idx[live]
    mm, vv, r_, sc_, sh_ = stats(s1, s2)

    def running(mean_v, var_v, mut):
        w_old, w_new = (m, 1 - m) if mut == "momentum_swapped" else (1 - m, m)
        f = 1.0 if mut == "biased_running_var" else unb
        rm, rv = rm0.clone(), rv0.clone()
        if mut == "real_of_ignored":
            k = min(len(rm), c.C)
            rm[:k] = w_old * rm0[:k] + w_new * mean_v[:k]
            rv[:k] = w_old * rv0[:k] + w_new * var_v[:k] * f
        else:
            rm[tgt] = w_old * rm0[tgt] + w_new * mean_v[live]
            rv[tgt] = w_old * rv0[tgt] + w_new * var_v[live] * f
        return rm, rv

    rm, rv = running(mm, vv, mut)
    t_rm, t_rv = torch.zeros_like(rm0), torch.zeros_like(rv0)
    t_rm[tgt] = m * t_mean[live] + 4 * U * (rm0[tgt].abs() + m * mean[live].abs())
    t_rv[tgt] = m * unb * t_var[live] + 4 * U * (rv0[tgt].abs() + m * unb * var[live])
    return dict(coef=Out(torch.stack([sc_, sh_, mm, r_]), torch.stack([t_sc, t_sh, t_mean, t_rstd])), running_mean=Out(rm, t_rm),
                running_var=Out(rv, t_rv))


def bn_train_bwd_coeffs_ref(i: Dict[str, torch.Tensor], fwd_coef: torch.Tensor, c: BnCase, mut: Optional[str] = None) -> Dict[str, Out]:
    """fwd_coef fp32 [4][C]: the values the kernel is handed (read as exact).  coef [5][C] = A (= scale), B, C, dgamma, dbeta.
    mut: 'drop_last_row', 'dgamma_no_mean', 'B_sign'."""
    n = i["n"]
    sc, mean, rstd = fwd_coef[0].double(), fwd_coef[2].double(), fwd_coef[3].double()
    S1e, S2e, t_S1, t_S2 = _bn_sums(i["bwd_partial"], c, None)
    S1, S2, _, _ = _bn_sums(i["bwd_partial"], c, mut)

    def coefs(S1, S2, mut=None):
        dg = rstd * (S2 - (0.0 if mut == "dgamma_no_mean" else mean * S1))
        Bc = -sc * rstd * dg / n
        return dg, (-Bc if mut == "B_sign" else Bc), (sc / n) * (mean * rstd * dg - S1)

    dg, Bc, Cc = coefs(S1e, S2e)
    t_dg = rstd * (t_S2 + mean.abs() * t_S1 + U * (S2e.abs() + 2 * (mean * S1e).abs())) + U * dg.abs()
    t_B = (sc * rstd / n).abs() * t_dg + 4 * U * Bc.abs()
    mrd = (mean * rstd * dg).abs()
    t_C = (sc / n).abs() * ((mean * rstd).abs() * t_dg + t_S1 + 4 * U * mrd + U * (mrd + S1e.abs())) + 2 * U * Cc.abs()
    dgm, Bm, Cm = coefs(S1, S2, mut)
    return dict(coef=Out(torch.stack([sc, Bm, Cm, dgm, S1]), torch.stack([torch.zeros_like(sc), t_B, t_C, t_dg, t_S1])))


BN_FWD_MUTANTS = ("drop_last_row", "biased_running_var", "momentum_swapped", "real_of_ignored")
BN_BWD_MUTANTS = ("drop_last_row", "dgamma_no_mean", "B_sign")


# ---- the element-wise token passes: srk_affine_act_bf16, srk_lincomb2_bf16, srk_dgelu_affine_bf16, srk_mul_bwd_bf16 -------------------------
EW_C8 = (1, 5, 24, 48, 64)


def ew_lanes(C8: int) -> int:
    return 256 // min(C8, 256)


@dataclass(frozen=True)
class EwCase:
    C8: int
    rows: int
    rps: int             # 0: one coefficient vector for all rows

    @property
    def id(self) -> str:
        return f"C8_{self.C8}-rows{self.rows}-rps{self.rps}"


def _ew_cases() -> List[EwCase]:
    out = []
    for i, C8 in enumerate(EW_C8):
        L4 = 4 * ew_lanes(C8)
        rows = (1, 3, L4 - 1, L4 + 1, 1000)
        for j, r in enumerate(rows):
            for rps in {0: (0, r), 1: (1, 7), 2: (0, 7), 3: (1, r), 4: (7, 0)}[(i + j) % 5]:
                if rps <= r:
                    out.append(EwCase(C8, r, rps))
    return out


EW_CASES = _ew_cases()
EW_PATTERNS = ("copy", "c_acc", "ap", "ap_bq_c", "p_acc")      # what tpu_superresolution_amd/dat_train.py asks of lincomb2


def ew_coverage(cases: List[EwCase]) -> Dict[str, object]:
    return dict(C8=sorted({c.C8 for c in cases}), rps_kinds=sorted({"none" if c.rps == 0 else "row" if c.rps == 1 else "whole" if c.rps == c.rows else
                                                                    "ragged" if c.rows % c.rps else "even" for c in cases}),
                second_step=any(c.rows > 4 * ew_lanes(c.C8) for c in cases), short_step=any(c.rows < 4 * ew_lanes(c.C8) for c in cases),
                idle_lanes=any(256 % c.C8 for c in cases), single_row=any(c.rows == 1 for c in cases))


def ew_inputs(c: EwCase) -> Dict[str, torch.Tensor]:
    g = _gen(5, c.C8, c.rows, c.rps)
    C = 8 * c.C8
    ns = 1 if c.rps == 0 else -(-c.rows // c.rps)
    mk = lambda s=1.0: (torch.randn(c.rows, C, generator=g) * s).to(BF)
    p, q, old = mk(), mk(2.0), mk()
    p[0, 0], p[0, 1 % C] = 0.0, -0.0
    return dict(p=p, q=q, old=old, A=torch.randn(ns, C, generator=g), B=torch.randn(ns, C, generator=g), C=torch.randn(ns, C, generator=g) * 0.5)


def _coef_rows(c: EwCase, mut: Optional[str]) -> torch.Tensor:
    t = torch.arange(c.rows)
    if c.rps == 0:
        return torch.zeros(c.rows, dtype=torch.long)
    ns = -(-c.rows // c.rps)
    if mut == "rps_off_by_one":
        return ((t + 1) // c.rps).clamp_max(ns - 1)
    if mut == "mod_index":
        return (t % c.rps).clamp_max(ns - 1)
    return t // c.rps


def ew_index_identity(mut: str, c: EwCase) -> bool:
    """the two index mutants read the same coefficient rows as the reference"""
    return mut in ("rps_off_by_one", "mod_index") and bool((_coef_rows(c, mut) == _coef_rows(c, None)).all())


def affine_act_ref(i, c: EwCase, act: int, mut: Optional[str] = None) -> Dict[str, Out]:
    """out = act(x * s + t), x = p, s = A, t = B of ew_inputs.  mut: 'rps_off_by_one', 'mod_index', 'no_shift'."""
    x = i["p"].double()
    idx0 = _coef_rows(c, None)
    s, t = i["A"].double()[idx0], i["B"].double()[idx0]
    v = x * s + t
    t_v = 2 * U * ((x * s).abs() + t.abs())
    exact, tol = (G.gelu(v), t_bf16(G.gelu(v), GELU_LIP * t_v + 8 * U * v.abs())) if act else (v, t_bf16(v, t_v))
    if mut is not None:
        idx = _coef_rows(c, mut)
        vm = x * i["A"].double()[idx] + (0.0 if mut == "no_shift" else i["B"].double()[idx])
        exact = G.gelu(vm) if act else vm
    return dict(out=Out(exact, tol))


def affine_act_bits(i, c: EwCase) -> Tuple[torch.Tensor, torch.Tensor]:
    """act 0: (the contracted form bf16(fma(x, s, t)), the two-rounding form bf16(fp32(x s) + t))"""
    idx = _coef_rows(c, None)
    x, s, t = i["p"].float(), i["A"][idx], i["B"][idx]
    return fma32(x, s, t).to(BF), (x * s + t).to(BF)


def lincomb2_ref(i, c: EwCase, pattern: str, mut: Optional[str] = None) -> Dict[str, Out]:
    """out (+)= A p + B q + C by operand pattern.  mut: 'rps_off_by_one', 'mod_index', 'acc_ignores_old', 'b_on_p' (B multiplies p)."""
    idx0, idx = _coef_rows(c, None), _coef_rows(c, mut)
    z = torch.zeros(c.rows, 8 * c.C8, dtype=torch.float64)
    p, q, old = i["p"].double(), i["q"].double(), i["old"].double()

    def terms(ix, m=None):
        A, Bc, Cc = i["A"].double()[ix], i["B"].double()[ix], i["C"].double()[ix]
        o = z if m == "acc_ignores_old" else old
        return {"copy": (z, p, z, z), "c_acc": (o, z, z, Cc), "ap": (z, A * p, z, z), "ap_bq_c": (z, A * p, Bc * (p if m == "b_on_p" else q), Cc),
                "p_acc": (o, p, z, z)}[pattern]

    e = terms(idx0)
    exact = sum(e)
    tol = t_bf16(exact, Tol.delta(4, sum(t.abs() for t in e)))
    return dict(out=Out(sum(terms(idx, mut)), tol))


def lincomb2_bits(i, c: EwCase, pattern: str) -> Optional[torch.Tensor]:
    """the single-operation patterns as one fp32 operation and one RNE store (None for ap_bq_c)"""
    idx = _coef_rows(c, None)
    p, old = i["p"].float(), i["old"].float()
    zero = torch.zeros_like(p)
    if pattern == "copy":
        return (zero + p).to(BF)
    if pattern == "c_acc":
        return (old + i["C"][idx]).to(BF)
    if pattern == "ap":
        return (zero + i["A"][idx] * p).to(BF)
    if pattern == "p_acc":
        return (old + p).to(BF)
    return None


LINCOMB_MUTANTS = ("rps_off_by_one", "mod_index", "acc_ignores_old", "b_on_p")
AFFINE_MUTANTS = ("rps_off_by_one", "mod_index", "no_shift")


def lincomb2_identity(mut: str, c: EwCase, pattern: str) -> bool:
    if mut in ("rps_off_by_one", "mod_index"):
        return pattern in ("copy", "p_acc") or ew_index_identity(mut, c)
    if mut == "acc_ignores_old":
        return pattern in ("copy", "ap", "ap_bq_c")
    return pattern != "ap_bq_c"                   # b_on_p


FLAT_GRID_CAP = 16384
FLAT_PASS = FLAT_GRID_CAP * 256                   # pieces per pass of the flat kernels' capped grid


@dataclass(frozen=True)
class FlatCase:
    rows: int
    C8: int

    @property
    def id(self) -> str:
        return f"rows{self.rows}-C8_{self.C8}"


FLAT_CASES = [FlatCase(1, 1), FlatCase(51, 5), FlatCase(255, 1), FlatCase(257, 1), FlatCase(77, 5), FlatCase(3, 64)]
FLAT_WRAP = FlatCase(65537, 64)


def flat_coverage(cases: List[FlatCase]) -> Dict[str, object]:
    n = [c.rows * c.C8 for c in cases]
    return dict(pieces=sorted(n), one_thread=1 in n, partial_group=any(k % 256 for k in n), two_groups=any(256 < k for k in n),
                wrap=any(k > FLAT_PASS for k in n), division=any(c.C8 not in (1, 64) for c in cases))


def flat_inputs(c: FlatCase) -> Dict[str, torch.Tensor]:
    """dy, x, a, b bf16 [rows][C]; scale / shift [C] such that the GELU' arguments x s + t spread over [-8, 8]; x holds +0 and -0 (and s +-1, t 0
    in column 0, so that the argument itself is +-0 there)."""
    g = _gen(6, c.rows, c.C8)
    C = 8 * c.C8
    mk = lambda: torch.randn(c.rows, C, generator=g).to(BF)
    x = (torch.rand(c.rows, C, generator=g) * 16 - 8).to(BF)
    x[0, 0] = 0.0
    if c.rows > 1:
        x[1, 0] = -0.0
    s, t = torch.rand(C, generator=g) * 0.5 + 0.5, torch.randn(C, generator=g) * 0.2
    s[0], t[0] = 1.0, 0.0
    return dict(dy=mk(), x=x, a=mk(), b=mk(), scale=s, shift=t)


def dgelu_affine_ref(i, mut: Optional[str] = None) -> Dict[str, Out]:
    """out = dy * gelu'(x s + t).  mut: 'gelu_not_dgelu', 'no_shift', 'tanh_form' (the derivative of the tanh approximation)."""
    dy, x, s, t = i["dy"].double(), i["x"].double(), i["scale"].double(), i["shift"].double()
    v = x * s + t
    exact = dy * G.dgelu(v)
    tol = t_bf16(exact, dy.abs() * (GELU_LIP * 2 * U * ((x * s).abs() + t.abs()) + 8 * U))
    if mut == "gelu_not_dgelu":
        exact = dy * G.gelu(v)
    elif mut == "no_shift":
        exact = dy * G.dgelu(x * s)
    elif mut == "tanh_form":
        vv = v.clone().requires_grad_(True)
        F.gelu(vv, approximate="tanh").sum().backward()
        exact = dy * vv.grad
    return dict(out=Out(exact, tol))


def mul_bwd_bits(i) -> Tuple[torch.Tensor, torch.Tensor]:
    """(da, db) = (bf16(dy b), bf16(dy a)): the fp32 product of two bf16 values is exact"""
    return (i["dy"].float() * i["b"].float()).to(BF), (i["dy"].float() * i["a"].float()).to(BF)


def mul_bwd_ref(i, mut: Optional[str] = None) -> Dict[str, Out]:
    """mut: 'swapped' (da = dy a)"""
    dy, a, b = i["dy"].double(), i["a"].double(), i["b"].double()
    da, db = dy * b, dy * a
    if mut == "swapped":
        return dict(da=Out(db, t_bf16(da, 0.0)), db=Out(da, t_bf16(db, 0.0)))
    return dict(da=Out(da, t_bf16(da, 0.0)), db=Out(db, t_bf16(db, 0.0)))


DGELU_MUTANTS = ("gelu_not_dgelu", "no_shift", "tanh_form")


# ---- srk_dual_gate_combine, srk_dual_gate_bwd ---------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class GateCase:
    CA: int
    HW: int
    B: int

    @property
    def id(self) -> str:
        return f"CA{self.CA}-HW{self.HW}-B{self.B}"


GATE_CASES = [GateCase(8, 1, 1), GateCase(8, 65, 3), GateCase(64, 63, 3), GateCase(64, 130, 1), GateCase(192, 64, 1), GateCase(192, 65, 3),
              GateCase(192, 1, 3), GateCase(256, 130, 3), GateCase(256, 63, 1), GateCase(64, 64, 3), GateCase(256, 1, 1), GateCase(8, 130, 1)]


def gate_coverage(cases: List[GateCase]) -> Dict[str, object]:
    return dict(CA=sorted({c.CA for c in cases}), idle_pieces=any(c.CA < 256 for c in cases), all_pieces=any(c.CA == 256 for c in cases),
                chunks=sorted({-(-c.HW // 64) for c in cases}), chunk_tail=any(c.HW % 64 and c.HW > 64 for c in cases),
                partial_token_lanes=any(c.HW % 8 for c in cases), B=sorted({c.B for c in cases}))


def gate_inputs(c: GateCase) -> Dict[str, torch.Tensor]:
    """a, b, dcomb bf16 [B HW][CA]; cgate fp32 [B][CA] and tgate fp32 [B HW] post-sigmoid, tgate with an exact 0 (token 0) and an exact 1
    (the last token)."""
    g = _gen(7, c.CA, c.HW, c.B)
    T = c.B * c.HW
    mk = lambda: torch.randn(T, c.CA, generator=g).to(BF)
    tg = torch.sigmoid(torch.randn(T, generator=g) * 2)
    tg[0] = 0.0
    tg[T - 1] = 1.0
    return dict(a=mk(), b=mk(), d=mk(), cgate=torch.sigmoid(torch.randn(c.B, c.CA, generator=g)), tgate=tg)


def dual_gate_combine_ref(i, c: GateCase, tok_gate_on_a: int, mut: Optional[str] = None) -> Dict[str, Out]:
    """mut: 'gate_wrong_operand', 'sample_off' (the channel gate of the next sample)"""
    a, b = i["a"].double(), i["b"].double()
    smp = torch.arange(c.B).repeat_interleave(c.HW)
    cg, tg = i["cgate"].double()[smp], i["tgate"].double()[:, None]
    ta, tb = (a * tg, b * cg) if tok_gate_on_a else (a * cg, b * tg)
    tol = t_bf16(ta + tb, Tol.delta(2, ta.abs() + tb.abs()))
    if mut == "gate_wrong_operand":
        ta, tb = (a * cg, b * tg) if tok_gate_on_a else (a * tg, b * cg)
    if mut == "sample_off":
        cg = i["cgate"].double()[(smp + 1) % c.B]
        ta, tb = (a * tg, b * cg) if tok_gate_on_a else (a * cg, b * tg)
    return dict(out=Out(ta + tb, tol))


def dual_gate_combine_bits(i, c: GateCase, tok_gate_on_a: int) -> List[torch.Tensor]:
    """the three evaluations of a g1 + b g2: two products and a sum; fma(a, g1, fl(b g2)); fma(b, g2, fl(a g1))"""
    a, b = i["a"].float(), i["b"].float()
    smp = torch.arange(c.B).repeat_interleave(c.HW)
    cg, tg = i["cgate"][smp], i["tgate"][:, None].expand(-1, c.CA)
    g1, g2 = (tg, cg) if tok_gate_on_a else (cg, tg)
    return [(a * g1 + b * g2).to(BF), fma32(a, g1, b * g2).to(BF), fma32(b, g2, a * g1).to(BF)]


def dual_gate_bwd_bits(i, c: GateCase) -> Tuple[torch.Tensor, torch.Tensor]:
    smp = torch.arange(c.B).repeat_interleave(c.HW)
    d = i["d"].float()
    return (d * i["cgate"][smp]).to(BF), (d * i["tgate"][:, None]).to(BF)


def dual_gate_bwd_ref(i, c: GateCase, mut: Optional[str] = None) -> Dict[str, Out]:
    """a_chan = a, a_tok = b.  d_chan, d_tok bf16; dcg_partial fp32 [B][chunks][CA]; dsmap fp32 [B HW].
    mut: 'no_sigmoid_grad', 'chunk_tail_dropped', 'sample_off', 'dsmap_uses_a_chan'."""
    d, ac, at = i["d"].double(), i["a"].double(), i["b"].double()
    smp = torch.arange(c.B).repeat_interleave(c.HW)
    cgi = (smp + 1) % c.B if mut == "sample_off" else smp
    cg, tg = i["cgate"].double(), i["tgate"].double()
    d_chan, d_tok = d * cg[cgi], d * tg[:, None]
    dot = (d * (ac if mut == "dsmap_uses_a_chan" else at)).sum(1)
    sg = tg * (1 - tg)
    dsmap = dot if mut == "no_sigmoid_grad" else dot * sg
    t_ds = Tol.delta(c.CA, (d * at).abs().sum(1)) * sg + 4 * U * ((d * at).sum(1) * sg).abs()
    nck = -(-c.HW // 64)
    pad = nck * 64 - c.HW
    keep = (torch.arange(c.HW) < c.HW // 64 * 64).double()[None, :, None] if mut == "chunk_tail_dropped" else 1.0
    chunked = lambda v: F.pad(v, (0, 0, 0, pad)).view(c.B, nck, 64, c.CA).sum(2)
    terms = (d * ac).view(c.B, c.HW, c.CA)
    n_in = torch.tensor([min(64, c.HW - k * 64) for k in range(nck)], dtype=torch.float64)[None, :, None]
    return dict(d_chan=Out(d_chan, t_bf16(d * cg[smp], U * (d * cg[smp]).abs())), d_tok=Out(d_tok, t_bf16(d_tok, U * d_tok.abs())),
                dcg_partial=Out(chunked(terms * keep), Tol.delta(n_in, chunked(terms.abs()))), dsmap=Out(dsmap, t_ds))


GATE_COMBINE_MUTANTS = ("gate_wrong_operand", "sample_off")
GATE_BWD_MUTANTS = ("no_sigmoid_grad", "chunk_tail_dropped", "sample_off", "dsmap_uses_a_chan")


def gate_identity(mut: str, c: GateCase) -> bool:
    """with a single token its gate is exactly 1 (gate_inputs), so dsmap is 0 whatever the dot product was"""
    return (mut == "sample_off" and c.B == 1) or (mut == "chunk_tail_dropped" and c.HW % 64 == 0) or \
        (mut == "dsmap_uses_a_chan" and c.B * c.HW == 1)


# ---- srk_dwconv3x3, srk_dwconv3x3_wgrad -------------------------------------------------------------------------------------------------
DW_TH, DW_TW, DW_CB = 8, 16, 64


@dataclass(frozen=True)
class DwCase:
    B: int
    H: int
    W: int
    C8: int

    @property
    def id(self) -> str:
        return f"{self.B}x{self.H}x{self.W}-C8_{self.C8}"


DW_CASES = [DwCase(1, 1, 1, 1), DwCase(2, 1, 17, 8), DwCase(2, 8, 16, 9), DwCase(1, 9, 33, 17), DwCase(2, 9, 17, 1), DwCase(2, 8, 1, 17),
            DwCase(1, 1, 33, 9), DwCase(2, 9, 16, 8), DwCase(1, 8, 17, 1), DwCase(2, 9, 33, 9), DwCase(2, 1, 1, 8), DwCase(1, 9, 1, 9),
            DwCase(2, 8, 33, 17), DwCase(1, 1, 16, 17)]
DW_VARIANTS = ((0, False), (1, False), (0, True), (1, True))           # (act, with mul)


def dw_coverage(cases: List[DwCase]) -> Dict[str, object]:
    return dict(H=sorted({c.H for c in cases}), W=sorted({c.W for c in cases}), C8=sorted({c.C8 for c in cases}), B=sorted({c.B for c in cases}),
                channel_blocks=sorted({-(-8 * c.C8 // DW_CB) for c in cases}), ragged_block=any(8 * c.C8 % DW_CB for c in cases),
                tiles_y=sorted({-(-c.H // DW_TH) for c in cases}), tiles_x=sorted({-(-c.W // DW_TW) for c in cases}),
                neighbour_image=any(c.B > 1 for c in cases))


def dw_inputs(c: DwCase) -> Dict[str, torch.Tensor]:
    g = _gen(8, c.B, c.H, c.W, c.C8)
    C = 8 * c.C8
    mk = lambda: torch.randn(c.B * c.H * c.W, C, generator=g).to(BF)
    return dict(x=mk(), dy=mk(), mul=mk(), w=torch.randn(C, 9, generator=g) * 0.3, scale=torch.rand(C, generator=g) + 0.5,
                shift=torch.randn(C, generator=g) * 0.1)


def _dw_windows(x: torch.Tensor, c: DwCase, mut: Optional[str]) -> List[torch.Tensor]:
    """the nine shifted copies x[pix + (r - 1, dx - 1)] (zero outside the image) as [B H W][C], tap index r * 3 + dx.
    mut 'halo_from_neighbour': the B images are treated as one image of B H rows; 'transpose_taps': r <-> dx."""
    C = x.shape[1]
    xd = x.double()
    img = xd.view(1, c.B * c.H, c.W, C) if mut == "halo_from_neighbour" else xd.view(c.B, c.H, c.W, C)
    Hh = img.shape[1]
    p = F.pad(img, (0, 0, 1, 1, 1, 1))
    wins = []
    for t in range(9):
        r, dx = (t % 3, t // 3) if mut == "transpose_taps" else (t // 3, t % 3)
        wins.append(p[:, r:r + Hh, dx:dx + c.W].reshape(-1, C))
    return wins


def dwconv_ref(i, c: DwCase, act: int, with_mul: bool, mut: Optional[str] = None) -> Dict[str, Out]:
    """out = act(conv(x) * scale + shift) * mul.  mut: 'halo_from_neighbour', 'transpose_taps', 'mul_ignored', 'no_shift'."""
    w, sc, sh = i["w"].double(), i["scale"].double(), i["shift"].double()

    def run(m):
        wins = _dw_windows(i["x"], c, m)
        conv = sum(wins[t] * w[:, t] for t in range(9))
        S = sum(wins[t].abs() * w[:, t].abs() for t in range(9))
        return conv, S

    conv, S = run(None)
    v = conv * sc + sh
    t_v = sc.abs() * Tol.delta(9, S) + 2 * U * ((conv * sc).abs() + sh.abs())
    m = i["mul"].double() if with_mul else 1.0

    def finish(v, m):
        return (G.gelu(v) if act else v) * m

    t_a = GELU_LIP * t_v + 8 * U * v.abs() if act else t_v
    exact = finish(v, m)
    tol = t_bf16(exact, t_a * (m.abs() if with_mul else 1.0) + U * exact.abs())
    if mut is None:
        return dict(out=Out(exact, tol))
    cm, _ = run(mut)
    vm = cm * sc + (0.0 if mut == "no_shift" else sh)
    return dict(out=Out(finish(vm, 1.0 if mut == "mul_ignored" else m), tol))


def dwconv_wgrad_ref(i, c: DwCase, mut: Optional[str] = None) -> Dict[str, Out]:
    """partial fp32 [B][bands of 8 rows][10][C]: rows 0..8 sum over the band of dy[pix] x[pix + off(tap)], row 9 sum dy.
    mut: 'halo_from_neighbour', 'transpose_taps', 'band_tail_dropped' (the image rows after the last full band of 8)."""
    C = 8 * c.C8
    dy = i["dy"].double()
    nb = -(-c.H // DW_TH)

    def run(m, absolute=False):
        wins = _dw_windows(i["x"], c, m)
        terms = torch.stack([(dy * wv).abs() if absolute else dy * wv for wv in wins] + [dy.abs() if absolute else dy], 1)   # [T][10][C]
        terms = terms.view(c.B, c.H, c.W, 10, C)
        if m == "band_tail_dropped":
            terms = terms * (torch.arange(c.H) < c.H // DW_TH * DW_TH).double()[None, :, None, None, None]
        return F.pad(terms, (0, 0, 0, 0, 0, 0, 0, nb * DW_TH - c.H)).view(c.B, nb, DW_TH, c.W, 10, C).sum((2, 3))

    n_in = torch.tensor([min(DW_TH, c.H - k * DW_TH) * c.W for k in range(nb)], dtype=torch.float64)[None, :, None, None]
    return dict(partial=Out(run(mut), Tol.delta(n_in, run(None, absolute=True))))


DW_MUTANTS = ("halo_from_neighbour", "transpose_taps", "mul_ignored", "no_shift")
DW_WGRAD_MUTANTS = ("halo_from_neighbour", "transpose_taps", "band_tail_dropped")


def dw_identity(mut: str, c: DwCase, with_mul: bool = True) -> bool:
    if mut == "halo_from_neighbour":
        return c.B == 1
    if mut == "transpose_taps":
        return c.H == 1 and c.W == 1
    if mut == "band_tail_dropped":
        return c.H % DW_TH == 0
    if mut == "mul_ignored":
        return not with_mul
    return False


# ---- channel attention: srk_chan_gram, srk_chan_apply_mat, srk_channel_attention_fwd ----------------------------------------------------------
GRAM_CH, GRAM_SZ = 256, 32 * 32 + 64


@dataclass(frozen=True)
class ChanCase:
    N: int
    nH: int
    d: int
    B: int

    @property
    def id(self) -> str:
        return f"N{self.N}-h{self.nH}-d{self.d}-B{self.B}"

    @property
    def CA(self) -> int:
        return 32 * self.nH


CHAN_CASES = [ChanCase(1, 1, 1, 1), ChanCase(255, 6, 30, 2), ChanCase(256, 1, 32, 1), ChanCase(257, 6, 12, 2), ChanCase(600, 6, 30, 1),
              ChanCase(600, 1, 12, 2), ChanCase(1, 6, 32, 2), ChanCase(255, 1, 1, 1), ChanCase(257, 1, 30, 1), ChanCase(256, 6, 12, 1)]


def chan_coverage(cases: List[ChanCase]) -> Dict[str, object]:
    return dict(N=sorted({c.N for c in cases}), nH=sorted({c.nH for c in cases}), d=sorted({c.d for c in cases}), B=sorted({c.B for c in cases}),
                chunks=sorted({-(-c.N // GRAM_CH) for c in cases}), chunk_tail=any(c.N > GRAM_CH and c.N % GRAM_CH for c in cases),
                partial_wave=any(c.N % 16 for c in cases), full_heads=any(c.d == 32 for c in cases))


def chan_inputs(c: ChanCase) -> Dict[str, torch.Tensor]:
    """qkv bf16 [B N][3 CA] (q | k | v, head h at + 32 h, channels d .. 31 of every head zero: the layout's padding); channel 0 of head 0 of
    q is all zero in sample 0 (the 1e-12 clamp of F.normalize applies).  M fp32 [B][nH][32][32], diag fp32 [B][nH][32], src2 / old bf16
    [B N][CA], temperature [nH] (none of them 1)."""
    g = _gen(9, c.N, c.nH, c.d, c.B)
    T = c.B * c.N
    qkv = torch.zeros(T, 3, c.nH, 32)
    qkv[..., :c.d] = torch.randn(T, 3, c.nH, c.d, generator=g)
    qkv[:c.N, 0, 0, 0] = 0.0
    mk = lambda: torch.randn(T, c.CA, generator=g).to(BF)
    return dict(qkv=qkv.reshape(T, 3 * c.CA).to(BF), temperature=torch.rand(c.nH, generator=g) * 2 + 1.5,
                M=torch.randn(c.B, c.nH, 32, 32, generator=g) * 0.3, diag=torch.randn(c.B, c.nH, 32, generator=g), src2=mk(), old=mk())


def _heads(t: torch.Tensor, c: ChanCase) -> torch.Tensor:
    """[B N][CA] -> fp64 [B][nH][N][32]"""
    return t.double().view(c.B, c.N, c.nH, 32).permute(0, 2, 1, 3)


def chan_gram_ref(x, y, c: ChanCase, mut: Optional[str] = None) -> Dict[str, Out]:
    """partial fp32 [B][nH][chunks][1088]: G[i][j] = sum_n x[n][i] y[n][j] (1024), sum_n x[n][i]^2 (32), sum_n y[n][j]^2 (32) per 256-token
    chunk.  mut: 'G_transposed', 'chunk_tail_dropped', 'next_sample' (y of the next sample), 'norms_swapped'."""
    nck = -(-c.N // GRAM_CH)
    xh, yh = _heads(x, c), _heads(y, c)
    if mut == "next_sample":
        yh = yh.roll(-1, 0)
    pad = nck * GRAM_CH - c.N
    keep = (torch.arange(c.N) < c.N // GRAM_CH * GRAM_CH).double()[:, None] if mut == "chunk_tail_dropped" else 1.0

    def run(xv, yv, kp):
        xc = F.pad(xv * kp, (0, 0, 0, pad)).view(c.B, c.nH, nck, GRAM_CH, 32)
        yc = F.pad(yv, (0, 0, 0, pad)).view(c.B, c.nH, nck, GRAM_CH, 32)
        G_ = xc.transpose(-1, -2) @ yc
        yk = F.pad(yv * kp, (0, 0, 0, pad)).view(c.B, c.nH, nck, GRAM_CH, 32)
        return G_, (xc * xc).sum(3), (yk * yk).sum(3)

    G_, sx, sy = run(xh, yh, keep)
    Ga, sxa, sya = run(_heads(x, c).abs(), _heads(y, c).abs(), 1.0)
    if mut == "G_transposed":
        G_ = G_.transpose(-1, -2)
    if mut == "norms_swapped":
        sx, sy = sy, sx
    n_in = torch.tensor([min(GRAM_CH, c.N - k * GRAM_CH) for k in range(nck)], dtype=torch.float64)[None, None, :, None]
    ref = torch.cat([G_.reshape(c.B, c.nH, nck, 1024), sx, sy], -1)
    tol = Tol.delta(n_in, torch.cat([Ga.reshape(c.B, c.nH, nck, 1024), sxa, sya], -1))
    return dict(partial=Out(ref, tol))


def chan_apply_mat_ref(i, c: ChanCase, with_diag: bool, accumulate: int, mut: Optional[str] = None) -> Dict[str, Out]:
    """out[n][32 h + i] (+)= sum_j M[b][h][i][j] src[n][32 h + j] + diag[b][h][i] src2[n][32 h + i]; src = the v slice of qkv.
    mut: 'M_transposed', 'diag_on_src', 'acc_ignores_old', 'next_sample' (the matrices of the next sample)."""
    src = i["qkv"][:, 2 * c.CA:]
    s, s2, old = _heads(src, c), _heads(i["src2"], c), _heads(i["old"], c)
    M, dg = i["M"].double(), i["diag"].double()
    Mm = M.roll(-1, 0) if mut == "next_sample" else M.transpose(-1, -2) if mut == "M_transposed" else M
    val = s @ Mm.transpose(-1, -2)
    S = s.abs() @ M.abs().transpose(-1, -2)
    if with_diag:
        val = val + dg[:, :, None, :] * (s if mut == "diag_on_src" else s2)
        S = S + (dg[:, :, None, :] * s2).abs()
    if accumulate:
        S = S + old.abs()
        if mut != "acc_ignores_old":
            val = val + old
    exact = s @ M.transpose(-1, -2) + (dg[:, :, None, :] * s2 if with_diag else 0.0) + (old if accumulate else 0.0)
    back = lambda t: t.permute(0, 2, 1, 3).reshape(c.B * c.N, c.CA)
    return dict(out=Out(back(val), t_bf16(back(exact), Tol.delta(34, back(S)))))


def channel_attention_ref(i, c: ChanCase, mut: Optional[str] = None) -> Dict[str, Out]:
    """out bf16 [B N][CA]: q, k L2-normalised over the tokens (norm clamped at 1e-12), A = softmax_j(temperature q^T k) over the d real
    channels, out[n][i] = sum_j A[i][j] v[n][j]; channels d .. 31 of every head 0.
    Bound: dG = Tol.delta(N + chunks, sum |q k|); a norm is off by (N + chunks + 2) u relative; logit t_l = |t| dG / (|q| |k|) + (2 (N + chunks)
    + 8) u |l|; the softmax's relative error rho = 2 max_j t_l + (d + 8) u; A is handed to the matrix cores as bf16 (2^-8); the product
    sum_j (2^-8 + rho) A |v| + Tol.delta(32, sum A |v|); then the output's own rounding.
    mut: 'no_clamp', 'no_temperature', 'softmax_over_32', 'transposed'."""
    d, nck = c.d, -(-c.N // GRAM_CH)
    q, k, v = (_heads(i["qkv"][:, j * c.CA:(j + 1) * c.CA], c) for j in range(3))
    t = i["temperature"].double()[None, :, None, None]
    qn = q.pow(2).sum(2).sqrt()
    kn = k.pow(2).sum(2).sqrt()
    if mut != "no_clamp":
        qn, kn = qn.clamp_min(1e-12), kn.clamp_min(1e-12)
    den = qn[..., :, None] * kn[..., None, :]
    G_ = q.transpose(-1, -2) @ k
    l = G_ / den * (1.0 if mut == "no_temperature" else t)
    lex = G_ / (qn.clamp_min(1e-12)[..., :, None] * kn.clamp_min(1e-12)[..., None, :]) * t
    dm = d if mut != "softmax_over_32" else 32
    A = torch.zeros_like(l)
    A[..., :d, :dm] = l[..., :d, :dm].softmax(-1)
    A[..., :d, d:] = 0.0
    if mut == "transposed":
        A = A.transpose(-1, -2)
    Aex = torch.zeros_like(l)
    Aex[..., :d, :d] = lex[..., :d, :d].softmax(-1)
    L = c.N + nck
    dG = Tol.delta(L, q.abs().transpose(-1, -2) @ k.abs())
    t_l = t.abs() * dG / (qn.clamp_min(1e-12)[..., :, None] * kn.clamp_min(1e-12)[..., None, :]) + (2 * L + 8) * U * lex.abs()
    rho = 2 * t_l[..., :d, :d].amax(-1, keepdim=True) + (d + 8) * U if d else 0.0
    rho_full = torch.zeros_like(l[..., :1])
    rho_full[..., :d, :] = rho
    av = v.abs() @ ((BF16_REL + rho_full) * Aex).transpose(-1, -2) + Tol.delta(32, v.abs() @ Aex.transpose(-1, -2))
    back = lambda x_: x_.permute(0, 2, 1, 3).reshape(c.B * c.N, c.CA)
    exact = v @ Aex.transpose(-1, -2)
    tol = t_bf16(back(exact), back(av))
    tol[back(torch.zeros_like(exact) + (torch.arange(32) >= d).double()) > 0] = 0.0          # pad channels: exactly 0
    return dict(out=Out(back(v @ A.transpose(-1, -2)), tol))


CHAN_GRAM_MUTANTS = ("G_transposed", "chunk_tail_dropped", "next_sample", "norms_swapped")
CHAN_APPLY_MUTANTS = ("M_transposed", "diag_on_src", "acc_ignores_old", "next_sample")
CHAN_ATTN_MUTANTS = ("no_clamp", "no_temperature", "softmax_over_32", "transposed")


def chan_identity(mut: str, c: ChanCase, with_diag: bool = True, accumulate: int = 1) -> bool:
    if mut == "chunk_tail_dropped":
        return c.N % GRAM_CH == 0
    if mut == "next_sample":
        return c.B == 1
    if mut == "diag_on_src":
        return not with_diag
    if mut == "acc_ignores_old":
        return not accumulate
    if mut == "softmax_over_32":
        return c.d == 32
    if mut in ("no_temperature", "transposed", "G_transposed"):      # a 1 x 1 softmax is 1 whatever its logit; a 1 x 1 Gram block is symmetric
        return c.d == 1
    return False


# ---- srk_spatial_gate_train ---------------------------------------------------------------------------------------------------------------
SGT_BLOCK = 256


@dataclass(frozen=True)
class SgtCase:
    C: int
    S: int
    rows: int

    @property
    def id(self) -> str:
        return f"C{self.C}-S{self.S}-rows{self.rows}"


SGT_CASES = [SgtCase(64, 1, 1), SgtCase(64, 16, 257), SgtCase(128, 7, 255), SgtCase(128, 16, 700), SgtCase(192, 7, 256), SgtCase(192, 1, 700),
             SgtCase(192, 16, 1), SgtCase(256, 16, 257), SgtCase(256, 7, 700), SgtCase(256, 1, 255), SgtCase(64, 7, 700), SgtCase(128, 1, 256)]


def sgt_coverage(cases: List[SgtCase]) -> Dict[str, object]:
    return dict(NV=sorted({c.C // 64 for c in cases}), S=sorted({c.S for c in cases}), rows=sorted({c.rows for c in cases}),
                blocks=sorted({-(-c.rows // SGT_BLOCK) for c in cases}), block_tail=any(c.rows > SGT_BLOCK and c.rows % SGT_BLOCK for c in cases),
                partial_step=any(c.rows % 16 for c in cases), every_NV_with_tail=sorted({c.C // 64 for c in cases if c.rows % SGT_BLOCK}))


def _sgt_forward(x, W0, b0):
    xd = x.double()
    return xd @ W0.double().t() + b0.double()


def sgt_inputs(c: SgtCase) -> Dict[str, torch.Tensor]:
    """x bf16 [rows][C], W0 [S][C], b0, w3 [S], dsmap [rows]; bn_scale / bn_shift: the train-mode BatchNorm coefficients of y1 from the fp64
    reference, rounded ONCE to fp32 (what the kernel is handed); cA, cB, cC: the BatchNorm-backward coefficients from the fp64 backward
    statistics, rounded once; old bf16 [rows][C] for accumulate = 1."""
    g = _gen(10, c.C, c.S, c.rows)
    x = torch.randn(c.rows, c.C, generator=g).to(BF)
    W0, b0 = torch.randn(c.S, c.C, generator=g) * (2.0 / math.sqrt(c.C)), torch.randn(c.S, generator=g) * 0.5
    w3, ds = torch.randn(c.S, generator=g), torch.randn(c.rows, generator=g)
    gamma, beta = torch.rand(c.S, generator=g) + 0.5, torch.randn(c.S, generator=g) * 0.3
    y1 = _sgt_forward(x, W0, b0)
    n = float(c.rows)
    mean = y1.mean(0)
    var = (y1 * y1).mean(0) - mean * mean
    rstd = (var.clamp_min(0) + 1e-5).rsqrt()
    sc = (gamma.double() * rstd).float()
    sh = (beta.double() - mean * gamma.double() * rstd).float()
    z = y1 * sc.double() + sh.double()
    dz = ds.double()[:, None] * w3.double() * G.dgelu(z)
    S1, S2 = dz.sum(0), (dz * y1).sum(0)
    dg = rstd * (S2 - mean * S1)
    cA, cB, cC = sc.double(), -sc.double() * rstd * dg / n, (sc.double() / n) * (mean * rstd * dg - S1)
    return dict(x=x, W0=W0, b0=b0, w3=w3, dsmap=ds, bn_scale=sc, bn_shift=sh, cA=cA.float(), cB=cB.float(), cC=cC.float(),
                old=torch.randn(c.rows, c.C, generator=g).to(BF), gamma=gamma, beta=beta)


def _sgt_blocks(v: torch.Tensor, rows: int) -> torch.Tensor:
    """[rows][...] -> [blocks][...]: sums over each block of 256 rows"""
    nb = -(-rows // SGT_BLOCK)
    pad = nb * SGT_BLOCK - rows
    flat = v.reshape(rows, -1)
    return F.pad(flat, (0, 0, 0, pad)).view(nb, SGT_BLOCK, -1).sum(1).view(nb, *v.shape[1:])


def _sgt_pad16(v: torch.Tensor) -> torch.Tensor:
    return F.pad(v, (0, 16 - v.shape[-1]))


def spatial_gate_train_ref(i, c: SgtCase, what: int, accumulate: int = 0, mut: Optional[str] = None) -> Dict[str, Out]:
    """what 0: partial [blocks][2][16]; what 1: partial [blocks][4][16]; what 2: dx bf16 [rows][C], partial [blocks][16 (C + 1)] (d W0 [16][C],
    then d b0 [16]); slots s >= S are 0.  Bounds: y1  Tol.delta(C, sum |x W0|) + u (|b0| + |y1|);  z  |scale| t_y1 + 2u (|y1 scale| + |shift|);
    dz = ds w3 gelu'(z)  |ds w3| (GELU_LIP t_z + 8u) + 2u |dz|;  dy1  |cA| t_dz + |cB| t_y1 + Tol.delta(3, sum of the absolute terms);  every sum
    over a block's n rows: the sum of the terms' bounds + Tol.delta(n, sum |terms|);  dx: sum_s |W0| t_dy1 + Tol.delta(17, sum |W0 dy1| + |old|), then bf16.
    mut: 'no_bias', 'block_tail_dropped' (what 0); 'gelu_not_dgelu', 'no_w3' (what 1); 'no_cB_term', 'acc_ignores_old', 'dW_uses_dz' (what 2)."""
    x, W0 = i["x"].double(), i["W0"].double()
    rows = c.rows
    n_in = torch.tensor([min(SGT_BLOCK, rows - k * SGT_BLOCK) for k in range(-(-rows // SGT_BLOCK))], dtype=torch.float64)
    y1 = _sgt_forward(i["x"], i["W0"], i["b0"])
    t_y1 = Tol.delta(c.C, x.abs() @ W0.abs().t()) + U * (i["b0"].double().abs() + y1.abs())
    blk = lambda v: _sgt_blocks(v, rows)
    nshape = lambda v: n_in.view(-1, *([1] * (v.dim() - 1)))

    def summed(terms, t_terms):
        s = blk(terms.abs())
        return blk(t_terms) + Tol.delta(nshape(s), s)

    if what == 0:
        ym = y1 - i["b0"].double() if mut == "no_bias" else y1
        keep = (torch.arange(rows) < rows // SGT_BLOCK * SGT_BLOCK).double()[:, None] if mut == "block_tail_dropped" else 1.0
        ref = torch.stack([_sgt_pad16(blk(ym * keep)), _sgt_pad16(blk(ym * ym * keep))], 1)
        tol = torch.stack([_sgt_pad16(summed(y1, t_y1)), _sgt_pad16(summed(y1 * y1, 2 * y1.abs() * t_y1 + U * y1 * y1))], 1)
        return dict(partial=Out(ref, tol))
    sc, sh, w3, ds = i["bn_scale"].double(), i["bn_shift"].double(), i["w3"].double(), i["dsmap"].double()[:, None]
    z = y1 * sc + sh
    t_z = sc.abs() * t_y1 + 2 * U * ((y1 * sc).abs() + sh.abs())
    dz = ds * w3 * G.dgelu(z)
    t_dz = (ds * w3).abs() * (GELU_LIP * t_z + 8 * U) + 2 * U * dz.abs()
    if what == 1:
        dzm = ds * (1.0 if mut == "no_w3" else w3) * (G.gelu(z) if mut == "gelu_not_dgelu" else G.dgelu(z))
        a = ds * G.gelu(z)
        d0 = torch.zeros_like(dz)
        d0[:, 0] = ds[:, 0]
        ref = torch.stack([_sgt_pad16(blk(v)) for v in (dzm, dzm * y1, a, d0)], 1)
        tol = torch.stack([_sgt_pad16(v) for v in (summed(dz, t_dz), summed(dz * y1, t_dz * y1.abs() + dz.abs() * t_y1 + U * (dz * y1).abs()),
                                                   summed(a, ds.abs() * (GELU_LIP * t_z + 8 * U * z.abs()) + U * a.abs()),
                                                   summed(d0, torch.zeros_like(d0)))], 1)
        return dict(partial=Out(ref, tol))
    cA, cB, cC = i["cA"].double(), i["cB"].double(), i["cC"].double()
    dy1 = cA * dz + cB * y1 + cC
    t_dy1 = cA.abs() * t_dz + cB.abs() * t_y1 + Tol.delta(3, (cA * dz).abs() + (cB * y1).abs() + cC.abs())
    dym = cA * dz + (0.0 if mut == "no_cB_term" else cB * y1) + cC
    old = i["old"].double() if accumulate else torch.zeros_like(x)
    dx_exact = dy1 @ W0 + old
    dx = dym @ W0 + (torch.zeros_like(x) if mut == "acc_ignores_old" else old)
    t_dx = t_dy1 @ W0.abs() + Tol.delta(17, dy1.abs() @ W0.abs() + old.abs())
    dWsrc = dz if mut == "dW_uses_dz" else dym
    dW = blk(dWsrc[:, :, None] * x[:, None, :])                                   # [blocks][S][C]
    t_dW = summed(dy1[:, :, None] * x[:, None, :], t_dy1[:, :, None] * x.abs()[:, None, :])
    db = blk(dym)
    t_db = summed(dy1, t_dy1)
    nb = dW.shape[0]
    padS = lambda v: F.pad(v, (0, 0, 0, 16 - c.S)).reshape(nb, 16 * c.C)
    part = torch.cat([padS(dW), _sgt_pad16(db)], 1)
    t_part = torch.cat([padS(t_dW), _sgt_pad16(t_db)], 1)
    return dict(dx=Out(dx, t_bf16(dx_exact, t_dx)), partial=Out(part, t_part))


SGT_MUTANTS = {0: ("no_bias", "block_tail_dropped"), 1: ("gelu_not_dgelu", "no_w3"), 2: ("no_cB_term", "acc_ignores_old", "dW_uses_dz")}


def sgt_identity(mut: str, c: SgtCase, accumulate: int = 1) -> bool:
    return (mut == "block_tail_dropped" and c.rows % SGT_BLOCK == 0) or (mut == "acc_ignores_old" and not accumulate)


def sgt_exercises(mut: str, c: SgtCase) -> bool:
    """One token is its own batch: y1 equals the batch mean, so d gamma and with it cB vanish (nothing for 'no_cB_term' to leave out) and
    z = shift sits behind rstd = eps^-1/2, whose bound swallows a factor w3 ('no_w3'); dy1 = scale (dz - S1) is 0 up to that bound, so the
    weight gradient cannot tell dy1 from dz ('dW_uses_dz') and the bound of dx = W0^T dy1 exceeds the old values ('acc_ignores_old').  At
    rows = 1 the case checks the statistics of what 0, the index arithmetic, the guards and the pads."""
    return not (c.rows == 1 and mut in ("no_cB_term", "no_w3", "dW_uses_dz", "acc_ignores_old"))
