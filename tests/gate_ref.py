"""fp64 restatements, case lists and derived tolerances of HAT's CAB tail (include/srk.h: srk_channel_gate / srk_channel_gate_act,
srk_cab_add_ln, srk_cab_bwd; csrc/hat.hip, csrc/hat_train.hip) and of DAT's small functions (srk_channel_interaction_fwd / _bwd, their
_frozen_ forms, srk_chan_attn_matrix_fwd / _bwd; csrc/dat_small.hip).

Plain torch on the CPU, no GPU import.  tests/test_gate_ref.py pins the restatements against torch.autograd in fp64 and exercises their
negative controls; tests/test_gpu_gate_direct.py compares the kernels with them through the C ABI.

Tolerances.  u = U = 2^-24.  An fp32 sum whose additions form a tree of depth n is off by at most Tol.delta(n, S) = 2 n u S, S the sum of
the absolute terms (for a sequential chain n is the number of terms; the factor 2 also covers a product rounded before it is added, so a
contracted and an uncontracted multiply-add are both inside).  A hardware function (__expf, rsqrtf, the reciprocal, sqrtf, a division)
costs 8u relative, the project's figure per device function.  gelu_f: GELU_LIP times the bound of its argument plus 8u |argument| (that
term holds the 2.5u absolute error of erf_fast times |argument| / 2, its reciprocal, its exp and the three roundings); gelu' (
dgelu_shared_exp): DGELU_LIP (block_ref: max |gelu''| = 0.798) times the bound of the argument plus 8u.  sigmoid s(v): s (1 - s) t_v exp(t_v) -- the
derivative s (1 - s) changes by at most the factor exp(t_v) across the interval (|d log(s (1 - s)) / dv| = |1 - 2 s| <= 1) -- plus 8u s
for __expf and the division.  bf16 outputs: t_bf16 (dat_ref).  No figure is a fraction of max|ref| and none is fitted to what
the kernels return.

  pooling (channel_gate, cab_bwd)   a thread adds at most 32 tokens of its chunk (TM_ROWS = 256 tokens, 8 row groups), then the 8 row
                  groups are added, then the chunks: a chain of depth POOL_DEPTH + nchunk = 40 + nchunk.
                    sum      Tol.delta(40 + nchunk, sum |x|)                       (x bf16: exact addends)
                    mean     t_sum / HW + u |mean|
                    dgate    Tol.delta(41 + nchunk, sum |g conv|)                  (cab_bwd: sum_t g conv; one more for the product)
  gate MLP        z = b1 + sum_c w1 mean    sum_c |w1| t_mean + Tol.delta(C + 1, |b1| + sum |w1 mean|)
                  a = act(z)                ReLU: t_z;  GELU: GELU_LIP t_z + 8u |z|
                  v = b2 + sum_s w2 a       sum_s |w2| t_a + Tol.delta(S + 1, |b2| + sum |w2 a|)
                  sg = sigmoid(v)           sg (1 - sg) t_v exp(t_v) + 8u sg
                  gate = out_scale sg       |out_scale| t_sg + u |gate|;  pad columns exactly +0
  cab_add_ln      x' = x + conv gate        Tol.delta(2, |x| + |conv gate|); pad columns: 0 + conv * 0 = +0 exactly
                  LayerNorm: a lane adds NV groups of four ((a + b) + (c + d)), then four butterfly levels: depth LN_DEPTH(NV) = NV + 6
                    mean     (sum t_x' + Tol.delta(NV + 6, sum |x'|)) / C + 2u |mean|          (1 / C rounded, one product)
                    d        t_x' + t_mean + u |d|
                    var      (sum (2 |d| t_d + t_d^2 + 2u d^2) + Tol.delta(NV + 6, sum d^2)) / C + 3u (var + eps)
                    rstd     rstd^3 t_var / 2 + 8u rstd
                    xn       |gamma| (rstd t_d + |d| t_rstd) + Tol.delta(2, |d rstd gamma| + |beta|), then bf16; pad columns +0
  cab_bwd         z1, a, v, sg as the gate MLP (ReLU).  The inputs keep every z1 further from 0 than t_z1 (asserted on the CPU), so the
                  ReLU mask of the device is the reference's.
                    d = dgate out_scale sg (1 - sg)      |out_scale| (t_dgate sg (1 - sg) + |dgate| t_sg (1 + t_sg)) + 4u |d|
                    db2 = fill + sum_b d                 float atomics, ANY order over the B addends and the fill:
                                                         sum_b t_d + Tol.delta(B + 1, |fill| + sum |d|)
                    dw2 = fill + sum_b d a               sum_b (t_d |a| + |d| t_a) + Tol.delta(B + 1, |fill| + sum |d a|)
                    da = sum_c w2 d  (dz1 = da where z1 > 0)    sum_c |w2| t_d + Tol.delta(C, sum |w2 d|)
                    db1 = fill + sum_b dz1               sum_b t_dz1 + Tol.delta(B + 1, |fill| + sum |dz1|)
                    dw1 = fill + sum_b dz1 mean          sum_b (t_dz1 |mean| + |dz1| t_mean) + Tol.delta(B + 1, |fill| + sum |dz1 mean|)
                    dmean = sum_s w1 dz1 / HW            (sum_s |w1| t_dz1 + Tol.delta(S, sum |w1 dz1|)) / HW + u |dmean|
                    d_conv = bf16(g gate + dmean)        t_dmean + Tol.delta(2, |g gate| + |dmean|), then bf16 (gate is an exact input)
  channel interaction (trained)   pm = pooled[pad_of] inv_hw: u |pm| (one product).  y = b1 + sum_c pm w1: sum_c |w1| t_pm +
                  Tol.delta(C + 1, .).  Batch statistics over the B samples, sequentially:
                    m        (sum_b t_y + Tol.delta(B, sum |y|)) / B + u |m|
                    d        t_y + t_m + u |d|
                    v        (sum_b (2 |d| t_d + t_d^2 + 2u d^2) + Tol.delta(B, sum d^2)) / B + 2u (v + eps)
                    rstd     rstd^3 t_v / 2 + 8u rstd          (rsqrtf; first order in t_v: the inputs keep v >= 100 eps, asserted)
                    z        rstd t_d + |d| t_rstd + 2u |z|
                    arg = z gamma + beta       |gamma| t_z + Tol.delta(1, |z gamma| + |beta|)
                    a = gelu(arg)              GELU_LIP t_arg + 8u |arg|
                    o = sigmoid(b2 + sum_s a w2)     the sigmoid bound of t_pre = sum_s |w2| t_a + Tol.delta(S + 1, .);  padding exactly +0
                    running_mean = (1 - mom) old + mom m       mom t_m + Tol.delta(3, |old| + |m|)
                    running_var  = (1 - mom) old + mom v B / (B - 1)     mom B / (B - 1) t_v + Tol.delta(4, |old| + v B / (B - 1))
                  backward (pm is an exact fp32 input; the forward chain above with t_pm = 0):
                    dpre = dcg o (1 - o)       |dcg| t_o (1 + t_o) + 2u |dpre|
                    dW2 = sum_b dpre a         sum_b (t_dpre |a| + |dpre| t_a) + Tol.delta(B, sum |dpre a|);   db2: sum_b t_dpre + Tol.delta(B, .)
                    da = sum_c dpre w2         sum_c t_dpre |w2| + Tol.delta(C, .)
                    dyo = da gelu'(arg)        t_da |gelu'| + |da| (DGELU_LIP t_arg + 8u) + u |dyo|
                    dgamma = sum_b dyo z       sum_b (t_dyo |z| + |dyo| t_z) + Tol.delta(B, .);   dbeta = sum_b dyo: sum_b t_dyo + Tol.delta(B, .)
                    inner = dyo - dbeta / B - z dgamma / B      t_dyo + t_dbeta / B + (t_z |dgamma| + |z| t_dgamma) / B + Tol.delta(3, sum of the |terms|)
                    dy = gamma rstd inner      |gamma| (rstd t_inner + t_rstd |inner|) + 2u |dy|
                    dW1 = sum_b dy pm          sum_b t_dy |pm| + Tol.delta(B, .);   db1 = sum_b dy (exactly 0 in exact arithmetic): sum_b t_dy + Tol.delta(B, sum |dy|)
                    dpool = inv_hw sum_s dy w1         inv_hw (sum_s t_dy |w1| + Tol.delta(S, .)) + u |dpool|;  padding exactly +0
  channel interaction (frozen)    mean = running_mean (exact), rstd = 1 / sqrtf(running_var + eps): 2 x 8u + u relative; z = (y - mean) rstd:
                  rstd (t_y + u |y - mean|) + |y - mean| t_rstd + 2u |z|; the rest as above with dy = gamma rstd dyo.
  attention matrix   gram is a fixed sequence of IEEE additions: restated in fp32 (gram_f32) and compared bit for bit; everything else is
                  bounded from THAT gram (and, in the backward, from the fp32 A handed in and the restated fp32 dA), so no sum over
                  chunks is counted twice.
                    l = G / (nq nk) t          (3 x 8 + 2) u |l|          two sqrtf, one division, two products
                    A = softmax_j l            e_j = exp(l_j - max): relative D_j = t_l(j) + t_l(argmax) + u |l_j - max| + 8u; the sum (depth 7)
                                               and its reciprocal: max_j D_j + Tol.delta(7, 1) + 8u + u:   A (D_j + max_k D_k + 23u)
                                               rows / columns >= dh exactly +0; a zero-norm channel gives exactly 1 / dh
                    dot = sum_j dA A           Tol.delta(dh, sum |dA A|)
                    dl = A (dA - dot)          A t_dot + 2u A (|dA| + |dot|) + u |dl|
                    cos = G rq rk              (4 x 8 + 2) u |cos|         rq, rk: sqrtf and a division each
                    dG = dl t rq rk            t_dl t rq rk + (4 x 8 + 3) u |dG|;   dGt: bit-equal to dG transposed
                    dtemp = sum dl cos         sum (t_dl |cos| + |dl| t_cos) + Tol.delta(64, sum |dl cos|)      32 per row, then 32 rows
                    LL = dl cos t              t (t_dl |cos| + |dl| t_cos) + 2u |LL|
                    dsq2 = -sum_j LL / sq      (sum_j t_LL + Tol.delta(32, sum |LL|)) / sq + 9u |dsq2|    the 1 / sq amplification; dsk2 by columns
                                               channels with sq <= 1e-24 (clamped) exactly 0

Cases: GATE_CASES x act 0 / 1, ADDLN_CASES, CABBWD_CASES, CI_CASES (trained; CI_FROZEN_CASES adds B 1), MAT_CASES; *_coverage say what
each list reaches and tests/test_gate_ref.py asserts it.  Negative controls: every restatement takes mut = <name>; *_MUTANTS lists them
per family and *_identity names the (mutant, case) pairs on which a mutant IS the reference by construction."""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Dict, List, Optional

import torch

import gemm_ex_ref as G
from block_ref import DGELU_LIP
from dat_ref import BF, _gen, t_bf16
from gemm_ex_ref import GELU_LIP, LN_EPS, U, Tol
from glue_ref import Out, accepts, bits, same_bits  # noqa: F401  (re-exported for the tests)

F64 = torch.float64
TM_ROWS = 256                  # tokens per chunk of the pooling passes
POOL_DEPTH = 32 + 8            # a thread's 32 tokens, then the 8 row groups
DEV = 8 * U                    # one device function


def _sigmoid_tol(sg, t_v):
    return sg * (1 - sg) * t_v * torch.exp(t_v) + DEV * sg


# ---- srk_channel_gate / srk_channel_gate_act -----------------------------------------------------------------------------------------
@dataclass(frozen=True)
class GateCase:
    B: int
    HW: int
    C: int
    CP: int
    S: int
    dead: bool = False             # cab_bwd: every hidden unit dead (b1 strongly negative)
    out_scale: float = 0.01

    @property
    def id(self) -> str:
        return f"B{self.B}-HW{self.HW}-C{self.C}of{self.CP}-S{self.S}" + ("-dead" if self.dead else "")

    @property
    def nchunk(self) -> int:
        return -(-self.HW // TM_ROWS)


GATE_HW = (1, 7, 8, 255, 256, 257, 700)
GATE_C_CP = ((64, 64), (30, 64), (90, 128), (180, 192), (250, 256), (256, 256))
GATE_S = (1, 6, 64)
GATE_B = (1, 3)
GATE_CASES = [GateCase(1, 1, 64, 64, 1), GateCase(3, 7, 30, 64, 6), GateCase(1, 8, 90, 128, 64), GateCase(3, 255, 180, 192, 6),
              GateCase(1, 256, 180, 192, 1), GateCase(3, 257, 256, 256, 6), GateCase(3, 700, 180, 192, 6), GateCase(1, 257, 30, 64, 64),
              GateCase(3, 256, 90, 128, 6), GateCase(1, 700, 250, 256, 64), GateCase(3, 8, 64, 64, 6), GateCase(1, 255, 256, 256, 1)]


def gate_coverage(cases: List[GateCase]) -> Dict[str, object]:
    return dict(HW=sorted({c.HW for c in cases}), C_CP=sorted({(c.C, c.CP) for c in cases}), S=sorted({c.S for c in cases}),
                B=sorted({c.B for c in cases}), full_chunk=any(c.HW == TM_ROWS for c in cases),
                one_token_tail=any(c.HW % TM_ROWS == 1 and c.HW > TM_ROWS for c in cases), under_8_tokens=any(c.HW < 8 for c in cases),
                c_not_multiple_of_4=any(c.C % 4 for c in cases), chunks=sorted({c.nchunk for c in cases}))


def gate_inputs(c: GateCase) -> Dict[str, torch.Tensor]:
    """x bf16 [B*HW][C] (tokens around a per-(sample, channel) offset, so that the means differ between samples), w1 [S][C], b1 [S],
    w2 [C][S], b2 [C].  S == 1: b1 = +1.5 and a smaller w1: the one hidden unit is live under ReLU, away from the
    flat stretch of GELU and from where GELU meets ReLU, so that the gate depends on the mean and on the activation."""
    g = _gen(11, c.B, c.HW, c.C, c.S)
    off = torch.randn(c.B, 1, c.C, generator=g) * 0.5
    x = (torch.randn(c.B, c.HW, c.C, generator=g) + off).reshape(c.B * c.HW, c.C).to(BF)
    w1 = torch.randn(c.S, c.C, generator=g) * ((2.0 if c.S > 1 else 0.5) / math.sqrt(c.C))
    b1 = torch.randn(c.S, generator=g) if c.S > 1 else torch.full((1,), 1.5)
    w2 = torch.randn(c.C, c.S, generator=g) / math.sqrt(c.S)
    b2 = torch.randn(c.C, generator=g) * 0.5
    return dict(x=x, w1=w1, b1=b1, w2=w2, b2=b2)


def _pool(x: torch.Tensor, c: GateCase, mut: Optional[str]):
    """per-sample token sums fp64 [B][C] under the pooling mutants, and the bound of the sum"""
    xd = x.double().reshape(c.B, c.HW, -1)
    keep = torch.ones(c.HW, dtype=F64)
    r = torch.arange(c.HW)
    if mut == "chunk_tail_dropped":
        keep[r >= c.HW // TM_ROWS * TM_ROWS] = 0.0
    if mut == "rowgroup7_dropped":
        keep[(r % TM_ROWS) % 8 == 7] = 0.0
    s = (xd * keep[None, :, None]).sum(1)
    return s, Tol.delta(POOL_DEPTH + c.nchunk, xd.abs().sum(1))


def _mlp(mean, t_mean, w1, b1, w2, b2, act: int, mut: Optional[str] = None):
    """z, a, v, sg and their bounds (fp64; w1 [S][C], w2 [C][S])"""
    S, C = w1.shape
    w1d, w2d = w1.double(), w2.double()
    if mut == "w2_transposed":
        w2d = w2d.reshape(S, C).t()
    z = mean @ w1d.t() + b1.double()
    t_z = t_mean @ w1d.abs().t() + Tol.delta(C + 1, mean.abs() @ w1d.abs().t() + b1.double().abs())
    if (act == 1) != (mut == "act_swapped"):
        a, t_a = G.gelu(z), GELU_LIP * t_z + DEV * z.abs()
    else:
        a, t_a = torch.relu(z), t_z
    v = a @ w2d.t() + b2.double()
    t_v = t_a @ w2d.abs().t() + Tol.delta(S + 1, a.abs() @ w2d.abs().t() + b2.double().abs())
    sg = torch.sigmoid(v)
    return z, t_z, a, t_a, v, t_v, sg, _sigmoid_tol(sg, t_v)


def channel_gate_ref(x, w1, b1, w2, b2, c: GateCase, act: int, mut: Optional[str] = None) -> Dict[str, Out]:
    """gate fp32 [B][CP], pad columns 0.  mut: 'div_cp', 'chunk_tail_dropped', 'rowgroup7_dropped', 'w1_stride_cp' (the hidden layer walks
    CP columns per row of w1: the mean over CP columns), 'act_swapped', 'w2_transposed'."""
    def run(m):
        s, t_s = _pool(x, c, m)
        mean = s / (c.CP if m == "div_cp" else c.HW)
        t_mean = t_s / c.HW + U * mean.abs()
        w1m = w1
        if m == "w1_stride_cp":
            w1m = w1.reshape(-1)[(torch.arange(c.S)[:, None] * c.CP + torch.arange(c.C)[None, :]) % (c.S * c.C)]
        *_, sg, t_sg = _mlp(mean, t_mean, w1m, b1, w2, b2, act, m)
        return c.out_scale * sg, abs(c.out_scale) * t_sg + U * (c.out_scale * sg).abs()

    exact, tol = run(None)
    val = run(mut)[0] if mut else exact
    ref, t = torch.zeros(c.B, c.CP, dtype=F64), torch.zeros(c.B, c.CP, dtype=F64)
    ref[:, :c.C], t[:, :c.C] = val, tol
    return dict(gate=Out(ref, t))


GATE_MUTANTS = ("div_cp", "chunk_tail_dropped", "rowgroup7_dropped", "w1_stride_cp", "act_swapped", "w2_transposed")


def gate_identity(mut: str, c: GateCase) -> bool:
    return (mut == "div_cp" and c.HW == c.CP) or (mut == "chunk_tail_dropped" and c.HW % TM_ROWS == 0) or \
        (mut == "rowgroup7_dropped" and c.HW < 8) or (mut == "w1_stride_cp" and (c.C == c.CP or c.S == 1)) or \
        (mut == "w2_transposed" and (c.S == 1 or c.C == 1))


# ---- srk_cab_add_ln --------------------------------------------------------------------------------------------------------------------
ADDLN_GRID_CAP = 8192          # workgroups of 16 rows
ADDLN_ROWS_PER_GROUP = 16


@dataclass(frozen=True)
class AddLnCase:
    C: int
    CP: int
    rps: int
    B: int
    ln: bool = True                # False: the xn == nullptr form, gamma and beta null

    @property
    def rows(self) -> int:
        return self.rps * self.B

    @property
    def NV(self) -> int:
        return self.CP // 64

    @property
    def id(self) -> str:
        return f"C{self.C}of{self.CP}-rps{self.rps}-B{self.B}" + ("" if self.ln else "-noln")


ADDLN_CASES = [AddLnCase(C, CP, 7, 3) for C, CP in ((64, 64), (61, 64), (128, 128), (90, 128), (192, 192), (181, 192), (256, 256), (250, 256))] + \
    [AddLnCase(61, 64, 7, 3, ln=False), AddLnCase(30, 64, 7, 18728)]


def addln_coverage(cases: List[AddLnCase]) -> Dict[str, object]:
    return dict(NV_full=sorted({c.NV for c in cases if c.C == c.CP and c.ln}), NV_ragged=sorted({c.NV for c in cases if c.C % 4 and c.ln}),
                rows_not_multiple_of_4=any(c.rows % 4 for c in cases), sample_edge_in_group=any(c.rps % 4 and c.B > 1 for c in cases),
                no_ln=any(not c.ln for c in cases), wrap=any(c.rows > ADDLN_GRID_CAP * ADDLN_ROWS_PER_GROUP and c.ln for c in cases))


def addln_inputs(c: AddLnCase) -> Dict[str, torch.Tensor]:
    """x fp32 [rows][CP] around a row mean of 2 (pad columns ZERO: the contract), conv bf16 [rows][CP] (pad columns finite and non-zero),
    gate fp32 [B][CP] (pad columns zero), gamma, beta [C]."""
    g = _gen(12, c.C, c.CP, c.rps, c.B)
    x = torch.zeros(c.rows, c.CP)
    x[:, :c.C] = torch.randn(c.rows, c.C, generator=g) + 2.0
    conv = torch.randn(c.rows, c.CP, generator=g).to(BF)
    gate = torch.zeros(c.B, c.CP)
    gate[:, :c.C] = torch.rand(c.B, c.C, generator=g) * 0.5 + 0.1
    return dict(x=x, conv=conv, gate=gate, gamma=torch.rand(c.C, generator=g) + 0.5, beta=torch.randn(c.C, generator=g) * 0.1)


def cab_add_ln_ref(x, conv, gate, gamma, beta, c: AddLnCase, mut: Optional[str] = None) -> Dict[str, Out]:
    """x fp32 [rows][CP] (in place) and, with c.ln, xn bf16 [rows][CP].  mut: 'sample_off' (the gate of sample b + 1), 'ln_div_cp',
    'var_with_pads', 'last_masked_kept' (the components of the float4 that straddles C all count in the variance), 'wrap_skipped' (rows
    beyond the capped grid's first pass untouched: x stays, xn receives 0)."""
    C, CP, rows = c.C, c.CP, c.rows
    b = torch.arange(rows) // c.rps
    gd = gate.double()
    cg = conv.double() * gd[b]
    x1 = x.double() + cg
    t_x = Tol.delta(2, x.double().abs() + cg.abs())
    xv = x.double() + conv.double() * gd[(b + 1) % c.B] if mut == "sample_off" else x1.clone()
    first_pass = torch.arange(rows) < ADDLN_GRID_CAP * ADDLN_ROWS_PER_GROUP
    if mut == "wrap_skipped":
        xv[~first_pass] = x.double()[~first_pass]
    out = dict(x=Out(xv, t_x))
    if not c.ln:
        return out
    depth = c.NV + 6

    def ln(xx, m):
        n = CP if m == "ln_div_cp" else C
        hi = CP if m == "var_with_pads" else -(-C // 4) * 4 if m == "last_masked_kept" else C
        mean = xx.sum(1, keepdim=True) / n
        d = xx - mean
        var = (d[:, :hi] ** 2).sum(1, keepdim=True) / n
        return mean, d, var, (var + LN_EPS).rsqrt()

    mean, d, var, rstd = ln(x1, None)
    ga, be = gamma.double(), beta.double()
    t_mean = (t_x.sum(1, keepdim=True) + Tol.delta(depth, x1.abs().sum(1, keepdim=True))) / C + 2 * U * mean.abs()
    t_d = (t_x + t_mean + U * d.abs())[:, :C]
    dr = d[:, :C]
    t_var = ((2 * dr.abs() * t_d + t_d ** 2 + 2 * U * dr ** 2).sum(1, keepdim=True) + Tol.delta(depth, (dr ** 2).sum(1, keepdim=True))) / C \
        + 3 * U * (var + LN_EPS)
    t_rstd = rstd ** 3 * t_var / 2 + DEV * rstd
    exact = dr * rstd * ga + be
    t = ga.abs() * (rstd * t_d + dr.abs() * t_rstd) + Tol.delta(2, (dr * rstd * ga).abs() + be.abs())
    val = exact
    if mut is not None:
        _, dm, _, rm = ln(xv, mut)
        val = dm[:, :C] * rm * ga + be
        if mut == "wrap_skipped":
            val[~first_pass] = 0.0
    ref, tol = torch.zeros(rows, CP, dtype=F64), torch.zeros(rows, CP, dtype=F64)
    ref[:, :C], tol[:, :C] = val, t_bf16(exact, t)
    out["xn"] = Out(ref, tol)
    return out


ADDLN_MUTANTS = ("sample_off", "ln_div_cp", "var_with_pads", "last_masked_kept", "wrap_skipped")


def addln_identity(mut: str, c: AddLnCase) -> bool:
    if mut == "sample_off":
        return c.B == 1
    if mut == "wrap_skipped":
        return c.rows <= ADDLN_GRID_CAP * ADDLN_ROWS_PER_GROUP
    if not c.ln:
        return True                                     # the LayerNorm mutants do not reach the xn == nullptr form
    return (mut in ("ln_div_cp", "var_with_pads") and c.C == c.CP) or (mut == "last_masked_kept" and c.C % 4 == 0)


# ---- srk_cab_bwd -----------------------------------------------------------------------------------------------------------------------
DCONV_GRID_CAP = 16384         # workgroups of 256 float4
BWD_SCALE = 0.25
CABBWD_CASES = [GateCase(3, 1, 64, 64, 6, out_scale=BWD_SCALE), GateCase(3, 7, 30, 64, 6, out_scale=BWD_SCALE),
                GateCase(3, 8, 90, 128, 64, out_scale=BWD_SCALE), GateCase(3, 255, 180, 192, 6, out_scale=BWD_SCALE),
                GateCase(1, 256, 180, 192, 1, out_scale=BWD_SCALE), GateCase(3, 257, 256, 256, 6, out_scale=BWD_SCALE),
                GateCase(3, 700, 180, 192, 6, out_scale=BWD_SCALE), GateCase(1, 257, 250, 256, 64, out_scale=BWD_SCALE),
                GateCase(3, 7, 30, 64, 1, dead=True, out_scale=BWD_SCALE), GateCase(2, 32800, 250, 256, 6, out_scale=BWD_SCALE)]


def cabbwd_coverage(cases: List[GateCase]) -> Dict[str, object]:
    cov = gate_coverage(cases)
    cov.update(all_dead=any(c.dead and c.S == 1 for c in cases),
               wrap=any(c.B * c.HW * (c.CP // 4) > DCONV_GRID_CAP * 256 for c in cases))
    return cov


def cabbwd_inputs(c: GateCase) -> Dict[str, torch.Tensor]:
    """conv bf16 [B*HW][C], g fp32 [B*HW][CP] (pad columns finite and non-zero), gate fp32 [B][CP] = the forward's gate rounded once (pad
    columns zero), the gate MLP's parameters and the non-zero fills of the four accumulated gradients.  Hidden unit 0 is live (b1 = +2)
    and unit 1 dead (b1 = -2) for every sample; the others have b1 = 0, so that their masks follow the sample's mean.  S == 1: live
    (b1 = +2), or dead (b1 = -5) in the all-dead case."""
    g = _gen(13, c.B, c.HW, c.C, c.S, int(c.dead))
    off = torch.randn(c.B, 1, c.C, generator=g) * 0.5
    conv = (torch.randn(c.B, c.HW, c.C, generator=g) + off).reshape(c.B * c.HW, c.C).to(BF)
    w1 = torch.randn(c.S, c.C, generator=g) * (2.0 / math.sqrt(c.C))
    b1 = torch.zeros(c.S)
    b1[0] = -5.0 if c.dead else 2.0
    if c.S > 1:
        b1[1] = -2.0
    w2 = torch.randn(c.C, c.S, generator=g) / math.sqrt(c.S)
    b2 = torch.randn(c.C, generator=g) * 0.5
    gg = torch.randn(c.B * c.HW, c.CP, generator=g)
    fwd = channel_gate_ref(conv, w1, b1, w2, b2, c, 0)["gate"].ref.float()
    fill = {k: torch.randn(s, generator=g) * 0.5 + 1.0 for k, s in (("dw1", (c.S, c.C)), ("db1", (c.S,)), ("dw2", (c.C, c.S)), ("db2", (c.C,)))}
    return dict(conv=conv, g=gg, gate=fwd, w1=w1, b1=b1, w2=w2, b2=b2, fill=fill)


def cab_bwd_ref(i: Dict[str, torch.Tensor], c: GateCase, mut: Optional[str] = None) -> Dict[str, Out]:
    """dw1, db1, dw2, db2 (fill + gradient), dmean fp32 [B][CP], d_conv bf16 [B*HW][CP], and z1 / t_z1 for the live/dead assertions.
    mut: 'dmean_no_hw', 'dgate_no_scale', 'mask_other_sample', 'dconv_no_pool', 'overwrite'."""
    B, HW, C, CP, S = c.B, c.HW, c.C, c.CP, c.S
    cd = i["conv"].double().reshape(B, HW, C)
    gd = i["g"].double().reshape(B, HW, CP)
    w1d, w2d = i["w1"].double(), i["w2"].double()
    s, t_s = _pool(i["conv"], c, None)
    mean, t_mean = s / HW, t_s / HW
    t_mean = t_mean + U * mean.abs()
    prod = gd[:, :, :C] * cd
    dgate, t_dgate = prod.sum(1), Tol.delta(POOL_DEPTH + 1 + c.nchunk, prod.abs().sum(1))
    z1, t_z1, a, t_a, v, t_v, sg, t_sg = _mlp(mean, t_mean, i["w1"], i["b1"], i["w2"], i["b2"], 0)
    scale = 1.0 if mut == "dgate_no_scale" else c.out_scale
    d = dgate * scale * sg * (1 - sg)
    t_d = abs(c.out_scale) * (t_dgate * sg * (1 - sg) + dgate.abs() * t_sg * (1 + t_sg)) + 4 * U * (dgate * c.out_scale * sg * (1 - sg)).abs()
    fill = {k: (torch.zeros_like(f) if mut == "overwrite" else f).double() for k, f in i["fill"].items()}
    fa = {k: f.double().abs() for k, f in i["fill"].items()}
    db2 = fill["db2"] + d.sum(0)
    t_db2 = t_d.sum(0) + Tol.delta(B + 1, fa["db2"] + d.abs().sum(0))
    dw2 = fill["dw2"] + d.t() @ a
    t_dw2 = t_d.t() @ a.abs() + d.abs().t() @ t_a + Tol.delta(B + 1, fa["dw2"] + d.abs().t() @ a.abs())
    da = d @ w2d
    t_da = t_d @ w2d.abs() + Tol.delta(C, d.abs() @ w2d.abs())
    live = (z1 > 0)
    if mut == "mask_other_sample":
        live = live.roll(-1, 0)
    dz1, t_dz1 = da * live, t_da * (z1 > 0)
    db1 = fill["db1"] + dz1.sum(0)
    t_db1 = t_dz1.sum(0) + Tol.delta(B + 1, fa["db1"] + dz1.abs().sum(0))
    dw1 = fill["dw1"] + dz1.t() @ mean
    t_dw1 = t_dz1.t() @ mean.abs() + dz1.abs().t() @ t_mean + Tol.delta(B + 1, fa["dw1"] + dz1.abs().t() @ mean.abs())
    dm_exact = (da * (z1 > 0)) @ w1d / HW
    dm = dz1 @ w1d / (1 if mut == "dmean_no_hw" else HW)
    t_dm = (t_dz1 @ w1d.abs() + Tol.delta(S, dz1.abs() @ w1d.abs())) / HW + U * dm_exact.abs()
    gt = i["gate"].double()
    gg = gd[:, :, :C] * gt[:, None, :C]
    exact = gg + dm_exact[:, None, :]
    t32 = t_dm[:, None, :] + Tol.delta(2, gg.abs() + dm_exact.abs()[:, None, :])
    dc = gg + (0.0 if mut == "dconv_no_pool" else dm[:, None, :])
    ref_dm, tol_dm = torch.zeros(B, CP, dtype=F64), torch.zeros(B, CP, dtype=F64)
    ref_dm[:, :C], tol_dm[:, :C] = dm, t_dm
    ref_dc, tol_dc = torch.zeros(B, HW, CP, dtype=F64), torch.zeros(B, HW, CP, dtype=F64)
    ref_dc[:, :, :C], tol_dc[:, :, :C] = dc, t_bf16(exact, t32)
    return dict(dw1=Out(dw1, t_dw1), db1=Out(db1, t_db1), dw2=Out(dw2, t_dw2), db2=Out(db2, t_db2), dmean=Out(ref_dm, tol_dm),
                d_conv=Out(ref_dc.reshape(B * HW, CP), tol_dc.reshape(B * HW, CP)), z1=Out(z1, t_z1))


CABBWD_OUTPUTS = ("dw1", "db1", "dw2", "db2", "dmean", "d_conv")
CABBWD_MUTANTS = ("dmean_no_hw", "dgate_no_scale", "mask_other_sample", "dconv_no_pool", "overwrite")


def cabbwd_identity(mut: str, c: GateCase) -> bool:
    """With every hidden unit dead nothing flows to dmean; a mask from another sample changes nothing with one sample or with the one
    hidden unit whose sign b1 fixes."""
    return (mut == "dmean_no_hw" and (c.HW == 1 or c.dead)) or (mut == "mask_other_sample" and (c.B == 1 or c.S == 1)) or \
        (mut == "dconv_no_pool" and c.dead)


# ---- srk_channel_interaction_fwd / _bwd and the frozen forms ---------------------------------------------------------------------------
CI_MAX_LDS = 150 * 1024
CI_EPS = 1e-5
CI_MOMENTUM = 0.1


def ci_lds_floats(B: int, C: int, S: int, bwd: bool) -> int:
    """csrc/dat_small.hip: W1 | W2 | pm [B][C] | zh, a [B][S] | mean, rstd, var [64]  (+ backward: dpre [B][C] | dy [B][S] | two [64])"""
    return 2 * S * C + B * C + 2 * B * S + 3 * 64 + ((B * C + B * S + 2 * 64) if bwd else 0)


def ci_covered(B: int, C: int, S: int, frozen: bool = False) -> bool:
    return B > (0 if frozen else 1) and C > 0 and 0 < S <= 64 and ci_lds_floats(B, C, S, True) * 4 <= CI_MAX_LDS


def ci_largest_B(C: int, S: int) -> int:
    B = 2
    while ci_covered(B + 1, C, S):
        B += 1
    return B


@dataclass(frozen=True)
class CiCase:
    B: int
    C: int
    S: int
    nH: int
    running: bool = True           # trained forward: the running buffers given (False: both null)

    @property
    def dh(self) -> int:
        return self.C // self.nH

    @property
    def CA(self) -> int:
        return self.nH * 32

    @property
    def ldp(self) -> int:
        return self.CA + 8

    @property
    def ldg(self) -> int:
        return self.CA + 16

    @property
    def id(self) -> str:
        return f"B{self.B}-C{self.C}-S{self.S}-nH{self.nH}" + ("" if self.running else "-norunning")


CI_SHAPES = ((2, 24, 3, 2), (3, 60, 7, 4), (16, 180, 22, 6), (5, 64, 64, 2), (4, 30, 1, 1))
CI_CASES = [CiCase(*s) for s in CI_SHAPES] + [CiCase(ci_largest_B(180, 22), 180, 22, 6), CiCase(3, 60, 7, 4, running=False)]
CI_FROZEN_CASES = [CiCase(*s) for s in CI_SHAPES] + [CiCase(ci_largest_B(180, 22), 180, 22, 6), CiCase(1, 60, 7, 4), CiCase(1, 180, 22, 6)]
CI_INV_HW = 1.0 / 64


def ci_coverage(cases: List[CiCase]) -> Dict[str, object]:
    return dict(shapes=sorted({(c.B, c.C, c.S, c.nH) for c in cases}), largest_covered=any(ci_covered(c.B, c.C, c.S) and not ci_covered(c.B + 1, c.C, c.S)
                                                                                           for c in cases),
                strides_crossed=max(-(-c.B * c.C // 512) for c in cases), running_null=any(not c.running for c in cases),
                dh_32=any(c.dh == 32 for c in cases), dh_not_multiple_of_4=any(c.dh % 4 for c in cases), B1=any(c.B == 1 for c in cases),
                ldp_wider=all(c.ldp > c.CA for c in cases), ldg_wider=all(c.ldg > c.CA for c in cases))


def ci_pad_of(c: CiCase) -> torch.Tensor:
    ch = torch.arange(c.C)
    return ((ch // c.dh) * 32 + ch % c.dh).to(torch.int32)


def ci_inputs(c: CiCase, frozen: bool = False) -> Dict[str, torch.Tensor]:
    """pooled fp32 [B][ldp]: token sums at the positions pad_of names, NaN elsewhere; the parameters; the running buffers; dcg fp32
    [B][ldg] (NaN where pad_of does not point).  The samples' pooled means differ by O(1) per channel, so that the batch variance of
    every hidden unit stays far above eps."""
    g = _gen(14, c.B, c.C, c.S, c.nH, int(frozen))
    po = ci_pad_of(c).long()
    pooled = torch.full((c.B, c.ldp), float("nan"))
    pooled[:, po] = torch.randn(c.B, c.C, generator=g) / CI_INV_HW
    dcg = torch.full((c.B, c.ldg), float("nan"))
    dcg[:, po] = torch.randn(c.B, c.C, generator=g)
    return dict(pooled=pooled, dcg=dcg, W1=torch.randn(c.S, c.C, generator=g) * (1.5 / math.sqrt(c.C)), b1=torch.randn(c.S, generator=g) * 0.3,
                gamma=torch.rand(c.S, generator=g) + 0.5, beta=torch.randn(c.S, generator=g) * 0.3,
                W2=torch.randn(c.C, c.S, generator=g) / math.sqrt(c.S), b2=torch.randn(c.C, generator=g) * 0.5,
                running_mean=torch.randn(c.S, generator=g) * 0.3, running_var=torch.rand(c.S, generator=g) + 0.5)


def _ci_forward(pm, t_pm, i, c: CiCase, frozen: bool, mut: Optional[str] = None):
    """the chain up to o = sigmoid(.) in fp64 with its bounds; pm fp64 [B][C]"""
    B, C, S = c.B, c.C, c.S
    W1, W2 = i["W1"].double(), i["W2"].double()
    b1, b2, ga, be = i["b1"].double(), i["b2"].double(), i["gamma"].double(), i["beta"].double()
    y = pm @ W1.t() + b1
    t_y = t_pm @ W1.abs().t() + Tol.delta(C + 1, pm.abs() @ W1.abs().t() + b1.abs())
    if frozen and mut != "batch_stats":
        m, var = i["running_mean"].double(), i["running_var"].double()
        rstd = (var + CI_EPS).rsqrt()
        t_rstd = (2 * DEV + U) * rstd
        d = y - m
        t_d = t_y + U * d.abs()
        t_m = t_v = torch.zeros_like(m)
    else:
        m = y.mean(0)
        d = y - m
        var = (d * d).mean(0)
        t_m = (t_y.sum(0) + Tol.delta(B, y.abs().sum(0))) / B + U * m.abs()
        t_d = t_y + t_m + U * d.abs()
        t_v = ((2 * d.abs() * t_d + t_d ** 2 + 2 * U * d * d).sum(0) + Tol.delta(B, (d * d).sum(0))) / B + 2 * U * (var + CI_EPS)
        vn = var * B / (B - 1) if mut == "norm_unbiased" and B > 1 else var
        rstd = (vn + CI_EPS).rsqrt()
        t_rstd = rstd ** 3 * t_v / 2 + DEV * rstd
    z = d * rstd
    t_z = rstd * t_d + d.abs() * t_rstd + 2 * U * z.abs()
    arg = z * ga + be
    t_arg = ga.abs() * t_z + Tol.delta(1, (z * ga).abs() + be.abs())
    a = G.gelu(arg)
    t_a = GELU_LIP * t_arg + DEV * arg.abs()
    pre = a @ W2.t() + b2
    t_pre = t_a @ W2.abs().t() + Tol.delta(S + 1, a.abs() @ W2.abs().t() + b2.abs())
    o = torch.sigmoid(pre)
    return dict(y=y, m=m, var=var, t_m=t_m, t_v=t_v, rstd=rstd, t_rstd=t_rstd, z=z, t_z=t_z, arg=arg, t_arg=t_arg, a=a, t_a=t_a, o=o,
                t_o=_sigmoid_tol(o, t_pre))


def _scatter(v, t, c: CiCase, mut: Optional[str]):
    ref, tol = torch.zeros(c.B, c.CA, dtype=F64), torch.zeros(c.B, c.CA, dtype=F64)
    po = ci_pad_of(c).long()
    ref[:, torch.arange(c.C) if mut == "pad_of_ignored" else po] = v
    tol[:, po] = t
    return Out(ref, tol)


def channel_interaction_fwd_ref(i, c: CiCase, frozen: bool = False, mut: Optional[str] = None) -> Dict[str, Out]:
    """pm_out [B][C], cgate [B][CA] and (trained, running buffers given) running_mean / running_var [S] after the update.
    mut: 'norm_unbiased', 'running_biased', 'momentum_swapped', 'pad_of_ignored'; frozen: 'pad_of_ignored', 'batch_stats'."""
    po = ci_pad_of(c).long()

    def run(m):
        src = i["pooled"].double()
        pm = (src[:, :c.C] if m == "pad_of_ignored" else src[:, po]) * CI_INV_HW
        f = _ci_forward(pm, U * pm.abs(), i, c, frozen, m)
        return pm, f

    pm, f = run(None)
    pmm, fm = run(mut) if mut else (pm, f)
    out = dict(pm_out=Out(pmm, U * pm.abs()), cgate=_scatter(fm["o"], f["t_o"], c, mut))
    if not frozen and c.running:
        mom, k = CI_MOMENTUM, c.B / (c.B - 1)
        rm0, rv0 = i["running_mean"].double(), i["running_var"].double()
        a, b = (mom, 1 - mom) if mut == "momentum_swapped" else (1 - mom, mom)
        out["running_mean"] = Out(a * rm0 + b * fm["m"], mom * f["t_m"] + Tol.delta(3, rm0.abs() + f["m"].abs()))
        out["running_var"] = Out(a * rv0 + b * fm["var"] * (1.0 if mut == "running_biased" else k),
                                 mom * k * f["t_v"] + Tol.delta(4, rv0.abs() + f["var"] * k))
    return out


def channel_interaction_bwd_ref(i, pm32: torch.Tensor, c: CiCase, frozen: bool = False, mut: Optional[str] = None) -> Dict[str, Out]:
    """dW1 [S][C], db1, dgamma, dbeta [S], dW2 [C][S], db2 [C] (OVERWRITTEN) and dpool [B][CA] from pm32 fp32 [B][C] (the forward's pm_out)
    and dcg.  mut: 'norm_unbiased', 'pad_of_ignored', 'db1_nonzero' (trained: the frozen form's sum), 'no_inv_hw'; frozen: 'batch_stats'."""
    B, C, S = c.B, c.C, c.S
    po = ci_pad_of(c).long()
    pm = pm32.double()
    W1, W2, ga = i["W1"].double(), i["W2"].double(), i["gamma"].double()

    def run(m):
        f = _ci_forward(pm, torch.zeros_like(pm), i, c, frozen, m)
        dc = i["dcg"].double()
        dc = dc[:, :C] if m == "pad_of_ignored" else dc[:, po]
        o, t_o, a, t_a, z, t_z = f["o"], f["t_o"], f["a"], f["t_a"], f["z"], f["t_z"]
        dpre = dc * o * (1 - o)
        t_dpre = dc.abs() * t_o * (1 + t_o) + 2 * U * dpre.abs()
        r = dict(dW2=(dpre.t() @ a, t_dpre.t() @ a.abs() + dpre.abs().t() @ t_a + Tol.delta(B, dpre.abs().t() @ a.abs())),
                 db2=(dpre.sum(0), t_dpre.sum(0) + Tol.delta(B, dpre.abs().sum(0))))
        da = dpre @ W2
        t_da = t_dpre @ W2.abs() + Tol.delta(C, dpre.abs() @ W2.abs())
        dg = G.dgelu(f["arg"])
        dyo = da * dg
        t_dyo = t_da * dg.abs() + da.abs() * (DGELU_LIP * f["t_arg"] + DEV) + U * dyo.abs()
        dgamma, dbeta = (dyo * z).sum(0), dyo.sum(0)
        t_dgamma = (t_dyo * z.abs() + dyo.abs() * t_z).sum(0) + Tol.delta(B, (dyo * z).abs().sum(0))
        t_dbeta = t_dyo.sum(0) + Tol.delta(B, dyo.abs().sum(0))
        r.update(dgamma=(dgamma, t_dgamma), dbeta=(dbeta, t_dbeta))
        if frozen and m != "batch_stats":
            inner, t_inner = dyo, t_dyo
        else:
            inner = dyo - dbeta / B - z * dgamma / B
            t_inner = t_dyo + t_dbeta / B + (t_z * dgamma.abs() + z.abs() * t_dgamma) / B + \
                Tol.delta(3, dyo.abs() + dbeta.abs() / B + (z * dgamma).abs() / B)
        dy = ga * f["rstd"] * inner
        t_dy = ga.abs() * (f["rstd"] * t_inner + f["t_rstd"] * inner.abs()) + 2 * U * dy.abs()
        r["dW1"] = (dy.t() @ pm, t_dy.t() @ pm.abs() + Tol.delta(B, dy.abs().t() @ pm.abs()))
        db1 = (ga * f["rstd"] * dyo).sum(0) if m == "db1_nonzero" else dy.sum(0)
        r["db1"] = (db1, t_dy.sum(0) + Tol.delta(B, dy.abs().sum(0)))
        k = 1.0 if m == "no_inv_hw" else CI_INV_HW
        dp = dy @ W1 * k
        r["dpool"] = (dp, (t_dy @ W1.abs() + Tol.delta(S, dy.abs() @ W1.abs())) * CI_INV_HW + U * (dy @ W1 * CI_INV_HW).abs())
        return r

    exact = run(None)
    val = run(mut) if mut else exact
    out = {k: Out(val[k][0], exact[k][1]) for k in ("dW1", "db1", "dgamma", "dbeta", "dW2", "db2")}
    out["dpool"] = _scatter(val["dpool"][0], exact["dpool"][1], c, mut)
    return out


CI_FWD_MUTANTS = ("norm_unbiased", "running_biased", "momentum_swapped", "pad_of_ignored")
CI_BWD_MUTANTS = ("norm_unbiased", "pad_of_ignored", "db1_nonzero", "no_inv_hw")
CI_FROZEN_MUTANTS = ("pad_of_ignored", "batch_stats")
CI_FROZEN_BWD_MUTANTS = ("pad_of_ignored", "batch_stats", "no_inv_hw")


def ci_identity(mut: str, c: CiCase) -> bool:
    return (mut == "pad_of_ignored" and (c.dh == 32 or c.nH == 1)) or (mut in ("running_biased", "momentum_swapped") and not c.running)


# ---- srk_chan_attn_matrix_fwd / _bwd ---------------------------------------------------------------------------------------------------
GSZ = 1088                     # G [32][32] | sum q^2 [32] | sum k^2 [32]
MAT_TOKENS = 16                # tokens per chunk of the test partials
CLAMP = 1e-24


@dataclass(frozen=True)
class MatCase:
    dh: int
    nchunk: int
    B: int
    nH: int
    clamp: bool = False            # q channel 1 and k channel 2 all zero, q channel 3 tiny (sum q^2 < 1e-24 but G != 0)
    temp: float = 0.0              # 0: per-head temperatures in 0.5 .. 1.5

    @property
    def id(self) -> str:
        return f"dh{self.dh}-ck{self.nchunk}-B{self.B}-nH{self.nH}" + ("-clamp" if self.clamp else "") + (f"-t{self.temp:g}" if self.temp else "")


MAT_DH = (32, 30, 15, 12, 1)
MAT_NCHUNK = (1, 2, 3, 4, 5, 9)
MAT_CASES = [MatCase(32, 1, 1, 1), MatCase(30, 2, 2, 6), MatCase(15, 3, 1, 1), MatCase(12, 4, 2, 6), MatCase(1, 5, 1, 1), MatCase(30, 9, 2, 6),
             MatCase(30, 5, 1, 1, clamp=True), MatCase(30, 4, 2, 6, temp=20.0), MatCase(32, 9, 2, 6)]


def mat_coverage(cases: List[MatCase]) -> Dict[str, object]:
    return dict(dh=sorted({c.dh for c in cases}), nchunk=sorted({c.nchunk for c in cases}), B_nH=sorted({(c.B, c.nH) for c in cases}),
                clamp=any(c.clamp for c in cases), saturated=any(c.temp >= 20 for c in cases),
                fwd_unrolled_body=any(c.nchunk >= 4 for c in cases), fwd_tail_after_body=any(c.nchunk > 4 and c.nchunk % 4 for c in cases),
                bwd_odd_tail=any(c.nchunk % 2 and c.nchunk > 2 for c in cases), mask_inside_float4=any(c.dh % 4 for c in cases))


def _gram_partials(p: torch.Tensor, q: torch.Tensor, c: MatCase) -> torch.Tensor:
    """chunk partials [B*nH][nchunk][GSZ] in fp32 of p^T q | sum p^2 | sum q^2 from bf16 [B*nH][nchunk][tokens][dh]"""
    pf, qf = p.float(), q.float()
    out = torch.zeros(c.B * c.nH, c.nchunk, GSZ)
    Gm = torch.zeros(c.B * c.nH, c.nchunk, 32, 32)
    Gm[:, :, :c.dh, :c.dh] = pf.transpose(2, 3) @ qf
    out[:, :, :1024] = Gm.reshape(c.B * c.nH, c.nchunk, 1024)
    out[:, :, 1024:1024 + c.dh] = (pf * pf).sum(2)
    out[:, :, 1056:1056 + c.dh] = (qf * qf).sum(2)
    return out


def mat_inputs(c: MatCase) -> Dict[str, torch.Tensor]:
    """partial = Gram partials of bf16 (q, k), dpartial = those of bf16 (d_out, v), computed in fp32 per chunk of MAT_TOKENS tokens (so
    |G_ij| <= |q_i| |k_j| holds), temperature [nH]."""
    g = _gen(15, c.dh, c.nchunk, c.B, c.nH, int(c.clamp))
    shape = (c.B * c.nH, c.nchunk, MAT_TOKENS, c.dh)
    q, k, v, do = (torch.randn(shape, generator=g).to(BF) for _ in range(4))
    if c.clamp:
        q[..., 1] = 0.0
        k[..., 2] = 0.0
        q[..., 3] = (torch.sign(q[..., 3].float()) * 2.0 ** -45).to(BF)
    temp = torch.full((c.nH,), c.temp) if c.temp else torch.rand(c.nH, generator=g) + 0.5
    return dict(partial=_gram_partials(q, k, c), dpartial=_gram_partials(do, v, c), temp=temp)


def gram_f32(partial: torch.Tensor) -> torch.Tensor:
    """the forward's sum over chunks as the kernel orders it, in fp32: four accumulators over chunks strided by 4, the tail onto the
    first, (a0 + a1) + (a2 + a3)"""
    n = partial.shape[1]
    acc = [torch.zeros_like(partial[:, 0]) for _ in range(4)]
    body = n // 4 * 4
    for ck in range(body):
        acc[ck % 4] = acc[ck % 4] + partial[:, ck]
    for ck in range(body, n):
        acc[0] = acc[0] + partial[:, ck]
    return (acc[0] + acc[1]) + (acc[2] + acc[3])


def dA_f32(dpartial: torch.Tensor) -> torch.Tensor:
    """the backward's sum over chunks: two accumulators over chunks strided by 2, the tail onto the first, a0 + a1; the G part only"""
    n = dpartial.shape[1]
    a0, a1 = torch.zeros_like(dpartial[:, 0, :1024]), torch.zeros_like(dpartial[:, 0, :1024])
    body = n // 2 * 2
    for ck in range(0, body, 2):
        a0, a1 = a0 + dpartial[:, ck, :1024], a1 + dpartial[:, ck + 1, :1024]
    for ck in range(body, n):
        a0 = a0 + dpartial[:, ck, :1024]
    return a0 + a1


def _mat_parts(gram: torch.Tensor, temp: torch.Tensor, c: MatCase, clamp: bool = True):
    gd = gram.double()
    Gm = gd[:, :1024].reshape(-1, 32, 32)
    sq, sk = gd[:, 1024:1056], gd[:, 1056:1088]
    lim = CLAMP if clamp else 0.0
    nq, nk = sq.clamp_min(lim).sqrt(), sk.clamp_min(lim).sqrt()
    t = temp.double().repeat(c.B)[:, None, None]
    return Gm, sq, sk, nq, nk, t


def chan_attn_matrix_fwd_ref(gram: torch.Tensor, temp: torch.Tensor, c: MatCase, mut: Optional[str] = None) -> Dict[str, Out]:
    """A [B*nH][32][32] from the fp32 gram [B*nH][GSZ] (gram_f32 of the partials).  mut: 'softmax32', 'no_clamp'."""
    dh = c.dh

    def run(m):
        Gm, sq, sk, nq, nk, t = _mat_parts(gram, temp, c, clamp=m != "no_clamp")
        l = Gm / (nq[:, :, None] * nk[:, None, :]) * t
        n = 32 if m == "softmax32" else dh
        A = torch.zeros_like(l)
        A[:, :dh, :n] = torch.softmax(l[:, :dh, :n], 2)
        A[:, :, dh:] = 0.0
        return l, A

    l, A = run(None)
    lr = l[:, :dh, :dh]
    t_l = (3 * 8 + 2) * U * lr.abs()
    mx, am = lr.max(2, keepdim=True)
    D = t_l + t_l.gather(2, am) + U * (lr - mx).abs() + DEV
    tol = torch.zeros_like(A)
    tol[:, :dh, :dh] = A[:, :dh, :dh] * (D + D.amax(2, keepdim=True) + Tol.delta(7, 1.0) + DEV + U)
    return dict(A=Out(run(mut)[1] if mut else A, tol))


def chan_attn_matrix_bwd_ref(dA32: torch.Tensor, gram: torch.Tensor, A32: torch.Tensor, temp: torch.Tensor, c: MatCase,
                             mut: Optional[str] = None) -> Dict[str, Out]:
    """dG, dGt [B*nH][32][32], dsq2, dsk2 [B*nH][32], dtemp [B*nH] from the fp32 dA (dA_f32 of the partials), the fp32 gram and the fp32 A.
    mut: 'dgt_not_transposed', 'dtemp_no_cos', 'clamped_grad'."""
    dh = c.dh
    Gm, sq, sk, nq, nk, t = _mat_parts(gram, temp, c)
    rq, rk = 1.0 / nq, 1.0 / nk
    live = torch.zeros(32, 32, dtype=F64)
    live[:dh, :dh] = 1.0
    A, dA = A32.double().reshape(-1, 32, 32) * live, dA32.double().reshape(-1, 32, 32) * live
    dot = (dA * A).sum(2, keepdim=True)
    t_dot = Tol.delta(dh, (dA * A).abs().sum(2, keepdim=True))
    dl = A * (dA - dot)
    t_dl = A * t_dot + 2 * U * A * (dA.abs() + dot.abs()) + U * dl.abs()
    cos = Gm * rq[:, :, None] * rk[:, None, :] * live
    t_cos = (4 * 8 + 2) * U * cos.abs()
    scale = t * rq[:, :, None] * rk[:, None, :]
    dG = dl * scale
    t_dG = t_dl * scale + (4 * 8 + 3) * U * dG.abs()
    dtemp = (dl if mut == "dtemp_no_cos" else dl * cos).sum((1, 2))
    t_dtemp = (t_dl * cos.abs() + dl.abs() * t_cos).sum((1, 2)) + Tol.delta(64, (dl * cos).abs().sum((1, 2)))
    LL = dl * cos * t
    t_LL = t * (t_dl * cos.abs() + dl.abs() * t_cos) + 2 * U * LL.abs()
    real = (torch.arange(32) < dh)[None, :]

    def diag(sums, t_sums, abs_sums, s2):
        ok = real & (s2 > CLAMP)
        den = s2.clamp_min(CLAMP)
        val = torch.where(real if mut == "clamped_grad" else ok, -sums / den, torch.zeros_like(sums))
        exact = torch.where(ok, -sums / den, torch.zeros_like(sums))
        tol = torch.where(ok, (t_sums + Tol.delta(32, abs_sums)) / den + 9 * U * exact.abs(), torch.zeros_like(sums))
        return Out(val, tol)

    return dict(dG=Out(dG, t_dG), dGt=Out(dG if mut == "dgt_not_transposed" else dG.transpose(1, 2), t_dG.transpose(1, 2)),
                dsq2=diag(LL.sum(2), t_LL.sum(2), LL.abs().sum(2), sq), dsk2=diag(LL.sum(1), t_LL.sum(1), LL.abs().sum(1), sk),
                dtemp=Out(dtemp, t_dtemp))


MAT_FWD_MUTANTS = ("softmax32", "no_clamp")
MAT_BWD_MUTANTS = ("dgt_not_transposed", "dtemp_no_cos", "clamped_grad")


def mat_identity(mut: str, c: MatCase) -> bool:
    """dh == 1: A = 1 and d l = A (dA - dA A) = 0 exactly, so every backward output is zero."""
    return (mut == "softmax32" and c.dh == 32) or (mut in ("no_clamp", "clamped_grad") and not c.clamp) or \
        (mut in ("dgt_not_transposed", "dtemp_no_cos") and c.dh == 1)
