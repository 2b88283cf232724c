"""fp64 restatements, case lists and derived tolerances of the kernels that sit between the GEMMs of the host-orchestrated models
(include/srk.h: srk_layernorm_fwd / _bwd, srk_rowscale_bf16, srk_add_f32_bf16, srk_add_bf16_into_f32, srk_add_f32, srk_cast_f32_bf16,
srk_img_prep, srk_stem_conv, srk_win_attention_fwd_padded, srk_channel_gate_act(act = 1), srk_spatial_gate_dev).

Plain torch on the CPU, no GPU import.  The restatements are pinned against torch.nn.functional / autograd and their negative controls
are exercised in tests/test_glue_ref.py; tests/test_gpu_glue.py compares the kernels with them.

Tolerances.  u = 2^-24 is the unit roundoff of fp32; a sum of L terms in ANY order is off by at most Tol.delta(L, S) = 2 L u S with
S = the sum of the absolute terms (tests/gemm_ex_ref.py::Tol; the factor 2 is its margin).  None of the figures below is fitted to what
the kernels give.

  LayerNorm forward (x is an exact fp32 input, d_i = x_i - mean):
    mean    Tol.delta(C, sum|x|) / C + u |mean|                      the C additions in any order, then one multiply by 1/C
    rstd    the variance bound propagated through (var + eps)^-1/2, plus 4u relative for the hardware reciprocal square root:
              t_d   = t_mean + u |d_i|                               d_i is formed from the device's mean
              t_var = (sum_i (2 |d_i| t_d + u d_i^2) + Tol.delta(C, sum d^2)) / C + 2u (var + eps)
              t_rstd = rstd^3 t_var / 2 + 4u rstd
    y_f32   32u (|gamma| sqrt(C) + |beta|)  -- the fp32 LayerNorm term of Tol.ln_fwd (|xhat| <= sqrt(C), a handful of fp32 operations per
            element) -- plus the statistics' own bounds carried to the output, |gamma| (rstd t_d + |d| t_rstd)
    y_bf16  no bound of its own: bit-equal to the round-to-nearest-even of the device's y_f32
  LayerNorm backward (dy is an exact bf16 input; mean / rstd are the fp64 statistics rounded ONCE to fp32 and handed to the kernel, and the
  reference reads those same fp32 values, so the forward's error is not counted twice):
    gx      Tol.lnbwd with a GEMM delta of 0: 16u times the sum of the absolute terms of the formula, |old| included
    dgamma  Tol.delta(rows, sum_rows |dy xhat|) + u (|old| + |ref|)   float atomics: no order assumed; the last term is the accumulating add
    dbeta   Tol.delta(rows, sum_rows |dy|)      + u (|old| + |ref|)
  stem conv: Tol.delta(36, sum |p| |w|) + u (|bias| + |ref|)          36 = 9 taps x 4 stored channels, products and sums in fp32
  img_prep, rowscale, the three adds, cast: a fixed sequence of IEEE operations -> the expectation is the same sequence on the CPU in fp32
    (and torch's round-to-nearest-even conversion to bf16), compared with torch.equal on the bit patterns; NaN compares as NaN-ness.
  window attention forward: the project's attention-forward bound, 2e-2 max|ref| (tests/test_gpu_hat.py).
  channel gate with GELU: the 1e-6 absolute of the ReLU test (tests/test_gpu_hat.py) times GELU_LIP.

Negative controls: every reference takes mut = <name>; *_MUTANTS lists them per family.  ln_identity / img_identity / stem_identity /
attn_identity name the (mutant, case) pairs on which a mutant is the reference itself BY CONSTRUCTION (a divisor CP at C == CP, reflection against edge repetition with nothing to pad,
...); tests/test_glue_ref.py asserts that those really are identities and that every other pair is rejected."""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch
import torch.nn.functional as F

import gemm_ex_ref as G
from gemm_ex_ref import GELU_LIP, LN_EPS, U, Tol
from oracle import dat_oracle as DO

ATTN_TOL = 2e-2                      # x max|ref|: tests/test_gpu_hat.py, attention kernels alone
GATE_TOL = 1e-6 * GELU_LIP           # tests/test_gpu_hat.py::test_channel_gate_and_cab_add_ln_vs_torch, through the GELU; the derived
                                     # per-element bound of the gate is tests/gate_ref.py (tests/test_gpu_gate_direct.py)


@dataclass
class Out:
    ref: torch.Tensor                # fp64
    tol: torch.Tensor                # fp64, broadcastable to ref


def accepts(got: Dict[str, torch.Tensor], exp: Dict[str, Out]) -> Tuple[bool, Dict[str, float]]:
    """(all outputs within their bounds, max(err / tol) per output).  A NaN anywhere is a rejection."""
    ok, ratios = True, {}
    for k, o in exp.items():
        err = (got[k].double() - o.ref).abs()
        tol = o.tol.expand_as(o.ref)
        ok = ok and bool((err <= tol).all())
        r = err / tol.clamp_min(1e-300)
        ratios[k] = float(torch.nan_to_num(r, nan=float("inf")).max()) if r.numel() else 0.0
    return ok, ratios


def bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def same_bits(got: torch.Tensor, want: torch.Tensor) -> bool:
    """Bit patterns equal; a NaN matches any NaN (nothing promises the payload)."""
    assert got.dtype == want.dtype and got.shape == want.shape
    return bool(((bits(got) == bits(want)) | (got.isnan() & want.isnan())).all())


def same_bits_or_flushed(got: torch.Tensor, want: torch.Tensor) -> bool:
    """same_bits, or a zero of the same sign where `want` is subnormal (a conversion that flushes)."""
    sub = (want != 0) & (want.float().abs() < 2.0 ** -126)
    sign = torch.iinfo(torch.int32 if got.dtype == torch.float32 else torch.int16).min
    flushed = sub & (bits(got) == (bits(want) & sign))
    return bool(((bits(got) == bits(want)) | (got.isnan() & want.isnan()) | flushed).all())


# ---- LayerNorm ---------------------------------------------------------------------------------------------------------------------
LN_C_CP = ((64, 64), (61, 64), (1, 64), (100, 128), (180, 192), (181, 192), (129, 192), (250, 256), (256, 256))
LN_ROWS = (1, 19, 67)
LN_ROWS_PER_GROUP = 16               # a 256-thread workgroup holds 16 rows, a wave 4
LN_FWD_GRID_CAP, LN_BWD_GRID_CAP = 4096, 1024


@dataclass(frozen=True)
class LnCase:
    C: int
    CP: int
    rows: int

    @property
    def id(self) -> str:
        return f"C{self.C}of{self.CP}-rows{self.rows}"


LN_FWD_CASES = [LnCase(C, CP, r) for C, CP in LN_C_CP for r in LN_ROWS] + [LnCase(61, 64, LN_FWD_GRID_CAP * LN_ROWS_PER_GROUP + 19)]
LN_BWD_CASES = [LnCase(C, CP, r) for C, CP in LN_C_CP for r in LN_ROWS] + [LnCase(61, 64, LN_BWD_GRID_CAP * LN_ROWS_PER_GROUP + 19)]
LN_GATHER = dict(H=16, W=24, B=2, C=60, CP=64, shifts=(0, 4))


def ln_coverage(cases: List[LnCase], grid_cap: int) -> Dict[str, object]:
    """What a case list instantiates: the NV template values, a ragged float4, a partial wave / workgroup, a second grid pass."""
    return dict(NV=sorted({c.CP // 64 for c in cases}), ragged_float4=any(c.C % 4 for c in cases),
                partial_wave=any(c.rows % 4 for c in cases), partial_group=any(c.rows % LN_ROWS_PER_GROUP for c in cases),
                grid_passes=max(-(-c.rows // (grid_cap * LN_ROWS_PER_GROUP)) for c in cases))


def ln_inputs(c: LnCase, seed_salt: int = 0) -> Dict[str, torch.Tensor]:
    """x fp32 [rows][CP] (pads 0) with a row scale that cycles through 3e-3 (variance ~ eps: the eps of the formula matters), 1.5 and
    2e-2 around a common offset 0.3; gamma / beta [C]; for the backward dy bf16 [rows][CP] (pads 0), old gx [rows][CP] (pads NON-zero:
    the accumulate contract of the pad columns) and old dgamma / dbeta, which grow with the row count so that they stay far above the
    any-order bound of a sum of `rows` terms."""
    g = torch.Generator().manual_seed(1000 * c.C + 10 * c.CP + c.rows % 1000 + seed_salt)
    scale = torch.tensor([3e-3, 1.5, 2e-2])[torch.arange(c.rows) % 3][:, None]
    x = torch.zeros(c.rows, c.CP)
    x[:, :c.C] = torch.randn(c.rows, c.C, generator=g) * scale + 0.3
    dy = torch.zeros(c.rows, c.CP)
    dy[:, :c.C] = torch.randn(c.rows, c.C, generator=g)
    big = max(1.0, c.rows / 16.0)
    sign = lambda n: (torch.randint(0, 2, (n,), generator=g) * 2 - 1).float()
    return dict(x=x, gamma=torch.rand(c.C, generator=g) + 0.5, beta=torch.randn(c.C, generator=g) * 0.1, dy=dy.to(torch.bfloat16),
                gx0=torch.randn(c.rows, c.CP, generator=g), dgamma0=sign(c.C) * (1 + torch.rand(c.C, generator=g)) * big,
                dbeta0=sign(c.C) * (1 + torch.rand(c.C, generator=g)) * big)


def ln_stats(x: torch.Tensor, C: int, divisor: Optional[int] = None, eps: float = LN_EPS):
    xc = x[:, :C].double()
    n = divisor or C
    mean = xc.sum(1) / n
    d = xc - mean[:, None]
    var = (d * d).sum(1) / n
    return mean, (var + eps).rsqrt(), d, var


def ln_fwd_ref(x, gamma, beta, C: int, mut: Optional[str] = None) -> Dict[str, Out]:
    """-> y [rows][CP] (pads 0), mean, rstd [rows].  mut: 'div_cp' (statistics divided by CP), 'no_eps', 'swap_stats'."""
    CP = x.shape[1]
    mean, rstd, d, var = ln_stats(x, C, CP if mut == "div_cp" else None, 0.0 if mut == "no_eps" else LN_EPS)
    y = torch.zeros(x.shape, dtype=torch.float64)
    y[:, :C] = d * rstd[:, None] * gamma.double() + beta.double()
    # bounds, from the exact statistics
    m0, r0, d0, v0 = ln_stats(x, C)
    xc = x[:, :C].double()
    t_mean = Tol.delta(C, xc.abs().sum(1)) / C + U * m0.abs()
    t_d = t_mean[:, None] + U * d0.abs()
    t_var = ((2 * d0.abs() * t_d + U * d0 * d0).sum(1) + Tol.delta(C, (d0 * d0).sum(1))) / C + 2 * U * (v0 + LN_EPS)
    t_rstd = 0.5 * r0 ** 3 * t_var + 4 * U * r0
    ga, ba = gamma.double().abs(), beta.double().abs()
    t_y = torch.zeros(x.shape, dtype=torch.float64)
    t_y[:, :C] = 32 * U * (ga * math.sqrt(C) + ba)[None] + ga[None] * (r0[:, None] * t_d + d0.abs() * t_rstd[:, None])
    if mut == "swap_stats":
        mean, rstd = rstd, mean
    return dict(y=Out(y, t_y), mean=Out(mean, t_mean), rstd=Out(rstd, t_rstd))


def ln_bwd_ref(dy, x, mean32, rstd32, gamma, C: int, accumulate: int, gx0, dgamma0, dbeta0, calls: int = 1,
               mut: Optional[str] = None) -> Dict[str, Out]:
    """gx [rows][CP], dgamma, dbeta [C] after `calls` calls.  mean32 / rstd32: the fp32 values the kernel is handed.
    mut: 'div_cp', 'no_xhat_term' (dx without xhat s2), 'dgamma_no_xhat', 'acc_ignores_old', 'dgamma_overwrite'."""
    CP = x.shape[1]
    xd, dyd, ga = x.double(), dy.double(), gamma.double()
    mean, rstd = mean32.double(), rstd32.double()
    if mut is None:
        dx, dg, db = G.ln_bwd(dyd, xd, mean, rstd, ga, C)
    else:
        n = CP if mut == "div_cp" else C
        xh = (xd[:, :C] - mean[:, None]) * rstd[:, None]
        g = dyd[:, :C] * ga
        s2 = 0.0 if mut == "no_xhat_term" else xh * ((g * xh).sum(1, keepdim=True) / n)
        dx = torch.zeros_like(dyd)
        dx[:, :C] = rstd[:, None] * (g - g.sum(1, keepdim=True) / n - s2)
        dg = (dyd[:, :C] * (1.0 if mut == "dgamma_no_xhat" else xh)).sum(0)
        db = dyd[:, :C].sum(0)
    old = gx0.double() if accumulate else torch.zeros_like(dx)
    gx = (torch.zeros_like(dx) if mut == "acc_ignores_old" else old) + (calls if accumulate else 1) * dx
    dgamma = (0.0 if mut == "dgamma_overwrite" else dgamma0.double()) + (1 if mut == "dgamma_overwrite" else calls) * dg
    dbeta = dbeta0.double() + calls * db
    xh = (xd[:, :C] - mean[:, None]) * rstd[:, None]
    rows = x.shape[0]
    t = torch.zeros_like(dx)
    t[:, :C] = (calls if accumulate else 1) * Tol.lnbwd(torch.zeros_like(xh), dyd[:, :C], xh, ga, rstd, old[:, :C])[0]
    t_dg = calls * Tol.delta(rows, (dyd[:, :C] * xh).abs().sum(0)) + calls * U * (dgamma0.double().abs() + dgamma.abs())
    t_db = calls * Tol.delta(rows, dyd[:, :C].abs().sum(0)) + calls * U * (dbeta0.double().abs() + dbeta.abs())
    return dict(gx=Out(gx, t), dgamma=Out(dgamma, t_dg), dbeta=Out(dbeta, t_db))


LN_FWD_MUTANTS = ("div_cp", "no_eps", "swap_stats")
LN_BWD_MUTANTS = ("div_cp", "no_xhat_term", "dgamma_no_xhat", "acc_ignores_old", "dgamma_overwrite")


def ln_identity(mut: str, c: LnCase) -> bool:
    """div_cp at C == CP is the reference; at C == 1 xhat is exactly 0 (x - mean = 0), so the xhat s2 term of dx is too."""
    return (mut == "div_cp" and c.C == c.CP) or (mut == "no_xhat_term" and c.C == 1)


# ---- special values and the element-wise helpers ------------------------------------------------------------------------------------
SPECIAL_BITS = (
    0x3F808000,   # 1 + 2^-8: half way between bf16 0x3F80 and 0x3F81 -> ties to even, DOWN to 0x3F80
    0x3F818000,   # half way between 0x3F81 and 0x3F82 -> ties to even, UP to 0x3F82
    0xBF808000, 0xBF818000,                                  # the same two, negative
    0x3F808001, 0x3F807FFF,                                  # just above / below a tie
    0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F8000,                      # FLT_MAX, -FLT_MAX, the tie below it: round up to bf16 infinity
    0x00000000, 0x80000000,                                  # +0, -0
    0x7F800000, 0xFF800000,                                  # +Inf, -Inf
    0x7FC00000, 0xFFC12345, 0x7F800001,                      # quiet NaN, NaN with sign and payload, a NaN whose upper half alone is Inf
    0x00000001, 0x807FFFFF, 0x00400000, 0x80000001,          # fp32 subnormals: smallest, largest (negative), middle
    0x00008000, 0x00018000, 0x00017FFF, 0x80008001,          # subnormal ties (down to 0, up to 0x0002) and their neighbours
)


def specials() -> torch.Tensor:
    return torch.tensor(np.array(SPECIAL_BITS, dtype=np.uint32).view(np.int32)).view(torch.float32)


ELEM_N = (4, 1028)
ELEM_PASS_8192 = 8192 * 256 * 4            # elements per grid pass of the launchers capped at 8192 workgroups (float4 per thread)
ELEM_PASS_16384 = 16384 * 256 * 4
ELEM_BIG = {"add_f32_bf16": ELEM_PASS_8192 + 1028, "add_bf16_into_f32": ELEM_PASS_8192 + 1028, "cast_f32_bf16": ELEM_PASS_8192 + 1028,
            "add_f32": ELEM_PASS_16384 + 1028}


def elem_inputs(n: int, seed: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
    """Two fp32 vectors: every ordered pair of special values first (as far as n allows; Inf - Inf, tie + subnormal, ... among them),
    then random values of mixed magnitude."""
    g = torch.Generator().manual_seed(seed + n)
    mag = 10.0 ** torch.randint(-3, 4, (n,), generator=g).float()
    a, b = torch.randn(n, generator=g) * mag, torch.randn(n, generator=g) * mag
    s = specials()
    k = len(s)
    pa, pb = s.repeat_interleave(k), s.repeat(k)
    if n >= 4 * k:                                  # every special value on its own (b = 0 keeps it) in front of the pairs
        pa, pb = torch.cat([s, pa]), torch.cat([torch.zeros(k), pb])
    m = min(n, len(pa))
    a[:m], b[:m] = pa[:m], pb[:m]
    return a, b


def elem_expected(name: str, a: torch.Tensor, b: torch.Tensor) -> Dict[str, torch.Tensor]:
    """The fp32 CPU expression itself (IEEE add, torch's round-to-nearest-even conversion).  b of add_bf16_into_f32 is b.to(bf16)."""
    if name == "add_f32_bf16":
        s = a + b
        return dict(a=s, ab=s.to(torch.bfloat16))
    if name == "add_bf16_into_f32":
        return dict(a=a + b.to(torch.bfloat16).float())
    if name == "add_f32":
        return dict(out=a + b)
    assert name == "cast_f32_bf16"
    return dict(y=a.to(torch.bfloat16))


# ---- rowscale ------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class RowscaleCase:
    CP: int
    rps: int
    rows: int

    @property
    def id(self) -> str:
        return f"CP{self.CP}-rps{self.rps}-rows{self.rows}"


ROWSCALE_GRID_CAP = 16384
# rows end in the middle of a sample (rps 1: every row is a sample); the last case needs more than one pass of the capped grid
ROWSCALE_CASES = [RowscaleCase(CP, rps, 3 * rps + max(1, rps // 2)) for CP in (64, 192) for rps in (1, 50, 64)] + \
                 [RowscaleCase(64, 50, ROWSCALE_GRID_CAP * 256 // 16 + 77)]


def rowscale_inputs(c: RowscaleCase):
    g = torch.Generator().manual_seed(c.CP + c.rps + c.rows % 997)
    src = torch.randn(c.rows, c.CP, generator=g).to(torch.bfloat16)
    ns = -(-c.rows // c.rps)
    vals = (1.0 / 0.9, 0.0, 1.0 / 0.8, 1.0, 1.0 / 0.95, 2.0)     # DropPath factors: an exact 0 (a dropped sample), 1 / keep, 1
    f = torch.tensor([vals[i % len(vals)] for i in range(ns)], dtype=torch.float32)
    return src, f


def rowscale_expected(src: torch.Tensor, f: torch.Tensor, rps: int, mut: Optional[str] = None) -> torch.Tensor:
    """mut 'mod_index': f[t % rps] instead of f[t / rps] (f read cyclically where the wrong index runs past its end)."""
    t = torch.arange(src.shape[0])
    idx = (t % rps) % len(f) if mut == "mod_index" else t // rps
    return (src.float() * f[idx][:, None]).to(torch.bfloat16)


# ---- img_prep ------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class ImgCase:
    Cimg: int
    H0: int
    W0: int
    H: int
    W: int
    B: int = 2

    @property
    def id(self) -> str:
        return f"c{self.Cimg}-{self.H0}x{self.W0}to{self.H}x{self.W}"


IMG_GRID_PASS = 8192 * 256                # pixels per pass of the launcher's capped grid
IMG_GEOMS = ((8, 8, 8, 8), (8, 12, 8, 16), (12, 8, 16, 8), (9, 9, 17, 16))      # none / one axis / the other / H at the largest legal pad H0 - 1
IMG_CASES = [ImgCase(c, *g) for c in (1, 2, 3) for g in IMG_GEOMS] + [ImgCase(3, 1024, 1024, 1024, 1040)]
IMG_MEAN = (0.4488, 0.4371, 0.4040)
IMG_RANGE = 255.0


def img_inputs(c: ImgCase) -> torch.Tensor:
    g = torch.Generator().manual_seed(c.Cimg * 7 + c.H + c.W)
    return torch.rand(c.B, c.Cimg, c.H0, c.W0, generator=g)


def img_prep_expected(x: torch.Tensor, H: int, W: int, mean=IMG_MEAN, rng: float = IMG_RANGE, mut: Optional[str] = None) -> torch.Tensor:
    """fp32 NHWC4: 'reflect' at the bottom / right by index arithmetic, one fp32 subtract, one fp32 multiply; channels >= Cimg are +0.
    mut: 'symmetric' (edge-repeating padding), 'mean0' (the mean of channel 0 for every channel)."""
    B, Cimg, H0, W0 = x.shape
    k = 1 if mut == "symmetric" else 2
    ys, xs = torch.arange(H), torch.arange(W)
    ys = torch.where(ys < H0, ys, 2 * H0 - k - ys)
    xs = torch.where(xs < W0, xs, 2 * W0 - k - xs)
    m = torch.tensor([mean[0 if mut == "mean0" else i] for i in range(Cimg)], dtype=torch.float32).view(1, Cimg, 1, 1)
    v = (x[:, :, ys][:, :, :, xs] - m) * torch.tensor(rng, dtype=torch.float32)
    out = torch.zeros(B, H, W, 4)
    out[..., :Cimg] = v.permute(0, 2, 3, 1)
    return out


def img_identity(mut: str, c: ImgCase) -> bool:
    return (mut == "symmetric" and c.H == c.H0 and c.W == c.W0) or (mut == "mean0" and c.Cimg == 1)


IMG_MUTANTS = ("symmetric", "mean0")


# ---- stem conv -----------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class StemCase:
    Cin: int
    C: int
    CP: int
    B: int
    H: int
    W: int

    @property
    def id(self) -> str:
        return f"cin{self.Cin}-C{self.C}of{self.CP}-{self.B}x{self.H}x{self.W}"


STEM_C_CP = ((60, 64), (96, 128), (180, 192), (181, 192), (250, 256))
STEM_BHW = ((1, 1, 1), (1, 5, 7), (2, 8, 8), (2, 3, 16))
STEM_CASES = [StemCase(cin, C, CP, *bhw) for cin in (1, 3) for C, CP in STEM_C_CP for bhw in STEM_BHW]


def stem_inputs(c: StemCase):
    """img4 fp32 [B][H][W][4]: channels < Cin random, channels Cin..2 finite junk the kernel must ignore (its weights there are 0),
    channel 3 zero as srk_img_prep leaves it; weight [C][Cin][3][3], bias [C]."""
    g = torch.Generator().manual_seed(c.Cin * 1000 + c.C + c.H * 31 + c.W)
    img = torch.randn(c.B, c.H, c.W, 4, generator=g)
    img[..., 3] = 0
    return img, torch.randn(c.C, c.Cin, 3, 3, generator=g) * 0.3, torch.randn(c.C, generator=g)


def stem_ref(img4, w, bias, CP: int, mut: Optional[str] = None) -> Out:
    """[B*H*W][CP] fp64 by a loop over the nine taps on the zero-padded image.  mut: 'transpose_taps' (ky <-> kx), 'no_bias'."""
    B, H, W, _ = img4.shape
    C, Cin = w.shape[:2]
    p = F.pad(img4[..., :Cin].double(), (0, 0, 1, 1, 1, 1))
    wd = w.double().transpose(2, 3) if mut == "transpose_taps" else w.double()
    ref, S = torch.zeros(B, H, W, C, dtype=torch.float64), torch.zeros(B, H, W, C, dtype=torch.float64)
    for ky in range(3):
        for kx in range(3):
            win = p[:, ky:ky + H, kx:kx + W]                    # [B][H][W][Cin]
            ref += win @ wd[:, :, ky, kx].t()
            S += win.abs() @ w.double()[:, :, ky, kx].abs().t()
    bd = bias.double()
    out = torch.zeros(B * H * W, CP, dtype=torch.float64)
    out[:, :C] = (ref + (0.0 if mut == "no_bias" else bd)).reshape(-1, C)
    tol = torch.zeros_like(out)
    exact = ref + bd
    tol[:, :C] = (Tol.delta(36, S) + U * (bd.abs() + exact.abs())).reshape(-1, C)
    return Out(out, tol)


def stem_identity(mut: str, c: StemCase) -> bool:
    return mut == "transpose_taps" and c.H == 1 and c.W == 1        # only the centre tap sees the image


STEM_MUTANTS = ("transpose_taps", "no_bias")


# ---- rectangular / padded window attention forward -----------------------------------------------------------------------------------
@dataclass(frozen=True)
class AttnCase:
    wh: int
    ww: int
    shift: bool
    H: int
    W: int
    B: int = 2
    nH: int = 2          # heads of one launch ...
    layout_heads: int = 4     # ... of a layout with this many
    dh: int = 12

    @property
    def id(self) -> str:
        return f"{self.wh}x{self.ww}-{'shift' if self.shift else 'noshift'}-{self.H}x{self.W}"

    @property
    def frame(self) -> Tuple[int, int]:
        big = max(self.wh, self.ww)
        return (self.H + big - 1) // big * big, (self.W + big - 1) // big * big

    @property
    def shifts(self) -> Tuple[int, int]:
        return (self.wh // 2, self.ww // 2) if self.shift else (0, 0)


# the cases of tests/test_gpu_dat.py::test_dat_rect_window_attention_backward_vs_autograd
ATTN_CASES = [AttnCase(8, 32, True, 32, 64), AttnCase(32, 8, False, 24, 40), AttnCase(8, 16, True, 24, 40), AttnCase(16, 8, True, 32, 32),
              AttnCase(16, 16, True, 32, 48)]


def attn_inputs(c: AttnCase, heads: Optional[int] = None):
    """qkv bf16 [T][3 * CA] with `heads` heads of the layout filled (head_dim zero-padded to 32), dense bias fp32 [heads][N][N]."""
    heads = heads or c.nH
    g = torch.Generator().manual_seed(c.wh * 100 + c.ww + c.H + heads)
    T, CA, N = c.B * c.H * c.W, c.layout_heads * 32, c.wh * c.ww
    qkv = torch.zeros(T, 3, c.layout_heads, 32)
    qkv[..., :heads, :c.dh] = torch.randn(T, 3, heads, c.dh, generator=g)
    return qkv.reshape(T, 3 * CA).to(torch.bfloat16), torch.randn(heads, N, N, generator=g) * 0.5


def attn_fwd_ref(qkv, bias, c: AttnCase, heads: Optional[int] = None, mut: Optional[str] = None) -> torch.Tensor:
    """[B][H][W][heads][dh] fp64: q / k / v zero-padded to the frame, partitioned with DO.rect_window_token_index, DO.rect_shift_mask and
    the dense bias added, softmax over ALL N keys of a window (padded ones score = bias), scattered back, cropped to H x W.
    mut: 'real_keys_only' (padded tokens left out of the softmax), 'no_mask', 'shift_sign' (the cyclic shift with the wrong sign)."""
    heads = heads or c.nH
    B, H, W, dh = c.B, c.H, c.W, c.dh
    Hp, Wp = c.frame
    sy, sx = c.shifts
    N, scale = c.wh * c.ww, dh ** -0.5
    x = qkv.double().view(B, H, W, 3, c.layout_heads, 32)[..., :heads, :dh]
    xp = F.pad(x, (0, 0, 0, 0, 0, 0, 0, Wp - W, 0, Hp - H)).reshape(B, Hp * Wp, 3, heads, dh)
    if mut == "shift_sign":
        idx = torch.from_numpy(DO.rect_window_token_index(Hp, Wp, c.wh, c.ww, (Hp - sy) % Hp, (Wp - sx) % Wp))
    else:
        idx = torch.from_numpy(DO.rect_window_token_index(Hp, Wp, c.wh, c.ww, sy, sx))
    nW = idx.shape[0]
    win = xp[:, idx.reshape(-1)].reshape(B * nW, N, 3, heads, dh).permute(2, 0, 3, 1, 4)
    attn = (win[0] * scale) @ win[1].transpose(-2, -1) + bias.double()[None]
    if c.shift and mut != "no_mask":
        mask = torch.from_numpy(DO.rect_shift_mask(Hp, Wp, c.wh, c.ww, sy, sx)).double()
        attn = (attn.reshape(B, nW, heads, N, N) + mask[None, :, None]).reshape(-1, heads, N, N)
    if mut == "real_keys_only":
        real = ((idx // Wp < H) & (idx % Wp < W)).reshape(1, nW, 1, 1, N)
        attn = attn.reshape(B, nW, heads, N, N).masked_fill(~real, float("-inf")).reshape(-1, heads, N, N)
        attn = torch.where(torch.isinf(attn).all(-1, keepdim=True), torch.zeros_like(attn), attn)     # windows made of padding only
    o = (attn.softmax(-1) @ win[2]).transpose(1, 2).reshape(B, nW * N, heads, dh)
    return torch.zeros(B, Hp * Wp, heads, dh, dtype=torch.float64).index_copy(1, idx.reshape(-1), o).reshape(B, Hp, Wp, heads, dh)[:, :H, :W]


def attn_identity(mut: str, c: AttnCase) -> bool:
    if mut == "real_keys_only":
        return c.frame == (c.H, c.W)
    return not c.shift


ATTN_MUTANTS = ("real_keys_only", "no_mask", "shift_sign")


def attn_accepts(got: torch.Tensor, ref: torch.Tensor) -> Tuple[bool, float]:
    tol = ATTN_TOL * float(ref.abs().max())
    err = float((got.double() - ref).abs().max())
    return err <= tol, err / tol


def attn_uniform_case() -> AttnCase:
    """The padded-token rule in isolation: 8 x 16 windows on a 24 x 40 map (frame 32 x 48), no shift."""
    return AttnCase(8, 16, False, 24, 40)


def attn_uniform_inputs(c: AttnCase):
    """q = 0, bias = 0, v small integers: every score is 0, every weight exactly 1 / N, so an output is (sum of the window's v) / N with the
    padded tokens counted in N -- an integer times 2^-7, exact in fp32.  -> (qkv, bias, expected bf16 [B][H][W][nH][dh])."""
    g = torch.Generator().manual_seed(5)
    T, CA, N = c.B * c.H * c.W, c.layout_heads * 32, c.wh * c.ww
    qkv = torch.zeros(T, 3, c.layout_heads, 32)
    qkv[:, 1, :c.nH, :c.dh] = torch.randn(T, c.nH, c.dh, generator=g)              # k is irrelevant under q = 0: any value
    v = torch.randint(-4, 5, (T, c.nH, c.dh), generator=g).float()
    qkv[:, 2, :c.nH, :c.dh] = v
    Hp, Wp = c.frame
    vp = F.pad(v.view(c.B, c.H, c.W, c.nH, c.dh), (0, 0, 0, 0, 0, Wp - c.W, 0, Hp - c.H))
    sums = vp.view(c.B, Hp // c.wh, c.wh, Wp // c.ww, c.ww, c.nH, c.dh).sum((2, 4), keepdim=True).expand(-1, -1, c.wh, -1, c.ww, -1, -1)
    want = (sums.reshape(c.B, Hp, Wp, c.nH, c.dh)[:, :c.H, :c.W] / N).to(torch.bfloat16)
    return qkv.reshape(T, 3 * CA).to(torch.bfloat16), torch.zeros(c.nH, N, N), want


# ---- channel gate with GELU, spatial gate ---------------------------------------------------------------------------------------------
GATE_SHAPE = dict(B=3, HW=700, C=180, CP=192, S=6, out_scale=0.01)


def channel_gate_inputs():
    """The inputs of tests/test_gpu_hat.py::test_channel_gate_and_cab_add_ln_vs_torch."""
    B, HW, C, CP, S = (GATE_SHAPE[k] for k in ("B", "HW", "C", "CP", "S"))
    g = torch.Generator().manual_seed(1)
    conv = torch.zeros(B * HW, CP)
    conv[:, :C] = torch.randn(B * HW, C, generator=g)
    return conv.to(torch.bfloat16), torch.randn(S, C, generator=g) * 0.3, torch.randn(S, generator=g), torch.randn(C, S, generator=g), \
        torch.randn(C, generator=g)


def channel_gate_ref(conv, w1, b1, w2, b2, act: int) -> torch.Tensor:
    """[B][CP] fp64: out_scale * sigmoid(W2 act(W1 mean + b1) + b2), mean over the HW tokens; pad columns 0.  act 0 ReLU, 1 exact-erf GELU."""
    B, HW, C, CP = (GATE_SHAPE[k] for k in ("B", "HW", "C", "CP"))
    mean = conv.double().reshape(B, HW, CP)[:, :, :C].mean(1)
    z = mean @ w1.double().t() + b1.double()
    z = G.gelu(z) if act == 1 else torch.relu(z)
    out = torch.zeros(B, CP, dtype=torch.float64)
    out[:, :C] = GATE_SHAPE["out_scale"] * torch.sigmoid(z @ w2.double().t() + b2.double())
    return out


def spatial_gate_inputs():
    """The spatial-gate inputs of tests/test_gpu_dat.py::test_dwconv_rowln_gates_vs_torch: its generator replayed through the draws that
    come before them.  -> (a bf16 [T][CP], W0 [S][CP], b0 [S], w3 [S], b3, T, CP, S)."""
    g = torch.Generator().manual_seed(0)
    B, H, W, C = 2, 11, 21, 40
    torch.randn(B, H, W, 64, generator=g); torch.randn(C, 9, generator=g); torch.rand(C, generator=g); torch.randn(C, generator=g)
    torch.randn(B * H * W, 48, generator=g)
    torch.randn(300, 768, generator=g); torch.rand(360, generator=g); torch.randn(360, generator=g)
    T, CP, S = 4 * 50, 192, 11
    a = torch.randn(T, CP, generator=g).to(torch.bfloat16)
    torch.randn(T, CP, generator=g)
    return a, torch.randn(S, CP, generator=g) * 0.1, torch.randn(S, generator=g), torch.randn(S, generator=g), 0.3, T, CP, S
