"""fp64 restatement of srk_gemm_ex (include/srk.h), its derived tolerances, and the case matrix of tests/test_gpu_gemm_ex.py.

Everything here is plain torch on the CPU.  The functions restate what the header comments of ``srk_gemm_args`` promise for each
(loader, epilogue) from the bf16-rounded operands; they are pinned against torch.nn.functional / torch.autograd in
tests/test_gemm_ex_ref.py, and the GPU tests compare the kernels with them.

Layout conventions (the device buffers hold exactly these, see ``make_inputs``):
  A        LD_ROWS bf16 [M][lda];  LD_CONV3 bf16 NHWC [B][H][Wd][CinP];  LD_CONV3_PS bf16 [B][H*r][Wd*r][Cs]
  W        bf16 [N][K], K = 9 * CinP tap-major for the conv loaders: k = ((dy + 1) * 3 + (dx + 1)) * CinP + ci
  outputs  row epilogues [M][ldo]; EP_PS NHWC [B][H*r][Wd*r][Cs]; image heads NCHW [B][Cimg][Hc][Wc]
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import torch

LD_ROWS, LD_CONV3, LD_CONV3_PS = 0, 1, 2
EP_BF16, EP_GELU, EP_RES, EP_DGELU, EP_LRELU, EP_PS, EP_IMG, EP_PS_IMG, EP_RES_BF16, EP_DLRELU, EP_F32_BF16, EP_LNBWD = (
    0, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13)
LOADERS = {LD_ROWS: "rows", LD_CONV3: "conv3", LD_CONV3_PS: "conv3ps"}
EPILOGUES = {EP_BF16: "bf16", EP_GELU: "gelu", EP_RES: "res", EP_DGELU: "dgelu", EP_LRELU: "lrelu", EP_PS: "ps", EP_IMG: "img",
             EP_PS_IMG: "psimg", EP_RES_BF16: "resbf16", EP_DLRELU: "dlrelu", EP_F32_BF16: "f32bf16", EP_LNBWD: "lnbwd"}
# the pairs srk_launch_gemm instantiates (the table of the coverage matrix); every other pair is SRK_E_UNSUPPORTED
SUPPORTED = {
    LD_ROWS: (EP_BF16, EP_GELU, EP_RES, EP_RES_BF16, EP_LRELU, EP_DGELU, EP_DLRELU, EP_LNBWD),
    LD_CONV3: (EP_BF16, EP_GELU, EP_DGELU, EP_RES, EP_RES_BF16, EP_LRELU, EP_DLRELU, EP_PS, EP_F32_BF16, EP_IMG, EP_PS_IMG),
    LD_CONV3_PS: (EP_BF16, EP_DLRELU),
}
INDEX_MAP_PAIRS = ((LD_ROWS, EP_BF16), (LD_CONV3, EP_BF16), (LD_CONV3, EP_PS), (LD_CONV3, EP_IMG), (LD_CONV3, EP_PS_IMG),
                   (LD_CONV3_PS, EP_BF16))

U = 2.0 ** -24            # unit roundoff of fp32
BF16_REL = 2.0 ** -8      # unit roundoff of bf16 (8 significant bits, round to nearest): one rounding of the stored value
BF16_TINY = 2.0 ** -133   # the smallest bf16 step, so that zeros compare
LN_EPS = 1e-5
GELU_LIP = 1.13           # max |gelu'| = 1.1290 (exact-erf GELU)


@dataclass(frozen=True)
class Case:
    loader: int
    ep: int
    M: int = 0
    N: int = 0
    K: int = 0
    lda: int = 0                                   # LD_ROWS (0 -> K)
    ldo: int = 0                                   # 0 -> N
    conv: Optional[Tuple[int, int, int, int]] = None   # (B, H, Wd, CinP): the LOGICAL conv input
    r: int = 0                                     # EP_PS / EP_PS_IMG / LD_CONV3_PS
    Cs: int = 0                                    # EP_PS / LD_CONV3_PS
    bias: bool = True
    outb: bool = True                              # request the optional bf16 output (GELU u, RES / F32_BF16 / LNBWD copy)
    xn_C: int = 0                                  # EP_RES: fused LayerNorm over xn_C columns (0: none)
    rps: int = 0                                   # rows_per_sample of a row scale (0: none)
    ln_C: int = 0                                  # EP_LNBWD
    Cimg: int = 0
    crop: Tuple[int, int] = (0, 0)                 # image heads: rows / columns cut off the full H*r x Wd*r image
    res4: bool = False                             # EP_PS_IMG denoising residual [M][4]
    scale: float = 0.2                             # LeakyReLU slope
    exact: bool = False                            # delta-weight / integer-input case (bit-exact gather)
    seed: int = 0

    @property
    def id(self) -> str:
        s = f"{LOADERS[self.loader]}-{EPILOGUES[self.ep]}-M{self.M}-N{self.N}-K{self.K}"
        if self.loader == LD_ROWS:
            s += f"-lda{self.lda or self.K}"
        else:
            s += "-c" + "x".join(str(v) for v in self.conv)
        if self.ldo and self.ldo != self.N:
            s += f"-ldo{self.ldo}"
        if self.r:
            s += f"-r{self.r}" + (f"s{self.Cs}" if self.Cs else "")
        if self.ep in (EP_IMG, EP_PS_IMG):
            s += f"-img{self.Cimg}c{self.crop[0]}x{self.crop[1]}" + ("-res" if self.res4 else "")
        if self.xn_C:
            s += f"-ln{self.xn_C}"
        if self.ln_C:
            s += f"-C{self.ln_C}"
        if self.rps:
            s += f"-rps{self.rps}"
        if not self.bias and self.ep not in (EP_DGELU, EP_DLRELU, EP_LNBWD, EP_F32_BF16):
            s += "-nobias"
        if not self.outb and self.ep in (EP_GELU, EP_RES, EP_F32_BF16, EP_LNBWD):
            s += "-noutb"
        return s + ("-exact" if self.exact else "")

    @property
    def LDO(self) -> int:
        return self.ldo or self.N

    @property
    def LDA(self) -> int:
        return self.lda or self.K

    @property
    def has_bias(self) -> bool:
        return self.bias and not self.exact and self.ep not in (EP_DGELU, EP_DLRELU, EP_LNBWD, EP_F32_BF16)

    @property
    def img_hw(self) -> Tuple[int, int]:
        B, H, Wd, _ = self.conv
        r = self.r if self.ep == EP_PS_IMG else 1
        return H * r - self.crop[0], Wd * r - self.crop[1]


def conv_case(loader, ep, B, H, Wd, CinP, N, **kw) -> Case:
    return Case(loader, ep, M=B * H * Wd, N=N, K=9 * CinP, conv=(B, H, Wd, CinP), **kw)


def stream_path(c: Case, n_cus: int, stream_on: bool) -> str:
    """Which implementation srk_launch_gemm picks (csrc/gemm.hip:409, csrc/gemm_stream.hip:1363), restated for the test log."""
    cus = n_cus & ~7
    if not stream_on or c.loader != LD_ROWS or cus < 8:
        return "tile"
    if c.N % 192 or c.M % 64 or c.LDA % 8 or c.N // 192 > cus // 8 or c.M < 64 * cus or c.M >= 1 << 24:
        return "tile"
    if c.rps and c.rps % 64:
        return "tile"
    if c.ep in (EP_BF16, EP_GELU, EP_DGELU):
        return "stream" if c.K in (192, 384) else "tile"
    if c.ep == EP_RES:
        return "stream" if c.N == 192 and c.K in (192, 384) else "tile"
    if c.ep == EP_LNBWD:
        return "stream" if c.N == 192 and c.K in (192, 384, 576) else "tile"
    return "tile"


# ---- inputs ------------------------------------------------------------------------------------------------------------------
IMG_INV_RANGE = 0.8
IMG_MEAN = (0.4488, 0.4371, 0.4040, 0.25)
EXACT_INV_RANGE = 0.5
EXACT_MEAN = (3.0, -2.0, 5.0, 1.0)


def _ints(shape, salt: int) -> torch.Tensor:
    """Small integers in [-120, 120], exactly representable in bf16, scrambled so that neighbours in every direction differ."""
    n = int(math.prod(shape))
    idx = torch.arange(n, dtype=torch.int64) + 7919 * salt
    v = ((idx * 2654435761) >> 7) % 241 - 120
    return v.reshape(shape).to(torch.float32)


def delta_table(n: int, CinP: int) -> Tuple[int, int]:
    """(tap, channel) of the single 1.0 in row n of a delta weight: asymmetric in n, covers all nine taps."""
    return (n * 5 + 3) % 9, (n * 37 + 11) % CinP


def sample_scale(ns: int) -> torch.Tensor:
    """Row-scale factors: distinct from one sample to the next (golden-ratio sequence in [0.25, 1.75]), one exact 0 as DropPath gives."""
    s = 0.25 + 1.5 * ((torch.arange(ns, dtype=torch.float64) * 0.6180339887498949) % 1.0)
    if ns >= 3:
        s[ns - 1] = 0.0
    return s.float()


def make_inputs(c: Case) -> Dict[str, torch.Tensor]:
    """Seeded operands in the device's own dtypes and layouts (bf16 / fp32 CPU tensors)."""
    g = torch.Generator().manual_seed(1234 + c.seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    bf = torch.bfloat16
    M, N, K, LDO = c.M, c.N, c.K, c.LDO
    inp: Dict[str, torch.Tensor] = {}
    if c.loader == LD_ROWS:
        A = (_ints((M, c.LDA), 1) if c.exact else rn(M, c.LDA))
        A[:, K:] = 1000.0                                   # beyond K: never read into the product
        inp["A"] = A.to(bf)
    else:
        B, H, Wd, CinP = c.conv
        if c.loader == LD_CONV3:
            shape = (B, H, Wd, CinP)
        else:
            assert CinP == c.r * c.r * c.Cs
            shape = (B, H * c.r, Wd * c.r, c.Cs)
        inp["A"] = (_ints(shape, 2) if c.exact else rn(*shape)).to(bf)
    if c.exact:
        W = torch.zeros(N, K)
        for n in range(N):
            if c.loader == LD_ROWS:
                W[n, (n * 37 + 11) % K] = 1.0
            else:
                tap, ch = delta_table(n, c.conv[3])
                W[n, tap * c.conv[3] + ch] = 1.0
    else:
        W = rn(N, K) * K ** -0.5
    Cpad = c.xn_C or c.ln_C
    if Cpad:
        W[Cpad:] = 0.0                                      # pad rows of W are zero (the ABI's padded-width convention)
    inp["W"] = W.to(bf)
    if c.has_bias:
        b = 0.5 * rn(N)
        b[b.abs() < 0.05] = 0.25                            # no accidental zero: a dropped bias shows in every column
        if Cpad:
            b[Cpad:] = 0.0
        inp["bias"] = b
    if c.ep in (EP_RES, EP_RES_BF16):
        res = rn(M, LDO)
        if Cpad:
            res[:, Cpad:] = 0.0
        inp["res"] = res
    if c.ep == EP_DGELU:
        aux = 1.5 * rn(M, LDO)
        pick = torch.rand(M, LDO, generator=g) < 0.03
        aux[pick] = (12.0 * torch.rand(M, LDO, generator=g) - 6.0)[pick]      # |u| up to 6
        inp["aux"] = aux.to(bf)
    if c.ep == EP_DLRELU:
        aux = rn(M, LDO)
        sel = torch.rand(M, LDO, generator=g)
        aux[sel < 0.05] = 0.0
        aux[(sel >= 0.05) & (sel < 0.10)] = -0.0            # the `> 0` edge, both signs of zero
        inp["aux"] = aux.to(bf)
    if c.rps:
        inp["rowscale"] = sample_scale((M + c.rps - 1) // c.rps)
    if c.xn_C:
        gam, bet = 1.0 + 0.5 * rn(N), 0.3 * rn(N)
        gam[c.xn_C:] = 0.0
        bet[c.xn_C:] = 0.0
        inp["xn_gamma"], inp["xn_beta"] = gam, bet
    if c.ep == EP_LNBWD:
        C = c.ln_C
        x = 1.5 * rn(M, N) + 0.3
        x[:, C:] = 0.0
        mean = x[:, :C].double().mean(1)
        var = ((x[:, :C].double() - mean[:, None]) ** 2).mean(1)
        gam = 1.0 + 0.5 * rn(N)
        gam[C:] = 0.0
        inp.update(ln_x=x, ln_mean=mean.float(), ln_rstd=(var + LN_EPS).rsqrt().float(), ln_gamma=gam,
                   outf0=rn(M, N), dgamma0=rn(N), dbeta0=rn(N))
    if c.ep == EP_PS_IMG and c.res4:
        inp["res"] = _ints((M, 4), 3) if c.exact else rn(M, 4)
    return inp


def img_params(c: Case) -> Tuple[float, Tuple[float, ...]]:
    return (EXACT_INV_RANGE, EXACT_MEAN) if c.exact else (IMG_INV_RANGE, IMG_MEAN)


# ---- loaders -----------------------------------------------------------------------------------------------------------------
def unshuffle_source(S: torch.Tensor, r: int) -> torch.Tensor:
    """LD_CONV3_PS: stored [B][H*r][Wd*r][Cs] -> the logical conv input [B][H][Wd][r*r*Cs], channel (i*r + j)*Cs + c (the order
    in which EP_PS stores its columns)."""
    B, Hr, Wr, Cs = S.shape
    H, Wd = Hr // r, Wr // r
    return S.reshape(B, H, r, Wd, r, Cs).permute(0, 1, 3, 2, 4, 5).reshape(B, H, Wd, r * r * Cs)


def im2col3(x: torch.Tensor, mirror_tap: Optional[int] = None) -> torch.Tensor:
    """NHWC [B][H][Wd][C] -> [B*H*Wd][9*C], 3x3 / stride 1 / zero pad 1, tap-major.  mirror_tap: a negative control (that tap reads
    dx -> -dx)."""
    B, H, Wd, C = x.shape
    xp = torch.zeros(B, H + 2, Wd + 2, C, dtype=x.dtype)
    xp[:, 1:H + 1, 1:Wd + 1] = x
    cols = []
    for tap in range(9):
        dy, dx = tap // 3 - 1, tap % 3 - 1
        if tap == mirror_tap:
            dx = -dx
        cols.append(xp[:, 1 + dy:1 + dy + H, 1 + dx:1 + dx + Wd])
    return torch.stack(cols, dim=3).reshape(B * H * Wd, 9 * C)


def a_matrix(c: Case, inp, mirror_tap=None, swap_ij=False) -> torch.Tensor:
    A = inp["A"].double()
    if c.loader == LD_ROWS:
        return A[:, :c.K]
    if c.loader == LD_CONV3_PS:
        if swap_ij:                                         # negative control: sub-pixel (i, j) read as (j, i)
            B, Hr, Wr, Cs = A.shape
            r = c.r
            A = A.reshape(B, Hr // r, r, Wr // r, r, Cs).permute(0, 1, 4, 3, 2, 5).reshape(B, Hr, Wr, Cs)
        A = unshuffle_source(A, c.r)
    return im2col3(A, mirror_tap)


# ---- epilogue pieces -----------------------------------------------------------------------------------------------------------
def gelu(u):
    return 0.5 * u * (1.0 + torch.erf(u / math.sqrt(2.0)))


def dgelu(u):
    return 0.5 * (1.0 + torch.erf(u / math.sqrt(2.0))) + u * torch.exp(-0.5 * u * u) / math.sqrt(2.0 * math.pi)


def ln_fwd(x: torch.Tensor, gamma, beta, C: int):
    """LayerNorm (eps 1e-5, biased variance) over the first C of N columns; pad columns of the output are 0."""
    xc = x[:, :C]
    mean = xc.mean(1)
    var = ((xc - mean[:, None]) ** 2).mean(1)
    rstd = (var + LN_EPS).rsqrt()
    out = torch.zeros_like(x)
    out[:, :C] = (xc - mean[:, None]) * rstd[:, None] * gamma[:C].double() + beta[:C].double()
    return out, mean, rstd


def ln_bwd(dy, x, mean, rstd, gamma, C: int):
    """Backward of ln_fwd through (x, mean, rstd, gamma): dx [M][N] (0 in the pad columns), dgamma [C], dbeta [C]."""
    xh = (x[:, :C] - mean[:, None]) * rstd[:, None]
    g = dy[:, :C] * gamma[:C]
    dx = torch.zeros_like(dy)
    dx[:, :C] = rstd[:, None] * (g - g.mean(1, keepdim=True) - xh * (g * xh).mean(1, keepdim=True))
    return dx, (dy[:, :C] * xh).sum(0), dy[:, :C].sum(0)


def ps_store(u: torch.Tensor, B, H, Wd, r, Cs, swap_ij=False) -> torch.Tensor:
    """EP_PS: column (i*r + j)*Cs + c of pixel (b, y, x) -> NHWC [B][H*r][Wd*r][Cs] at (y*r + i, x*r + j)."""
    t = u.reshape(B, H, Wd, r, r, Cs)
    if swap_ij:
        t = t.transpose(3, 4)
    return t.permute(0, 1, 3, 2, 4, 5).reshape(B, H * r, Wd * r, Cs)


def ps_img_store(u: torch.Tensor, B, H, Wd, r, Cimg, swap_ij=False) -> torch.Tensor:
    """EP_PS_IMG: column c*r*r + i*r + j of pixel (b, y, x) -> NCHW [B][Cimg][H*r][Wd*r] at (y*r + i, x*r + j)."""
    t = u[:, :Cimg * r * r].reshape(B, H, Wd, Cimg, r, r)
    if swap_ij:
        t = t.transpose(4, 5)
    return t.permute(0, 3, 1, 4, 2, 5).reshape(B, Cimg, H * r, Wd * r)


@dataclass
class Out:
    ref: torch.Tensor          # fp64, in the layout of the device buffer's data window
    tol: torch.Tensor          # fp64, same shape
    kind: str                  # "f32" | "bf16"

    def rounded(self) -> torch.Tensor:
        return round_as(self.ref, self.kind)


def round_as(t: torch.Tensor, kind: str) -> torch.Tensor:
    return t.to(torch.bfloat16 if kind == "bf16" else torch.float32).double()


class Tol:
    """Every tolerance of the srk_gemm_ex tests, derived from the number formats -- none is fitted to what the kernels give.

    u = 2^-24 is the unit roundoff of fp32, 2^-8 that of bf16.  The operands are exact bf16 values, so every product a_k w_k is exact
    in fp32 (8 x 8 significant bits); the only error of the accumulator v = sum_k a_k w_k is that of K - 1 fp32 additions in whatever
    order the MFMA and the K loop take.  For any order, |v - v_exact| <= (K - 1) u S + O(u^2) with S = sum_k |a_k w_k| (Higham, Accuracy
    and Stability of Numerical Algorithms, 4.2).  With a factor 2 of margin for the additions inside one MFMA,

        delta = 2 K u S,        S = sum_k |a_k w_k| + |bias| + |res|   (the absolute terms of the epilogue's sum; a row scale f
                                                                         multiplies the terms it scales, an image head's inv_range too)

      f32(ref, delta)           fp32 output: delta + 2u |ref| (the epilogue's own additions and the final rounding)
      bf16(ref, delta, L)       bf16 output: 2^-8 |ref| (its one rounding) + L delta + tiny; L is the Lipschitz constant of the
                                epilogue (1 for the linear ones, 1.13 for GELU, max(1, |slope|) for LeakyReLU and its gradient,
                                |inv_range| is already folded into an image head's S); tiny = the smallest bf16 step, so that zeros compare
      dgelu(ref, delta, v)      v gelu'(aux): aux is an exact bf16 input, so beyond bf16(ref, delta, 1.13) only the device's erf / exp
                                contribute: 8u |v|
      ln_fwd(...)               fused LayerNorm, checked against the fp64 LayerNorm of the DEVICE's own fp32 row (so rstd does not amplify
                                the GEMM's error into this bound): output 2^-8 |ref| + 32u (|gamma| sqrt(C) + |beta|) -- |xhat| <= sqrt(C),
                                a handful of fp32 operations per element; mean 8u max|row|; rstd 8u relative
      lnbwd(...)                dx = rstd (g dy - mean(g dy) - xhat mean(g dy xhat)), dy = v: delta propagated to first order,
                                rstd_m (|g_n| delta_mn + mean_n(|g| delta_m:) + |xhat_mn| mean_n(|g xhat| delta_m:)), plus 16u times the
                                sum of the absolute terms of the formula (|old| included); the bf16 copy: 2^-8 |ref| + |f| that + tiny;
                                dgamma / dbeta: sum_m delta |xhat| resp. sum_m delta, plus M u sum_m |dy xhat| resp. M u sum_m |dy| for
                                the M fp32 (atomic) additions in any order

    Measured on MI355X (max err / tol over all cases): bf16 outputs 0.996 -- the bound is the rounding itself; fp32 outputs 0.013 (the
    2 K u S term is a worst case, rounding errors add like a random walk); xn_rstd 0.33; dgamma 0.11.  No factor had to be replaced."""

    @staticmethod
    def delta(K, S):
        return 2.0 * K * U * S

    @staticmethod
    def f32(ref, delta):
        return delta + 2 * U * ref.abs()

    @staticmethod
    def bf16(ref, delta, lip=1.0):
        return BF16_REL * ref.abs() + lip * delta + BF16_TINY

    @staticmethod
    def dgelu(ref, delta, v):
        return Tol.bf16(ref, delta, GELU_LIP) + 8 * U * v.abs()

    @staticmethod
    def ln_fwd(xn, x, rstd, gamma, beta, C):
        t = BF16_REL * xn.abs() + 32 * U * (gamma.abs() * math.sqrt(C) + beta.abs())[None, :]
        t[:, :C] += BF16_TINY                                   # pad columns: exactly 0
        return t, (8 * U * x.abs().amax(1))[:, None], (8 * U * rstd)[:, None]

    @staticmethod
    def lnbwd(delta, dy, xh, gamma, rstd, old):
        """-> (tolerance of outf [M][C], of ln_dgamma [C], of ln_dbeta [C]); all arguments restricted to the C real columns."""
        M = dy.shape[0]
        ga, r_, ax = gamma.abs(), rstd[:, None], xh.abs()
        prop = r_ * (ga * delta + (ga * delta).mean(1, keepdim=True) + ax * (ga * ax * delta).mean(1, keepdim=True))
        ag = dy.abs() * ga
        absterms = old.abs() + r_ * (ag + ag.mean(1, keepdim=True) + ax * (ag * ax).mean(1, keepdim=True))
        return (prop + 16 * U * absterms, (delta * ax).sum(0) + M * U * (dy.abs() * ax).sum(0), delta.sum(0) + M * U * dy.abs().sum(0))

    @staticmethod
    def scaled_bf16(ref, f, t):
        """bf16(outf * f) where outf carries the tolerance t."""
        return BF16_REL * ref.abs() + f.abs() * t + BF16_TINY


tol_f32, tol_bf16 = Tol.f32, Tol.bf16


@dataclass
class Variant:
    """Negative controls: each flag makes `reference` compute a deliberately WRONG result."""
    no_bias: bool = False
    swap_ij: bool = False
    shift_rowscale: bool = False
    ln_over_N: bool = False
    crop_off_by_one: bool = False
    neg_slope: bool = False
    mirror_tap: Optional[int] = None


def gemm_core(c: Case, inp, v: Variant = Variant()):
    """v[m][n] = sum_k A W and S[m][n] = sum_k |A W| in fp64 from the bf16 operands."""
    A = a_matrix(c, inp, v.mirror_tap, v.swap_ij and c.loader == LD_CONV3_PS)
    W = inp["W"].double()
    return A @ W.t(), A.abs() @ W.abs().t()


def reference(c: Case, inp, core=None, v: Variant = Variant()) -> Dict[str, Out]:
    """All outputs of one srk_gemm_ex call with their derived tolerances (see `Tol`)."""
    acc, S = core if core is not None else gemm_core(c, inp, v)
    M, N, K = c.M, c.N, c.K
    bias = inp["bias"].double() if (c.has_bias and not v.no_bias) else torch.zeros(N, dtype=torch.float64)
    babs = inp["bias"].double().abs() if c.has_bias else torch.zeros(N, dtype=torch.float64)
    u = acc + bias
    Su = S + babs
    k2u = Tol.delta(K, 1.0)
    out: Dict[str, Out] = {}
    ep = c.ep
    slope = float(torch.tensor(c.scale, dtype=torch.float32))      # the ABI passes the slope as a float
    scale = -slope if v.neg_slope else slope
    f = None
    if c.rps:
        idx = torch.arange(M) // c.rps
        rs = inp["rowscale"].double()
        if v.shift_rowscale:
            idx = (idx + 1) % rs.numel()
        f = rs[idx][:, None]
    if ep == EP_BF16:
        out["outb"] = Out(u, tol_bf16(u, k2u * Su), "bf16")
    elif ep == EP_GELU:
        d = k2u * Su
        if c.outb:
            out["outb"] = Out(u, tol_bf16(u, d), "bf16")
        y = gelu(u)
        out["outb2"] = Out(y, tol_bf16(y, d, GELU_LIP), "bf16")
    elif ep in (EP_RES, EP_RES_BF16):
        res = inp["res"].double()[:, :N]
        fu = u if f is None else f * u
        y = res + fu
        d = k2u * ((Su if f is None else f.abs() * Su) + res.abs())
        if ep == EP_RES:
            out["outf"] = Out(y, tol_f32(y, d), "f32")
            if c.outb:
                out["outb"] = Out(y, tol_bf16(y, d), "bf16")
        else:
            out["outb"] = Out(y, tol_bf16(y, d), "bf16")
    elif ep == EP_LRELU:
        y = torch.where(u > 0, u, u * scale)
        out["outb"] = Out(y, tol_bf16(y, k2u * Su, max(1.0, abs(c.scale))), "bf16")
    elif ep == EP_DGELU:
        aux = inp["aux"].double()[:, :N]
        y = acc * dgelu(aux)
        out["outb"] = Out(y, Tol.dgelu(y, k2u * S, acc), "bf16")
    elif ep == EP_DLRELU:
        aux = inp["aux"].double()[:, :N]
        y = torch.where(aux > 0, acc, acc * scale)
        out["outb"] = Out(y, tol_bf16(y, k2u * S, max(1.0, abs(c.scale))), "bf16")
    elif ep == EP_PS:
        B, H, Wd, _ = c.conv
        y = ps_store(u, B, H, Wd, c.r, c.Cs, v.swap_ij).reshape(-1, c.Cs)
        out["outb"] = Out(y, tol_bf16(y, k2u * ps_store(Su, B, H, Wd, c.r, c.Cs).reshape(-1, c.Cs)), "bf16")
    elif ep in (EP_IMG, EP_PS_IMG):
        B, H, Wd, _ = c.conv
        inv, mean = img_params(c)
        r = c.r if ep == EP_PS_IMG else 1
        mean_t = torch.tensor(mean[:c.Cimg], dtype=torch.float32).double()[None, :, None, None]
        uu, SS = u, Su
        if c.res4:
            add = torch.zeros(M, N, dtype=torch.float64)
            add[:, :4] = inp["res"].double()                 # r == 1: column n is channel n
            uu, SS = u + add, Su + add.abs()
        full = ps_img_store(uu, B, H, Wd, r, c.Cimg, v.swap_ij) * float(torch.tensor(inv, dtype=torch.float32)) + mean_t
        Sfull = ps_img_store(SS, B, H, Wd, r, c.Cimg) * abs(inv) + mean_t.abs()
        Hc, Wc = c.img_hw
        o = 1 if v.crop_off_by_one else 0
        y = full[:, :, o:o + Hc, o:o + Wc]
        if y.shape[2:] != (Hc, Wc):
            raise ValueError("crop_off_by_one applies to cropped cases only")
        d = k2u * Sfull[:, :, :Hc, :Wc]
        out["outf"] = Out(y.reshape(-1, Wc), tol_f32(y, d).reshape(-1, Wc), "f32")
    elif ep == EP_F32_BF16:
        out["outf"] = Out(u, tol_f32(u, k2u * Su), "f32")
        if c.outb:
            out["outb"] = Out(u, tol_bf16(u, k2u * Su), "bf16")
    elif ep == EP_LNBWD:
        C = c.ln_C
        Cn = N if v.ln_over_N else C
        x, mean, rstd = inp["ln_x"].double(), inp["ln_mean"].double(), inp["ln_rstd"].double()
        gam = inp["ln_gamma"].double()
        old = inp["outf0"].double()
        dx, dg, db = ln_bwd(acc, x, mean, rstd, gam, Cn)
        if v.ln_over_N:
            dx[:, C:] = 0.0
            dg, db = dg[:C], db[:C]
        y = old + dx
        xh = ((x[:, :C] - mean[:, None]) * rstd[:, None])
        t_dx, t_dg, t_db = Tol.lnbwd((k2u * S)[:, :C], acc[:, :C], xh, gam[:C], rstd, old[:, :C])
        t = torch.zeros(M, N, dtype=torch.float64)              # pad columns: unchanged, bit for bit
        t[:, :C] = t_dx
        out["outf"] = Out(y, t, "f32")
        if c.outb:
            ff = f if f is not None else torch.ones(M, 1, dtype=torch.float64)
            out["outb"] = Out(y * ff, Tol.scaled_bf16(y * ff, ff, t), "bf16")
        out["ln_dgamma"] = Out((inp["dgamma0"].double()[:C] + dg)[None], t_dg[None], "f32")
        out["ln_dbeta"] = Out((inp["dbeta0"].double()[:C] + db)[None], t_db[None], "f32")
    else:
        raise ValueError(ep)
    return out


def ln_stage2(c: Case, inp, outf_dev: torch.Tensor) -> Dict[str, Out]:
    """Fused LayerNorm of EP_RES, second stage: the fp64 LayerNorm of the DEVICE's own fp32 `outf` rows, so that the GEMM's error is
    not amplified by rstd into this bound."""
    C = c.xn_C
    gam, bet = inp["xn_gamma"].double(), inp["xn_beta"].double()
    x = outf_dev.double()
    xn, mean, rstd = ln_fwd(x, gam, bet, C)
    t, t_mean, t_rstd = Tol.ln_fwd(xn, x, rstd, gam, bet, C)
    return {"xn_out": Out(xn, t, "bf16"), "xn_mean": Out(mean[:, None], t_mean, "f32"), "xn_rstd": Out(rstd[:, None], t_rstd, "f32")}


def ln_stage2_over_N(c: Case, inp, outf_dev: torch.Tensor) -> Dict[str, torch.Tensor]:
    """Negative control for ln_stage2: the statistics taken over all N columns instead of the first xn_C."""
    xn, mean, rstd = ln_fwd(outf_dev.double(), inp["xn_gamma"].double(), inp["xn_beta"].double(), c.N)     # gamma / beta pads are 0
    return {"xn_out": xn, "xn_mean": mean[:, None], "xn_rstd": rstd[:, None]}


def compare(got: torch.Tensor, out: Out) -> Tuple[bool, float]:
    """The comparator of every value check: (accepted, max(err / tol)); a non-finite `got` is never accepted.  Where tol == 0 the
    values must be equal."""
    got = got.double()
    if got.shape != out.ref.shape:
        return False, float("inf")
    if not torch.isfinite(got).all():
        return False, float("inf")
    err = (got - out.ref).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / out.tol.clamp_min(1e-300))
    mx = float(ratio.max()) if ratio.numel() else 0.0
    return mx <= 1.0, mx


# ---- exact (delta-weight) expectation: a gather written with slices, not through im2col / reshape-permute ----------------------------
def exact_expected(c: Case, inp) -> torch.Tensor:
    """What a delta-weight case must produce bit for bit: every output element is one input element (or 0 at the border), moved by
    the loader's tap / sub-pixel map and the epilogue's store map."""
    assert c.exact
    M, N = c.M, c.N
    A = inp["A"].double()
    if c.loader == LD_ROWS:
        u = torch.stack([A[:, (n * 37 + 11) % c.K] for n in range(N)], dim=1)
    else:
        B, H, Wd, CinP = c.conv
        if c.loader == LD_CONV3_PS:
            r, Cs = c.r, c.Cs
            x = torch.zeros(B, H, Wd, CinP, dtype=torch.float64)
            for i in range(r):
                for j in range(r):
                    x[..., (i * r + j) * Cs:(i * r + j + 1) * Cs] = A[:, i::r, j::r, :]
        else:
            x = A
        xp = torch.zeros(B, H + 2, Wd + 2, CinP, dtype=torch.float64)
        xp[:, 1:-1, 1:-1] = x
        u = torch.zeros(B, H, Wd, N, dtype=torch.float64)
        for n in range(N):
            tap, ch = delta_table(n, CinP)
            u[..., n] = xp[:, tap // 3:tap // 3 + H, tap % 3:tap % 3 + Wd, ch]
        u = u.reshape(M, N)
    if c.ep == EP_BF16:
        return u
    B, H, Wd, _ = c.conv
    if c.ep == EP_PS:
        r, Cs = c.r, c.Cs
        o = torch.zeros(B, H * r, Wd * r, Cs, dtype=torch.float64)
        u5 = u.reshape(B, H, Wd, N)
        for i in range(r):
            for j in range(r):
                o[:, i::r, j::r, :] = u5[..., (i * r + j) * Cs:(i * r + j + 1) * Cs]
        return o.reshape(-1, Cs)
    inv, mean = img_params(c)
    r = c.r if c.ep == EP_PS_IMG else 1
    o = torch.zeros(B, c.Cimg, H * r, Wd * r, dtype=torch.float64)
    u5 = u.reshape(B, H, Wd, N)
    for ch in range(c.Cimg):
        for i in range(r):
            for j in range(r):
                t = u5[..., ch * r * r + i * r + j]
                if c.res4:
                    t = t + inp["res"].double()[:, ch].reshape(B, H, Wd)
                o[:, ch, i::r, j::r] = t * inv + mean[ch]
    Hc, Wc = c.img_hw
    return o[:, :, :Hc, :Wc].reshape(-1, Wc)


# ---- the case matrix -------------------------------------------------------------------------------------------------------------
TILE_M = (1, 127, 128, 129, 351, 1000)
TILE_N = (64, 128, 192, 320, 384, 576)
TILE_K = (64, 192, 384, 576)
LN_NC = ((64, 60), (64, 64), (128, 96), (192, 180))
CONV_SHAPES = ((1, 1, 1), (1, 1, 7), (1, 8, 8), (3, 13, 9), (2, 5, 128), (2, 24, 40))
CONV_CIN = (64, 192)
CONV_N = (64, 192, 256)
PS_RC = ((2, 64), (3, 64), (4, 64), (2, 128))
STREAM_M = (16384, 16384 + 64 * 37, 32768)


def _rows_family(ep, off, **kw) -> List[Case]:
    """Six tile-path shapes per epilogue: every M once, N / K / lda / ldo rotated by `off` so that the families together cover the
    pairs of the axes."""
    out = []
    for i, M in enumerate(TILE_M):
        N = TILE_N[(i + off) % 6]
        K = TILE_K[(i + 3 * off + off // 2) % 4]
        out.append(Case(LD_ROWS, ep, M=M, N=N, K=K, lda=K + 64 * ((i + off) % 2), ldo=N + 64 * (((i // 2) + off) % 2), seed=i + 10 * off, **kw))
    return out


def _conv_family(ep, off, ldo_ok=True, **kw) -> List[Case]:
    out = []
    for i, (B, H, Wd) in enumerate(CONV_SHAPES):
        N = CONV_N[(i + off) % 3]
        CinP = CONV_CIN[(i // 3 + i + off) % 2]
        ldo = N + 64 * ((i + off) % 2) if ldo_ok else 0
        out.append(conv_case(LD_CONV3, ep, B, H, Wd, CinP, N, ldo=ldo, seed=100 + i + 10 * off, **kw))
    return out


def value_cases() -> List[Case]:
    cs: List[Case] = []
    # --- LD_ROWS, tile path
    cs += _rows_family(EP_BF16, 0)
    cs += _rows_family(EP_GELU, 1)
    cs += _rows_family(EP_GELU, 2, outb=False)
    cs += _rows_family(EP_RES, 3, outb=False)
    cs += _rows_family(EP_RES, 4)
    cs += _rows_family(EP_RES_BF16, 5)
    cs += _rows_family(EP_LRELU, 6)
    cs += _rows_family(EP_DGELU, 7)
    cs += _rows_family(EP_DLRELU, 8)
    cs += [Case(LD_ROWS, EP_BF16, M=129, N=192, K=192, bias=False, seed=9)]
    for i, (N, C) in enumerate(LN_NC):          # fused LayerNorm, plain and with a row scale (ldo == N is part of the contract)
        M1, M2 = TILE_M[i], TILE_M[5 - i]
        cs.append(Case(LD_ROWS, EP_RES, M=M1, N=N, K=TILE_K[i], lda=TILE_K[i] + 64 * (i % 2), xn_C=C, outb=bool(i % 2), seed=20 + i))
        cs.append(Case(LD_ROWS, EP_RES, M=M2, N=N, K=TILE_K[3 - i], xn_C=C, outb=not i % 2, seed=30 + i))
        cs.append(Case(LD_ROWS, EP_RES, M=TILE_M[(i + 2) % 6 if i != 2 else 5], N=N, K=TILE_K[(i + 1) % 4], xn_C=C, rps=(50, 64, 96, 100)[i],
                       outb=bool(i % 2), seed=40 + i))
    cs.append(Case(LD_ROWS, EP_RES, M=351, N=384, K=192, ldo=448, rps=100, seed=45))        # a row scale without the LayerNorm, N > 192
    for i, (N, C) in enumerate(LN_NC):          # LayerNorm backward: with / without outb x with / without a row scale
        cs.append(Case(LD_ROWS, EP_LNBWD, M=TILE_M[i + 1], N=N, K=TILE_K[i], ln_C=C, outb=bool(i & 1), rps=(0, 0, 40, 64)[i], seed=50 + i))
        cs.append(Case(LD_ROWS, EP_LNBWD, M=TILE_M[(i + 4) % 6], N=N, K=TILE_K[(i + 2) % 4], lda=TILE_K[(i + 2) % 4] + 64, ln_C=C,
                       outb=not i & 1, rps=(32, 50, 0, 0)[i], seed=60 + i))
    # --- LD_CONV3
    cs += _conv_family(EP_BF16, 0)
    cs += _conv_family(EP_GELU, 1)
    cs += _conv_family(EP_GELU, 2, outb=False)
    cs += _conv_family(EP_DGELU, 3)
    cs += _conv_family(EP_RES_BF16, 4)
    cs += _conv_family(EP_LRELU, 5)
    cs += _conv_family(EP_DLRELU, 6)
    cs += _conv_family(EP_F32_BF16, 7)
    cs += _conv_family(EP_F32_BF16, 8, outb=False)
    for i, (B, H, Wd) in enumerate(CONV_SHAPES):      # EP_RES: N = 256 plain (with ldo > N), N = 64 / 192 with the fused LayerNorm
        N = CONV_N[i % 3]
        C = {64: 60, 192: 180, 256: 0}[N]
        cs.append(conv_case(LD_CONV3, EP_RES, B, H, Wd, CONV_CIN[(i // 3 + i) % 2], N, ldo=0 if C else N + 64, xn_C=C, outb=bool(i % 2), seed=170 + i))
    cs.append(conv_case(LD_CONV3, EP_RES, 3, 13, 9, 64, 128, xn_C=96, seed=177))
    cs.append(conv_case(LD_CONV3, EP_RES, 2, 5, 128, 64, 64, xn_C=64, seed=178))
    for i, (B, H, Wd) in enumerate(CONV_SHAPES):
        r, Cs = PS_RC[i % 4]
        cs.append(conv_case(LD_CONV3, EP_PS, B, H, Wd, CONV_CIN[i % 2], r * r * Cs, r=r, Cs=Cs, seed=180 + i))
    for i, (B, H, Wd) in enumerate(CONV_SHAPES):
        crop = (3, 5) if (i % 2 and H > 3 and Wd > 5) else (0, 0)
        cs.append(conv_case(LD_CONV3, EP_IMG, B, H, Wd, CONV_CIN[i % 2], 16, Cimg=(1, 3)[i % 2], crop=crop, seed=190 + i))
    cs.append(conv_case(LD_CONV3, EP_IMG, 2, 24, 40, 64, 16, Cimg=1, crop=(3, 5), seed=196))
    cs.append(conv_case(LD_CONV3, EP_IMG, 2, 5, 128, 192, 16, Cimg=3, crop=(3, 5), seed=197))
    for i, (r, Cimg, res4) in enumerate(((1, 3, True), (2, 3, False), (3, 1, False), (4, 1, False))):
        for k, crop in enumerate(((0, 0), (3, 5))):
            B, H, Wd = CONV_SHAPES[2 + (i + 2 * k) % 4]
            cs.append(conv_case(LD_CONV3, EP_PS_IMG, B, H, Wd, CONV_CIN[(i + k) % 2], 16, r=r, Cimg=Cimg, res4=res4, crop=crop, seed=200 + 2 * i + k))
    cs.append(conv_case(LD_CONV3, EP_PS_IMG, 1, 1, 1, 64, 16, r=2, Cimg=3, seed=208))
    cs.append(conv_case(LD_CONV3, EP_PS_IMG, 1, 1, 7, 64, 16, r=4, Cimg=1, seed=209))
    # --- LD_CONV3_PS (dgrad of conv + PixelShuffle): B >= 2, the widths that move the tap rotation
    for i, ((r, Cs), Wd) in enumerate(zip(PS_RC, (9, 40, 128, 160))):
        for k, ep in enumerate((EP_BF16, EP_DLRELU)):
            N = CONV_N[(i + k) % 3]
            cs.append(conv_case(LD_CONV3_PS, ep, 2, (5, 4, 3, 2)[i] + k, Wd, r * r * Cs, N, r=r, Cs=Cs, ldo=N + 64 * ((i + k) % 2), seed=210 + 2 * i + k))
    cs.append(conv_case(LD_CONV3_PS, EP_BF16, 3, 7, 40, 256, 64, r=2, Cs=64, seed=219))
    return cs


def stream_cases() -> List[Case]:
    """Shapes the persistent streaming kernel covers on a 256-CU part (M >= 16384); each runs with gemm_stream on and off."""
    cs: List[Case] = []
    for k, ep in enumerate((EP_BF16, EP_GELU, EP_DGELU)):
        for i, M in enumerate(STREAM_M):
            N = (192, 384, 576)[(i + k) % 3]
            K = (192, 384, 576)[(i + 2 * k) % 3]
            cs.append(Case(LD_ROWS, ep, M=M, N=N, K=K, lda=K + 64 * (i % 2), ldo=N + 64 * ((i + k) % 2), seed=300 + 10 * k + i))
    cs.append(Case(LD_ROWS, EP_RES, M=16384, N=192, K=192, seed=330))
    cs.append(Case(LD_ROWS, EP_RES, M=16384 + 64 * 37, N=192, K=384, lda=448, xn_C=180, seed=331))
    cs.append(Case(LD_ROWS, EP_RES, M=32768, N=192, K=192, xn_C=180, rps=4096, outb=False, seed=332))
    cs.append(Case(LD_ROWS, EP_RES, M=16384, N=192, K=384, xn_C=180, rps=64, seed=333))
    cs.append(Case(LD_ROWS, EP_RES, M=16384 + 64 * 37, N=192, K=192, xn_C=180, rps=96, seed=334))     # rps % 64 != 0: tile kernel
    cs.append(Case(LD_ROWS, EP_LNBWD, M=16384, N=192, K=192, ln_C=180, seed=340))
    cs.append(Case(LD_ROWS, EP_LNBWD, M=16384 + 64 * 37, N=192, K=384, ln_C=180, rps=64, outb=False, seed=341))
    cs.append(Case(LD_ROWS, EP_LNBWD, M=32768, N=192, K=576, ln_C=180, rps=4096, seed=342))
    cs.append(Case(LD_ROWS, EP_LNBWD, M=16384, N=192, K=576, lda=640, ln_C=180, outb=False, seed=343))
    return cs


def exact_cases() -> List[Case]:
    cs = [Case(LD_ROWS, EP_BF16, M=129, N=192, K=192, lda=256, ldo=256, exact=True),
          Case(LD_ROWS, EP_BF16, M=1000, N=320, K=576, exact=True),
          conv_case(LD_CONV3, EP_BF16, 3, 13, 9, 64, 192, exact=True),
          conv_case(LD_CONV3, EP_BF16, 2, 5, 128, 192, 64, ldo=128, exact=True),
          conv_case(LD_CONV3, EP_BF16, 1, 1, 7, 64, 256, exact=True)]
    for i, (r, Cs) in enumerate(PS_RC):
        B, H, Wd = CONV_SHAPES[2 + i]
        cs.append(conv_case(LD_CONV3, EP_PS, B, H, Wd, CONV_CIN[i % 2], r * r * Cs, r=r, Cs=Cs, exact=True))
    cs += [conv_case(LD_CONV3, EP_IMG, 3, 13, 9, 64, 16, Cimg=3, crop=(3, 5), exact=True),
           conv_case(LD_CONV3, EP_IMG, 2, 24, 40, 192, 16, Cimg=1, exact=True)]
    for i, (r, Cimg, res4) in enumerate(((1, 3, True), (2, 3, False), (3, 1, False), (4, 1, False))):
        B, H, Wd = CONV_SHAPES[2 + i]
        cs.append(conv_case(LD_CONV3, EP_PS_IMG, B, H, Wd, 64, 16, r=r, Cimg=Cimg, res4=res4, crop=(3, 5) if i % 2 == 0 else (0, 0), exact=True))
    for (r, Cs), Wd in zip(PS_RC, (9, 40, 128, 160)):
        cs.append(conv_case(LD_CONV3_PS, EP_BF16, 2, 3, Wd, r * r * Cs, 192 if r == 2 else 64, r=r, Cs=Cs, exact=True))
    return cs


def unsupported_case(loader: int, ep: int) -> Case:
    """A small, otherwise valid argument block for a pair that srk_launch_gemm does not instantiate."""
    kw = {}
    N = 64
    if ep == EP_PS:
        kw.update(r=2, Cs=64)
        N = 256
    if ep in (EP_IMG, EP_PS_IMG):
        kw.update(Cimg=3)
        N = 16
        if ep == EP_PS_IMG:
            kw.update(r=2)
    if ep == EP_LNBWD:
        kw.update(ln_C=60)
    if loader == LD_CONV3_PS:
        kw.update(r=2, Cs=64)
        return conv_case(loader, ep, 2, 4, 8, 256, N, **kw)
    if loader == LD_CONV3:
        return conv_case(loader, ep, 2, 4, 8, 64, N, **kw)
    return Case(loader, ep, M=64, N=N, K=64, conv=(2, 4, 8, 64), **kw)


def controls_for(c: Case) -> Dict[str, Variant]:
    """The negative controls that apply to a value case."""
    out: Dict[str, Variant] = {}
    if c.has_bias:
        out["bias omitted"] = Variant(no_bias=True)
    if (c.ep in (EP_PS, EP_PS_IMG) or c.loader == LD_CONV3_PS) and c.r > 1:
        out["(i, j) swapped"] = Variant(swap_ij=True)
    if c.rps and c.M > c.rps and (c.ep != EP_LNBWD or c.outb):      # EP_LNBWD: the scale only enters outb
        out["rowscale shifted by one sample"] = Variant(shift_rowscale=True)
    if c.ep == EP_LNBWD and c.ln_C < c.N:
        out["LayerNorm over N columns"] = Variant(ln_over_N=True)
    if c.ep in (EP_IMG, EP_PS_IMG) and c.crop != (0, 0):
        out["crop off by one"] = Variant(crop_off_by_one=True)
    if c.ep in (EP_LRELU, EP_DLRELU):
        out["slope negated"] = Variant(neg_slope=True)
    if c.loader != LD_ROWS and c.conv[2] > 1:
        out["tap mirrored"] = Variant(mirror_tap=5)
    return out
