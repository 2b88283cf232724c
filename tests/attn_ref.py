"""fp64 restatement of window attention and of its gradient, the derived per-element bound and the case matrix of
tests/test_gpu_attn_direct.py.  Plain torch on the CPU; pinned in tests/test_attn_ref.py.

  entry point (include/srk.h)                 production kernel (csrc/)                      front-end
  srk_window_attention_fwd / _bwd             attn.hip  attn_fwd_kernel / attn_bwd_kernel    win8   (window-ordered, q pre-scaled)
  srk_window_attention_bwd_fused              attn_bwd_fused.hip  qkv_attn_bwd_kernel        win8 on `fused_project` (re-projected operands)
  srk_win_small_attention_fwd / _bwd          attn_small.hip / attn_small_bwd.hip            small  (raster, ws 2..7, table in closed form)
  srk_win256_attention_fwd / _bwd             attn256.hip / attn256_bwd.hip                  w256   (raster, 16 x 16, table 961 rows)
  srk_win256_attention_fwd / _bwd, overlap 8  the same                                       oca    (24 x 24 zero-padded keys, table 1521 rows)
  srk_win_attention_bwd_padded                attn_rect_bwd.hip                              rect   (wh x ww on an Hp x Wp frame, dense bias)

ONE core (`core`) per (window, head) on gathered fp64 operands:

  S = a q k^T + bias (+ mask),  P = softmax(S),  O = P v
  dV = P^T dO,  dP = dO v^T,  dS = P (dP - rowsum(P dP)),  dq = cq dS k,  dk = a dS^T q,  d bias += dS

with (a, cq) = (1, scale) where the buffer holds the pre-scaled q (win8: the gradient is the one of the UNSCALED q) and (scale, scale)
where it holds q itself.  The front-ends only build index maps: `qtok` / `ktok` [windows][N] / [windows][NK] give the raster token of
every window position (-1: a zero-padded position, gathered as a zero vector), `mask` the additive {0, -100} shift mask, `bias` the
dense [nH][N][NK] bias.  They are written from the model sources the kernel headers cite (network_swinir.py:216-279, hat_arch.py:
298-319 / :403-439 / :881-941, dat_arch.py:334-384): roll(-shift), window partition, the img_mask slices (0, -w), (-w, -s), (-s, None).
A padded QUERY has d_out = 0 by construction (its output row is dropped), so it contributes exactly nothing; a padded KEY takes part
with score = bias and has no destination for its dk / dv.  The small-window kernel's own padding to 32 / 64 keys is no part of the
operation: those keys do not exist here.

THE BOUND (`bound`), per element, none of it fitted to the device.  u = 2^-24; the operands are exact bf16 values, so every product of
an MFMA is exact in fp32 and an accumulation of K terms is off by at most 2 K u S (gemm_ex_ref.Tol), S the sum of the absolute terms.

  scores        ds_j = 2 * 32 u a sum_d |q k| + 2u (|bias_j| + 100)   BTol.attn's own (the 100 covers the mask addition and the
                exp2 argument s log2e - max log2e); + 2u a sum_d |q k| where the kernel multiplies the accumulator by the scale
  P             e_j = exp2(.) carries 8u (the project's convention for the device exponential).  To first order
                rho_j = |dP_j| / P_j <= (ds_j + 8u) + max_j (ds_j + 8u) + (NK + 4) u   -- numerator, denominator (any-order fp32 sum of
                NK positive terms), the reciprocal and the product
  dP            d dP = 2 * 32 u sum_d |dO v|
  dl            rowsum(P dP):  d dl = sum_j P (rho |dP| + d dP) + (NK + 2) u sum_j P |dP|
  dS            d dS = P (rho |dP - dl| + d dP + d dl + 3u (|dP| + |dl|))
  dq / dk / dv  one bf16 rounding of the output (2^-8 |ref|, gemm_ex_ref.BF16_REL) on top of
                  dq: cq (sum_j (2^-8 |dS| + d dS) |k| + 2 NK u sum_j |dS k|)         bf16 copy of dS as the MFMA operand
                  dk: a  (sum_i (2^-8 |dS| + d dS) |q| + 2 N u sum_i |dS q|)
                  dv:     sum_i (2^-8 + rho) P |dO| + 2 N u sum_i P |dO|              bf16 copy of P
                + 2u |ref| for the scale product + tiny.  In the overlapping form the per-window terms before the rounding ADD over
                the (up to four) key windows of a token (fp32 atomics, one more u per addition), then one bf16 rounding
  d table       an fp32 sum of UNROUNDED dS in any order: sum of d dS over the (window, i, j) that land on the entry + n u sum |dS|,
                n the number of such terms; accumulating onto a fill f adds n_atomic u (|f| + sum |dS|) -- see `table_grad`
  O (forward)   BTol.attn with the same ds
  operand uncertainties (dq_, dk_, dv_, ddo_; the fused kernel re-projects its operands, so an element within the projection's
                accumulation bound of a rounding boundary may come out one bf16 step away): first order into ds, d dP and the final sums
  pad channels  (head_dim .. 31) and every element the header says is zero: tolerance 0

The operand-copy term is the unit roundoff of bf16, 2^-8 (gemm_ex_ref.BF16_REL), not the 2^-9 the first derivation took: rounding to
nearest is off by up to half a step, and half a step is 2^-8 relative at the bottom of a binade (1 + 2^-8 rounds to 1).  The first GPU
run showed it: dq of win8-2x16x24-h3d32-w8x8-s4_4 at 1.18 of the 2^-9 bound, and exact arithmetic with nothing but the bf16 copy of dS and
the output rounding gives the same 1.18 at the same element (a row whose dS is carried by few keys, so the roundings do not average).
The kernel is right; the figure was not a bound.
"""
from __future__ import annotations

from dataclasses import dataclass, replace
from typing import Dict, List, Optional, Tuple

import torch

import block_ref as BR
from block_ref import BTol
from gemm_ex_ref import BF16_REL, BF16_TINY, U, Out

DP = 32
F32_TINY = 2.0 ** -126


# ---- negative controls -------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Variant:
    """Each flag makes the restatement compute a deliberately WRONG result."""
    shift_sign: bool = False          # roll(+shift)
    swap_hw: bool = False             # H and W exchanged in the row map
    no_mask: bool = False
    mask_first: bool = False          # mask on the first instead of the last window row / column
    half_labels: bool = False         # region labels from the half-window shift when the shift is another
    bias_transposed: bool = False     # bias / table read at (j, i)
    no_rowsum: bool = False           # dS = P dP
    dk_no_scale: bool = False         # dk without the scale (raster kernels) / with it (pre-scaled q)
    dq_scale_twice: bool = False
    pad_keys_in: bool = False         # small windows: the kernel's padding keys (to 32 / 64) take part with score 0
    pad_keys_out: bool = False        # overlapping / rectangular: zero-padded keys excluded from the softmax
    pad_queries_in: bool = False      # padded queries take d_out of token 0 of their sample
    one_key_window: bool = False      # overlapping form: dk / dv from the first key window of a token only
    oca_clamp: bool = False           # negative OCA index clamped to 0 instead of wrapped
    swap_whww: bool = False
    swap_sysx: bool = False
    drop_slice: bool = False          # d table: windows 32 .. 63 (the second reduce slice) dropped
    next_window: bool = False         # the walk: window b_ + 1's operands used for window b_


OK = Variant()


# ---- the core -----------------------------------------------------------------------------------------------------------------------------
def core(q, k, v, do, bias, a: float, cq: float, kvalid=None, var: Variant = OK) -> Dict[str, torch.Tensor]:
    """q, do [.., N, D]; k, v [.., NK, D]; bias [.., N, NK] (bias + mask, broadcastable); kvalid [.., 1, NK] bool or None (False: the
    key is excluded from the softmax).  All fp64.  -> P, O, dP, dl, dS, dq, dk, dv."""
    s = a * (q @ k.transpose(-1, -2)) + bias
    if kvalid is not None:
        s = s.masked_fill(~kvalid, float("-inf"))
    p = torch.softmax(s, -1)
    o = p @ v
    dp = do @ v.transpose(-1, -2)
    dl = (p * dp).sum(-1, keepdim=True)
    ds = p * dp if var.no_rowsum else p * (dp - dl)
    dq = (cq * cq if var.dq_scale_twice else cq) * (ds @ k)
    ak = (1.0 if a != 1.0 else cq) if var.dk_no_scale else a
    dk = ak * (ds.transpose(-1, -2) @ q)
    dv = p.transpose(-1, -2) @ do
    return dict(P=p, O=o, dP=dp, dl=dl, dS=ds, dq=dq, dk=dk, dv=dv)


def forward_only(q, k, v, bias, a: float, kvalid=None):
    s = a * (q @ k.transpose(-1, -2)) + bias
    if kvalid is not None:
        s = s.masked_fill(~kvalid, float("-inf"))
    p = torch.softmax(s, -1)
    return p, p @ v


def score_bound(q, k, bias_abs, a: float, unc=None):
    sabs = a * (q.abs() @ k.abs().transpose(-1, -2))
    ds = 2 * DP * U * sabs + 2 * U * (bias_abs + 100.0)
    if a != 1.0:
        ds = ds + 2 * U * sabs
    if unc is not None:
        ds = ds + a * (unc["q"] @ k.abs().transpose(-1, -2) + q.abs() @ unc["k"].transpose(-1, -2))
    return ds


def bound(q, k, v, do, bias_abs, c: Dict[str, torch.Tensor], a: float, cq: float, unc=None) -> Dict[str, torch.Tensor]:
    """The error bounds of one core evaluation `c` BEFORE the output roundings (see the module docstring): e_dq, e_dk, e_dv, d_dS, and
    the forward tolerance t_o.  bias_abs: |bias| without the mask."""
    P, dP, dl, dS = c["P"], c["dP"], c["dl"], c["dS"]
    N, NK = q.shape[-2], k.shape[-2]
    ds = score_bound(q, k, bias_abs, a, unc)
    r = ds + 8 * U
    rho = r + r.amax(-1, keepdim=True) + (NK + 4) * U
    ddP = 2 * DP * U * (do.abs() @ v.abs().transpose(-1, -2))
    if unc is not None:
        ddP = ddP + unc["do"] @ v.abs().transpose(-1, -2) + do.abs() @ unc["v"].transpose(-1, -2)
    ddl = (P * (rho * dP.abs() + ddP)).sum(-1, keepdim=True) + (NK + 2) * U * (P * dP.abs()).sum(-1, keepdim=True)
    ddS = P * (rho * (dP - dl).abs() + ddP + ddl + 3 * U * (dP.abs() + dl.abs()))
    w = BF16_REL * dS.abs() + ddS
    e_dq = cq * (w @ k.abs() + 2 * NK * U * (dS.abs() @ k.abs()))
    e_dk = a * (w.transpose(-1, -2) @ q.abs() + 2 * N * U * (dS.abs().transpose(-1, -2) @ q.abs()))
    e_dv = ((BF16_REL + rho) * P).transpose(-1, -2) @ do.abs() + 2 * N * U * (P.transpose(-1, -2) @ do.abs())
    if unc is not None:
        e_dq = e_dq + cq * (dS.abs() @ unc["k"])
        e_dk = e_dk + a * (dS.abs().transpose(-1, -2) @ unc["q"])
        e_dv = e_dv + P.transpose(-1, -2) @ unc["do"]
    A, As = P @ v.abs(), (P * ds) @ v.abs()
    t_o = BTol.attn(c["O"], A, As, ds.amax(-1, keepdim=True))
    return dict(e_dq=e_dq, e_dk=e_dk, e_dv=e_dv, d_dS=ddS, t_o=t_o)


def out_tol(ref, e, n_add: int = 0, sum_abs=None):
    """One bf16 rounding of an output whose value before the rounding is within e (+ n_add fp32 atomic additions of terms sum_abs)."""
    t = BF16_REL * ref.abs() + e + 2 * U * ref.abs() + BF16_TINY
    if n_add:
        t = t + n_add * U * sum_abs
    return t


# ---- cases ----------------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class ACase:
    kern: str                 # win8 | small | w256 | oca | rect
    B: int
    H: int
    W: int
    nH: int
    d: int
    wh: int = 8
    ww: int = 8
    sy: int = 0
    sx: int = 0
    Hp: int = 0               # rect: the frame (0: H, W)
    Wp: int = 0
    spare: int = 0            # heads' worth of extra column blocks in CA (small: a spare block; rect: the other branch's heads)
    ops: str = "rand"         # rand | peaked
    fwd: bool = False         # forward entry point only (win8: the forward's own wpw threshold)
    scratch: bool = True      # rect: per-window tiles + reduce (True) or float atomics (False)

    @property
    def frame(self) -> Tuple[int, int]:
        return (self.Hp or self.H, self.Wp or self.W)

    @property
    def N(self) -> int:
        return self.wh * self.ww

    @property
    def NK(self) -> int:
        return 576 if self.kern == "oca" else self.N

    @property
    def nW(self) -> int:
        Hp, Wp = self.frame
        return (Hp // self.wh) * (Wp // self.ww)

    @property
    def windows(self) -> int:
        return self.B * self.nW

    @property
    def T(self) -> int:
        return self.B * self.H * self.W

    @property
    def CA(self) -> int:
        return (self.nH + self.spare) * DP

    @property
    def scale(self) -> float:
        return float(torch.tensor(self.d ** -0.5, dtype=torch.float32))      # the ABI passes a float

    @property
    def table_rows(self) -> int:
        if self.kern == "oca":
            return 39 * 39
        if self.kern == "rect":
            return 0
        return (2 * self.wh - 1) ** 2

    @property
    def id(self) -> str:
        s = f"{self.kern}-{'fwd-' if self.fwd else ''}{self.B}x{self.H}x{self.W}-h{self.nH}d{self.d}-w{self.wh}x{self.ww}-s{self.sy}_{self.sx}"
        if self.Hp or self.Wp:
            s += f"-f{self.frame[0]}x{self.frame[1]}"
        if self.spare:
            s += f"-spare{self.spare}"
        if self.kern == "rect" and not self.scratch:
            s += "-atomics"
        return s + ("" if self.ops == "rand" else "-" + self.ops)


def win8_wpw(B_: int, nH: int, fwd: bool) -> int:
    """Windows per workgroup (csrc/attn.hip: srk_launch_attn_fwd / srk_attn_bwd_slabs; the slot count is a constant of the source, 8 resp.
    3 workgroups on each of 256 CUs, whatever the device)."""
    slots = (8 if fwd else 3) * 256
    wpw = max(1, -(-B_ * nH // slots))
    while -(-B_ // wpw) * nH > slots and wpw < B_:
        wpw += 1
    return wpw


def win8_cases() -> List[ACase]:
    c = [ACase("win8", 2, 16, 16, 2, 12), ACase("win8", 2, 16, 24, 3, 32, sy=4, sx=4),
         ACase("win8", 9, 24, 40, 6, 30), ACase("win8", 9, 24, 40, 6, 30, sy=4, sx=4), ACase("win8", 9, 24, 40, 6, 30, sy=4, sx=4, ops="peaked"),
         ACase("win8", 23, 24, 40, 6, 30, sy=4, sx=4, fwd=True), ACase("win8", 23, 24, 40, 6, 30, fwd=True)]
    assert win8_wpw(c[2].windows, 6, False) == 2 and c[2].windows % 2 == 1 and win8_wpw(c[1].windows, 3, False) == 1
    assert win8_wpw(c[5].windows, 6, True) == 2 and c[5].windows % 2 == 1
    return c


def small_cases() -> List[ACase]:
    """Every ws in 2..7 with shift 0, ws // 2 and one other legal shift (ws 2 has none; ws 7: 1 and 6); nH 1, 6, 9; 30 windows each (one
    reduce slice), ws 2 on 12 x 12 x 1: 36 windows (a second slice of 4); a spare column block; a peaked case."""
    cs: List[ACase] = []
    heads = {2: (6, 30), 3: (1, 24), 4: (2, 16), 5: (6, 30), 6: (1, 24), 7: (9, 20)}
    other = {3: (2,), 4: (1, 3), 5: (4,), 6: (1, 5), 7: (1, 6)}
    for ws in range(2, 8):
        nH, d = heads[ws]
        for s in (0, ws // 2) + other.get(ws, ()):
            cs.append(ACase("small", 2, 3 * ws, 5 * ws, nH, d, ws, ws, s, s))
    cs += [ACase("small", 1, 12, 12, 6, 30, 2, 2, 1, 1), ACase("small", 1, 12, 12, 2, 16, 2, 2, 0, 0),
           ACase("small", 2, 10, 15, 2, 16, 5, 5, 2, 2, spare=1), ACase("small", 2, 21, 14, 6, 30, 7, 7, 3, 3, ops="peaked"),
           ACase("small", 3, 21, 28, 2, 16, 7, 7, 6, 6)]       # 36 windows of 49 tokens
    return cs


def w256_cases() -> List[ACase]:
    k = dict(wh=16, ww=16)
    return [ACase("w256", 2, 32, 48, 3, 30, **k), ACase("w256", 2, 32, 48, 3, 30, sy=8, sx=8, **k), ACase("w256", 2, 32, 48, 3, 30, sy=5, sx=11, **k),
            ACase("w256", 3, 48, 64, 2, 30, sy=5, sx=11, **k),                   # 36 windows: a second reduce slice with a tail
            ACase("w256", 1, 16, 16, 3, 30, **k), ACase("w256", 1, 16, 16, 3, 30, sy=8, sx=8, **k),
            ACase("w256", 2, 32, 32, 3, 30, sy=8, sx=8, ops="peaked", **k),
            ACase("oca", 2, 32, 48, 3, 30, **k), ACase("oca", 1, 16, 16, 3, 30, **k), ACase("oca", 3, 48, 64, 2, 30, **k),
            ACase("oca", 1, 32, 32, 3, 30, ops="peaked", **k)]


def rect_cases() -> List[ACase]:
    """8 x 32, 32 x 8, 8 x 16, 16 x 8, 16 x 16; frames with partially and fully padded windows; shift off / half / neither half; 36 windows;
    both d-bias paths; a launch covering half the heads of a wider CA."""
    R = lambda *a, **k: ACase("rect", *a, **k)
    return [R(2, 32, 64, 2, 12, wh=8, ww=32, sy=4, sx=16, spare=2), R(2, 24, 40, 2, 12, wh=32, ww=8, Hp=32, Wp=40, spare=2),
            R(2, 24, 40, 2, 12, wh=8, ww=16, sy=4, sx=8, Hp=32, Wp=48), R(2, 32, 32, 2, 12, wh=16, ww=8, sy=8, sx=4, scratch=False),
            R(2, 32, 48, 2, 12, wh=16, ww=16, sy=8, sx=8), R(2, 12, 40, 2, 12, wh=8, ww=32, sy=3, sx=21, Hp=32, Wp=64),      # window row 2 fully padded after the roll
            R(2, 40, 48, 2, 12, wh=8, ww=16, Hp=48, Wp=48),                      # 36 windows, window row 5 fully padded
            R(2, 40, 48, 2, 12, wh=8, ww=16, sy=5, sx=3, Hp=48, Wp=48),           # 36 windows, the padding rolled into rows 4 and 5
            R(2, 40, 48, 2, 12, wh=8, ww=16, sy=5, sx=3, Hp=48, Wp=48, scratch=False),
            R(1, 24, 24, 2, 12, wh=16, ww=8, sy=11, sx=2, Hp=32, Wp=32, spare=2), R(2, 24, 40, 2, 12, wh=8, ww=16, sy=4, sx=8, Hp=32, Wp=48, ops="peaked")]


def all_cases() -> List[ACase]:
    return win8_cases() + small_cases() + w256_cases() + rect_cases()


def with_(c: ACase, **kw) -> ACase:
    return replace(c, **kw)


# ---- operands ---------------------------------------------------------------------------------------------------------------------------------
PEAK = {"win8": 2.0, "small": 8.0, "w256": 8.0, "oca": 8.0, "rect": 8.0}


def make_inputs(c: ACase) -> Dict[str, torch.Tensor]:
    """Seeded operands of a case in the device's dtypes, token (raster) order: q, k, v, do bf16 [T][nH][32] with zero pad channels, table
    fp32 [rows][nH] or (rect) bias fp32 [nH][N][N].  win8's q is the PRE-SCALED q.  peaked: q times a power-of-two factor."""
    g = torch.Generator().manual_seed(977 + 131 * c.B + 17 * c.H + 3 * c.W + 1009 * c.wh + 7 * c.ww + c.nH + 31 * c.d + len(c.kern))
    sd = 0.7 if c.kern == "win8" else 0.8

    def op(std):
        t = torch.zeros(c.T, c.nH, DP)
        t[..., :c.d] = torch.randn(c.T, c.nH, c.d, generator=g) * std
        return t.to(torch.bfloat16)
    q = op(sd)
    if c.ops == "peaked":
        q = (q.float() * PEAK[c.kern]).to(torch.bfloat16)
    inp = dict(q=q, k=op(sd), v=op(1.0), do=op(0.5))
    if c.kern == "rect":
        inp["bias"] = 0.5 * torch.randn(c.nH, c.N, c.N, generator=g)
    else:
        inp["table"] = 0.5 * torch.randn(c.table_rows, c.nH, generator=g)
    return inp


# ---- geometry, from the model sources -------------------------------------------------------------------------------------------------------------
def frame_tokens(c: ACase, var: Variant = OK) -> torch.Tensor:
    """[windows][N] raster token of every window position after zero-padding to the frame, roll(-sy, -sx) and the window partition
    (view(B, Hp / wh, wh, Wp / ww, ww).permute(0, 1, 3, 2, 4)); -1: a padded position."""
    H, W = c.H, c.W
    Hp, Wp = c.frame
    wh, ww, sy, sx = c.wh, c.ww, c.sy, c.sx
    if var.swap_whww:
        wh, ww = ww, wh
    if var.swap_sysx:
        sy, sx = sx, sy
    t = torch.full((c.B, Hp, Wp), -1, dtype=torch.int64)
    t[:, :H, :W] = torch.arange(c.T).view(c.B, H, W)
    if var.swap_hw:
        t = t.reshape(c.B, Wp, Hp)
        Hp, Wp = Wp, Hp
    sgn = 1 if var.shift_sign else -1
    t = torch.roll(t, shifts=(sgn * sy, sgn * sx), dims=(1, 2))
    return t.view(c.B, Hp // wh, wh, Wp // ww, ww).permute(0, 1, 3, 2, 4).reshape(-1, wh * ww)


def frame_mask(c: ACase, var: Variant = OK) -> Optional[torch.Tensor]:
    """[nW][N][N] fp64 in {0, -100}, or None without a shift: img_mask from the slices (0, -w), (-w, -s), (-s, None) per axis, window
    partition, mask[w][p][q] = -100 where the labels of p and q differ."""
    if (c.sy == 0 and c.sx == 0) or var.no_mask:
        return None
    Hp, Wp = c.frame
    wh, ww, sy, sx = c.wh, c.ww, c.sy, c.sx
    if var.swap_whww:
        wh, ww = ww, wh
    if var.swap_sysx:
        sy, sx = sx, sy
    if var.swap_hw:
        Hp, Wp = Wp, Hp
    if var.half_labels:
        sy, sx = wh // 2, ww // 2
    img = torch.zeros(Hp, Wp)
    cnt = 0
    for hs in (slice(0, -wh), slice(-wh, -sy), slice(-sy, None)):
        for ws_ in (slice(0, -ww), slice(-ww, -sx), slice(-sx, None)):
            img[hs, ws_] = cnt
            cnt += 1
    if var.mask_first:
        img = img.flip(0, 1)
    lab = img.view(Hp // wh, wh, Wp // ww, ww).permute(0, 2, 1, 3).reshape(-1, wh * ww)
    return torch.where(lab[:, None, :] != lab[:, :, None], -100.0, 0.0).double()


def table_index(c: ACase, var: Variant = OK) -> torch.Tensor:
    """[N][NK] row of the relative-position table.  Square windows: (y_i - y_j + ws - 1) (2 ws - 1) + (x_i - x_j + ws - 1)
    (network_swinir.py:89-103, hat_arch.py:881-894).  Overlapping form (hat_arch.py:896-918): (y_k - y_q + off) (ws + wse - 1) +
    (x_k - x_q + off) with off = ws - wse + 1 = -7; the model indexes the table with it as it is, so negative entries wrap."""
    ws = c.wh
    p = torch.arange(c.N)
    yi, xi = p // ws, p % ws
    if c.kern == "oca":
        kq = torch.arange(576)
        yk, xk = kq // 24, kq % 24
        off = ws - 24 + 1
        dy, dx = yk[None, :] - yi[:, None] + off, xk[None, :] - xi[:, None] + off
        idx = (dx * 39 + dy) if var.bias_transposed else (dy * 39 + dx)
        return idx.clamp_min(0) if var.oca_clamp else torch.where(idx < 0, idx + 39 * 39, idx)
    dy, dx = yi[:, None] - yi[None, :] + ws - 1, xi[:, None] - xi[None, :] + ws - 1
    return (dx * (2 * ws - 1) + dy) if var.bias_transposed else (dy * (2 * ws - 1) + dx)


def dense_bias(c: ACase, inp, var: Variant = OK) -> torch.Tensor:
    """[nH][N][NK] fp64."""
    if c.kern == "rect":
        b = inp["bias"].double()
        return b.transpose(-1, -2).contiguous() if var.bias_transposed else b
    if c.kern == "win8":
        return BR.dense_bias(inp["table"].double(), BR.Variant(bias_transposed=var.bias_transposed))
    idx = table_index(c, var)
    return inp["table"].double()[idx.reshape(-1)].reshape(c.N, c.NK, c.nH).permute(2, 0, 1).contiguous()


def oca_key_tokens(c: ACase) -> torch.Tensor:
    """[windows][576]: nn.Unfold(kernel 24, stride 16, padding 4) of the UNSHIFTED map (hat_arch.py:403-418); -1 in the zero padding."""
    t = torch.full((c.B, c.H + 8, c.W + 8), -1, dtype=torch.int64)
    t[:, 4:-4, 4:-4] = torch.arange(c.T).view(c.B, c.H, c.W)
    u = t.unfold(1, 24, 16).unfold(2, 24, 16)                 # [B][nWh][nWw][24][24]
    return u.reshape(-1, 576)


def geometry(c: ACase, var: Variant = OK):
    """-> qtok [windows][N], ktok [windows][NK], mask [nW][N][NK] or None."""
    if c.kern == "win8":
        bv = BR.Variant(shift_sign=var.shift_sign, swap_hw=var.swap_hw, no_mask=var.no_mask)
        qtok = BR.win_to_token(c.B, c.H, c.W, c.sy, bv).view(-1, 64)
        mask = None
        if c.sy and not var.no_mask:
            mask = BR.shift_mask(c.H, c.W, bv) if not var.mask_first else frame_mask(c, var)
        return qtok, qtok, mask
    qtok = frame_tokens(c, var)
    if c.kern == "oca":
        return qtok, oca_key_tokens(c), None
    return qtok, qtok, frame_mask(c, var)


# ---- reference of one call ------------------------------------------------------------------------------------------------------------------------
def _gather(x: torch.Tensor, tok: torch.Tensor) -> torch.Tensor:
    """x [T][nH][32], tok [Wn][n] (-1: zero vector) -> [Wn][nH][n][32] fp64."""
    z = torch.cat([x.double(), torch.zeros(1, *x.shape[1:], dtype=torch.float64)])
    return z[torch.where(tok < 0, x.shape[0], tok)].permute(0, 2, 1, 3)


def _scatter(t: torch.Tensor, tok: torch.Tensor, T: int, first_only: bool = False) -> torch.Tensor:
    """t [Wn][nH][n][32] -> [T][nH][32], summed over the positions that hold a token; padded positions have no destination."""
    flat = t.permute(0, 2, 1, 3).reshape(-1, t.shape[1], t.shape[3])
    idx = tok.reshape(-1)
    keep = idx >= 0
    if first_only:                                               # negative control: the first window that holds the token only
        seen = torch.zeros(T + 1, dtype=torch.bool)
        for n, i in enumerate(idx.tolist()):
            if i >= 0 and seen[i]:
                keep[n] = False
            seen[i] = True
    out = torch.zeros(T, t.shape[1], t.shape[3], dtype=torch.float64)
    return out.index_add_(0, idx[keep], flat[keep])


def small_pad_keys(N: int) -> int:
    return (32 if N <= 32 else 64) - N


@dataclass
class Ref:
    out: Dict[str, Out]           # o, dq, dk, dv [T][nH][32]; dtab [rows][nH] or dbias [nH][N][N] WITHOUT the fill
    maxP: float
    dS_abs_sum: torch.Tensor      # per table / bias entry: sum |dS| (the any-order summation term of a second evaluation)
    n_terms: torch.Tensor


def table_grad(c: ACase, dS_w: torch.Tensor, ddS_w: torch.Tensor, var: Variant = OK):
    """dS_w, ddS_w [windows][nH][N][NK] -> (d table or d bias, its tolerance without a fill, sum |dS| per entry, terms per entry)."""
    if var.drop_slice:
        dS_w = dS_w.clone()
        dS_w[32:64] = 0.0
    d, e, s = dS_w.sum(0), ddS_w.sum(0), dS_w.abs().sum(0)          # [nH][N][NK]
    n = torch.full_like(d, float(dS_w.shape[0]))
    if c.kern != "rect":
        idx = (BR.rel_pos_index() if c.kern == "win8" else table_index(c)).reshape(-1)
        fold = lambda t: torch.zeros(c.table_rows, c.nH, dtype=torch.float64).index_add_(0, idx, t.reshape(c.nH, -1).t())
        d, e, s, n = fold(d), fold(e), fold(s), fold(n)
    return d, e + n * U * s + F32_TINY, s, n


def fill_tol(tol, s, n_atomic, fill: float):
    """Accumulating onto a fill: every atomic addition rounds a value of at most |fill| + sum |dS|."""
    return tol + n_atomic * U * (abs(fill) + s)


def reference(c: ACase, inp, var: Variant = OK, unc=None, need_bwd: bool = True) -> Ref:
    """Every output of one backward call (and the forward's o) in TOKEN order with its tolerance."""
    qtok, ktok, mask = geometry(c, var)
    a, cq = (1.0, c.scale) if c.kern == "win8" else (c.scale, c.scale)
    do_src = inp["do"]
    q, do = _gather(inp["q"], qtok), _gather(do_src, qtok)
    if var.pad_queries_in:
        first = (torch.arange(qtok.shape[0]) // c.nW * c.H * c.W)[:, None].expand_as(qtok)
        do = _gather(do_src, torch.where(qtok < 0, first, qtok))
    k, v = _gather(inp["k"], ktok), _gather(inp["v"], ktok)
    if var.next_window:
        nxt = torch.arange(q.shape[0]).roll(-1)
        nxt[1::2] = torch.arange(q.shape[0])[1::2]               # the even windows of a pair read their successor
        q, k, v, do = q[nxt], k[nxt], v[nxt], do[nxt]
    bias = dense_bias(c, inp, var)
    bias_abs = dense_bias(c, inp).abs()[None]
    full = bias[None]
    if mask is not None:
        Wn = q.shape[0]
        full = (full.expand(Wn, -1, -1, -1).reshape(c.B, -1, c.nH, c.N, c.NK) + mask[None, :, None]).reshape(Wn, c.nH, c.N, c.NK)
    kvalid = None
    if var.pad_keys_out:
        kvalid = ((ktok >= 0) | (ktok < 0).all(1, keepdim=True))[:, None, None, :]      # a fully padded window stays as it is
    if var.pad_keys_in:
        npad = small_pad_keys(c.N)
        zk = torch.zeros(*k.shape[:2], npad, DP, dtype=torch.float64)
        k, v = torch.cat([k, zk], 2), torch.cat([v, zk], 2)
        full = torch.cat([full.expand(q.shape[0], -1, -1, -1), torch.zeros(q.shape[0], c.nH, c.N, npad, dtype=torch.float64)], 3)
        bias_abs = torch.cat([bias_abs, torch.zeros(1, c.nH, c.N, npad, dtype=torch.float64)], 3)
    cr = core(q, k, v, do, full, a, cq, kvalid, var)
    if var.pad_keys_in:
        for key in ("P", "dP", "dS"):
            cr[key] = cr[key][..., :c.NK]
        cr["dk"], cr["dv"] = cr["dk"][..., :c.NK, :], cr["dv"][..., :c.NK, :]
        k, v, bias_abs = k[..., :c.NK, :], v[..., :c.NK, :], bias_abs[..., :c.NK]
    uw = None
    if unc is not None:
        uw = dict(q=_gather(unc["q"], qtok), k=_gather(unc["k"], ktok), v=_gather(unc["v"], ktok), do=_gather(unc["do"], qtok))
    b = bound(q, k, v, do, bias_abs, cr, a, cq, uw)
    pad = lambda t: t.index_fill(-1, torch.arange(c.d, DP), 0.0)
    out: Dict[str, Out] = {}
    o_t = _scatter(b["t_o"], qtok, c.T)
    out["o"] = Out(_scatter(cr["O"], qtok, c.T), pad(o_t), "bf16")
    multi = c.kern == "oca"
    for name, tok in (("dq", qtok), ("dk", ktok), ("dv", ktok)):
        ref = _scatter(cr[name], tok, c.T, first_only=var.one_key_window and name != "dq")
        e = _scatter(b["e_" + name], tok, c.T)
        sa = _scatter(cr[name].abs(), tok, c.T) if multi and name != "dq" else None
        out[name] = Out(ref, pad(out_tol(ref, e, 4 if sa is not None else 0, sa)), "bf16")
    d, t, s, n = table_grad(c, cr["dS"], b["d_dS"], var)
    out["dbias" if c.kern == "rect" else "dtab"] = Out(d, t, "f32")
    return Ref(out, float(cr["P"].amax()), s, n)


# ---- which negative controls apply ----------------------------------------------------------------------------------------------------------------
def controls_for(c: ACase) -> Dict[str, Tuple[Variant, bool]]:
    """name -> (variant, applies): applies False means the mutant EQUALS the reference by construction at this case, which the CPU test
    asserts as an identity."""
    Hp, Wp = c.frame
    shifted = c.sy > 0 or c.sx > 0
    padded = c.kern == "rect" and (Hp > c.H or Wp > c.W)
    if padded:                                       # padding matters only in a window that also holds real tokens
        neg = frame_tokens(c) < 0
        padded = bool((neg.any(1) & ~neg.all(1)).any())
    raster = c.kern != "win8"
    out: Dict[str, Tuple[Variant, bool]] = {}
    if c.kern != "oca":
        # a roll by +s equals the roll by -s where 2 s is a multiple of the frame (and the mask is the same: it lives on the frame)
        out["roll(+shift)"] = (Variant(shift_sign=True), shifted and bool((2 * c.sy) % Hp or (2 * c.sx) % Wp))
        out["mask omitted"] = (Variant(no_mask=True), shifted)
        # the flipped label map gives the same partition where an axis has one window and its shift is the half window
        sym = Hp == c.wh and 2 * c.sy == c.wh and Wp == c.ww and 2 * c.sx == c.ww
        out["mask on the first window row / column"] = (Variant(mask_first=True), shifted and not sym)
        if raster:
            out["region labels of the half-window shift"] = (Variant(half_labels=True), shifted and (c.sy != c.wh // 2 or c.sx != c.ww // 2))
            out["sy / sx exchanged"] = (Variant(swap_sysx=True), c.sy != c.sx)
    if c.kern == "rect":
        if Hp % c.ww == 0 and Wp % c.wh == 0:
            out["wh / ww exchanged"] = (Variant(swap_whww=True), c.wh != c.ww)
        out["padded keys excluded"] = (Variant(pad_keys_out=True), padded)
        out["padded queries contribute"] = (Variant(pad_queries_in=True), padded)
    if c.kern in ("win8", "small", "w256") or c.kern == "rect" and (Hp, Wp) == (c.H, c.W) and not (c.H % c.ww or c.W % c.wh):
        out["H and W exchanged"] = (Variant(swap_hw=True), c.H != c.W)
    if c.kern == "small":
        out["padding keys in the softmax"] = (Variant(pad_keys_in=True), small_pad_keys(c.N) > 0)
    if c.kern == "oca":
        out["padded keys excluded"] = (Variant(pad_keys_out=True), True)
        out["dk / dv from one key window"] = (Variant(one_key_window=True), c.windows > 1)
        out["negative OCA index clamped"] = (Variant(oca_clamp=True), True)
    out["bias / table transposed"] = (Variant(bias_transposed=True), True)
    out["dS without the rowsum term"] = (Variant(no_rowsum=True), True)
    out["dk scale confused"] = (Variant(dk_no_scale=True), True)
    out["dq scaled twice"] = (Variant(dq_scale_twice=True), True)
    out["second 32-window slice of d table dropped"] = (Variant(drop_slice=True), c.windows > 32)
    out["next window's operands"] = (Variant(next_window=True), c.windows > 1)
    return out


# ---- exact expectations ---------------------------------------------------------------------------------------------------------------------------
def uniform_cases() -> List[ACase]:
    """Unshifted and half-window-shifted maps with power-of-two windows: every mask region is a power of two."""
    return [ACase("win8", 2, 16, 32, 2, 16), ACase("win8", 2, 16, 32, 2, 16, sy=4, sx=4), ACase("small", 2, 8, 12, 2, 16, 4, 4),
            ACase("small", 3, 6, 4, 1, 24, 2, 2), ACase("w256", 1, 32, 48, 2, 16, 16, 16), ACase("w256", 1, 32, 48, 2, 16, 16, 16, 8, 8),
            ACase("rect", 1, 32, 32, 2, 16, 8, 16), ACase("rect", 1, 32, 32, 2, 16, 8, 16, 4, 8),
            ACase("rect", 1, 32, 64, 2, 16, 32, 8, 16, 4, scratch=False)]


def uniform_inputs(c: ACase) -> Dict[str, torch.Tensor]:
    """q = 0 and table / bias = 0: P is uniform over the keys of the query's mask region.  d_out: integers times 2^k chosen so that every
    region mean over a power-of-two region is a bf16 number (multiples of 256 below 2^15: 7 significant bits after dividing by up to 256)."""
    g = torch.Generator().manual_seed(5 + c.T)
    z = torch.zeros(c.T, c.nH, DP)
    do = z.clone()
    do[..., :c.d] = torch.randint(-1, 2, (c.T, c.nH, c.d), generator=g).float() * 256.0
    v = z.clone()
    v[..., :c.d] = torch.randint(-3, 4, (c.T, c.nH, c.d), generator=g).float()
    inp = dict(q=z.to(torch.bfloat16), k=(v * 0.5).to(torch.bfloat16), v=v.to(torch.bfloat16), do=do.to(torch.bfloat16))
    if c.kern == "rect":
        inp["bias"] = torch.zeros(c.nH, c.N, c.N)
    else:
        inp["table"] = torch.zeros(c.table_rows, c.nH)
    return inp


def uniform_dv(c: ACase, inp) -> Tuple[torch.Tensor, torch.Tensor]:
    """-> (dv [T][nH][32] = the mean of d_out over the token's mask region, exact [T] bool: the region's size is a power of two and the
    token's window holds no padded position).  Written with an explicit loop over windows and regions, not through the core."""
    qtok, _, mask = geometry(c)
    do = inp["do"].double()
    dv = torch.zeros(c.T, c.nH, DP, dtype=torch.float64)
    exact = torch.zeros(c.T, dtype=torch.bool)
    for w in range(qtok.shape[0]):
        tok = qtok[w]
        same = torch.ones(c.N, c.N, dtype=torch.bool) if mask is None else mask[w % c.nW] == 0
        full = bool((tok >= 0).all())
        for p in range(c.N):
            if tok[p] < 0:
                continue
            grp = tok[same[p]]
            n = int(same[p].sum())
            dv[tok[p]] = do[grp[grp >= 0]].sum(0) / n
            exact[tok[p]] = full and (n & (n - 1)) == 0
    return dv, exact


# ---- the re-projecting 8 x 8 backward (csrc/attn_bwd_fused.hip) ---------------------------------------------------------------------------------
C180, CP192 = 180, 192


def fused_lists(B_: int, n_cus: int) -> Tuple[int, int]:
    """(fewest, most) windows a workgroup pair walks: cus / 2 window lists, list g holds windows g, g + cus / 2, ... (qkv_attn_bwd_kernel)."""
    lists = 8 * (n_cus // 16)
    return B_ // lists, -(-B_ // lists)


def fused_cases(n: int = 256) -> List[ACase]:
    """B_ == n (every list 2 windows on 256 CUs); a B_ with lists of 2 and of 3; B_ >= 3 n / 2 + 1 on a non-square map: every list walks
    at least 3 windows and some 4, the steady state of the two alternating row slots.  n = 256: (4, 64, 64) -> 256, (23, 24, 40) -> 345,
    (11, 48, 40) -> 330 (shift 0, lists of 2 and 3), (13, 40, 48) -> 390."""
    need3 = 3 * (8 * (n // 16)) + 1
    cs = [ACase("win8", -(-n // 64), 64, 64, 6, 30, sy=4, sx=4), ACase("win8", -(-(n * 345 // 256) // 15), 24, 40, 6, 30, sy=4, sx=4),
          ACase("win8", -(-(n * 330 // 256) // 30), 48, 40, 6, 30), ACase("win8", -(-need3 // 30), 40, 48, 6, 30, sy=4, sx=4),
          ACase("win8", -(-need3 // 30), 40, 48, 6, 30, ops="peaked")]
    assert all(c.windows >= n for c in cs) and fused_lists(cs[-1].windows, n)[0] >= 3 and fused_lists(cs[-2].windows, n)[0] >= 3
    return cs


def fused_inputs(c: ACase) -> Dict[str, torch.Tensor]:
    """xn, g bf16 [T][192] (token order; columns 180 .. 191 zero), w_qkv bf16 [576 (which, head, d)][192], b_qkv fp32 [576], w_proj_t bf16
    [192 attention channel][192 channel] (pads zero), table fp32 [225][6].  peaked: the q rows of w_qkv and b_qkv times 4."""
    g = torch.Generator().manual_seed(4242 + 7 * c.B + c.H + 3 * c.W)
    pad = lambda t: BR._heads(t)
    xn, gr = torch.zeros(c.T, CP192), torch.zeros(c.T, CP192)
    xn[:, :C180] = torch.randn(c.T, C180, generator=g)
    gr[:, :C180] = 0.5 * torch.randn(c.T, C180, generator=g)
    w = torch.zeros(576, CP192)
    w[:, :C180] = 0.08 * torch.randn(576, C180, generator=g)
    b = 0.2 * torch.randn(576, generator=g)
    if c.ops == "peaked":
        w[:192] *= 4.0
        b[:192] *= 4.0
    wpt = torch.zeros(192, CP192)
    wpt[:, :C180] = 0.08 * torch.randn(192, C180, generator=g)
    return dict(xn=xn.to(torch.bfloat16), g=gr.to(torch.bfloat16), wqkv=pad(w.t()).t().contiguous().to(torch.bfloat16), bqkv=pad(b[None])[0].contiguous(),
                wproj_t=pad(wpt.t()).t().contiguous().to(torch.bfloat16), table=0.5 * torch.randn(225, 6, generator=g))


def fused_project(c: ACase, f) -> Tuple[Dict[str, torch.Tensor], Dict[str, torch.Tensor]]:
    """The operands as the kernel forms them: q = bf16(fma(x W, scale, b scale)) (ONE fp32 rounding, then bf16), k, v = bf16(x W + b),
    dO = bf16(g Wproj_t^T), here the bf16 rounding of the fp64 value.  -> (inp of `reference`, unc): unc is the width of the bf16 interval
    the device's element may fall into, |bf16(y + delta) - bf16(y - delta)| with delta = 2 * 192 u S + 2u |y| the projection's accumulation
    bound: zero unless y lies within delta of a rounding boundary, one bf16 step where it does."""
    xn, gr = f["xn"].double(), f["g"].double()
    w, b, wp = f["wqkv"].double(), f["bqkv"].double(), f["wproj_t"].double()
    sc = torch.ones(576, dtype=torch.float64)
    sc[:192] = c.scale
    y = (xn @ w.t() + b) * sc
    dy = (2 * CP192 * U * (xn.abs() @ w.abs().t() + b.abs()) + 0.0) * sc + 2 * U * y.abs()
    o = gr @ wp.t()
    do_ = 2 * CP192 * U * (gr.abs() @ wp.abs().t()) + 2 * U * o.abs()
    bf = lambda t: t.to(torch.bfloat16)
    width = lambda t, d: (bf(t + d).double() - bf(t - d).double()).abs()
    yq, uq = bf(y).view(c.T, 3, c.nH, DP), width(y, dy).view(c.T, 3, c.nH, DP)
    inp = dict(q=yq[:, 0], k=yq[:, 1], v=yq[:, 2], do=bf(o).view(c.T, c.nH, DP), table=f["table"])
    unc = dict(q=uq[:, 0], k=uq[:, 1], v=uq[:, 2], do=width(o, do_).view(c.T, c.nH, DP))
    return inp, unc
