"""fp64 restatement of the weight-gradient entry points of include/srk.h, their derived tolerances, and the case matrix of
tests/test_gpu_wgrad.py.

Everything here is plain torch on the CPU.  `reference` restates what the header promises per entry point from the operands as the
device holds them (bf16 or fp32); it is pinned against torch.autograd in tests/test_wgrad_ref.py, and the GPU tests compare the kernels
with it.

  linear   srk_linear_wgrad_bf16 / srk_linear_wgrad_multi_bf16   dW[n][k] = dW0 + sum_m Y[m][n] X[m][k],  db[n] = db0 + sum_m Y[m][n]
  conv     srk_conv3x3_wgrad_bf16      the same with X shifted by the tap, zero outside the image; dW [N][9 * CinP] tap-major,
                                       k = ((dy + 1) * 3 + (dx + 1)) * CinP + ci
  convps   srk_conv3x3_wgrad_ps_bf16   Y stored shuffled [B][H * r][W * r][Cs], n = (i * r + j) * Cs + c
  imgprep  srk_img_grad_prep           gy [B * H * W][CoP] = d_pred * inv_range, un-shuffled (n = c * r * r + i * r + j), zero in the pad
                                       channels and outside the Hc x Wc crop
  smallw   srk_smallconv_wgrad         dw fp32 [Co][Cin][3][3], db [Co] from x bf16 [..][CinP] and gy fp32 [..][CoP]
  smalld   srk_smallconv_dgrad         dx bf16 [..][CinP] (pad channels zero) from gy and the fp32 weight [Co][Cin][3][3]
  stem     srk_stem_wgrad              dw [C][Cin][3][3], db [C] from the NHWC4 image and gy fp32 [B * H * W][CP]

Three input classes (the field `cls` of a Case):

  exact    small integers (|y| <= 2, |x| <= 3, dW0 / db0 non-zero integers): every partial sum in any order is an integer below 2^24, so
           the fp32 result is exact whatever the split, the wave shape, atomics or partials -- the assertion is torch.equal.  This class
           carries the detection: the worst-case fp32 bound of an M-term sum is 2 M u S (S = sum |y| |x|), about 2e-3 S at M = 16384,
           while one missing row changes the result by about S / M = 6e-5 S; a tolerance the correct kernel passes hides a missing row.
  dyadic   fp32-dY entry points only: values with 12 - 16 significant bits (not one bf16), the other operand powers of two: the lo
           halves of the kernels' hi + lo splits carry part of the answer.
  random   normal operands with a per-(row, column) ramp, non-zero dW0: realistic cancellation, derived tolerance.
"""
from __future__ import annotations

from dataclasses import dataclass, replace
from typing import Dict, List, Optional, Tuple

import torch

import gemm_ex_ref as G
from gemm_ex_ref import BF16_REL, BF16_TINY, U, Out, compare  # noqa: F401  (re-exported for the tests)

KINDS = ("linear", "conv", "convps", "imgprep", "smallw", "smalld", "stem")
ACCUMULATING = ("linear", "conv", "convps", "smallw", "stem")          # dW / db are += outputs
FP32_DY = ("smallw", "smalld", "stem")
EXACT_INV_RANGE, IMG_INV_RANGE = 0.5, 0.8


@dataclass(frozen=True)
class Prob:
    """One problem of a linear weight-gradient launch.  Y is the column slice [yoff, yoff + N) of a buffer of row stride ldy (0: N);
    problems with the same ybuf >= 0 read slices of ONE buffer (qkv-style).  X likewise (xoff, ldx)."""
    N: int
    K: int
    ldy: int = 0
    ldx: int = 0
    yoff: int = 0
    xoff: int = 0
    ybuf: int = -1
    db: bool = True

    @property
    def LDY(self) -> int:
        return self.ldy or self.N

    @property
    def LDX(self) -> int:
        return self.ldx or self.K


@dataclass(frozen=True)
class Case:
    kind: str
    cls: str                                           # exact | dyadic | random
    M: int = 0                                         # rows (linear) / pixels B * H * W
    probs: Tuple[Prob, ...] = ()                       # linear: 1 problem = srk_linear_wgrad_bf16 unless `multi`
    multi: bool = False                                # go through srk_linear_wgrad_multi_bf16
    geo: Optional[Tuple[int, int, int]] = None         # (B, H, W) of the conv input / the LR grid
    CinP: int = 0
    N: int = 0                                         # conv / convps output channels
    r: int = 1
    Cs: int = 0
    Cin: int = 0                                       # smallw / smalld / stem: real input channels
    Co: int = 0                                        # smallw / smalld: real output channels; stem: C
    CoP: int = 0                                       # smallw / smalld / imgprep: padded; stem: CP
    Cimg: int = 0
    crop: Tuple[int, int] = (0, 0)                     # imgprep: rows / columns cut off the H * r x W * r image
    db: bool = True                                    # conv / convps
    seed: int = 0

    @property
    def id(self) -> str:
        s = self.kind
        if self.kind == "linear":
            s += ("-multi" if self.multi else "") + f"-M{self.M}-" + "+".join(
                f"{p.N}x{p.K}" + (f"(ld{p.LDY},{p.LDX})" if (p.ldy or p.ldx) else "") + ("" if p.db else "nodb") for p in self.probs)
            if any(p.ybuf >= 0 for p in self.probs):
                s += "-shared"
        else:
            s += "-" + "x".join(str(v) for v in self.geo)
            if self.kind in ("conv", "convps"):
                s += f"-c{self.CinP}-n{self.N}" + (f"-r{self.r}s{self.Cs}" if self.kind == "convps" else "") + ("" if self.db else "-nodb")
            elif self.kind == "imgprep":
                s += f"-r{self.r}-img{self.Cimg}p{self.CoP}-crop{self.crop[0]}x{self.crop[1]}"
            elif self.kind == "stem":
                s += f"-in{self.Cin}-c{self.Co}p{self.CoP}"
            else:
                s += f"-in{self.Cin}p{self.CinP}-co{self.Co}p{self.CoP}"
        return f"{s}-{self.cls}"

    @property
    def shape_key(self):
        """Everything but the input class and the seed: an exact case with the same key is the `twin` of a random / dyadic one."""
        return replace(self, cls="", seed=0)

    @property
    def img_hw(self) -> Tuple[int, int]:
        return self.geo[1] * self.r - self.crop[0], self.geo[2] * self.r - self.crop[1]


def linear_case(cls, M, *nk, multi=False, seed=0) -> Case:
    probs = tuple(p if isinstance(p, Prob) else Prob(*p) for p in nk)
    return Case("linear", cls, M=M, probs=probs, multi=multi or len(probs) > 1, seed=seed)


def conv_case(cls, B, H, W, CinP, N, r=1, Cs=0, **kw) -> Case:
    return Case("convps" if r > 1 else "conv", cls, M=B * H * W, geo=(B, H, W), CinP=CinP, N=N, r=r, Cs=Cs, **kw)


def head_case(kind, cls, B, H, W, Cin, CinP, Co, CoP, **kw) -> Case:
    return Case(kind, cls, M=B * H * W, geo=(B, H, W), Cin=Cin, CinP=CinP, Co=Co, CoP=CoP, **kw)


def stem_case(cls, B, H, W, Cin, C, CP, **kw) -> Case:
    return Case("stem", cls, M=B * H * W, geo=(B, H, W), Cin=Cin, CinP=4, Co=C, CoP=CP, **kw)


def prep_case(B, H, W, r, Cimg, CoP, crop=(0, 0), cls="exact", **kw) -> Case:
    return Case("imgprep", cls, M=B * H * W, geo=(B, H, W), r=r, Cimg=Cimg, CoP=CoP, crop=crop, **kw)


# ---- inputs ------------------------------------------------------------------------------------------------------------------
def _hash(shape, salt: int) -> torch.Tensor:
    """An independent non-negative 40-bit integer per element (seeded by salt): no two rows or columns are related, so that a dropped,
    doubled or misplaced row cannot cancel against another one."""
    g = torch.Generator().manual_seed(977 + 7919 * salt)
    return torch.randint(0, 1 << 40, tuple(shape), generator=g, dtype=torch.int64)


def ints(shape, amax: int, salt: int, nonzero: bool = False) -> torch.Tensor:
    """Integers in [-amax, amax] (exact in bf16); nonzero: none of them 0."""
    if nonzero:
        v = _hash(shape, salt) % (2 * amax) - amax
        return torch.where(v >= 0, v + 1, v).float()
    return (_hash(shape, salt) % (2 * amax + 1) - amax).float()


def dyadic(shape, salt: int) -> torch.Tensor:
    """Positive fp32 values 2^e * (1 + a / 128 + t / 2^b): a 7-bit bf16 mantissa plus a tail t / 2^b in [3/8, 1/2) of the bf16 step,
    b = 11 .. 15 (12 - 16 significant bits).  The tail is below half a step, so bf16 rounding always drops it: the lo half of a hi + lo
    split is positive for every element and its omission cannot cancel in a sum."""
    h = _hash(shape, salt)
    a = (h % 128).double()
    b = 11 + (h >> 9) % 5                                  # bits below the binary point of the mantissa
    steps = (2 ** (b - 7)).double()                        # tail units per bf16 step
    t = torch.floor(steps * (0.375 + 0.124 * ((h >> 14) % 1000).double() / 1000.0))
    t = torch.where(t % 2 == 0, t + 1, t)                  # odd: all b fractional bits are used
    e = ((h >> 25) % 4 - 2).double()
    v = (2.0 ** e) * (1.0 + a / 128.0 + t / (2.0 ** b.double()))
    assert bool((v.float().double() == v).all())
    return v.float()


def pow2(shape, salt: int) -> torch.Tensor:
    return (2.0 ** ((_hash(shape, salt) % 4) - 2).double()).float()


def _ramp_x(g, M, K) -> torch.Tensor:
    return torch.randn(M, K, generator=g) + 0.01 * torch.arange(K).float()[None, :] * ((torch.arange(M) % 7).float()[:, None] - 3.0)


def _operands(c: Case, g, M, N, K, salt):
    """(Y [M][N], X [M][K]) of one GEMM-shaped problem in fp32 (bf16-representable for the bf16 operands)."""
    bf = torch.bfloat16
    if c.cls == "exact":
        return ints((M, N), 2, salt, nonzero=True), ints((M, K), 3, salt + 1)      # no y is 0: a dropped row always shows in db
    return (0.1 * torch.randn(M, N, generator=g)).to(bf).float(), _ramp_x(g, M, K).to(bf).float()


def _init(c: Case, g, shape, salt) -> torch.Tensor:
    """dW0 / db0: what the output holds before the call."""
    if c.cls == "exact":
        return ints(shape, 5, salt, nonzero=True)
    return torch.randn(*shape, generator=g)


def make_inputs(c: Case) -> Dict[str, torch.Tensor]:
    """Seeded LOGICAL operands in the device's dtypes (the GPU test embeds them in NaN-padded buffers with the case's strides)."""
    g = torch.Generator().manual_seed(4321 + c.seed)
    bf = torch.bfloat16
    inp: Dict[str, torch.Tensor] = {}
    M = c.M
    ymax, xmax, wmax = 2.0, 3.0, 5.0
    if c.kind == "linear":
        for i, p in enumerate(c.probs):
            y, x = _operands(c, g, M, p.N, p.K, 10 * i + c.seed)
            inp[f"y{i}"], inp[f"x{i}"] = y.to(bf), x.to(bf)
            inp[f"dw{i}_0"] = _init(c, g, (p.N, p.K), 10 * i + 2)
            if p.db:
                inp[f"db{i}_0"] = _init(c, g, (p.N,), 10 * i + 3)
    elif c.kind in ("conv", "convps"):
        B, H, W = c.geo
        y, x = _operands(c, g, M, c.N, c.CinP, c.seed)
        x = x.reshape(B, H, W, c.CinP)
        if c.kind == "convps":
            assert c.N == c.r * c.r * c.Cs
            y = G.ps_store(y, B, H, W, c.r, c.Cs)             # the device holds the SHUFFLED tensor [B][H*r][W*r][Cs]
        inp["y"], inp["x"] = y.to(bf), x.to(bf)
        inp["dw_0"] = _init(c, g, (c.N, 9 * c.CinP), 2)
        if c.db:
            inp["db_0"] = _init(c, g, (c.N,), 3)
    elif c.kind == "imgprep":
        B = c.geo[0]
        Hc, Wc = c.img_hw
        shape = (B, c.Cimg, Hc, Wc)
        inp["d_pred"] = ints(shape, 100, c.seed) if c.cls == "exact" else torch.randn(*shape, generator=g)
    elif c.kind in ("smallw", "smalld"):
        B, H, W = c.geo
        gy = torch.zeros(M, c.CoP)
        if c.cls == "exact":
            gy[:, :c.Co] = ints((M, c.Co), 2, c.seed, nonzero=True)
        elif c.cls == "dyadic":
            gy[:, :c.Co] = dyadic((M, c.Co), c.seed)
        else:
            gy[:, :c.Co] = 0.1 * torch.randn(M, c.Co, generator=g) * (1.0 + (torch.arange(M) % 5).float()[:, None])
        inp["gy"] = gy
        if c.kind == "smallw":
            if c.cls == "exact":
                x = ints((M, c.CinP), 3, c.seed + 1)
            elif c.cls == "dyadic":
                x = pow2((M, c.CinP), c.seed + 1)
            else:
                x = _ramp_x(g, M, c.CinP)
            inp["x"] = x.reshape(B, H, W, c.CinP).to(bf)       # pad channels >= Cin carry values: dw has no entry for them
            inp["dw_0"] = _init(c, g, (c.Co, c.Cin, 3, 3), 2)
            inp["db_0"] = _init(c, g, (c.Co,), 3)
        else:
            shape = (c.Co, c.Cin, 3, 3)
            if c.cls == "exact":
                w = ints(shape, 1, c.seed + 1)                  # 9 * Co * 2 <= 216: every dx is an integer that bf16 holds
                xmax = 1.0
                assert 9 * c.Co * 2 <= 256
            elif c.cls == "dyadic":
                w = dyadic(shape, c.seed + 1)
            else:
                w = 0.2 * torch.randn(*shape, generator=g)
            inp["weight"] = w
    elif c.kind == "stem":
        B, H, W = c.geo
        img = torch.zeros(M, 4)
        gy = torch.zeros(M, c.CoP)
        if c.cls == "exact":
            img[:, :c.Cin], gy[:, :c.Co] = ints((M, c.Cin), 3, c.seed + 1), ints((M, c.Co), 2, c.seed, nonzero=True)
        elif c.cls == "dyadic":
            img[:, :c.Cin], gy[:, :c.Co] = dyadic((M, c.Cin), c.seed + 1), dyadic((M, c.Co), c.seed)
        else:
            img[:, :c.Cin] = torch.randn(M, c.Cin, generator=g) + 0.1 * ((torch.arange(M) % 7).float()[:, None] - 3.0)
            gy[:, :c.Co] = 0.1 * torch.randn(M, c.Co, generator=g)
        inp["img4"], inp["gy"] = img.reshape(B, H, W, 4), gy
        inp["dw_0"] = _init(c, g, (c.Co, c.Cin, 3, 3), 2)
        inp["db_0"] = _init(c, g, (c.Co,), 3)
    else:
        raise ValueError(c.kind)
    if c.cls == "exact" and c.kind != "imgprep":
        # the precondition of the class: every partial sum in any order is an integer that fp32 holds
        terms = 9 * c.Co if c.kind == "smalld" else M
        assert terms * ymax * xmax + wmax < 2 ** 24
    return inp


def embed(t: torch.Tensor, ld: int, off: int, fill: float = float("nan"), before: int = 0, after: int = 0) -> torch.Tensor:
    """[rows][cols] -> a buffer [before + rows + after][ld] filled with `fill` that holds t in the columns [off, off + cols) of the rows
    [before, before + rows): the operand as a column slice of a wider buffer, with rows in front of and after it."""
    rows, cols = t.shape
    assert off + cols <= ld
    buf = torch.full((before + rows + after, ld), fill, dtype=t.dtype)
    buf[before:before + rows, off:off + cols] = t
    return buf


# ---- the restatement ---------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Mut:
    """Negative controls: each field makes `reference` compute a deliberately WRONG result (tests/test_wgrad_ref.py)."""
    drop_row: int = -1                # this row is left out of the sums
    drop_tail: bool = False           # the last M % 64 rows are left out
    double_row: int = -1              # this row is counted twice
    swap_taps: bool = False           # taps 1 (dy -1, dx 0) and 3 (dy 0, dx -1) change places
    swap_ij: bool = False             # sub-pixel (i, j) read as (j, i)
    overwrite: bool = False           # dW = increment, db = increment (no +=)
    db_from_tk1: bool = False         # the bias gradient is left to the workgroup of k-tile 1: with one k-tile nobody adds it
    no_lo: bool = False               # fp32 operands rounded to one bf16 (the lo half of the split is never added)
    no_crop: bool = False             # d_pred indexed as if it were the full H * r x W * r image


def _row_weights(M: int, m: Mut) -> torch.Tensor:
    w = torch.ones(M, dtype=torch.float64)
    if m.drop_row >= 0:
        w[m.drop_row] = 0.0
    if m.drop_tail:
        w[M - M % 64:] = 0.0
    if m.double_row >= 0:
        w[m.double_row] = 2.0
    return w


def _cols(x: torch.Tensor, m: Mut) -> torch.Tensor:
    """NHWC [B][H][W][C] -> [B*H*W][9*C], tap-major (gemm_ex_ref.im2col3: 3x3, stride 1, zero pad 1)."""
    cols = G.im2col3(x)
    if m.swap_taps:
        C = x.shape[-1]
        cols = cols.clone()
        t1, t3 = cols[:, C:2 * C].clone(), cols[:, 3 * C:4 * C].clone()
        cols[:, C:2 * C], cols[:, 3 * C:4 * C] = t3, t1
    return cols


def _hi(t: torch.Tensor, m: Mut) -> torch.Tensor:
    return t.to(torch.bfloat16).double() if m.no_lo else t.double()


def _dw_layout(t: torch.Tensor, Co: int, Cin: int, CinP: int) -> torch.Tensor:
    """[Co][9 * CinP] tap-major -> the state_dict layout [Co][Cin][3][3]."""
    return t.reshape(Co, 9, CinP)[:, :, :Cin].permute(0, 2, 1).reshape(Co, Cin, 3, 3)


def gemm_parts(c: Case, inp, m: Mut = Mut()):
    """The GEMM-shaped kinds as a list of (name suffix, Y [M][N] fp64, X [M][Kt] fp64, finish) -- dW increment = finish(Y^T X)."""
    if c.kind == "linear":
        return [(str(i), inp[f"y{i}"].double(), inp[f"x{i}"].double(), None) for i in range(len(c.probs))]
    B, H, W = c.geo
    if c.kind in ("conv", "convps"):
        y = inp["y"].double()
        if c.kind == "convps":
            if m.swap_ij:
                r = c.r
                y = y.reshape(B, H, r, W, r, c.Cs).permute(0, 1, 4, 3, 2, 5).reshape(B, H * r, W * r, c.Cs)
            y = G.unshuffle_source(y, c.r).reshape(c.M, c.N)
        return [("", y, _cols(inp["x"].double(), m), None)]
    if c.kind == "smallw":
        fin = lambda t: _dw_layout(t, c.Co, c.Cin, c.CinP)
        return [("", _hi(inp["gy"], m)[:, :c.Co], _cols(inp["x"].double(), m), fin)]
    if c.kind == "stem":
        fin = lambda t: _dw_layout(t, c.Co, c.Cin, 4)
        return [("", _hi(inp["gy"], m)[:, :c.Co], _cols(_hi(inp["img4"], m), m), fin)]
    raise ValueError(c.kind)


def _k_tiles(K: int) -> int:
    return K // (192 if K % 192 == 0 else (128 if K % 128 == 0 else 64))


def has_db(c: Case, i: int = 0) -> bool:
    return c.probs[i].db if c.kind == "linear" else (c.db if c.kind in ("conv", "convps") else c.kind in ("smallw", "stem"))


def prep_reference(c: Case, inp, m: Mut = Mut()) -> torch.Tensor:
    B, H, W = c.geo
    r, CoP = c.r, c.CoP
    Hc, Wc = c.img_hw
    inv = torch.tensor(EXACT_INV_RANGE if c.cls == "exact" else IMG_INV_RANGE, dtype=torch.float32)
    scaled = (inp["d_pred"] * inv).double()                                # the one fp32 multiplication of the kernel
    full = torch.zeros(B, c.Cimg, H * r, W * r, dtype=torch.float64)
    if m.no_crop:                                                          # the cropped buffer read with the full image's strides
        flat = torch.cat([scaled.reshape(B, -1), torch.zeros(B, full[0].numel() - scaled[0].numel(), dtype=torch.float64)], 1)
        full = flat.reshape(B, c.Cimg, H * r, W * r).clone()
    else:
        full[:, :, :Hc, :Wc] = scaled
    t = full.reshape(B, c.Cimg, H, r, W, r)                                # [b][c][y][i][x][j]
    t = t.transpose(3, 5) if m.swap_ij else t
    t = t.permute(0, 2, 4, 1, 3, 5).reshape(B, H, W, c.Cimg * r * r)       # n = c * r * r + i * r + j
    gy = torch.zeros(B, H, W, CoP, dtype=torch.float64)
    gy[..., :c.Cimg * r * r] = t
    return gy.reshape(c.M, CoP)


def dgrad_parts(c: Case, inp, m: Mut = Mut()):
    """smalld as a GEMM: dx[p][ci] = sum_{t, co} gy[p - off(t)][co] W[co][ci][t] = (cols of gy)[p][(8 - t) * CoP + co] Wm[..][ci]."""
    B, H, W = c.geo
    gcols = _cols(_hi(inp["gy"], m).reshape(B, H, W, c.CoP), Mut())
    w = _hi(inp["weight"], m)
    Wm = torch.zeros(9 * c.CoP, c.CinP, dtype=torch.float64)
    for t in range(9):
        ts = {1: 3, 3: 1}.get(t, t) if m.swap_taps else t
        Wm[(8 - t) * c.CoP:(8 - t) * c.CoP + c.Co, :c.Cin] = w[:, :, ts // 3, ts % 3]
    return gcols, Wm


def reference(c: Case, inp, m: Mut = Mut(), with_S: bool = False):
    """name -> fp64 expected value of every output (and, with_S, name -> S = the sum of the absolute terms, for `tolerance`)."""
    ref: Dict[str, torch.Tensor] = {}
    S: Dict[str, torch.Tensor] = {}
    if c.kind == "imgprep":
        ref["gy"] = prep_reference(c, inp, m)
        S["gy"] = torch.zeros_like(ref["gy"])
    elif c.kind == "smalld":
        gcols, Wm = dgrad_parts(c, inp, m)
        ref["dx"] = gcols @ Wm
        if with_S:
            S["dx"] = gcols.abs() @ Wm.abs()
    else:
        w = _row_weights(c.M, m)[:, None]
        for i, (sfx, Y, X, fin) in enumerate(gemm_parts(c, inp, m)):
            fin = fin or (lambda t: t)
            Yw = Y * w
            dw0 = inp[f"dw{sfx}_0"].double()
            ref[f"dw{sfx}"] = (0.0 if m.overwrite else dw0) + fin(Yw.t() @ X)
            if with_S:
                S[f"dw{sfx}"] = fin(Y.abs().t() @ X.abs())
            if has_db(c, i):
                db0 = inp[f"db{sfx}_0"].double()
                K = c.probs[i].K if c.kind == "linear" else c.CinP
                skip = m.db_from_tk1 and (c.kind not in ("linear", "conv", "convps") or _k_tiles(K) == 1)
                ref[f"db{sfx}"] = (0.0 if m.overwrite else db0) + (0.0 if skip else Yw.sum(0))
                if with_S:
                    S[f"db{sfx}"] = Y.abs().sum(0)
    return (ref, S) if with_S else ref


# The hi + lo paths.  A value v is split into hi = bf16(v) and lo = bf16(v - hi): |v - hi| <= BF16_REL |v| and the rounding of lo leaves
# |v - hi - lo| <= BF16_REL |v - hi| <= BF16_REL^2 |v|.  Per split operand one such term, plus one for the lo * lo product where both
# operands are split and the kernel leaves it out (|lo_a lo_b| <= BF16_REL^2 |a b|):
#   smallw  csrc/convwgrad.hip: `acc[q] = mfma(yfh, xf)` + `mfma(yfl, xf)` in smallconv_wgrad_mfma_kernel: dY split, x is bf16 -> the
#           rounding of lo(dY): c = 1
#   smalld  csrc/convwgrad.hip: `wh * xh + wl * xh + wh * xl` in imghead_dgrad_mfma_kernel: both split, lo * lo dropped -> c = 3
#   stem    csrc/misc.hip: `mfma(ah, bh) + mfma(ah, bl) + mfma(al, bh)` in stem_wgrad_mfma_kernel: both split, lo * lo dropped -> c = 3
# (the fp32 VALU kernels of the same entry points have none of these terms and stay inside the same bound)
HILO_TERMS = {"smallw": 1, "smalld": 3, "stem": 3}


def tolerance(c: Case, inp, refS=None) -> Dict[str, torch.Tensor]:
    """Derived bounds, per element.  fp32 accumulation of an L-term sum in any order: 2 L u S (gemm_ex_ref.Tol.delta with the reduction
    length L = M rows; per tap for a conv; 9 * Co for the dgrad), plus u (|dW0| + |ref|) for the final add into the accumulating
    output; the hi + lo entry points add HILO_TERMS * BF16_REL^2 * S; dx is rounded to bf16 once: + BF16_REL |ref| + BF16_TINY.
    The exact class and srk_img_grad_prep get 0: the comparator then demands equality."""
    ref, S = refS if refS is not None else reference(c, inp, with_S=True)
    if c.cls == "exact" or c.kind == "imgprep":
        return {k: torch.zeros_like(v) for k, v in ref.items()}
    tol = {}
    for k, v in ref.items():
        L = 9 * c.Co if c.kind == "smalld" else c.M
        t = G.Tol.delta(L, S[k]) + HILO_TERMS.get(c.kind, 0) * BF16_REL ** 2 * S[k]
        if c.kind == "smalld":
            t = t + BF16_REL * v.abs() + BF16_TINY
        else:
            t = t + U * (inp[k + "_0"].double().abs() + v.abs())
        tol[k] = t
    return tol


def expected(c: Case, inp) -> Dict[str, Out]:
    refS = reference(c, inp, with_S=True)
    tol = tolerance(c, inp, refS)
    return {k: Out(v, tol[k], "bf16" if k == "dx" else "f32") for k, v in refS[0].items()}


def accepts(c: Case, got: Dict[str, torch.Tensor], exp: Dict[str, Out]) -> Tuple[bool, Dict[str, float]]:
    """The comparator of every value check: exact class and imgprep -> torch.equal; otherwise max(err / tol) <= 1 (gemm_ex_ref.compare:
    a non-finite value is never accepted)."""
    ratios, ok = {}, True
    for k, o in exp.items():
        g = got[k].double()
        if c.cls == "exact" or c.kind == "imgprep":
            same = g.shape == o.ref.shape and torch.equal(g, o.ref)
            ratios[k] = 0.0 if same else float("inf")
        else:
            same, ratios[k] = compare(g, o)
        ok = ok and same
    return ok, ratios


# ---- fp32 emulation of the kernels' summation (CPU) ------------------------------------------------------------------------------
def _split(t: torch.Tensor):
    hi = t.to(torch.bfloat16).float()
    return hi, (t - hi).to(torch.bfloat16).float()


def emulate(c: Case, inp, m_per: int = 256) -> Dict[str, torch.Tensor]:
    """What a kernel of the family computes, in fp32 on the CPU: chunks of 64 rows accumulated per split of m_per rows, the splits'
    partials summed afterwards, the sum added to the old value; the fp32 operands as hi + lo with the products the kernels form."""
    f32 = torch.float32
    out: Dict[str, torch.Tensor] = {}
    if c.kind == "imgprep":
        return {"gy": prep_reference(c, inp).float()}
    if c.kind == "smalld":
        gcols, Wm = dgrad_parts(c, inp)
        (gh, gl), (wh, wl) = _split(gcols.float()), _split(Wm.float())
        return {"dx": ((gh @ wh + gl @ wh) + gh @ wl).to(torch.bfloat16)}
    for i, (sfx, Y, X, fin) in enumerate(gemm_parts(c, inp)):
        fin = fin or (lambda t: t)
        Y, X = Y.to(f32), X.to(f32)
        ys = _split(Y) if c.kind in FP32_DY else (Y, None)
        xs = _split(X) if c.kind == "stem" else (X, None)
        parts_w, parts_b = [], []
        for m0 in range(0, c.M, m_per):
            aw = torch.zeros(Y.shape[1], X.shape[1], dtype=f32)
            ab = torch.zeros(Y.shape[1], dtype=f32)
            for c0 in range(m0, min(c.M, m0 + m_per), 64):
                c1 = min(c.M, m0 + m_per, c0 + 64)
                aw += ys[0][c0:c1].t() @ xs[0][c0:c1]
                ab += ys[0][c0:c1].sum(0)
                if ys[1] is not None:
                    aw += ys[1][c0:c1].t() @ xs[0][c0:c1]
                    ab += ys[1][c0:c1].sum(0)
                if xs[1] is not None:
                    aw += ys[0][c0:c1].t() @ xs[1][c0:c1]
            parts_w.append(aw)
            parts_b.append(ab)
        sw, sb = parts_w[0].clone(), parts_b[0].clone()
        for aw, ab in zip(parts_w[1:], parts_b[1:]):
            sw += aw
            sb += ab
        out[f"dw{sfx}"] = inp[f"dw{sfx}_0"] + fin(sw)
        if has_db(c, i):
            out[f"db{sfx}"] = inp[f"db{sfx}_0"] + sb
    return out


# ---- which kernel runs: the launcher conditions restated ---------------------------------------------------------------------------
WS_FULL = 256 * 9216 * 16                     # srk_wgrad_workspace_bytes()
DEFAULTS = {"wgrad_stream": 1, "wgrad_stream_rows": 32, "wgrad_stream_nt": 1, "wgrad_stream_w8": 1, "wgrad_partials": 1,
            "conv_wgrad_taps": 2}
# the seven variants of test_streaming_linear_wgrad_vs_torch_and_register_staged_kernel
LINEAR_VARIANTS = {
    "ring32": {}, "ring32_w4": {"wgrad_stream_w8": 0},
    "ring64": {"wgrad_stream_rows": 64, "wgrad_stream_nt": 0}, "ring64_w4": {"wgrad_stream_rows": 64, "wgrad_stream_nt": 0, "wgrad_stream_w8": 0},
    "ring32_atomics": {"wgrad_partials": 0}, "ring32_atomics_w4": {"wgrad_partials": 0, "wgrad_stream_w8": 0},
    "staged": {"wgrad_stream": 0},
}
# further ring shapes, so that all eight instances of the streaming kernel run
LINEAR_EXTRA = {"ring32_plain": {"wgrad_stream_nt": 0}, "ring32_plain_w4": {"wgrad_stream_nt": 0, "wgrad_stream_w8": 0},
                "ring64_nt": {"wgrad_stream_rows": 64}, "ring64_nt_w4": {"wgrad_stream_rows": 64, "wgrad_stream_w8": 0}}
WORKSPACES = {"ws": WS_FULL, "nows": 0, "smallws": 1024}
CONV_VARIANTS = {f"taps{t}_partials{p}": {"conv_wgrad_taps": t, "wgrad_partials": p} for t in (2, 1, 0) for p in (1, 0)}

KERNELS = ([f"wgrad_kernel<{a}, {b}, false>" for a in (1, 2, 3) for b in (1, 2, 3)] + ["wgrad_kernel<*, *, true>"]
           + [f"wgrad_stream_kernel<{r}, {nt}, {w8}>" for r in (32, 64) for nt in ("false", "true") for w8 in ("false", "true")]
           + ["wgrad_reduce_kernel", "conv_wgrad_taps_kernel<false>", "conv_wgrad_taps_kernel<true>", "conv_wgrad_taps_dma_kernel<false>",
              "conv_wgrad_taps_dma_kernel<true>", "conv_wgrad_taps_reduce_kernel", "smallconv_wgrad_mfma_kernel<4>",
              "smallconv_wgrad_mfma_kernel<16>", "smallconv_wgrad_kernel<4>", "smallconv_wgrad_kernel<16>", "imghead_dgrad_mfma_kernel",
              "smallconv_dgrad_kernel", "stem_wgrad_mfma_kernel", "stem_wgrad_reduce_kernel", "stem_wgrad_kernel", "img_grad_prep_kernel"])


def _tile_class(N: int, K: int) -> Tuple[int, int]:
    f = lambda v: 3 if v % 192 == 0 else (2 if v % 128 == 0 else 1)          # csrc/wgrad.hip: tile_class
    return f(N), f(K)


def _cdiv(a, b):
    return -(-a // b)


def _linear_launch(c: Case, probs, o, ws) -> List[str]:
    """csrc/wgrad.hip: launch<TA, TB, false> for problems of one tile class."""
    a, b = _tile_class(probs[0].N, probs[0].K)
    tiles = sum((p.N // (64 * a)) * (p.K // (64 * b)) for p in probs)
    splits = max(1, 256 // tiles)
    m_per = max(256, 64 * _cdiv(_cdiv(c.M, splits), 64))
    splits = _cdiv(c.M, m_per)
    if (a, b) == (3, 3) and o["wgrad_stream"] and c.M % 64 == 0 and all(p.LDY % 8 == 0 and p.LDX % 8 == 0 for p in probs):
        tf = lambda v: "true" if v else "false"
        names = [f"wgrad_stream_kernel<{o['wgrad_stream_rows']}, {tf(o['wgrad_stream_nt'])}, {tf(o['wgrad_stream_w8'])}>"]
        if o["wgrad_partials"] and splits > 1 and tiles * splits * 9216 * 16 <= ws:
            names.append("wgrad_reduce_kernel")
        return names
    return [f"wgrad_kernel<{a}, {b}, false>"]


def EXPECTED_KERNEL(c: Case, options: Optional[Dict[str, int]] = None, workspace: int = WS_FULL) -> List[str]:
    """The kernels one call of the case's entry point launches under `options` (srk_set_option names) and a registered workspace of
    `workspace` bytes: csrc/wgrad.hip (launch / tile_class / srk_launch_wgrad_multi), csrc/convwgrad.hip (srk_launch_conv_wgrad_taps,
    srk_launch_smallconv_wgrad_mfma, srk_launch_imghead_dgrad_mfma), csrc/misc.hip (srk_launch_stem_wgrad / _smallconv_*)."""
    o = {**DEFAULTS, **(options or {})}
    taps = o["conv_wgrad_taps"]
    if c.kind == "linear":
        classes = {_tile_class(p.N, p.K) for p in c.probs}
        if len(classes) == 1:
            return _linear_launch(c, c.probs, o, workspace)
        return [n for p in c.probs for n in _linear_launch(c, (p,), o, workspace)]
    B, H, W = c.geo
    if c.kind in ("conv", "convps"):
        if taps and W % 64 == 0:
            shuf = "true" if c.kind == "convps" else "false"
            if taps == 1:
                return [f"conv_wgrad_taps_kernel<{shuf}>"]
            tiles = (c.N // 64) * (c.CinP // 64)
            nchunks = c.M // 64
            splits = min(max(1, 256 // tiles), nchunks)
            splits = _cdiv(nchunks, _cdiv(nchunks, splits))
            names = [f"conv_wgrad_taps_dma_kernel<{shuf}>"]
            if o["wgrad_partials"] and splits > 1 and tiles * splits * 9216 * 16 <= workspace:
                names.append("conv_wgrad_taps_reduce_kernel")
            return names
        return ["wgrad_kernel<*, *, true>"]
    if c.kind == "imgprep":
        return ["img_grad_prep_kernel"]
    if c.kind == "smallw":
        if taps and W % 64 == 0 and c.M % 64 == 0:
            return [f"smallconv_wgrad_mfma_kernel<{c.CoP}>"]
        return [f"smallconv_wgrad_kernel<{c.CoP}>"]
    if c.kind == "smalld":
        if taps and c.CoP == 4 and c.CinP == 64 and c.Co <= 4 and c.Cin <= 64 and c.M % 64 == 0:
            return ["imghead_dgrad_mfma_kernel"]
        return ["smallconv_dgrad_kernel"]
    if c.kind == "stem":
        if c.CoP == 192 and c.M % 32 == 0 and c.M >= 32 * 512 and 512 * 192 * 48 * 4 <= workspace:
            return ["stem_wgrad_mfma_kernel", "stem_wgrad_reduce_kernel"]
        return ["stem_wgrad_kernel"]
    raise ValueError(c.kind)


def smalld_lds_bytes(c: Case) -> int:
    """Dynamic LDS of smallconv_dgrad_kernel (csrc/misc.hip: srk_launch_smallconv_dgrad); above 64 KB the launcher raises the limit."""
    return (9 * c.Co * c.CinP + 16 * 9 * c.CoP) * 4


def option_sets(c: Case) -> Dict[str, Tuple[Dict[str, int], int]]:
    """name -> (options, workspace bytes) under which tests/test_gpu_wgrad.py runs the case.  Every set on an exact case must give the
    same bits."""
    if c.kind == "linear":
        if all(_tile_class(p.N, p.K) == (3, 3) for p in c.probs):
            sets = {f"{v}-{w}": (ov, wb) for v, ov in LINEAR_VARIANTS.items() for w, wb in WORKSPACES.items()}
            sets.update({f"{v}-ws": (ov, WS_FULL) for v, ov in LINEAR_EXTRA.items()})
            return sets
        return {"default-ws": ({}, WS_FULL), "default-nows": ({}, 0)}
    if c.kind in ("conv", "convps"):
        sets = {f"{v}-ws": (ov, WS_FULL) for v, ov in CONV_VARIANTS.items()}
        sets["taps2_partials1-nows"] = (CONV_VARIANTS["taps2_partials1"], 0)
        return sets
    if c.kind == "imgprep":
        return {"default": ({}, 0)}
    if c.kind in ("smallw", "smalld"):
        return {"taps2": ({}, 0), "taps0": ({"conv_wgrad_taps": 0}, 0)}
    return {"ws": ({}, WS_FULL), "nows": ({}, 0)}


# ---- the case matrix (ordered from the plain to the edge shapes) ---------------------------------------------------------------
BLOCK = ((576, 192), (192, 192), (384, 192), (192, 384))            # qkv, proj, fc1, fc2 of a classical-width block: (N, K)
LIGHT = ((576, 64), (64, 192), (128, 64), (64, 128))                # the light-width block: 64->576, 192->64, 64->128, 128->64
MIXED = ((192, 192), (64, 128), (128, 64), (192, 64))
LINEAR_M = (1, 63, 64, 100, 255, 256, 257, 700, 4096 + 64 * 5, 4096 + 64 * 5 + 17, 16384 + 64 * 37, 32768)
CONV_SHAPES = ((2, 8, 64, 64, 64), (1, 5, 128, 192, 192), (3, 3, 64, 128, 64), (1, 1, 64, 64, 256), (2, 16, 16, 64, 64),
               (1, 24, 16, 192, 192), (3, 13, 9, 64, 256), (4, 64, 64, 192, 192))
CONV_RANDOM = (1, 5, 7)
HEADS = ((64, 64, 3, 4), (64, 64, 1, 4), (180, 192, 12, 16), (60, 64, 12, 16))          # (Cin, CinP, Co, CoP)
HEAD_GEO = ((2, 4, 64), (1, 6, 24), (1, 7, 9))                      # W % 64 == 0 (MFMA) / W = 24 / an odd pixel count (VALU)


def _wide(nk) -> Tuple[Prob, ...]:
    """Every operand a column slice of a wider buffer: ldy = N + 64, ldx = 2 K (the slice is the second half)."""
    return tuple(Prob(N, K, ldy=N + 64, ldx=2 * K, yoff=64 * (i % 2), xoff=K) for i, (N, K) in enumerate(nk))


def _cases() -> List[Case]:
    cs: List[Case] = []
    E, R, D = "exact", "random", "dyadic"
    # --- linear, single problem: the nine tile classes, then the M edge values, then the large (3, 3) shapes
    for N in (64, 128, 192):
        for K in (64, 128, 192):
            cs.append(linear_case(E, 700, (N, K)))
    cs += [linear_case(E, 4096 + 64 * 5, (N, K)) for N, K in ((576, 192), (192, 384), (384, 384))]
    cs += [linear_case(R, 4096 + 64 * 5, (N, K), seed=1) for N, K in ((576, 192), (192, 384))]
    for M in LINEAR_M:
        if M != 700:
            cs.append(linear_case(E, M, (192, 192)))
    for M in (100, 257, 4096 + 64 * 5 + 17):                          # M % 64 != 0 on the other classes and on a wide (3, 3) shape
        cs += [linear_case(E, M, (64, 128)), linear_case(E, M, (128, 192)), linear_case(E, M, (576, 192))]
    cs += [linear_case(R, 4096 + 64 * 5, (192, 192), seed=2), linear_case(R, 16384 + 64 * 37, (192, 192), seed=3),
           linear_case(E, 16384 + 64 * 37, (576, 192)), linear_case(R, 16384 + 64 * 37, (576, 192), seed=4)]
    # --- linear, multi
    for M in (64 * 37, 16384):
        cs += [linear_case(E, M, *_wide(BLOCK)), linear_case(R, M, *_wide(BLOCK), seed=5)]
    for n in (1, 2, 3):
        cs.append(linear_case(E, 64 * 37, *_wide(BLOCK)[:n], multi=True))
    qkv = tuple(Prob(192, 192, ldy=576, yoff=192 * i, ybuf=0) for i in range(3))
    cs += [linear_case(E, 64 * 37, *qkv), linear_case(E, 16384, *qkv, Prob(192, 384))]
    cs += [linear_case(E, 64 * 37 + 5, *_wide(BLOCK)),                  # M % 64 != 0: the four problems leave the streaming kernel together
           linear_case(E, 1000, *MIXED), linear_case(E, 16384, *MIXED),
           linear_case(E, 64 * 37, Prob(192, 192), Prob(192, 384, db=False), Prob(384, 192)),
           linear_case(E, 1000, Prob(64, 128), Prob(64, 128, db=False), Prob(64, 128)),
           linear_case(E, 4096, *LIGHT), linear_case(E, 1000, *LIGHT)]
    # --- conv
    for i, s in enumerate(CONV_SHAPES):
        cs.append(conv_case(E, *s))
        if i in CONV_RANDOM:
            cs.append(conv_case(R, *s, seed=10 + i))
    cs.append(conv_case(E, 2, 8, 64, 64, 64, db=False))
    cs.append(conv_case(E, 2, 16, 16, 64, 64, db=False))
    # --- conv + PixelShuffle
    for r, N in ((2, 256), (3, 576)):
        cs += [conv_case(E, 2, 4, 64, 64, N, r=r, Cs=64), conv_case(E, 1, 6, 24, 64, N, r=r, Cs=64)]
    cs += [conv_case(R, 2, 4, 64, 64, 256, r=2, Cs=64, seed=20), conv_case(R, 1, 6, 24, 64, 576, r=3, Cs=64, seed=21),
           conv_case(E, 1, 5, 128, 192, 256, r=2, Cs=64)]
    # --- image head
    cs += [prep_case(2, 5, 9, 1, 3, 4), prep_case(2, 5, 9, 1, 1, 4), prep_case(2, 5, 9, 2, 3, 16), prep_case(2, 5, 9, 2, 3, 16, crop=(1, 3)),
           prep_case(1, 4, 64, 1, 3, 4, crop=(1, 3), cls=R, seed=30), prep_case(1, 4, 64, 2, 3, 16, crop=(1, 3), cls=R, seed=31)]
    for kind in ("smallw", "smalld"):
        for h in HEADS:
            for geo in HEAD_GEO:
                cs.append(head_case(kind, E, *geo, *h))
            cs.append(head_case(kind, D, *HEAD_GEO[0], *h, seed=40))
            cs.append(head_case(kind, R, *HEAD_GEO[0], *h, seed=41))
        cs.append(head_case(kind, D, *HEAD_GEO[1], *HEADS[0], seed=42))
    # --- stem
    for Cin in (3, 1):
        cs += [stem_case(E, 4, 64, 64, Cin, 180, 192), stem_case(E, 1, 32, 511, Cin, 180, 192), stem_case(E, 1, 24, 24, Cin, 60, 64),
               stem_case(E, 1, 24, 24, Cin, 96, 128)]
    cs += [stem_case(R, 4, 64, 64, 3, 180, 192, seed=50), stem_case(D, 4, 64, 64, 3, 180, 192, seed=51),
           stem_case(D, 1, 24, 24, 3, 60, 64, seed=52), stem_case(R, 1, 24, 24, 1, 96, 128, seed=53)]
    return cs


CASES: List[Case] = _cases()


def twin(c: Case) -> Optional[Case]:
    """The exact case of the same shape."""
    for e in CASES:
        if e.cls == "exact" and e.shape_key == c.shape_key:
            return e
    return None


def controls_for(c: Case) -> Dict[str, Mut]:
    """The negative controls that apply to a case."""
    out: Dict[str, Mut] = {}
    M = c.M
    if c.kind in ACCUMULATING:
        if M >= 2:
            b = min(256, 64 * ((M // 2) // 64)) if M >= 128 else M // 2           # the first row of the second split / chunk
            out["row dropped at a split boundary"] = Mut(drop_row=b)
            out["row counted twice"] = Mut(double_row=min(M - 1, b + 63))
        if M % 64 and M > 64:
            out["tail rows dropped"] = Mut(drop_tail=True)
        out["dW0 overwritten"] = Mut(overwrite=True)
        if any(has_db(c, i) and (c.kind != "linear" or _k_tiles(c.probs[i].K) == 1) for i in range(max(1, len(c.probs)))):
            out["db from k-tile 1"] = Mut(db_from_tk1=True)          # with two k-tiles that workgroup exists and db comes out right
    if c.kind not in ("linear", "imgprep"):
        out["taps swapped"] = Mut(swap_taps=True)
    if c.kind in ("convps", "imgprep") and c.r > 1:
        out["(i, j) swapped"] = Mut(swap_ij=True)
    if c.kind == "imgprep" and c.crop != (0, 0):
        out["crop ignored"] = Mut(no_crop=True)
    if c.cls == "dyadic":
        out["lo half omitted"] = Mut(no_lo=True)
    return out
