"""fp64 restatement of srk_swin_block_fwd (include/srk.h; csrc/block_light.hip: one whole Swin block of the SwinIR-light width per launch),
STAGE BY STAGE, its derived tolerances, the probes that expose the kernel's intermediates, a CPU emulation of the kernel and the case matrix
of tests/test_gpu_block_light.py.  Plain torch on the CPU; pinned in tests/test_light_ref.py.

The kernel has one output, y.  Its own arithmetic exposes the stages: an exact 0 or an identity weight passes a stage's bf16 result through
the later MFMAs unchanged (v * 1.0 + 0 is exact in fp32), so with chosen weights  y - base  IS an intermediate.  Every probe is one launch
on the same x with another weight set, all weights in the logical torch layout (`probe`):

  probe   weights                                                             y - base exposes
  P0      proj = 0, fc2 = 0, all biases 0                                     nothing: y == x BIT FOR BIT (gather, roll and scatter invert each other)
  P1      identity attention, V = I, proj = I, fc2 = 0                        xn = bf16(LN1(x)), through the window map and back
  P2v/P2k identity attention, V = Wv, bv (Wk, bk in the V slot), proj = I     v (k: phase 1 treats every fragment alike) from the device's xn
  P3      production q / k / v, table, mask; proj = I, fc2 = 0                ao (the bf16 attention output)
  P4      production first half, fc2 = 0, b2 = 0                              y == x1 exactly (fp32)
  P5      production first half, fc2 = selector of C hidden columns, b2 = 0   h = bf16(gelu(fc1(bf16(LN2(x1))) + b1)), ceil(hidden / C) launches
  P6      production                                                          y from the device's own x1 and h

Identity attention: a relative-position table that is 0 at offset (0, 0) (row 112 of 225) and -30000 elsewhere, zero q / k weights and
biases.  Then every score is table[rpi]: 0 on the diagonal, -30000 (-30100 under the shift mask) off it; the off-diagonal numerators are
exp2(-43000) = 0, the diagonal one is 1, the row sum 1, so ao == v.

Each stage is compared in fp64 with the restatement evaluated from the DEVICE's own previous intermediate (the method of block_ref.BTol):
a half-ulp flip upstream does not widen the bound downstream.  Two intermediates are never exposed and are restated with their bound
carried into the next stage instead:  q (the scale is applied before its rounding: restated from the device's xn with the scaled-bf16
bound e_q, and sum_d e_q |k| joins the score error), and bf16(LN2(x1)) (restated from the device's x1 with Tol.ln_fwd's bound t, and
t |W1|^T joins fc1's delta).

Recovering a bf16 intermediate t from y = fl32(base + t) (`recover`).  d = y - base is exact in fp64.
  x lies on a 2^-12 grid with |x| <= 7.5.  A bf16 t with 2^e <= |t| < 2^(e+1) has its last bit at 2^(e-7); base + t is a multiple of
  min(2^-12, 2^(e-7)) below 2^(e+17) (e = -14: 7.5 + 2^-13 < 8), which fp32 holds exactly: d == t for every |t| >= 2^-14.  The test sees d,
  not t; |d| >= 2^-13 implies |t| >= 2^-13 - 2^-21 > 2^-14, so that is the threshold it uses.
  Any base: |d - t| <= unc = u (|base| + |d|) (one fp32 rounding of the sum).  t is a bf16 number and its neighbours are >= 2^-8 |t| away, so
  where unc < 2^-10 |d| rounding d to bf16 returns t itself.
  Elsewhere d stands in for t with the uncertainty unc, which is added to the tolerance of the comparison and carried into the next
  stage's delta (unc |W|^T; sum_d |q| unc_k and sum_j p_j unc_v in the attention).

Layouts (include/srk.h): x, y fp32 [B*H*W][64] token-major, channels >= C zero; wqkv bf16 [3*192][64], row = which*192 + head*32 + d;
wproj bf16 [64][192], column = head*32 + d; w1 bf16 [128][64]; w2 bf16 [64][128]; fp32 biases in the same padded order; bias_dense fp32
[6][64][64] = table[rpi]; every pad row / column is zero.  gamma / beta are read below C only (the test poisons their pads with NaN).
"""
from __future__ import annotations

import math
from dataclasses import dataclass, replace
from typing import Callable, Dict, List, Tuple

import torch

from block_ref import OK, BTol, Variant, dense_bias, shift_mask, win_to_token
from gemm_ex_ref import BF16_REL, BF16_TINY, GELU_LIP, LN_EPS, U, Out, Tol, compare, gelu, ln_fwd, round_as  # noqa: F401

NH, CP, DP, HP, CA = 6, 64, 32, 128, 192
PRE = "b."
IDENT_OFF = -30000.0
K_QKV, K_QK, K_PROJ, K_FC1, K_FC2 = 64, 16, 96, 64, 128     # the K each MFMA chain accumulates over (zero pads included)
L2E = float(torch.tensor(1.4426950408889634, dtype=torch.float32))
RSQRT2 = float(torch.tensor(0.70710678118654752, dtype=torch.float32))
STAGES = ("map", "xn", "v", "k", "ao", "x1", "h", "y")


@dataclass(frozen=True)
class LVariant(Variant):
    """block_ref.Variant (shift_sign, swap_hw, no_mask, bias_transposed, ln_over_cp: here 64 columns instead of C) and the controls that
    only this kernel has.  `emulate` applies them: each makes the emulated kernel deliberately WRONG."""
    mask_last_row_only: bool = False    # the shift mask applied in the last window row but not in the last window column
    head_plus_one: bool = False         # the k tile of head h read from head h + 1
    gelu_of_rounded: bool = False       # h = bf16(gelu(bf16(u))) where the kernel takes gelu(u)


# ---- cases ----------------------------------------------------------------------------------------------------------------------------
WIDTHS = ((60, 10, 120), (48, 8, 96), (30, 5, 50), (6, 1, 6), (60, 10, 128))       # (C, head_dim, hidden), 6 heads
GEOMS = ((1, 8, 8), (1, 8, 16), (2, 16, 8), (3, 24, 40))


@dataclass(frozen=True)
class LCase:
    C: int
    dh: int
    hid: int
    B: int
    H: int
    W: int
    shift: int
    multi: bool = False       # more windows than are resident at once (3 workgroups per CU)

    @property
    def T(self) -> int:
        return self.B * self.H * self.W

    @property
    def nW(self) -> int:
        return (self.H // 8) * (self.W // 8)

    @property
    def id(self) -> str:
        return f"C{self.C}x{self.dh}-h{self.hid}-{self.B}x{self.H}x{self.W}-s{self.shift}" + ("-multi" if self.multi else "")

    @property
    def scale(self) -> float:
        return float(torch.tensor(self.dh ** -0.5, dtype=torch.float32))      # the ABI passes the q scale as a float


def multi_B(n: int) -> int:
    """The smallest B with B * 64 windows (H = W = 64) > 3 n resident workgroups; n = 256: 13."""
    return 3 * n // 64 + 1


def cases(n: int = 256) -> List[LCase]:
    """Every width at (3, 24, 40), every geometry at the cfg2 width, both shifts; the multi-round case once, with shift 4."""
    cs = [LCase(*w, *GEOMS[-1], s) for w in WIDTHS for s in (0, 4)]
    cs += [LCase(*WIDTHS[0], *g, s) for g in GEOMS[:-1] for s in (0, 4)]
    cs.append(LCase(*WIDTHS[0], multi_B(n), 64, 64, 4, multi=True))
    return cs


def for_device(c: LCase, n: int) -> LCase:
    """The case of a device with n CUs that corresponds to a case of the 256-CU matrix (the ids are those of the 256-CU matrix)."""
    return replace(c, B=multi_B(n)) if c.multi else c


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
def _seed(c: LCase) -> int:
    return 9000 + 131 * c.C + 17 * c.hid + 7 * c.H + 3 * c.W          # a SHAPE's operands: shift and B do not change the weights


def make_x(c: LCase) -> torch.Tensor:
    """fp32 [T][C]: per-row offsets up to +-3, unit spread, one outlier channel per row, on the 2^-12 grid with |x| <= 7.5."""
    g = torch.Generator().manual_seed(_seed(c) + 1)
    T, C = c.T, c.C
    x = torch.randn(T, C, generator=g) + (6.0 * torch.rand(T, 1, generator=g) - 3.0)
    j = torch.randint(0, C, (T,), generator=g)
    sign = torch.where(torch.rand(T, generator=g) < 0.5, -1.0, 1.0)
    x[torch.arange(T), j] += 4.0 * sign
    return (torch.round(x.clamp(-7.5, 7.5) * 4096.0) / 4096.0).float()


def _bias(g, n, std):
    b = std * torch.randn(n, generator=g)
    b[b.abs() < 0.1 * std] = 0.5 * std                     # no accidental zero: a dropped bias shows in every column
    return b


def make_weights(c: LCase) -> Dict[str, torch.Tensor]:
    """The block's state dict in the torch layout (fp32; the linear weights hold bf16 values, as the packed buffers do).  q / k rows scaled
    so that the scores have a spread of 2-3; table spread 0.5 with a few entries at +-8."""
    g = torch.Generator().manual_seed(_seed(c))
    C, hid = c.C, c.hid
    rb = lambda t: t.to(torch.bfloat16).float()
    r = lambda *s: torch.randn(*s, generator=g)
    wqkv = r(3 * C, C) * C ** -0.5
    wqkv[:2 * C] *= 1.6
    table = 0.5 * r(225, NH)
    pick = torch.randperm(225 * NH, generator=g)[:12]
    table.view(-1)[pick] = torch.tensor([8.0, -8.0] * 6)
    return {
        PRE + "norm1.weight": 1.0 + 0.2 * r(C), PRE + "norm1.bias": _bias(g, C, 0.2),
        PRE + "attn.relative_position_bias_table": table,
        PRE + "attn.qkv.weight": rb(wqkv), PRE + "attn.qkv.bias": _bias(g, 3 * C, 0.2),
        PRE + "attn.proj.weight": rb(r(C, C) * C ** -0.5), PRE + "attn.proj.bias": _bias(g, C, 0.2),
        PRE + "norm2.weight": 1.0 + 0.2 * r(C), PRE + "norm2.bias": _bias(g, C, 0.2),
        PRE + "mlp.fc1.weight": rb(r(hid, C) * C ** -0.5), PRE + "mlp.fc1.bias": _bias(g, hid, 0.2),
        PRE + "mlp.fc2.weight": rb(r(C, hid) * hid ** -0.5), PRE + "mlp.fc2.bias": _bias(g, C, 0.2),
    }


def probe(c: LCase, sd: Dict[str, torch.Tensor], name: str, j0: int = 0) -> Dict[str, torch.Tensor]:
    """The weight set of a probe (module docstring), in the torch layout."""
    C, hid = c.C, c.hid
    s = dict(sd)
    z = torch.zeros

    def put(**kw):
        for k, t in kw.items():
            s[PRE + k.replace("__", ".")] = t

    def identity_attention(vw, vb):
        t = torch.full((225, NH), IDENT_OFF)
        t[112] = 0.0                                           # offset (0, 0): (7 * 15 + 7)
        w, b = z(3 * C, C), z(3 * C)
        w[2 * C:], b[2 * C:] = vw, vb
        put(attn__relative_position_bias_table=t, attn__qkv__weight=w, attn__qkv__bias=b, attn__proj__weight=torch.eye(C), attn__proj__bias=z(C))

    wq, bq = sd[PRE + "attn.qkv.weight"], sd[PRE + "attn.qkv.bias"]
    if name != "P6":
        put(mlp__fc2__weight=z(C, hid), mlp__fc2__bias=z(C))
    if name == "P0":
        put(attn__proj__weight=z(C, C), attn__proj__bias=z(C), attn__qkv__bias=z(3 * C), mlp__fc1__bias=z(hid))
    elif name == "P1":
        identity_attention(torch.eye(C), z(C))
    elif name == "P2v":
        identity_attention(wq[2 * C:], bq[2 * C:])
    elif name == "P2k":
        identity_attention(wq[C:2 * C], bq[C:2 * C])
    elif name == "P3":
        put(attn__proj__weight=torch.eye(C), attn__proj__bias=z(C))
    elif name == "P5":
        w = z(C, hid)
        n = min(C, hid - j0)
        w[torch.arange(n), j0 + torch.arange(n)] = 1.0
        put(mlp__fc2__weight=w)
    elif name not in ("P4", "P6"):
        raise ValueError(name)
    return s


# ---- packing, from the layout include/srk.h states -------------------------------------------------------------------------------------
def head_map(nH: int, dh: int) -> torch.Tensor:
    """channel h * dh + d -> padded channel h * 32 + d"""
    c = torch.arange(nH * dh)
    return (c // dh) * DP + c % dh


def pack_linear(w: torch.Tensor, NP: int, KP: int, row_map=None, col_map=None) -> torch.Tensor:
    """fp32 [N][K] -> bf16 [NP][KP], row n at row_map[n], column k at col_map[k], zero elsewhere."""
    N, K = w.shape
    out = torch.zeros(NP, KP, dtype=torch.float32)
    rows = torch.arange(N) if row_map is None else row_map
    cols = torch.arange(K) if col_map is None else col_map
    for n in range(N):
        out[rows[n], cols] = w[n].float()
    return out.to(torch.bfloat16)


def pack_vec(b: torch.Tensor, NP: int, row_map=None) -> torch.Tensor:
    out = torch.zeros(NP, dtype=torch.float32)
    out[torch.arange(b.numel()) if row_map is None else row_map] = b.float()
    return out


def pack_block(c: LCase, sd: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """The operands of srk_swin_block_fwd as CPU tensors in the device's dtypes.  gamma / beta are 64 long with NaN beyond C."""
    hm = head_map(NH, c.dh)
    qrows = torch.cat([which * CA + hm for which in range(3)])       # row = which * 192 + head * 32 + d
    g = lambda k: sd[PRE + k]

    def poisoned(t):
        out = torch.full((CP,), float("nan"))
        out[:c.C] = t.float()
        return out

    return dict(
        n1w=poisoned(g("norm1.weight")), n1b=poisoned(g("norm1.bias")), n2w=poisoned(g("norm2.weight")), n2b=poisoned(g("norm2.bias")),
        wqkv=pack_linear(g("attn.qkv.weight"), 3 * CA, CP, row_map=qrows), bqkv=pack_vec(g("attn.qkv.bias"), 3 * CA, qrows),
        wproj=pack_linear(g("attn.proj.weight"), CP, CA, col_map=hm), bproj=pack_vec(g("attn.proj.bias"), CP),
        w1=pack_linear(g("mlp.fc1.weight"), HP, CP), b1=pack_vec(g("mlp.fc1.bias"), HP),
        w2=pack_linear(g("mlp.fc2.weight"), CP, HP), b2=pack_vec(g("mlp.fc2.bias"), CP),
        dense=dense_bias(g("attn.relative_position_bias_table").float()).contiguous())


# ---- recovered intermediates -------------------------------------------------------------------------------------------------------------
@dataclass
class Rec:
    val: torch.Tensor        # fp64: the intermediate (a bf16 value where unc == 0)
    unc: torch.Tensor        # fp64: |val - the device's value| <= unc


def exact(t: torch.Tensor) -> Rec:
    return Rec(t, torch.zeros_like(t))


def recover(y: torch.Tensor, base: torch.Tensor, grid: bool) -> Rec:
    """The bf16 t of y = fl32(base + t) (module docstring).  grid: base lies on the 2^-12 grid with |base| <= 7.5."""
    d = y.double() - base.double()
    unc = U * (base.double().abs() + d.abs())
    ok = unc < 2.0 ** -10 * d.abs()
    if grid:
        ok |= d.abs() >= 2.0 ** -13
    return Rec(torch.where(ok, round_as(d, "bf16"), d), torch.where(ok, torch.zeros_like(unc), unc))


def with_unc(out: Out, r: Rec) -> Out:
    return Out(out.ref, out.tol + r.unc, out.kind)


# ---- the stages (fp64) ----------------------------------------------------------------------------------------------------------------------
def _w(sd, key) -> torch.Tensor:
    """A linear weight as the packed bf16 buffer holds it."""
    return sd[PRE + key].to(torch.bfloat16).double()


def _f(sd, key) -> torch.Tensor:
    return sd[PRE + key].float().double()


def lin(a: Rec, w: torch.Tensor, b: torch.Tensor):
    """u = a W^T + b;  S = the absolute terms of that sum;  the input uncertainty propagated through |W|."""
    return a.val @ w.t() + b, a.val.abs() @ w.abs().t() + b.abs(), a.unc @ w.abs().t()


def st_xn(c: LCase, x: torch.Tensor, sd) -> Out:
    """xn = bf16(LayerNorm1(x)) over the C channels (eps 1e-5, biased variance): Tol.ln_fwd."""
    gam, bet = _f(sd, "norm1.weight"), _f(sd, "norm1.bias")
    xn, _, rstd = ln_fwd(x.double(), gam, bet, c.C)
    return Out(xn, Tol.ln_fwd(xn, x.double(), rstd, gam, bet, c.C)[0], "bf16")


def st_qkv(c: LCase, xn: Rec, sd, which: int) -> Out:
    """which 0: q = bf16((xn Wq^T + bq) * scale), Tol.bf16 with delta * scale and 2u |ref| for the extra product (BTol: q (scaled));
    which 1 / 2: k / v = bf16(xn W^T + b), Tol.bf16 with delta = 2 K u S."""
    C = c.C
    u, S, prop = lin(xn, _w(sd, "attn.qkv.weight")[which * C:(which + 1) * C], _f(sd, "attn.qkv.bias")[which * C:(which + 1) * C])
    d = Tol.delta(K_QKV, S) + prop
    if which:
        return Out(u, Tol.bf16(u, d), "bf16")
    r = u * c.scale
    return Out(r, Tol.bf16(r, d * c.scale) + 2 * U * r.abs(), "bf16")


def st_ao(c: LCase, q: Out, k: Rec, v: Rec, sd) -> Out:
    """ao = softmax(q k^T + table[rpi] + mask) v per window and head: BTol.attn, from the restated q (bound q.tol) and the device's k, v.
    Score error: ds_j = 2 * 16 u sum_d |q k| + 2u (|bias_j| + 100) + sum_d e_q |k_j| + sum_d |q| unc_k.  BTol.attn is first order in ds;
    the unexposed q makes ds ~ 1e-2, so ds is scaled by expm1(2 max ds) / (2 max ds) >= 1: a probability moves by at most
    exp(ds_j + max ds) - 1.  The uncertainty of a recovered v adds sum_j p_j unc_v."""
    C, dh = c.C, c.dh
    tok = win_to_token(c.B, c.H, c.W, c.shift)
    bias = dense_bias(_f(sd, "attn.relative_position_bias_table"))[None]
    mask = shift_mask(c.H, c.W)[:, None] if c.shift else None                     # [nW][1][64][64]
    ref, tol = torch.empty(c.T, C, dtype=torch.float64), torch.empty(c.T, C, dtype=torch.float64)
    n = c.H * c.W
    for b in range(c.B):                                                          # one image at a time (memory)
        rows = tok[b * n:(b + 1) * n]
        heads = lambda t: t[rows].view(c.nW, 64, NH, dh).permute(0, 2, 1, 3)
        qh, eq, kh, ku, vh, vu = heads(q.ref), heads(q.tol), heads(k.val), heads(k.unc), heads(v.val), heads(v.unc)
        kt = kh.transpose(-1, -2)
        s = qh @ kt + bias
        ds = 2 * K_QK * U * (qh.abs() @ kt.abs()) + 2 * U * (bias.abs() + 100.0) + eq @ kt.abs() + qh.abs() @ ku.transpose(-1, -2)
        if mask is not None:
            s = s + mask
        p = torch.softmax(s, -1)
        dm = ds.amax(-1, keepdim=True)
        grow = torch.expm1(2 * dm) / (2 * dm)
        ds, dm = ds * grow, dm * grow
        o, A, As = p @ vh, p @ vh.abs(), (p * ds) @ vh.abs()
        t = BTol.attn(o, A, As, dm) + p @ vu
        flat = lambda t_: t_.permute(0, 2, 1, 3).reshape(n, C)
        ref[rows], tol[rows] = flat(o), flat(t)
    return Out(ref, tol, "bf16")


def st_x1(c: LCase, x: torch.Tensor, ao: Rec, sd) -> Out:
    """x1 = x + ao Wp^T + bp (fp32): Tol.f32."""
    u, S, prop = lin(ao, _w(sd, "attn.proj.weight"), _f(sd, "attn.proj.bias"))
    y = x.double() + u
    return Out(y, Tol.f32(y, Tol.delta(K_PROJ, S + x.double().abs()) + prop), "f32")


def st_h(c: LCase, x1: torch.Tensor, sd) -> Out:
    """h = bf16(gelu(bf16(LN2(x1)) W1^T + b1)) from the device's fp32 x1.  The bf16 LN2 output is not exposed: the fp64 LayerNorm stands
    in for it with Tol.ln_fwd's bound t, carried through |W1|.  Tol.bf16 with the Lipschitz constant of GELU, plus 8u |u| for the
    device's erf (gelu = u (1 + erf) / 2: the project's 8u convention on erf costs at most 4u |u|)."""
    gam, bet = _f(sd, "norm2.weight"), _f(sd, "norm2.bias")
    xn, _, rstd = ln_fwd(x1.double(), gam, bet, c.C)
    t = Tol.ln_fwd(xn, x1.double(), rstd, gam, bet, c.C)[0]
    u, S, prop = lin(Rec(xn, t), _w(sd, "mlp.fc1.weight"), _f(sd, "mlp.fc1.bias"))
    r = gelu(u)
    return Out(r, Tol.bf16(r, Tol.delta(K_FC1, S) + prop, GELU_LIP) + 8 * U * u.abs(), "bf16")


def st_y(c: LCase, x1: torch.Tensor, h: Rec, sd) -> Out:
    """y = x1 + h W2^T + b2 (fp32) from the device's own x1 and h: Tol.f32."""
    u, S, prop = lin(h, _w(sd, "mlp.fc2.weight"), _f(sd, "mlp.fc2.bias"))
    y = x1.double() + u
    return Out(y, Tol.f32(y, Tol.delta(K_FC2, S + x1.double().abs()) + prop), "f32")


def composed(c: LCase, x: torch.Tensor, sd) -> Dict[str, torch.Tensor]:
    """The stages chained in fp64 WITHOUT any rounding: what network_swinir.py:239-279 computes."""
    o = {"xn": st_xn(c, x, sd).ref}
    xn = exact(o["xn"])
    o["k"], o["v"] = st_qkv(c, xn, sd, 1).ref, st_qkv(c, xn, sd, 2).ref
    o["ao"] = st_ao(c, st_qkv(c, xn, sd, 0), exact(o["k"]), exact(o["v"]), sd).ref
    o["x1"] = st_x1(c, x, exact(o["ao"]), sd).ref
    o["h"] = st_h(c, o["x1"], sd).ref
    o["y"] = st_y(c, o["x1"], exact(o["h"]), sd).ref
    return o


# ---- the probe pipeline: the same code drives the device (GPU test) and the emulation (CPU test) ---------------------------------------------
Runner = Callable[[Dict[str, torch.Tensor]], torch.Tensor]        # state dict (torch layout) -> y fp32 [T][C] of one launch on the case's x


def run_stages(c: LCase, x: torch.Tensor, sd, run: Runner) -> Dict[str, float]:
    """Launch every probe through `run` and compare stage by stage: stage -> max(err / tol) (inf: a non-finite value, or P0 not bit-equal)."""
    X = x.double()
    res: Dict[str, float] = {}
    res["map"] = 0.0 if torch.equal(run(probe(c, sd, "P0")).float(), x.float()) else float("inf")
    xn = recover(run(probe(c, sd, "P1")), X, True)
    res["xn"] = compare(xn.val, with_unc(st_xn(c, x, sd), xn))[1]
    v = recover(run(probe(c, sd, "P2v")), X, True)
    res["v"] = compare(v.val, with_unc(st_qkv(c, xn, sd, 2), v))[1]
    k = recover(run(probe(c, sd, "P2k")), X, True)
    res["k"] = compare(k.val, with_unc(st_qkv(c, xn, sd, 1), k))[1]
    ao = recover(run(probe(c, sd, "P3")), X, True)
    res["ao"] = compare(ao.val, with_unc(st_ao(c, st_qkv(c, xn, sd, 0), k, v, sd), ao))[1]
    x1 = run(probe(c, sd, "P4")).double()
    res["x1"] = compare(x1, st_x1(c, x, ao, sd))[1]
    if not torch.isfinite(x1).all():
        res["h"] = res["y"] = float("inf")
        return res
    parts = []
    for j0 in range(0, c.hid, c.C):
        r = recover(run(probe(c, sd, "P5", j0)), x1, False)
        n = min(c.C, c.hid - j0)
        parts.append(Rec(r.val[:, :n], r.unc[:, :n]))
    h = Rec(torch.cat([p.val for p in parts], 1), torch.cat([p.unc for p in parts], 1))
    res["h"] = compare(h.val, with_unc(st_h(c, x1, sd), h))[1]
    res["y"] = compare(run(sd).double(), st_y(c, x1, h, sd))[1]
    return res


# ---- CPU emulation of the kernel: fp32 arithmetic, bf16 at the rounding points the header of block_light.hip lists ------------------------------
def emulate(c: LCase, x: torch.Tensor, sd, v: LVariant = LVariant()) -> torch.Tensor:
    """y fp32 [T][C] of one launch.  `v` makes the emulated kernel wrong (negative controls)."""
    f32 = torch.float32
    bf = lambda t: t.to(torch.bfloat16).to(f32)
    C, dh, B_ = c.C, c.dh, c.B * c.nW
    tok = win_to_token(c.B, c.H, c.W, c.shift, v)
    g = lambda key: sd[PRE + key].to(f32)
    wl = lambda key: bf(sd[PRE + key])

    def layer_norm(rows, gam, bet):
        n = CP if v.ln_over_cp else C
        xp = torch.zeros(rows.shape[0], CP, dtype=f32)
        xp[:, :C] = rows
        mean = xp.sum(1, keepdim=True) / n
        d = xp - mean
        if not v.ln_over_cp:
            d[:, C:] = 0.0
        rstd = torch.rsqrt((d * d).sum(1, keepdim=True) / n + f32_(LN_EPS))
        return bf(d[:, :C] * rstd * gam + bet)

    f32_ = lambda s: torch.tensor(s, dtype=f32)
    xw = x.to(f32)[tok]
    xn = layer_norm(xw, g("norm1.weight"), g("norm1.bias"))
    u = xn @ wl("attn.qkv.weight").t() + g("attn.qkv.bias")
    heads = lambda t: t.reshape(B_, 64, NH, dh).permute(0, 2, 1, 3)
    qh, kh, vh = heads(bf(u[:, :C] * f32_(c.scale))), heads(bf(u[:, C:2 * C])), heads(bf(u[:, 2 * C:]))
    if v.head_plus_one:
        kh = kh.roll(-1, dims=1)
    s = qh @ kh.transpose(-1, -2) + dense_bias(g("attn.relative_position_bias_table"), v)[None]
    if c.shift and not v.no_mask:
        m = shift_mask(c.H, c.W, v).to(f32)
        if v.mask_last_row_only:
            nWw = (c.H if v.swap_hw else c.W) // 8
            m[torch.arange(c.nW) // nWw != c.nW // nWw - 1] = 0.0
        s = (s.view(c.B, c.nW, NH, 64, 64) + m[None, :, None]).view(B_, NH, 64, 64)
    e = torch.exp2(s * f32_(L2E) - s.amax(-1, keepdim=True) * f32_(L2E))
    o = (bf(e) @ vh) * (1.0 / e.sum(-1, keepdim=True))
    ao = bf(o).permute(0, 2, 1, 3).reshape(c.T, C)
    x1 = (xw + ao @ wl("attn.proj.weight").t()) + g("attn.proj.bias")
    u = layer_norm(x1, g("norm2.weight"), g("norm2.bias")) @ wl("mlp.fc1.weight").t() + g("mlp.fc1.bias")
    if v.gelu_of_rounded:
        u = bf(u)
    h = bf(0.5 * u * (1.0 + torch.erf(u * f32_(RSQRT2))))
    yw = (x1 + h @ wl("mlp.fc2.weight").t()) + g("mlp.fc2.bias")
    y = torch.empty_like(yw)
    y[tok] = yw
    return y


# ---- negative controls ----------------------------------------------------------------------------------------------------------------------
def controls_for(c: LCase) -> Dict[str, Tuple[LVariant, str]]:
    """name -> (the wrong kernel, the stage whose comparator must refuse it) for the controls that apply to a case."""
    out: Dict[str, Tuple[LVariant, str]] = {}
    if c.shift and ((2 * c.shift) % c.H or (2 * c.shift) % c.W):      # an 8-row image rolled by +4 is rolled by -4
        out["roll applied with the wrong sign"] = (LVariant(shift_sign=True), "ao")
    if c.H != c.W:
        out["H and W swapped in the row map"] = (LVariant(swap_hw=True), "ao")
    if c.shift:
        out["mask dropped"] = (LVariant(no_mask=True), "ao")
        if c.H > 8:                                                   # a window of the last column that is not in the last row
            out["mask on the last window row only"] = (LVariant(mask_last_row_only=True), "ao")
    out["bias table transposed"] = (LVariant(bias_transposed=True), "ao")
    out["LayerNorm over 64 columns instead of C"] = (LVariant(ln_over_cp=True), "xn")
    out["head h reads the k tile of head h + 1"] = (LVariant(head_plus_one=True), "ao")
    return out


# Undetectable, and why: h = bf16(gelu(bf16(u))) instead of bf16(gelu(u)) moves h by at most 1.13 * 2^-8 |u|.  The h stage cannot see
# the bf16 LayerNorm2 output, so its bound already carries that output's own rounding through fc1, 1.13 * 2^-8 sum_k |xn_k W1_k| >=
# 1.13 * 2^-8 |u - b1|: the bound is as wide as the control's effect (only at C = 6, where |b1| can outweigh the six-term sum, are some
# elements refused; tests/test_light_ref.py pins both).
UNDETECTABLE = {"GELU of the rounded pre-activation": LVariant(gelu_of_rounded=True)}
