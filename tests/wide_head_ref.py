"""What the tests of the wide one-step head's backward share (srk_widehead_grad_prep / _wgrad / _dgrad of include/srk.h, CoP 32 / 48 / 64):
the case matrix, the inputs, the derived tolerance, the negative controls and the G21 fixture's seeded tensors.  Plain torch on the CPU.

Reference.  tests/wgrad_ref.py restates the narrow family (kinds "imgprep", "smallw", "smalld") and takes the wide widths as they are;
`reference` here is that restatement.  tests/test_wide_head_train_ref.py pins it against torch.nn.functional.conv2d under autograd in
fp64 (`autograd_reference`), which is also what the negative controls are built from.

Inputs.  wgrad_ref.make_inputs, with two changes:
  * the exact dgrad class.  wgrad_ref draws every weight from {-1, 0, 1} and so asserts 9 * Co * 2 <= 256 (Co <= 14).  Here the weights
    of one input channel are non-zero at AT MOST 128 of the 9 * Co (tap, co) positions, chosen by a hash over all of them, with every
    output channel and every tap used by some input channel; |gy| <= 2.  Every dx is then an integer of magnitude <= 256, which bf16
    holds: the assertion is torch.equal.  `make_inputs` asserts the precondition.
  * the pad columns Co .. CoP - 1 of gy carry small non-zero integers instead of zeros: the kernels must not let them leak (the
    engine's gradient prep writes zeros there; the entry points do not rely on it).

Tolerance, per element, in the form of wgrad_ref.tolerance:
    2 L u S  +  u (|dW0| + |ref|)  or  2^-8 |ref| + tiny (dx: one bf16 rounding)  +  N_SPLIT * 2^-16 * S
with L = B H W (wgrad, per tap) or 9 Co (dgrad), S the sum of the absolute terms, u = 2^-24.  N_SPLIT is the number of hi + lo split
products the kernels make: csrc/headconv_wide.hip uses the fp32-input MFMA (an fp32 fmaf chain on the fp32 operands), so N_SPLIT = 0.
The exact class and the prep get 0: equality."""
from __future__ import annotations

from typing import Dict, List

import torch
import torch.nn.functional as F

import wgrad_ref as R
from gemm_ex_ref import BF16_REL, BF16_TINY, U, Out, Tol

N_SPLIT = 0                                   # split products of the kernels under test (fp32-input MFMA: none)
HEADS = ((60, 64, 27, 32), (60, 64, 48, 48), (60, 64, 64, 64), (180, 192, 48, 48), (240, 256, 25, 32))      # (Cin, CinP, Co, CoP)
# The wgrad kernel walks 64-pixel chunks, a workgroup at least 4 of them (csrc/headconv_wide.hip: WG_CHUNK, WG_MIN_CHUNKS), and keeps x
# in a 256-pixel ring when W <= 95.  (1, 9, 40) = 360 pixels = 6 chunks: workgroup 0 walks 4 chunks (its ring wraps: 2 * 40 + 66 + 3 * 64
# = 338 > 256 slots written) and a second split takes the last two.  (1, 3, 100) = 300 pixels: W > 95, the fallback staging, two splits.
GEO = ((2, 4, 64), (1, 6, 24), (1, 7, 9), (1, 1, 1), (1, 9, 40), (1, 3, 100))
LONG_GEO = (GEO[4], GEO[5])
NARROW_THROUGH_WIDE = (60, 64, 16, 32)        # a 16-channel head through the wide entries


def _cases() -> List[R.Case]:
    cs: List[R.Case] = []
    for kind in ("smallw", "smalld"):
        for h in HEADS:
            for geo in GEO:
                if geo in LONG_GEO and h not in (HEADS[1], HEADS[3]):
                    continue                                           # the long walks: one light and one classical width
                cs.append(R.head_case(kind, "exact", *geo, *h))
            cs.append(R.head_case(kind, "dyadic", *GEO[0], *h, seed=60))
            cs.append(R.head_case(kind, "random", *GEO[0], *h, seed=61))
        cs.append(R.head_case(kind, "random", *GEO[4], *HEADS[1], seed=62))
        cs.append(R.head_case(kind, "random", *GEO[2], *NARROW_THROUGH_WIDE, seed=63))
        cs.append(R.head_case(kind, "exact", *GEO[1], *NARROW_THROUGH_WIDE))
    # gradient prep: r = 3 / 4 RGB, 8 gray, 5 gray (25 of 32 columns), with and without a crop; one random
    cs += [R.prep_case(2, 5, 9, 3, 3, 32), R.prep_case(2, 5, 9, 3, 3, 32, crop=(1, 3)), R.prep_case(2, 5, 9, 4, 3, 48, crop=(1, 3)),
           R.prep_case(1, 3, 7, 8, 1, 64, crop=(5, 2)), R.prep_case(2, 5, 9, 5, 1, 32),
           R.prep_case(1, 4, 64, 4, 3, 48, crop=(1, 3), cls="random", seed=64)]
    return cs


CASES: List[R.Case] = _cases()


def exact_dgrad_weight(c: R.Case) -> torch.Tensor:
    """[Co][Cin][3][3] in {-1, 0, 1}: per input channel at most 128 non-zeros among its 9 * Co (tap, co) positions, the positions ranked
    by a hash; every (co, tap) is non-zero for at least one input channel."""
    n = 9 * c.Co
    keep = min(n, 128)
    h = R._hash((c.Cin, n), 500 + c.seed)
    rank = h.argsort(dim=1).argsort(dim=1)                              # rank of each position within its input channel
    sign = torch.where((h >> 20) % 2 == 0, 1.0, -1.0)
    w = torch.where(rank < keep, sign, torch.zeros_like(sign))         # [Cin][9 * Co], position = tap * Co + co
    assert int((w != 0).sum(1).max()) <= 128
    assert bool((w != 0).any(0).all()), "an output channel / tap that no input channel uses"
    return w.reshape(c.Cin, 9, c.Co).permute(2, 0, 1).reshape(c.Co, c.Cin, 3, 3).contiguous()


def make_inputs(c: R.Case) -> Dict[str, torch.Tensor]:
    if c.kind == "smalld" and c.cls == "exact" and 9 * c.Co * 2 > 256:
        gy = torch.zeros(c.M, c.CoP)
        gy[:, :c.Co] = R.ints((c.M, c.Co), 2, c.seed, nonzero=True)
        inp = {"gy": gy, "weight": exact_dgrad_weight(c)}
        bound = (inp["weight"] != 0).sum(dim=(0, 2, 3)).max() * 2       # per input channel: non-zeros * max |gy|
        assert int(bound) <= 256, "an exact dx that bf16 might not hold"
    else:
        inp = R.make_inputs(c)
    if c.kind in ("smallw", "smalld") and c.Co < c.CoP:
        inp["gy"][:, c.Co:] = R.ints((c.M, c.CoP - c.Co), 2, c.seed + 7, nonzero=True)
    return inp


def reference(c: R.Case, inp, m: R.Mut = R.Mut(), with_S: bool = False):
    return R.reference(c, inp, m, with_S)


def tolerance(c: R.Case, inp, refS=None) -> Dict[str, torch.Tensor]:
    ref, S = refS if refS is not None else reference(c, inp, with_S=True)
    if c.cls == "exact" or c.kind == "imgprep":
        return {k: torch.zeros_like(v) for k, v in ref.items()}
    tol = {}
    for k, v in ref.items():
        L = 9 * c.Co if c.kind == "smalld" else c.M
        t = Tol.delta(L, S[k]) + N_SPLIT * BF16_REL ** 2 * S[k]
        if c.kind == "smalld":
            t = t + BF16_REL * v.abs() + BF16_TINY
        else:
            t = t + U * (inp[k + "_0"].double().abs() + v.abs())
        tol[k] = t
    return tol


def expected(c: R.Case, inp) -> Dict[str, Out]:
    refS = reference(c, inp, with_S=True)
    tol = tolerance(c, inp, refS)
    return {k: Out(v, tol[k], "bf16" if k == "dx" else "f32") for k, v in refS[0].items()}


accepts = R.accepts


# ---- fp64 autograd of the conv itself, and the negative controls built on it ------------------------------------------------------
CONTROLS = ("tap dropped", "(co, ci) transposed", "lo half dropped", "pad column of gy leaks", "halo off by one")


def _pad(t: torch.Tensor, wrong_halo: bool) -> torch.Tensor:
    """NCHW -> zero pad 1; wrong_halo: the left halo column holds the row's last pixel instead of zero (a halo read one pixel off)"""
    p = F.pad(t, (1, 1, 1, 1))
    if wrong_halo:
        p[:, :, 1:-1, 0] = t[:, :, :, -1]
    return p


def autograd_reference(c: R.Case, inp, control: str = "") -> Dict[str, torch.Tensor]:
    """The case's outputs from torch.nn.functional.conv2d in fp64 (autograd for dw / db; the transposed conv for dx).  `control`: one of
    CONTROLS -- a deliberately WRONG result."""
    assert control in ("",) + CONTROLS
    B, H, W = c.geo
    drop_kx = 2 if W > 1 else 1                   # the dropped tap: the right neighbour, or the centre where the image has none
    gy = inp["gy"].double()
    if control == "lo half dropped":
        gy = inp["gy"].to(torch.bfloat16).double()
    g = gy[:, :c.Co].clone()
    if control == "pad column of gy leaks" and c.Co < c.CoP:
        g[:, c.Co - 1] += gy[:, c.Co]
    g = g.reshape(B, H, W, c.Co).permute(0, 3, 1, 2).contiguous()                     # NCHW
    if c.kind == "smalld":
        w = inp["weight"].double()
        if control == "lo half dropped":
            w = inp["weight"].to(torch.bfloat16).double()
        if control == "(co, ci) transposed":
            w = w.reshape(c.Cin, c.Co, 3, 3).permute(1, 0, 2, 3).contiguous()          # the buffer read as [Cin][Co][3][3]
        if control == "tap dropped":
            w = w.clone()
            w[:, :, 1, drop_kx] = 0.0
        wt = w.flip(2, 3).permute(1, 0, 2, 3).contiguous()                             # the transposed conv as a conv of gy
        dx = F.conv2d(_pad(g, control == "halo off by one"), wt)
        out = torch.zeros(c.M, c.CinP, dtype=torch.float64)
        out[:, :c.Cin] = dx.permute(0, 2, 3, 1).reshape(c.M, c.Cin)
        return {"dx": out}
    x = inp["x"].double()[..., :c.Cin].permute(0, 3, 1, 2).contiguous()
    w0 = torch.zeros(c.Co, c.Cin, 3, 3, dtype=torch.float64, requires_grad=True)
    b0 = torch.zeros(c.Co, dtype=torch.float64, requires_grad=True)
    F.conv2d(_pad(x, control == "halo off by one"), w0, b0).backward(g)
    dw, db = w0.grad, b0.grad
    if control == "(co, ci) transposed":
        dw = dw.reshape(c.Cin, c.Co, 3, 3).permute(1, 0, 2, 3).contiguous()
    if control == "tap dropped":
        dw = dw.clone()
        dw[:, :, 1, drop_kx] = 0.0
    return {"dw": inp["dw_0"].double() + dw, "db": inp["db_0"].double() + db}


def controls_for(c: R.Case):
    """the controls that can show on a case"""
    out = ["tap dropped", "(co, ci) transposed"]
    if c.geo[2] > 1:
        out.append("halo off by one")
    if c.Co < c.CoP:
        out.append("pad column of gy leaks")
    if c.cls == "dyadic":
        out.append("lo half dropped")
    return out


# ---- G21: the reference's train-mode loss and gradients through the wide heads -----------------------------------------------------
G21_NAME = "g21_wide_head_train"
G21_TAGS = ("psd3", "psd4", "psd8g")
G21_SIZES = ((16, 16), (11, 13))


def _g21_seed(tag, hw) -> int:
    return 2100 + 1000 * G21_TAGS.index(tag) + hw[0] * 17 + hw[1]


def g21_input(tag, hw) -> torch.Tensor:
    from golden_scales import CASES as SCALES, config
    return torch.rand(SCALES[tag][2], config(tag).in_chans, *hw, generator=torch.Generator().manual_seed(_g21_seed(tag, hw)))


def g21_target(tag, hw) -> torch.Tensor:
    from golden_scales import CASES as SCALES, config
    cfg = config(tag)
    return torch.rand(SCALES[tag][2], cfg.in_chans, hw[0] * cfg.upscale, hw[1] * cfg.upscale,
                      generator=torch.Generator().manual_seed(_g21_seed(tag, hw) + 500))


def g21_checked_weights(tag):
    """-> (golden, cfg, sd): the weights regenerated from the recorded seed and held to the stored digest (as G20)"""
    import hashlib

    import numpy as np

    from conftest import load_golden
    from golden_scales import config, weights
    g = load_golden(G21_NAME)
    sd = weights(tag)
    digest = hashlib.sha1(np.ascontiguousarray(np.concatenate([v.numpy().astype(np.float32).reshape(-1) for v in sd.values()])).tobytes()).hexdigest()
    assert digest == str(g[f"{tag}.weight_sha1"]), f"{tag}: weight generator drifted from the one the fixture was made with"
    return g, config(tag), sd
