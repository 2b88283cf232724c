"""The eight symmetries of the square (D4) on image batches: flip / rot90 training augmentation and the x8 self-ensemble.

An op code k in 0..7 names one transform: bit 0 = horizontal flip (x -> W-1-x), bit 1 = vertical flip (y -> H-1-y), bit 2 =
transpose, applied in that order, T_k = Tr^b2 . V^b1 . H^b0.  On the device the transform is one kernel (csrc/dihedral.hip,
`srk_dihedral_f32`) that reads one code per sample from device memory -- a mixed batch is one launch, and the launch is capturable --
and can scale and accumulate its result, which is what the self-ensemble average needs.  On the host (`apply_op_host`: DataLoader
workers, and the reference of the tests) it is torch.flip / transpose.
"""
from __future__ import annotations

import random
from typing import Optional, Sequence, Union

import torch

AUGMENT_MODES = ("none", "flip", "d4")


def _check_op(k) -> int:
    k = int(k)
    if not 0 <= k <= 7:
        raise ValueError(f"a D4 op code is in 0..7 (got {k})")
    return k


def inverse_op(k: int) -> int:
    """The code of T_k's inverse.  The flips are involutions and commute, so k < 4 is its own inverse.  With the transpose,
    H . Tr = Tr . V (and V . Tr = Tr . H), hence (Tr . V^b1 . H^b0)^-1 = H^b0 . V^b1 . Tr = Tr . V^b0 . H^b1: the flip bits swap."""
    k = _check_op(k)
    return k if k < 4 else 4 | ((k & 1) << 1) | ((k >> 1) & 1)


def apply_op_host(t: torch.Tensor, k: int) -> torch.Tensor:
    """T_k on the last two dimensions of a CPU (or any) tensor with stock torch operators; k == 0 returns `t` itself."""
    k = _check_op(k)
    if k & 1:
        t = torch.flip(t, dims=(-1,))
    if k & 2:
        t = torch.flip(t, dims=(-2,))
    if k & 4:
        t = t.transpose(-2, -1).contiguous()
    return t


def draw_op(mode: str) -> int:
    """One op code from the process-global `random`: 'none' -> 0 WITHOUT touching the generator (the default batches and the
    default consumption of `random` stay what they were), 'flip' -> one of the four flips (each flip with p = 0.5), 'd4' -> one of
    the eight symmetries."""
    if mode == "none":
        return 0
    if mode == "flip":
        return random.randrange(4)
    if mode == "d4":
        return random.randrange(8)
    raise ValueError(f"augment must be one of {AUGMENT_MODES} (got {mode!r})")


def dihedral(x: torch.Tensor, op: Union[int, Sequence[int], torch.Tensor], out: Optional[torch.Tensor] = None, alpha: float = 1.0,
             accumulate: bool = False) -> torch.Tensor:
    """out = alpha * T_op(x)  (accumulate: out += alpha * T_op(x)) for a CUDA fp32 batch x [B,C,H,W].

    op: one code for the whole batch, or one code per sample -- a sequence (range-checked here, then uploaded) or an int32 device
    tensor of B codes (the kernel reads their low three bits).  Per-sample codes need square images: the output geometry must not
    depend on them.  `out` must not alias `x`; it is allocated when absent (not with accumulate)."""
    from . import ops as K
    from ._lib import check, lib
    if x.dim() != 4 or x.dtype != torch.float32:
        raise ValueError(f"dihedral takes fp32 [B,C,H,W] (got {x.dtype} {tuple(x.shape)})")
    B, Cc, H, W = x.shape
    codes, op_all = None, 0
    if isinstance(op, torch.Tensor):
        if op.dtype != torch.int32 or op.numel() != B or op.device != x.device:
            raise ValueError(f"per-sample op codes: an int32 tensor of {B} codes on {x.device} "
                             f"(got {op.dtype} {tuple(op.shape)} on {op.device})")
        codes = op
    elif isinstance(op, (list, tuple, range)):
        host = [_check_op(k) for k in op]
        if len(host) != B:
            raise ValueError(f"per-sample op codes: {B} samples, {len(host)} codes")
        codes = torch.tensor(host, dtype=torch.int32).to(x.device)
    else:
        op_all = _check_op(op)
    if codes is not None and H != W:
        raise ValueError(f"per-sample op codes need square images (got {H} x {W})")
    shape = tuple(x.shape[:-2]) + ((W, H) if (codes is None and op_all & 4) else (H, W))
    if out is None:
        if accumulate:
            raise ValueError("accumulate=True needs the buffer to accumulate into (out=...)")
        out = torch.empty(shape, dtype=torch.float32, device=x.device)
    elif tuple(out.shape) != shape or out.dtype != torch.float32 or out.device != x.device:
        raise ValueError(f"out must be fp32 {shape} on {x.device} (got {out.dtype} {tuple(out.shape)} on {out.device})")
    check(lib().srk_dihedral_f32(K._p(x), K._p(out), K._p(codes), op_all, B, Cc, H, W, float(alpha), int(bool(accumulate)), K._stream()))
    return out


def self_ensemble(model, x: torch.Tensor, ops: Sequence[int] = range(8)) -> torch.Tensor:
    """The "+" of SwinIR+ / HAT+ / DAT+: the mean over `ops` of T_k^-1(model(T_k(x))), passes in the given order.

    On the device every pass costs two transform launches; the 1/len(ops) scaling and the sum are folded into the inverse transform
    (accumulate).  In the natural order 0..7 the four untransposed passes come first, so a non-square input changes the shape the
    model sees once.  CPU tensors take `apply_op_host`."""
    ks = [_check_op(k) for k in ops]
    if not ks:
        raise ValueError("self_ensemble needs at least one op")
    w = 1.0 / len(ks)
    acc = None
    with torch.no_grad():
        for k in ks:
            if x.is_cuda:
                y = model(dihedral(x.float().contiguous(), k)).float().contiguous()
                if acc is None:
                    acc = dihedral(y, inverse_op(k), alpha=w)
                else:
                    dihedral(y, inverse_op(k), out=acc, alpha=w, accumulate=True)
            else:
                y = apply_op_host(model(apply_op_host(x, k)), inverse_op(k)) * w
                acc = y if acc is None else acc + y
    return acc
