"""Thin torch wrappers over the building-block entry points of libsrk.so.

Tensors must live on the GPU ("cuda" == ROCm/HIP device in PyTorch-ROCm) and be contiguous; every
call is enqueued on the current torch stream.  Nothing here computes on the CPU: a CPU tensor or a
missing library raises.  This file holds the transformer building blocks, metrics, optimizer steps and
losses; the image ops of the data path live in image_ops.py and are re-exported here.
"""
from __future__ import annotations

import ctypes as C
import numbers
from typing import Optional, Tuple

import threading

import torch

from . import _lib
from ._lib import WinGeom, _p, _stream, check, lib
from .image_ops import *          # noqa: F401,F403  the image ops of the data path (image_ops.__all__): `ops.<name>` is their public spelling


def _geom(H: int, W: int, shift: int):
    return C.byref(WinGeom(H, W, shift))


# ---------------------------------------------------------------------------------------------------
# bit-exact index ops
# ---------------------------------------------------------------------------------------------------
def window_partition(x: torch.Tensor, window_size: int) -> torch.Tensor:
    """reference window_partition (network_swinir.py:33-45): (B,H,W,C) -> (B*nW, ws, ws, C)."""
    B, H, W, Cc = x.shape
    x = x.contiguous()
    out = torch.empty((B * (H // window_size) * (W // window_size), window_size, window_size, Cc), dtype=x.dtype, device=x.device)
    check(lib().srk_window_partition(_p(x), _p(out), B, H, W, Cc, window_size, x.element_size(), _stream()))
    return out


def window_reverse(windows: torch.Tensor, window_size: int, H: int, W: int) -> torch.Tensor:
    """reference window_reverse (network_swinir.py:48-62): (B*nW, ws, ws, C) -> (B,H,W,C)."""
    B = int(windows.shape[0] / (H * W / window_size / window_size))
    Cc = windows.shape[-1]
    windows = windows.contiguous()
    out = torch.empty((B, H, W, Cc), dtype=windows.dtype, device=windows.device)
    check(lib().srk_window_reverse(_p(windows), _p(out), B, H, W, Cc, window_size, windows.element_size(), _stream()))
    return out


def roll2d(x: torch.Tensor, shifts: Tuple[int, int]) -> torch.Tensor:
    """torch.roll(x, shifts, dims=(1, 2)) on (B,H,W,C)."""
    B, H, W, Cc = x.shape
    x = x.contiguous()
    out = torch.empty_like(x)
    check(lib().srk_roll2d(_p(x), _p(out), B, H, W, Cc, int(shifts[0]), int(shifts[1]), x.element_size(), _stream()))
    return out


def pixel_shuffle(x: torch.Tensor, r: int) -> torch.Tensor:
    B, Crr, H, W = x.shape
    Cc = Crr // (r * r)
    x = x.contiguous()
    out = torch.empty((B, Cc, H * r, W * r), dtype=x.dtype, device=x.device)
    check(lib().srk_pixel_shuffle(_p(x), _p(out), B, Cc, H, W, r, x.element_size(), _stream()))
    return out


def shift_mask(H: int, W: int, window_size: int, shift: int, device="cuda") -> torch.Tensor:
    N = window_size * window_size
    out = torch.empty(((H // window_size) * (W // window_size), N, N), dtype=torch.float32, device=device)
    check(lib().srk_shift_mask(_p(out), H, W, window_size, shift, _stream()))
    return out


def relative_position_index(window_size: int, device="cuda") -> torch.Tensor:
    N = window_size * window_size
    out = torch.empty((N, N), dtype=torch.int64, device=device)
    check(lib().srk_relative_position_index(_p(out), window_size, _stream()))
    return out


# ---------------------------------------------------------------------------------------------------
# building blocks in the kernels' internal (padded) layouts
# ---------------------------------------------------------------------------------------------------
def layernorm_fwd(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, C_real: int, *, geom=None,
                  out_bf16: bool = True, out_f32: bool = False):
    """x fp32 [rows, CP] -> (y_bf16 | None, y_f32 | None, mean, rstd).  geom=(H, W, shift) -> window order."""
    rows, CP = x.shape
    yb = torch.empty((rows, CP), dtype=torch.bfloat16, device=x.device) if out_bf16 else None
    yf = torch.empty((rows, CP), dtype=torch.float32, device=x.device) if out_f32 else None
    mean = torch.empty(rows, dtype=torch.float32, device=x.device)
    rstd = torch.empty(rows, dtype=torch.float32, device=x.device)
    g = _geom(*geom) if geom is not None else None
    check(lib().srk_layernorm_fwd(_p(x), _p(gamma), _p(beta), _p(yb), _p(yf), _p(mean), _p(rstd), rows, C_real, CP, g, _stream()))
    return yb, yf, mean, rstd


def window_attention_fwd(qkv: torch.Tensor, bias_dense: torch.Tensor, H: int, W: int, shift: int) -> torch.Tensor:
    """qkv bf16 [3, B_, nH, 64, 32]; bias_dense fp32 [nH, 64, 64] -> out bf16 [B_*64, nH*32]."""
    _, B_, nH, N, D = qkv.shape
    assert N == 64 and D == 32
    out = torch.empty((B_ * 64, nH * 32), dtype=torch.bfloat16, device=qkv.device)
    check(lib().srk_window_attention_fwd(_p(qkv), _p(bias_dense), _p(out), B_, nH, _geom(H, W, shift), _stream()))
    return out


def window_attention_bwd(qkv: torch.Tensor, bias_dense: torch.Tensor, d_out: torch.Tensor, scale: float, H: int, W: int,
                         shift: int):
    """-> (d_qkv bf16 [B_*64, 3*nH*32], d_table fp32 [225, nH])."""
    _, B_, nH, _, _ = qkv.shape
    d_qkv = torch.empty((B_ * 64, 3 * nH * 32), dtype=torch.bfloat16, device=qkv.device)
    d_table = torch.zeros((225, nH), dtype=torch.float32, device=qkv.device)
    slab = torch.empty(lib().srk_window_attention_bwd_scratch(B_, nH), dtype=torch.uint8, device=qkv.device)
    check(lib().srk_window_attention_bwd(_p(qkv), _p(bias_dense), _p(d_out), _p(d_qkv), _p(d_table), _p(slab), B_, nH,
                                         float(scale), _geom(H, W, shift), _stream()))
    return d_qkv, d_table


def window_attention_bwd_fused(xn: torch.Tensor, w_qkv: torch.Tensor, b_qkv: Optional[torch.Tensor], scale: float, d_x1: torch.Tensor,
                               w_proj_t: torch.Tensor, bias_dense: torch.Tensor, H: int, W: int, shift: int):
    """Attention backward with q/k/v re-projected from xn and the output-projection dgrad folded in (classical width).
    xn, d_x1 bf16 [B_*64, 192] window order; w_qkv bf16 [576, 192]; w_proj_t bf16 [192, 192]
    -> (d_qkv bf16 [B_*64, 576], d_table fp32 [225, 6])."""
    B_ = xn.shape[0] // 64
    nH = bias_dense.shape[0]
    d_qkv = torch.empty((B_ * 64, 3 * nH * 32), dtype=torch.bfloat16, device=xn.device)
    d_table = torch.zeros((225, nH), dtype=torch.float32, device=xn.device)
    slab = torch.empty(max(16, lib().srk_window_attention_bwd_fused_scratch(B_, nH)), dtype=torch.uint8, device=xn.device)
    check(lib().srk_window_attention_bwd_fused(_p(xn), xn.stride(0), _p(w_qkv), _p(b_qkv), float(scale), _p(d_x1), d_x1.stride(0),
                                               _p(w_proj_t), _p(bias_dense), _p(d_qkv), _p(d_table), _p(slab), B_, nH,
                                               _geom(H, W, shift), _stream()))
    return d_qkv, d_table


def window_attention_small_fwd(qkv: torch.Tensor, table: torch.Tensor, B: int, H: int, W: int, window_size: int, shift: int,
                               num_heads: int, scale: float) -> torch.Tensor:
    """(Shifted-)window attention for ws x ws windows, 2 <= ws <= 7, in raster token order.  qkv bf16 [B*H*W, 3*CA] (q | k | v at
    columns 0 / CA / 2 CA, head h at +32 h, head_dim zero-padded to 32, q not scaled); table = relative_position_bias_table fp32
    [(2 ws - 1)^2, num_heads] -> out bf16 [B*H*W, num_heads*32]."""
    T, ldq = qkv.shape
    if T != B * H * W or ldq % 3 or qkv.dtype != torch.bfloat16:
        raise ValueError(f"qkv must be bf16 [B*H*W = {B * H * W}, 3*CA], got {qkv.dtype} {tuple(qkv.shape)}")
    if 2 <= window_size <= 7 and (table.dtype != torch.float32 or tuple(table.shape) != ((2 * window_size - 1) ** 2, num_heads)):
        raise ValueError(f"table must be fp32 [{(2 * window_size - 1) ** 2}, {num_heads}], got {table.dtype} {tuple(table.shape)}")
    out = torch.empty((T, num_heads * 32), dtype=torch.bfloat16, device=qkv.device)
    check(lib().srk_win_small_attention_fwd(_p(qkv), ldq, ldq // 3, _p(table), _p(out), num_heads * 32, B, H, W, window_size, shift,
                                            num_heads, float(scale), _stream()))
    return out


def window_attention_small_bwd(qkv: torch.Tensor, table: torch.Tensor, d_out: torch.Tensor, B: int, H: int, W: int, window_size: int,
                               shift: int, num_heads: int, scale: float, d_table: Optional[torch.Tensor] = None):
    """Gradient of window_attention_small_fwd.  qkv, table as the forward took them; d_out bf16 [B*H*W, num_heads*32]
    -> (d_qkv bf16 [B*H*W, 3*CA], written in full; d_table fp32 [(2 ws - 1)^2, num_heads]).  A d_table that is passed in is
    ACCUMULATED into, otherwise a zeroed one is made."""
    T, ldq = qkv.shape
    if T != B * H * W or ldq % 3 or qkv.dtype != torch.bfloat16:
        raise ValueError(f"qkv must be bf16 [B*H*W = {B * H * W}, 3*CA], got {qkv.dtype} {tuple(qkv.shape)}")
    if d_out.dtype != torch.bfloat16 or d_out.dim() != 2 or d_out.shape[0] != T or d_out.shape[1] < num_heads * 32:
        raise ValueError(f"d_out must be bf16 [{T}, >= {num_heads * 32}], got {d_out.dtype} {tuple(d_out.shape)}")
    if 2 <= window_size <= 7:
        want = ((2 * window_size - 1) ** 2, num_heads)
        for name, t in (("table", table), ("d_table", d_table)):
            if t is not None and (t.dtype != torch.float32 or tuple(t.shape) != want):
                raise ValueError(f"{name} must be fp32 {list(want)}, got {t.dtype} {tuple(t.shape)}")
    d_qkv = torch.empty((T, ldq), dtype=torch.bfloat16, device=qkv.device)
    if d_table is None:
        d_table = torch.zeros_like(table)
    scratch = torch.empty(max(16, int(lib().srk_win_small_attention_bwd_scratch(B, H, W, window_size, num_heads))), dtype=torch.uint8,
                          device=qkv.device)
    check(lib().srk_win_small_attention_bwd(_p(qkv), ldq, ldq // 3, _p(table), _p(d_out), d_out.shape[1], _p(d_qkv), _p(d_table),
                                            _p(scratch), B, H, W, window_size, shift, num_heads, float(scale), _stream()))
    return d_qkv, d_table


def rel_pos_bias_expand(table: torch.Tensor) -> torch.Tensor:
    nH = table.shape[1]
    out = torch.empty((nH, 64, 64), dtype=torch.float32, device=table.device)
    check(lib().srk_rel_pos_bias_expand(_p(table), _p(out), nH, _stream()))
    return out


def linear_bf16(a: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor]) -> torch.Tensor:
    M, K = a.shape
    N = w.shape[0]
    y = torch.empty((M, N), dtype=torch.bfloat16, device=a.device)
    check(lib().srk_linear_bf16(_p(a), _p(w), _p(bias), _p(y), M, N, K, _stream()))
    return y


_WGRAD_WS = {}


def _bind_wgrad_workspace(device: torch.device) -> None:
    """Register this thread's weight-gradient workspace (a cached torch tensor: the caller owns the memory, the library never
    allocates) so that the stand-alone wgrad entry points reduce their row-splits in a fixed order."""
    key = (device.index if device.index is not None else torch.cuda.current_device())
    ws = _WGRAD_WS.get(key)
    if ws is None:
        ws = _WGRAD_WS[key] = torch.empty(int(lib().srk_wgrad_workspace_bytes()), dtype=torch.uint8, device=device)
    check(lib().srk_set_wgrad_workspace(_p(ws), ws.numel()))


def linear_wgrad_bf16(y: torch.Tensor, x: torch.Tensor, with_bias: bool = True):
    M, N = y.shape
    K = x.shape[1]
    dw = torch.zeros((N, K), dtype=torch.float32, device=y.device)
    db = torch.zeros((N,), dtype=torch.float32, device=y.device) if with_bias else None
    _bind_wgrad_workspace(y.device)
    check(lib().srk_linear_wgrad_bf16(_p(y), _p(x), _p(dw), _p(db), M, N, K, _stream()))
    return dw, db


class ZeroArena:
    """Zero-initialised fp32 accumulators of one backward pass carved out of ONE buffer that a single fill clears.  A HAT / DAT backward
    needs ~20 small zeroed tensors per block (weight / bias / LayerNorm gradient accumulators): as separate torch.zeros they are ~750
    fill launches of ~2.7 us each per step.  The arena learns its size in the first pass (requests beyond the buffer fall back to
    torch.zeros) and serves the following passes from one allocation; every piece starts on a 256-byte boundary."""

    def __init__(self):
        self.need = 0            # floats requested in the last pass
        self.buf = None
        self.off = 0

    def begin(self, device) -> None:
        want = max(self.need, self.off)
        self.need = want
        self.buf = torch.zeros(want, dtype=torch.float32, device=device) if want > 0 else None     # a fresh buffer per pass: the previous
        self.off = 0                                                                              # pass's gradients may still be referenced

    def zeros(self, shape, device) -> torch.Tensor:
        shape = tuple(shape) if not isinstance(shape, int) else (shape,)
        n = 1
        for d in shape:
            n *= int(d)
        n_al = (n + 63) // 64 * 64
        o = self.off
        self.off += n_al
        if self.buf is not None and self.buf.device == device and o + n_al <= self.buf.numel():
            return self.buf[o:o + n].view(shape)
        return torch.zeros(shape, dtype=torch.float32, device=device)


_ARENA = threading.local()


def zeros_f32(shape, device) -> torch.Tensor:
    """fp32 zeros from the backward pass's arena when one is active on this thread (arena_scope), else torch.zeros"""
    ar = getattr(_ARENA, "cur", None)
    if ar is None:
        return torch.zeros(shape, dtype=torch.float32, device=device)
    return ar.zeros(shape, device)


class arena_scope:
    """with arena_scope(arena, device): ...   -- zeros_f32 inside the block come from `arena` (not re-entrant across threads)"""

    def __init__(self, arena: "ZeroArena", device):
        self.arena, self.device = arena, device

    def __enter__(self):
        self.prev = getattr(_ARENA, "cur", None)
        self.arena.begin(self.device)
        _ARENA.cur = self.arena
        return self.arena

    def __exit__(self, *exc):
        _ARENA.cur = self.prev
        self.arena.need = max(self.arena.need, self.arena.off)
        return False


def linear_wgrad_multi_bf16(pairs):
    """pairs: up to four (y [M][N] bf16, x [M][K] bf16) with the same M (row-major, contiguous or column slices of contiguous rows) ->
    [(dw [N][K], db [N])] from ONE launch (include/srk.h: srk_linear_wgrad_multi_bf16)."""
    from ._lib import WgradProblem
    assert 1 <= len(pairs) <= 4
    M = pairs[0][0].shape[0]
    dev = pairs[0][0].device
    arr = (WgradProblem * len(pairs))()
    outs = []
    for i, (y, x) in enumerate(pairs):
        assert y.shape[0] == M and x.shape[0] == M and y.stride(1) == 1 and x.stride(1) == 1
        N, K = y.shape[1], x.shape[1]
        dw = zeros_f32((N, K), dev)
        db = zeros_f32((N,), dev)
        arr[i].y, arr[i].ldy, arr[i].x, arr[i].ldx = y.data_ptr(), y.stride(0), x.data_ptr(), x.stride(0)
        arr[i].dw, arr[i].db, arr[i].N, arr[i].K = dw.data_ptr(), db.data_ptr(), N, K
        outs.append((dw, db))
    _bind_wgrad_workspace(dev)
    check(lib().srk_linear_wgrad_multi_bf16(arr, len(pairs), M, _stream()))
    return outs


def conv3x3_bf16(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor]) -> torch.Tensor:
    """x bf16 NHWC [B,H,W,CinP], w bf16 [N, 9*CinP] (tap-major) -> y bf16 NHWC [B,H,W,N]."""
    B, H, W, CinP = x.shape
    N = w.shape[0]
    y = torch.empty((B, H, W, N), dtype=torch.bfloat16, device=x.device)
    check(lib().srk_conv3x3_bf16(_p(x), _p(w), _p(bias), _p(y), B, H, W, CinP, N, _stream()))
    return y


def conv3x3_wgrad_bf16(dy: torch.Tensor, x: torch.Tensor):
    B, H, W, N = dy.shape
    CinP = x.shape[-1]
    dw = torch.zeros((N, 9 * CinP), dtype=torch.float32, device=x.device)
    db = torch.zeros((N,), dtype=torch.float32, device=x.device)
    _bind_wgrad_workspace(x.device)
    check(lib().srk_conv3x3_wgrad_bf16(_p(dy), _p(x), _p(dw), _p(db), B, H, W, CinP, N, _stream()))
    return dw, db


def probe_trread(tile: torch.Tensor) -> torch.Tensor:
    """tile int16 [64,16] -> fragments int16 [64 lanes, 8]; expected[l, j] = tile[8*(l>>4)+j, l&15]."""
    out = torch.empty((64, 8), dtype=torch.int16, device=tile.device)
    check(lib().srk_probe_trread(_p(tile), _p(out), _stream()))
    return out


def batch_psnr(pred: torch.Tensor, target: torch.Tensor, max_val: float = 1.0, psnr_sum: Optional[torch.Tensor] = None,
               abs_sum: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Per-image PSNR [B] of fp32 [B, ...] images (finetune_swinir.py:69-74) in one fused pass; optionally ACCUMULATES the
    batch's PSNR sum and sum |pred - target| into the given fp32 scalars (validation loop without per-batch host syncs)."""
    assert pred.shape == target.shape and pred.dtype == torch.float32 and target.dtype == torch.float32
    pred, target = pred.contiguous(), target.contiguous()
    B = pred.shape[0]
    per_image = pred.numel() // B
    ws = torch.empty(int(lib().srk_batch_psnr_workspace(per_image, B)), dtype=torch.uint8, device=pred.device)
    out = torch.empty(B, dtype=torch.float32, device=pred.device)
    check(lib().srk_batch_psnr(_p(pred), _p(target), _p(ws), B, per_image, float(max_val), _p(out), _p(psnr_sum), _p(abs_sum), _stream()))
    return out


def eval_psnr(x: torch.Tensor, y: torch.Tensor, max_val: float = 1.0):
    """evaluate.py:24-29 on the device -> (per-image PSNR [B], batch mean [1]) without a host sync."""
    assert x.shape == y.shape and x.dtype == torch.float32 and y.dtype == torch.float32
    x, y = x.contiguous(), y.contiguous()
    B = x.shape[0]
    per_image = x.numel() // B
    ws = torch.empty(int(lib().srk_eval_psnr_workspace(per_image, B)), dtype=torch.uint8, device=x.device)
    per, mean = torch.empty(B, dtype=torch.float32, device=x.device), torch.empty(1, dtype=torch.float32, device=x.device)
    check(lib().srk_eval_psnr(_p(x), _p(y), _p(ws), B, per_image, float(max_val), _p(per), _p(mean), _stream()))
    return per, mean


def ssim(x: torch.Tensor, y: torch.Tensor, data_range: float = 1.0):
    """pytorch_msssim.ssim semantics on the device (csrc/metrics.hip; restated, parity unpinned) -> (per-image [B], batch mean [1])."""
    assert x.shape == y.shape and x.ndim == 4 and x.dtype == torch.float32 and y.dtype == torch.float32
    x, y = x.contiguous(), y.contiguous()
    B, Cc, H, W = x.shape
    ws = torch.empty(max(4, int(lib().srk_ssim_workspace(B, Cc, H, W))), dtype=torch.uint8, device=x.device)
    per, mean = torch.empty(B, dtype=torch.float32, device=x.device), torch.empty(1, dtype=torch.float32, device=x.device)
    check(lib().srk_ssim(_p(x), _p(y), _p(ws), B, Cc, H, W, float(data_range), _p(per), _p(mean), _stream()))
    return per, mean


BENCH_MODES = {"y": 0, "rgb": 1}          # SRK_BENCH_Y, SRK_BENCH_RGB


def bench_plane_shape(shape, border: int, mode: str) -> Tuple[int, int, int, int]:
    """[B, C, H, W] -> the [B, Cm, Hc, Wc] of the benchmark-protocol planes; ValueError for what srk_bench_planes_f32 refuses."""
    if mode not in BENCH_MODES:
        raise ValueError(f"bench metric: mode must be 'y' or 'rgb' (got {mode!r})")
    if len(shape) != 4:
        raise ValueError(f"bench metric: images must be [B, C, H, W] (got {tuple(shape)})")
    B, Cc, H, W = (int(v) for v in shape)
    if isinstance(border, bool) or not isinstance(border, numbers.Integral) or border < 0:
        raise ValueError(f"bench metric: crop border must be an integer >= 0 (got {border!r})")
    if min(B, Cc, H, W) < 1 or B > 1024:
        raise ValueError(f"bench metric: needs 1 <= B <= 1024 and non-empty images (got {tuple(shape)})")
    if 2 * border >= H or 2 * border >= W:
        raise ValueError(f"bench metric: a border of {border} leaves nothing of {H} x {W} images")
    if mode == "y" and Cc not in (1, 3):
        raise ValueError(f"bench metric: mode 'y' takes RGB (C = 3) or single-channel (C = 1) images (got C = {Cc})")
    return B, (1 if mode == "y" else Cc), H - 2 * int(border), W - 2 * int(border)


def bench_planes(pred: torch.Tensor, target: torch.Tensor, border: int, mode: str = "y", planes: bool = True):
    """The benchmark-protocol planes of fp32 [B, C, H, W] images (include/srk.h, DESIGN 7m: clamp, round to 8 bits, crop `border`,
    BT.601 luma for mode 'y') -> (planes of pred, planes of target: fp32 [B, Cm, Hc, Wc], or None each with planes=False,
    workspace fp32 [B, chunks] with the partial sums of their squared differences for bench_psnr).  One pass, no host read."""
    if pred.shape != target.shape or pred.dtype != torch.float32 or target.dtype != torch.float32:
        raise ValueError(f"bench metric: pred / target must be fp32 of one shape (got {pred.dtype} {tuple(pred.shape)}, "
                         f"{target.dtype} {tuple(target.shape)})")
    B, Cm, Hc, Wc = bench_plane_shape(pred.shape, border, mode)
    pred, target = pred.contiguous(), target.contiguous()
    ws = torch.empty((B, int(lib().srk_bench_workspace(B, Cm, Hc, Wc)) // (4 * B)), dtype=torch.float32, device=pred.device)
    pp = torch.empty((B, Cm, Hc, Wc), dtype=torch.float32, device=pred.device) if planes else None
    pt = torch.empty((B, Cm, Hc, Wc), dtype=torch.float32, device=pred.device) if planes else None
    check(lib().srk_bench_planes_f32(_p(pred), _p(target), _p(pp), _p(pt), _p(ws), B, pred.shape[1], pred.shape[2], pred.shape[3],
                                     int(border), BENCH_MODES[mode], _stream()))
    return pp, pt, ws


def bench_psnr(ws: torch.Tensor, plane_shape, psnr_sum: Optional[torch.Tensor] = None):
    """Finishes bench_planes' workspace for planes of plane_shape = (B, Cm, Hc, Wc) -> (sum of squared plane differences [B],
    PSNR on the 0..255 scale [B]; +inf for equal planes); ACCUMULATES the batch's PSNR sum into the fp32 scalar psnr_sum when given."""
    B, Cm, Hc, Wc = (int(v) for v in plane_shape)
    if min(B, Cm, Hc, Wc) < 1 or B > 1024:
        raise ValueError(f"bench metric: needs 1 <= B <= 1024 and non-empty planes (got {tuple(plane_shape)})")
    if ws.dtype != torch.float32 or ws.numel() * 4 != int(lib().srk_bench_workspace(B, Cm, Hc, Wc)):
        raise ValueError(f"bench metric: the workspace does not belong to planes of {(B, Cm, Hc, Wc)}")
    if psnr_sum is not None and (psnr_sum.dtype != torch.float32 or psnr_sum.numel() != 1):
        raise ValueError("bench metric: psnr_sum must be one fp32 scalar")
    sq, ps = torch.empty(B, dtype=torch.float32, device=ws.device), torch.empty(B, dtype=torch.float32, device=ws.device)
    check(lib().srk_bench_psnr(_p(ws), B, Cm, Hc, Wc, _p(sq), _p(ps), _p(psnr_sum), _stream()))
    return sq, ps


def psnrb_planes(planes_pred: torch.Tensor, planes_target: torch.Tensor):
    """PSNR-B of benchmark-protocol planes (include/srk.h "Full-reference scores"; csrc/fullref.hip): fp32 [B, Cm, Hc, Wc]
    planes of the restored image and of the target, Hc, Wc >= 16 -> (sums fp32 [B, Cm, 5] = squared error, Dh_b, Dh_n, Dv_b, Dv_n;
    psnrb fp32 [B]).  Restated from the published algorithm, parity unpinned."""
    if (planes_pred.shape != planes_target.shape or planes_pred.ndim != 4 or planes_pred.dtype != torch.float32
            or planes_target.dtype != torch.float32):
        raise ValueError(f"psnrb: planes must be fp32 [B, Cm, Hc, Wc] of one shape (got {planes_pred.dtype} {tuple(planes_pred.shape)}, "
                         f"{planes_target.dtype} {tuple(planes_target.shape)})")
    pp, pt = planes_pred.contiguous(), planes_target.contiguous()
    B, Cm, Hc, Wc = pp.shape
    ws = torch.empty(max(4, int(lib().srk_psnrb_workspace(B, Cm, Hc, Wc))), dtype=torch.uint8, device=pp.device)
    sums = torch.empty((B, Cm, 5), dtype=torch.float32, device=pp.device)
    out = torch.empty(B, dtype=torch.float32, device=pp.device)
    check(lib().srk_psnrb(_p(pp), _p(pt), _p(ws), B, Cm, Hc, Wc, _p(sums), _p(out), _stream()))
    return sums, out


def msssim_means(x: torch.Tensor, y: torch.Tensor, levels: int = 5, data_range: float = 255.0) -> torch.Tensor:
    """The per-level means of MS-SSIM (include/srk.h "Full-reference scores"; csrc/fullref.hip): fp32 [B, C, H, W] images ->
    fp32 [levels, B, C, 2] = (mean of the SSIM map, mean of its contrast-structure factor) on the 2 x 2-pooled pyramid; one launch per
    level and one to finish, no host read.  Restated from the published algorithm, parity unpinned."""
    if x.shape != y.shape or x.ndim != 4 or x.dtype != torch.float32 or y.dtype != torch.float32:
        raise ValueError(f"msssim: images must be fp32 [B, C, H, W] of one shape (got {x.dtype} {tuple(x.shape)}, {y.dtype} {tuple(y.shape)})")
    x, y = x.contiguous(), y.contiguous()
    B, Cc, H, W = x.shape
    ws = torch.empty(max(4, int(lib().srk_msssim_workspace(B, Cc, H, W, int(levels)))), dtype=torch.uint8, device=x.device)
    means = torch.empty((int(levels), B, Cc, 2), dtype=torch.float32, device=x.device)
    check(lib().srk_msssim(_p(x), _p(y), _p(ws), B, Cc, H, W, int(levels), float(data_range), _p(means), _stream()))
    return means


class TensorTable:
    """Host table of a list of fp32 device tensors for the multi-tensor kernels (srk_multi_*): one ctypes array of data pointers per
    role plus the element counts.  Only pointers are kept; the caller keeps the tensors alive until the launches have run."""

    def __init__(self, n: int):
        self.n = int(n)
        self.numel = (C.c_int64 * self.n)()
        self.ptrs = {}

    def set(self, role: str, tensors, first: bool = False) -> None:
        """first=True also records the element counts; every later role must match them."""
        if len(tensors) != self.n:
            raise ValueError(f"multi-tensor optimizer: {len(tensors)} {role} tensors for a table of {self.n}")
        arr = self.ptrs.get(role)
        if arr is None:
            arr = self.ptrs[role] = (C.c_void_p * self.n)()
        cur, numel, f32 = None, self.numel, torch.float32
        for i, t in enumerate(tensors):
            if t.dtype is not f32:
                raise TypeError(f"multi-tensor optimizer: {role}[{i}] must be float32 (got {t.dtype})")
            if cur is None and t.is_cuda:
                cur = torch.cuda.current_device()
            if not t.is_cuda or t.device.index != cur or not t.is_contiguous():
                _p(t)          # raises with the reason (CPU tensor, another device, not contiguous)
            arr[i] = t.data_ptr()
            if first:
                numel[i] = t.numel()
            elif t.numel() != numel[i]:
                raise ValueError(f"multi-tensor optimizer: {role}[{i}] has {t.numel()} elements, expected {numel[i]}")


def multi_grad_sumsq(table: TensorTable, sumsq: torch.Tensor, role: str = "grads") -> None:
    """sumsq[0] += sum over the table's tensors of sum(g * g); ceil(n / 160) launches, capturable."""
    check(lib().srk_multi_grad_sumsq(table.ptrs[role], table.numel, table.n, _p(sumsq), _stream()))


def _ema_decay(ema_decay) -> Optional[float]:
    """None / 0 -> None (EMA off); a decay in (0, 1) as a float; anything else raises."""
    if ema_decay is None:
        return None
    d = float(ema_decay)
    if not 0.0 <= d < 1.0:          # also refuses NaN
        raise ValueError(f"ema_decay must be in [0, 1) (got {ema_decay!r})")
    return d or None


def multi_adamw_clip_step(table: TensorTable, sumsq: Optional[torch.Tensor], max_norm: float, grad_div: float, lr: float, beta1: float,
                          beta2: float, eps: float, weight_decay: float, step: int, hyper: Optional[torch.Tensor] = None,
                          nonfinite: Optional[torch.Tensor] = None, ema_decay: Optional[float] = None) -> None:
    """clip + AdamW over the table's params / grads / exp_avg / exp_avg_sq (srk_multi_adamw_clip_step); ceil(n / 80) launches,
    capturable.  hyper: optional device {lr, bc1, bc2_sqrt} (adamw_hyper) that replaces `lr` and `step`.
    ema_decay (not None): srk_multi_adamw_clip_ema_step, which also advances the table's "ema" tensors toward the new weights;
    ceil(n / 72) launches.  The decay is a launch-time constant."""
    pt = table.ptrs
    if ema_decay is None:
        check(lib().srk_multi_adamw_clip_step(pt["params"], pt["grads"], pt["exp_avg"], pt["exp_avg_sq"], table.numel, table.n,
                                              _p(sumsq), float(max_norm), float(grad_div), float(lr), float(beta1), float(beta2),
                                              float(eps), float(weight_decay), int(step), _p(hyper), _p(nonfinite), _stream()))
        return
    check(lib().srk_multi_adamw_clip_ema_step(pt["params"], pt["grads"], pt["exp_avg"], pt["exp_avg_sq"], pt["ema"], table.numel, table.n,
                                              _p(sumsq), float(max_norm), float(grad_div), float(lr), float(beta1), float(beta2),
                                              float(eps), float(weight_decay), int(step), float(ema_decay), _p(hyper), _p(nonfinite),
                                              _stream()))


def adamw_clip_step(params: torch.Tensor, grads: torch.Tensor, exp_avg: torch.Tensor, exp_avg_sq: torch.Tensor,
                    sumsq: Optional[torch.Tensor], max_norm: float, grad_div: float, lr: float, beta1: float, beta2: float, eps: float,
                    weight_decay: float, step: int, nonfinite: Optional[torch.Tensor] = None, ema: Optional[torch.Tensor] = None,
                    ema_decay: Optional[float] = None, offset: int = 0, numel: Optional[int] = None) -> None:
    """The flat counterpart: clip + AdamW over elements [offset, offset + numel) of contiguous fp32 buffers (srk_adamw_clip_step), or,
    with `ema` and `ema_decay`, srk_adamw_clip_ema_step, which also advances the same range of `ema`."""
    n = params.numel() - offset if numel is None else int(numel)
    if offset < 0 or n < 0 or offset + n > params.numel():
        raise ValueError(f"adamw_clip_step: range [{offset}, {offset + n}) outside a buffer of {params.numel()} elements")
    bufs = [params, grads, exp_avg, exp_avg_sq] + ([ema] if ema_decay is not None else [])
    for t in bufs:
        if t is None or t.dtype is not torch.float32 or t.numel() != params.numel():
            raise ValueError("adamw_clip_step: params, grads, exp_avg, exp_avg_sq (and ema) must be float32 buffers of one size")
    at = [_p(t) + 4 * offset for t in bufs]
    tail = (_p(sumsq), float(max_norm), float(grad_div), float(lr), float(beta1), float(beta2), float(eps), float(weight_decay), int(step))
    if ema_decay is None:
        check(lib().srk_adamw_clip_step(*at, n, *tail, _p(nonfinite), _stream()))
    else:
        check(lib().srk_adamw_clip_ema_step(*at, n, *tail, float(ema_decay), _p(nonfinite), _stream()))


def adamw_hyper(lr: float, beta1: float, beta2: float, step: int) -> Tuple[float, float, float]:
    """(lr, 1 - beta1^step, sqrt(1 - beta2^step)) exactly as the step kernels' launchers compute them (host only)."""
    out = (C.c_float * 3)()
    check(lib().srk_adamw_hyper(float(lr), float(beta1), float(beta2), int(step), C.byref(out)))
    return out[0], out[1], out[2]


def l1_loss_fwd_bwd(pred: torch.Tensor, target: torch.Tensor, want_grad: bool = True, grad_scale: float = 1.0):
    """-> (loss fp32 [1], d_pred | None, nonfinite int32 [1])   (finetune_swinir.py:66-67, :133-143)."""
    loss = torch.zeros(1, dtype=torch.float32, device=pred.device)
    bad = torch.zeros(1, dtype=torch.int32, device=pred.device)
    d = torch.empty_like(pred) if want_grad else None
    check(lib().srk_l1_loss_fwd_bwd(_p(pred), _p(target), _p(d), _p(loss), _p(bad), pred.numel(), float(grad_scale), _stream()))
    return loss, d, bad


def pixel_loss_fwd_bwd(pred: torch.Tensor, target: torch.Tensor, kind: str = "l1", eps: float = 1e-3, want_grad: bool = True,
                       grad_scale: float = 1.0, d_pred: Optional[torch.Tensor] = None, accumulate: bool = False,
                       loss: Optional[torch.Tensor] = None, bad: Optional[torch.Tensor] = None):
    """mean |d| ('l1'), mean d^2 ('mse') or mean sqrt(d^2 + eps^2) ('charbonnier'), d = pred - target (csrc/loss.hip, fixed-order sums)
    -> (loss fp32 [1], d_pred | None, nonfinite int32 [1]).  `loss` / `bad` that are passed in are ACCUMULATED into; a `d_pred` that is
    passed in is overwritten, or added to with accumulate=True.  No host read: capturable."""
    if kind not in _lib.LOSS_KINDS:
        raise ValueError(f"pixel loss kind must be one of {sorted(_lib.LOSS_KINDS)} (got {kind!r})")
    if pred.shape != target.shape or pred.dtype != torch.float32 or target.dtype != torch.float32:
        raise ValueError(f"pixel loss: pred / target must be fp32 of one shape (got {pred.dtype} {tuple(pred.shape)}, "
                         f"{target.dtype} {tuple(target.shape)})")
    if loss is None:
        loss = torch.zeros(1, dtype=torch.float32, device=pred.device)
    if bad is None:
        bad = torch.zeros(1, dtype=torch.int32, device=pred.device)
    if d_pred is None and want_grad:
        if accumulate:
            raise ValueError("pixel loss: accumulate=True needs the d_pred to add to")
        d_pred = torch.empty_like(pred)
    n = pred.numel()
    ws = torch.empty(max(4, int(lib().srk_pixel_loss_workspace(n))), dtype=torch.uint8, device=pred.device)
    check(lib().srk_pixel_loss_fwd_bwd(_p(pred), _p(target), _p(d_pred), _p(loss), _p(bad), n, _lib.LOSS_KINDS[kind], float(eps),
                                       float(grad_scale), int(bool(accumulate)), _p(ws), _stream()))
    return loss, d_pred, bad


def ssim_loss_fwd_bwd(x: torch.Tensor, y: torch.Tensor, data_range: float = 1.0, alpha: float = 1.0, want_grad: bool = True,
                      d_x: Optional[torch.Tensor] = None, accumulate: bool = False, loss: Optional[torch.Tensor] = None):
    """The SSIM training term (csrc/loss.hip): S = ssim(x, y)'s batch mean -> (S fp32 [1], d_x | None, loss | None) with
    d_x = -alpha dS/dx (stored, or added to a given d_x with accumulate=True) and, when `loss` is given, loss[0] += alpha (1 - S).
    One fused kernel, fixed-order sums, no host read: capturable."""
    if x.shape != y.shape or x.ndim != 4 or x.dtype != torch.float32 or y.dtype != torch.float32:
        raise ValueError(f"ssim loss: x / y must be fp32 [B, C, H, W] of one shape (got {x.dtype} {tuple(x.shape)}, {y.dtype} {tuple(y.shape)})")
    B, Cc, H, W = x.shape
    if d_x is None and want_grad:
        if accumulate:
            raise ValueError("ssim loss: accumulate=True needs the d_x to add to")
        d_x = torch.empty_like(x)
    if d_x is not None and (d_x.shape != x.shape or d_x.dtype != torch.float32):
        raise ValueError(f"ssim loss: d_x must be fp32 {tuple(x.shape)} (got {d_x.dtype} {tuple(d_x.shape)})")
    ws = torch.empty(max(4, int(lib().srk_ssim_loss_workspace(B, Cc, H, W))), dtype=torch.uint8, device=x.device)
    mean = torch.empty(1, dtype=torch.float32, device=x.device)
    check(lib().srk_ssim_loss_fwd_bwd(_p(x), _p(y), _p(ws), B, Cc, H, W, float(data_range), float(alpha), _p(d_x), int(bool(accumulate)),
                                      _p(mean), _p(loss), _stream()))
    return mean, d_x, loss


def fft_loss_fwd_bwd(x: torch.Tensor, y: torch.Tensor, norm: str = "backward", alpha: float = 1.0, d_x: Optional[torch.Tensor] = None,
                     accumulate: bool = False, loss: Optional[torch.Tensor] = None, want_grad: bool = True):
    """The frequency loss (csrc/fft_loss.hip): L = mean(|Re D| + |Im D|) over the half spectrum D = rfft2(x - y, norm=norm), norm
    'backward' | 'ortho' -> (L fp32 [1], d_x | None, loss | None) with d_x = alpha dL/dx (stored, or added to a given d_x with
    accumulate=True; want_grad=False without a d_x: value only) and, when `loss` is given, loss[0] += alpha L.  H, W <= 512.
    Fixed-order sums, no host read: capturable."""
    if norm not in ("backward", "ortho"):
        raise ValueError(f"fft loss: norm must be 'backward' or 'ortho' (got {norm!r})")
    if x.shape != y.shape or x.ndim != 4 or x.dtype != torch.float32 or y.dtype != torch.float32:
        raise ValueError(f"fft loss: x / y must be fp32 [B, C, H, W] of one shape (got {x.dtype} {tuple(x.shape)}, {y.dtype} {tuple(y.shape)})")
    B, Cc, H, W = x.shape
    if d_x is None and want_grad:
        if accumulate:
            raise ValueError("fft loss: accumulate=True needs the d_x to add to")
        d_x = torch.empty_like(x)
    if d_x is not None and (d_x.shape != x.shape or d_x.dtype != torch.float32):
        raise ValueError(f"fft loss: d_x must be fp32 {tuple(x.shape)} (got {d_x.dtype} {tuple(d_x.shape)})")
    ws = torch.empty(max(4, int(lib().srk_fft_loss_workspace(B, Cc, H, W))), dtype=torch.uint8, device=x.device)
    value = torch.empty(1, dtype=torch.float32, device=x.device)
    check(lib().srk_fft_loss_fwd_bwd(_p(x), _p(y), _p(ws), B, Cc, H, W, int(norm == "ortho"), float(alpha), _p(d_x), int(bool(accumulate)),
                                     _p(value), _p(loss), _stream()))
    return value, d_x, loss
