"""Thin torch wrappers over the building-block entry points of libsrk.so.

Tensors must live on the GPU ("cuda" == ROCm/HIP device in PyTorch-ROCm) and be contiguous; every
call is enqueued on the current torch stream.  Nothing here computes on the CPU: a CPU tensor or a
missing library raises.
"""
from __future__ import annotations

import ctypes as C
import numbers
import struct
from typing import NamedTuple, Optional, Tuple

import threading

import torch

from . import _lib
from ._lib import WinGeom, check, lib


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _p(t: Optional[torch.Tensor]) -> Optional[int]:
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError("libsrk operates on GPU tensors only (got a CPU tensor); there is no CPU fallback")
    if t.device.index != torch.cuda.current_device():
        # the kernel would launch on the current device with another device's pointers (a GPU fault, not a Python error)
        raise RuntimeError(f"tensor on {t.device} but the current device is cuda:{torch.cuda.current_device()}; "
                           "libsrk ops launch on the current device (torch.cuda.set_device / one process per GPU)")
    if not t.is_contiguous():
        raise RuntimeError("libsrk needs contiguous tensors")
    return t.data_ptr()


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


def resize_aa(x: torch.Tensor, size, quant_bits: int = 0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Antialiased bicubic resize of a CUDA fp32 batch x [B,C,H,W] to size = (Ho, Wo), up or down (csrc/resize.hip,
    srk_resize_aa_f32): the Keys cubic with a = -0.5 in the convention of PIL's Image.BICUBIC and of
    F.interpolate(mode='bicubic', antialias=True, align_corners=False) -- fp64 weights rounded once to fp32, border taps dropped and
    renormalised, horizontal pass first.  quant_bits 8 rounds the result to k / 255 (what an 8-bit file of it would decode to);
    0 keeps the filtered values.  `out` must not alias `x`; it is allocated when absent.  One launch, no host read: capturable.
    An axis shrinking by more than 8x raises SrkUnsupported."""
    if x.dim() != 4 or x.dtype != torch.float32:
        raise ValueError(f"resize_aa takes fp32 [B,C,H,W] (got {x.dtype} {tuple(x.shape)})")
    try:
        Ho, Wo = (int(v) for v in size)
    except (TypeError, ValueError):
        raise ValueError(f"resize_aa: size must be (Ho, Wo) (got {size!r})") from None
    if Ho < 1 or Wo < 1 or min(x.shape) < 1:
        raise ValueError(f"resize_aa: every extent must be >= 1 (got {tuple(x.shape)} -> {(Ho, Wo)})")
    if quant_bits not in (0, 8):
        raise ValueError(f"resize_aa: quant_bits must be 0 or 8 (got {quant_bits!r})")
    B, Cc, H, W = x.shape
    shape = (B, Cc, Ho, Wo)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=x.device)
    elif tuple(out.shape) != shape or out.dtype != torch.float32 or out.device != x.device:
        raise ValueError(f"out must be fp32 {shape} on {x.device} (got {out.dtype} {tuple(out.shape)} on {out.device})")
    check(lib().srk_resize_aa_f32(_p(x), _p(out), B, Cc, H, W, Ho, Wo, int(quant_bits), _stream()))
    return out


def degrade_aa(hr: torch.Tensor, scale: int, quant_bits: int = 8) -> Tuple[torch.Tensor, torch.Tensor]:
    """(lr, hr_cropped) of `--synth_lr` validation / evaluation: hr [B,C,H,W] cropped to its top-left (H - H % s, W - W % s) region and
    that region's (H // s, W // s) antialiased bicubic downscale -- what DeviceHRPool's training patches are windows of."""
    H, W = hr.shape[-2:]
    s = int(scale)
    hr = hr[..., :H - H % s, :W - W % s].float().contiguous()
    return resize_aa(hr, (H // s, W // s), quant_bits), hr


BLUR_SIGMA_MAX = 2.5          # R = ceil(3 sigma) <= 8 taps on either side: what the 33-tap rows of csrc/resize.h hold at factors 2..4


def _f32_bits(v: float) -> int:
    return struct.unpack("<I", struct.pack("<f", v))[0]


def pack_degrade_params(blur, noise, noise_id: int, gray_noise: bool):
    """Slots 6..9 of a `srk_crop_degrade_blind_u8` descriptor / one row of `srk_degrade_blind_f32`'s table, as four signed 64-bit
    integers: fp32 bits of (sigma_y | sigma_x << 32), of (sigma_n | gain << 32), the noise id, the flags (bit 0 = gray noise).
    The one place that packs them; the ranges are checked here: sigmas in [0, 2.5] HR pixels, sigma_n and gain in [0, 1]."""
    (sy, sx), (sn, gain) = (float(v) for v in blur), (float(v) for v in noise)
    if not (0.0 <= sy <= BLUR_SIGMA_MAX and 0.0 <= sx <= BLUR_SIGMA_MAX):          # also refuses NaN
        raise ValueError(f"blur sigmas must be in [0, {BLUR_SIGMA_MAX}] HR pixels (got {(sy, sx)})")
    if not (0.0 <= sn <= 1.0 and 0.0 <= gain <= 1.0):
        raise ValueError(f"noise sigma and gain must be in [0, 1] (got {(sn, gain)})")
    noise_id = int(noise_id)
    if not -(1 << 63) <= noise_id < (1 << 64):
        raise ValueError(f"noise id must fit 64 bits (got {noise_id})")
    signed = lambda v: v - (1 << 64) if v >> 63 else v          # noqa: E731
    return [signed(_f32_bits(sy) | _f32_bits(sx) << 32), signed(_f32_bits(sn) | _f32_bits(gain) << 32),
            signed(noise_id & 0xFFFFFFFFFFFFFFFF), int(bool(gray_noise))]


def _per_sample(v, B: int, width: int, what: str):
    rows = [list(r) for r in v] if (len(v) and hasattr(v[0], "__len__")) else [list(v)] * B
    if len(rows) != B or any(len(r) != width for r in rows):
        raise ValueError(f"degrade_blind: {what} must be {width} numbers or one such row per sample (B={B}; got {v!r})")
    return rows


def degrade_blind(hr: torch.Tensor, scale: int, blur, noise, noise_ids, gray_noise=False, quant_bits: int = 8) -> Tuple[torch.Tensor, torch.Tensor]:
    """(lr, hr_cropped) like `degrade_aa`, with a Gaussian blur (sigma_y, sigma_x) in HR pixels composed into the bicubic tables and
    noise `v + sqrt(sigma_n^2 + gain max(v, 0)) z` added before the rounding (csrc/degrade.hip, srk_degrade_blind_f32): what
    DeviceHRPool's blind training patches are windows of.  blur = (sigma_y, sigma_x) and noise = (sigma_n, gain): one pair or one per
    sample; noise_ids: B integers (the Philox key; the same id and coordinates give the same draw); gray_noise: a bool or B of them --
    one draw for all channels (always so for C == 1).  hr [B,C,H,W] is cropped to a multiple of the factor (2..4).  One launch after one
    small upload; sigmas and amplitudes out of range raise ValueError."""
    if hr.dim() != 4 or not hr.is_cuda:
        raise ValueError(f"degrade_blind takes a CUDA [B,C,H,W] batch (got {tuple(hr.shape)} on {hr.device})")
    s = int(scale)
    if not 2 <= s <= 4:
        raise ValueError(f"degrade_blind: the factor must be in 2..4 (got {scale!r})")
    if quant_bits not in (0, 8):
        raise ValueError(f"degrade_blind: quant_bits must be 0 or 8 (got {quant_bits!r})")
    B, Cc, H, W = hr.shape
    if H < s or W < s or B < 1 or Cc < 1:
        raise ValueError(f"degrade_blind: {tuple(hr.shape)} is smaller than one output pixel at factor {s}")
    ids = [int(v) for v in noise_ids]
    grays = [bool(gray_noise)] * B if isinstance(gray_noise, (bool, int)) else [bool(v) for v in gray_noise]
    if len(ids) != B or len(grays) != B:
        raise ValueError(f"degrade_blind: one noise id and one gray flag per sample (B={B}; got {len(ids)} ids, {len(grays)} flags)")
    rows = [pack_degrade_params(b, n, i, g) for b, n, i, g in zip(_per_sample(blur, B, 2, "blur"), _per_sample(noise, B, 2, "noise"), ids, grays)]
    hr = hr[..., :H - H % s, :W - W % s].float().contiguous()
    par = torch.tensor(rows, dtype=torch.int64).to(hr.device)
    lr = torch.empty(B, Cc, H // s, W // s, dtype=torch.float32, device=hr.device)
    check(lib().srk_degrade_blind_f32(_p(hr), _p(lr), _p(par), B, Cc, H - H % s, W - W % s, s, int(quant_bits), _stream()))
    return lr, hr


def pack_psf(psf, B: int, checked: bool = False):
    """psf: one [ks][ks] table or B of them (a list of tables of different odd sizes, or an array [B][ks][ks]) -> (fp32 numpy
    [B][ks][ks], ks): every table checked by the host rule (blur_kernels.check_table) and zero-padded, centred, to the largest ks --
    which changes no bit of the result (include/srk.h "General 2-D blur").  checked: a list of fp32 tables that blur_kernels made or
    checked already (sr_datasets.PsfSpec's draws) is only padded."""
    from . import blur_kernels as bk
    import numpy as np
    if checked:
        ks = max(t.shape[0] for t in psf)
        out = np.zeros((len(psf), ks, ks), dtype=np.float32)
        for i, t in enumerate(psf):
            p = (ks - t.shape[0]) // 2
            out[i, p:p + t.shape[0], p:p + t.shape[0]] = t
        if len(psf) != B:
            raise ValueError(f"psf: one table per sample (B={B}; got {len(psf)})")
        return out, ks
    if isinstance(psf, torch.Tensor):
        psf = psf.detach().cpu().numpy()
    try:
        arr = np.asarray(psf, dtype=np.float32)
    except (ValueError, TypeError):          # tables of different sizes
        arr = None
    if arr is not None and arr.ndim == 2:
        tabs = [bk.check_table(arr)] * B
    else:
        tabs = [bk.check_table(t, f"psf[{i}]") for i, t in enumerate(psf if arr is None else arr)]
    if len(tabs) != B:
        raise ValueError(f"psf: one table or one per sample (B={B}; got {len(tabs)})")
    ks = max(t.shape[0] for t in tabs)
    return np.stack([bk.pad_to(t, ks) for t in tabs]), ks


class DeviceTables(NamedTuple):
    """Tables the device built (`kernel_tables`): `tab`, CUDA fp32 [n][ks][ks]; `ks`; `own`, the host list of the n sides before
    padding (what the radius-versus-extent checks run on: nothing is read back); `signed`: a sinc table is among them, so the batch
    goes through `filter2d` only."""
    tab: torch.Tensor
    ks: int
    own: Tuple[int, ...]
    signed: bool


def kernel_tables(descs, ks=None, bank=None, signed: bool = True, device=None) -> DeviceTables:
    """The tables of n `blur_kernels.TableDesc` built ON THE DEVICE (csrc/tables.hip, srk_kernel_tables_f32): one upload of n x 8
    doubles and one launch, in place of n fp64 numpy evaluations and an upload of n ks^2 floats.  ks: the side of the slots, by default
    the largest own side (smaller tables are centred in +0, `blur_kernels.pad_to`).  bank: the CUDA fp32 [n_bank][kb][kb] tables that
    kind-5 descriptors index (a numpy array is checked by `blur_kernels.check_table` and uploaded; keep the tensor to upload once).
    signed=False refuses sinc descriptors: what `blur2d` / `degrade_psf` need, whose mass rule has no negative taps.  Each tap is
    within one fp32 spacing of `TableDesc.table()`'s (tests/tables_ref.py derives the bound)."""
    from . import blur_kernels as bk
    ds = list(descs)
    if not ds or not all(isinstance(d, bk.TableDesc) for d in ds):
        raise ValueError(f"kernel_tables takes a non-empty list of blur_kernels.TableDesc (got {len(ds)} entries)")
    rows = [d.row() for d in ds]                                     # refuses what the table functions refuse
    for d in ds:                                                     # a NamedTuple built by hand gets the constructors' checks
        if d.kind == bk.KIND_SINC:
            bk.TableDesc.sinc(d.cutoff, d.ks)
        elif d.kind in (bk.KIND_GENERALIZED, bk.KIND_PLATEAU):
            bk._beta(d.beta)
    if not signed and any(d.kind == bk.KIND_SINC for d in ds):
        raise ValueError("kernel_tables(signed=False): a sinc table has negative taps (ops.filter2d takes it, ops.blur2d cannot)")
    own = tuple(d.ks for d in ds)
    ks = max(own) if ks is None else bk.check_ks(ks)
    if max(own) > ks:
        raise ValueError(f"kernel_tables: a table of side {max(own)} does not fit ks = {ks}")
    n_bank = kb = 0
    if bank is not None and isinstance(bank, torch.Tensor) and not any(d.kind == bk.KIND_BANK for d in ds):
        device, bank = bank.device, None                             # nothing indexes it: its side need not fit ks
    if bank is not None and not isinstance(bank, torch.Tensor):
        import numpy as np
        arr = np.asarray(bank)
        if arr.ndim != 3:
            raise ValueError(f"kernel_tables: a bank is [n][kb][kb] (got shape {arr.shape})")
        bank = torch.from_numpy(np.stack([bk.check_table(t, f"bank[{i}]") for i, t in enumerate(arr)])).to(_default_device(device))
    if bank is not None:
        if bank.dim() != 3 or not bank.is_cuda or bank.dtype != torch.float32 or bank.shape[1] != bank.shape[2] or bank.shape[0] < 1 or \
                not bank.is_contiguous():
            raise ValueError(f"kernel_tables: a bank is a contiguous CUDA fp32 [n][kb][kb] tensor (got {bank.dtype} {tuple(bank.shape)} on {bank.device})")
        n_bank, kb = int(bank.shape[0]), bk.check_ks(int(bank.shape[1]))
        if kb > ks:
            raise ValueError(f"kernel_tables: the bank's tables of side {kb} do not fit ks = {ks}")
    for i, d in enumerate(ds):
        if d.kind == bk.KIND_BANK and (bank is None or d.ks != kb or not 0 <= d.bank_index < n_bank):
            raise ValueError(f"kernel_tables: descriptor {i} names table {d.bank_index} of side {d.ks}, which the bank "
                             f"({n_bank} tables of side {kb}) does not hold")
    dev = bank.device if bank is not None else _default_device(device)
    desc = torch.tensor(rows, dtype=torch.float64).to(dev)
    tab = torch.empty(len(ds), ks, ks, dtype=torch.float32, device=dev)
    check(lib().srk_kernel_tables_f32(_p(desc), _p(bank), n_bank, kb, _p(tab), len(ds), ks, _stream()))
    return DeviceTables(tab, ks, own, any(d.kind == bk.KIND_SINC for d in ds))


def _default_device(device):
    return torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)


def _device_tables(t: DeviceTables, B: int, x: torch.Tensor, what: str) -> DeviceTables:
    if t.tab.dim() != 3 or t.tab.shape[0] != B or tuple(t.tab.shape[1:]) != (t.ks, t.ks) or len(t.own) != B or t.tab.device != x.device or \
            t.tab.dtype != torch.float32 or not t.tab.is_contiguous():
        raise ValueError(f"{what}: DeviceTables of one fp32 table per sample on {x.device} are needed (B={B}; got {tuple(t.tab.shape)} on {t.tab.device})")
    return t


def blur2d(x: torch.Tensor, psf, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x CUDA fp32 [B,C,H,W] blurred with one ks x ks table or one per sample (csrc/blur2d.hip, srk_blur2d_f32): a correlation (no flip,
    cv2.filter2D's convention) in which taps outside the image are dropped and the rest renormalised per pixel.  Tables: odd ks <= 21,
    taps finite and >= 0, centre > 0, sum within 1e-3 of 1 (ValueError otherwise); mixed sizes are zero-padded to the largest.  One
    launch after one small upload.  psf may be `DeviceTables` made with signed=False (one per sample): nothing is checked, packed or
    uploaded then."""
    if x.dim() != 4 or not x.is_cuda or x.dtype != torch.float32 or min(x.shape) < 1:
        raise ValueError(f"blur2d takes a non-empty CUDA fp32 [B,C,H,W] batch (got {x.dtype} {tuple(x.shape)} on {x.device})")
    x = x.contiguous()
    B, Cc, H, W = x.shape
    if isinstance(psf, DeviceTables):
        if psf.signed:
            raise ValueError("blur2d: these DeviceTables hold a sinc table (negative taps); build them with kernel_tables(signed=False)")
        k, ks = _device_tables(psf, B, x, "blur2d").tab, psf.ks
    else:
        tabs, ks = pack_psf(psf, B)
    if out is None:
        out = torch.empty_like(x)
    elif tuple(out.shape) != tuple(x.shape) or out.dtype != torch.float32 or out.device != x.device or not out.is_contiguous():
        raise ValueError(f"out must be contiguous fp32 {tuple(x.shape)} on {x.device} (got {out.dtype} {tuple(out.shape)} on {out.device})")
    if not isinstance(psf, DeviceTables):
        k = torch.from_numpy(tabs).to(x.device)
    check(lib().srk_blur2d_f32(_p(x), _p(k), _p(out), B, Cc, H, W, ks, _stream()))
    return out


def degrade_psf(hr: torch.Tensor, scale: int, psf, noise=(0.0, 0.0), noise_ids=None, gray_noise=False, quant_bits: int = 8) -> Tuple[torch.Tensor, torch.Tensor]:
    """(lr, hr_cropped) like `degrade_blind` with a general 2-D blur: LR = noise(resize_aa(blur2d(HR))), i.e. `blur2d` on the region
    cropped to a multiple of the factor, then `degrade_blind` with sigma (0, 0) -- the plain bicubic tables on the blurred values, the
    same noise and rounding.  What DeviceHRPool(psf=)'s training patches are windows of, bit for bit.  The HR target is not blurred."""
    if hr.dim() != 4 or not hr.is_cuda:
        raise ValueError(f"degrade_psf takes a CUDA [B,C,H,W] batch (got {tuple(hr.shape)} on {hr.device})")
    s = int(scale)
    if not 2 <= s <= 4:
        raise ValueError(f"degrade_psf: the factor must be in 2..4 (got {scale!r})")
    B, Cc, H, W = hr.shape
    if H < s or W < s or B < 1 or Cc < 1:
        raise ValueError(f"degrade_psf: {tuple(hr.shape)} is smaller than one output pixel at factor {s}")
    hr = hr[..., :H - H % s, :W - W % s].float().contiguous()
    lr, _ = degrade_blind(blur2d(hr, psf), s, (0.0, 0.0), noise, list(range(B)) if noise_ids is None else noise_ids, gray_noise, quant_bits)
    return lr, hr


def check_jpeg_quality(q, what: str = "quality") -> int:
    """A JPEG quality as an int in 1..100 (bools, floats with a fraction and anything else raise ValueError)."""
    if isinstance(q, bool) or not isinstance(q, numbers.Real) or q != q or int(q) != q or not 1 <= int(q) <= 100:          # q != q: NaN
        raise ValueError(f"jpeg {what} must be an integer in 1..100 (got {q!r})")
    return int(q)


def jpeg_roundtrip(x: torch.Tensor, quality, subsample: bool = False, return_coef: bool = False):
    """What a baseline JPEG file of the 8-bit image of x at `quality` decodes to (csrc/jpeg.hip, srk_jpeg_roundtrip_f32): x CUDA fp32
    [B,C,H,W] with C = 1 or 3 is levelled to 8 bits, converted to JFIF YCbCr, transformed in 8 x 8 blocks anchored at (0, 0),
    quantised with libjpeg's scaling of the Annex K tables, and decoded again; chroma at 4:2:0 (`subsample`, C == 3 only) is averaged
    over 2 x 2 cells and upsampled by replication.  quality: an int or one per sample, each in 1..100, or 0 = that sample passes through
    bit for bit.  return_coef: also the quantised coefficients, int16 [B,C,Hm,Wm] (a test port; the part of a subsampled chroma plane
    outside its top-left [Hm/2,Wm/2] is zero).  One launch after one small upload."""
    if x.dim() != 4 or not x.is_cuda or x.dtype != torch.float32:
        raise ValueError(f"jpeg_roundtrip takes a CUDA fp32 [B,C,H,W] batch (got {x.dtype} {tuple(x.shape)} on {x.device})")
    B, Cc, H, W = x.shape
    if Cc not in (1, 3) or min(B, H, W) < 1:
        raise ValueError(f"jpeg_roundtrip: C must be 1 or 3 and every extent >= 1 (got {tuple(x.shape)})")
    qs = [quality] * B if isinstance(quality, numbers.Real) else list(quality)
    if len(qs) != B:
        raise ValueError(f"jpeg_roundtrip: one quality or one per sample (B={B}; got {len(qs)})")
    qs = [0 if (not isinstance(q, bool) and q == 0) else check_jpeg_quality(q) for q in qs]
    x = x.contiguous()
    qd = torch.tensor(qs, dtype=torch.int32).to(x.device)
    out = torch.empty_like(x)
    coef = None
    if return_coef:
        m = 16 if (subsample and Cc == 3) else 8
        coef = torch.zeros(B, Cc, -(-H // m) * m, -(-W // m) * m, dtype=torch.int16, device=x.device)
    check(lib().srk_jpeg_roundtrip_f32(_p(x), _p(out), _p(qd), B, Cc, H, W, int(bool(subsample)), _p(coef), _stream()))
    return (out, coef) if return_coef else out


# ---- scale-1 restoration: denoising and JPEG-artifact pairs (csrc/restore.hip) ---------------------------------------
def pack_restore_params(jpeg_quality, noise, noise_id: int, gray_noise: bool):
    """Slots 6..9 of a `srk_crop_restore_u8` descriptor / one row of `srk_noise_f32`'s table: `pack_degrade_params` with the JPEG
    quality (0 = no JPEG stage, else 1..100) as the low word of slot 6 in place of the blur sigmas."""
    q = 0 if (not isinstance(jpeg_quality, bool) and jpeg_quality == 0) else check_jpeg_quality(jpeg_quality)
    return [q] + pack_degrade_params((0.0, 0.0), noise, noise_id, gray_noise)[1:]


def noise(x: torch.Tensor, noise, noise_ids, gray_noise=False, quant_bits: int = 0) -> torch.Tensor:
    """The noise stage of `degrade_blind` at scale 1 (csrc/restore.hip, srk_noise_f32): x CUDA fp32 [B,C,H,W], C = 1 or 3, gets
    `v + sqrt(sigma_n^2 + gain max(v, 0)) z` per element, z from Philox on the counter (x, y, ch | 0 with gray noise) under the key
    noise_id.  noise = (sigma_n, gain): one pair or one per sample, image units in [0, 1]; noise_ids: B integers; gray_noise: a bool or
    B of them (always so for C == 1).  Zero amplitudes pass the bits through; quant_bits 8 rounds to k / 255.  One launch after one small
    upload."""
    if x.dim() != 4 or not x.is_cuda or x.dtype != torch.float32:
        raise ValueError(f"noise takes a CUDA fp32 [B,C,H,W] batch (got {x.dtype} {tuple(x.shape)} on {x.device})")
    B, Cc, H, W = x.shape
    if Cc not in (1, 3) or min(B, H, W) < 1:
        raise ValueError(f"noise: C must be 1 or 3 and every extent >= 1 (got {tuple(x.shape)})")
    if quant_bits not in (0, 8):
        raise ValueError(f"noise: quant_bits must be 0 or 8 (got {quant_bits!r})")
    ids = [int(v) for v in noise_ids]
    grays = [bool(gray_noise)] * B if isinstance(gray_noise, (bool, int)) else [bool(v) for v in gray_noise]
    if len(ids) != B or len(grays) != B:
        raise ValueError(f"noise: one noise id and one gray flag per sample (B={B}; got {len(ids)} ids, {len(grays)} flags)")
    rows = [pack_restore_params(0, n, i, g) for n, i, g in zip(_per_sample(noise, B, 2, "noise"), ids, grays)]
    x = x.contiguous()
    par = torch.tensor(rows, dtype=torch.int64).to(x.device)
    out = torch.empty_like(x)
    check(lib().srk_noise_f32(_p(x), _p(out), _p(par), B, Cc, H, W, int(quant_bits), _stream()))
    return out


_noise_stage = noise          # `restore_degrade` names its amplitude pair `noise`, as `degrade_blind` does


def restore_degrade(x: torch.Tensor, noise, noise_ids, gray_noise=False, jpeg_quality=0, subsample: bool = False,
                    quant_bits: int = 0) -> torch.Tensor:
    """The whole-image degradation of the scale-1 tasks: `noise`, then `jpeg_roundtrip` where the quality (an int or one per sample,
    0 = no JPEG stage) is > 0.  What DeviceRestorePool's training patches are windows of, bit for bit.  It is the composition of the
    two entries, no kernel of its own."""
    y = _noise_stage(x, noise, noise_ids, gray_noise, quant_bits)
    qs = [jpeg_quality] * x.shape[0] if isinstance(jpeg_quality, numbers.Real) else list(jpeg_quality)
    if any((isinstance(q, bool) or q != 0) for q in qs):
        y = jpeg_roundtrip(y, qs, subsample)
    return y


# ---- second-order degradation: signed tables and ragged batches (csrc/filter2d.hip, csrc/ragged.hip) -----------------
class RaggedExt:
    """The extents of a ragged batch (include/srk.h "Ragged batches"): `host`, a list of B (h, w), and `dev`, the int32 [B][2] copy the
    kernels read.  The host copy is what the checks run on: nothing is read back from the device."""

    def __init__(self, ext, device):
        try:
            self.host = [(int(h), int(w)) for h, w in ext]
        except (TypeError, ValueError):
            raise ValueError(f"extents must be B pairs (h, w) (got {ext!r})") from None
        if not self.host or any(h < 1 or w < 1 for h, w in self.host):
            raise ValueError(f"every extent must be >= 1 (got {self.host})")
        self.dev = torch.tensor(self.host, dtype=torch.int32).to(device)

    def pad(self) -> Tuple[int, int]:
        return max(h for h, _ in self.host), max(w for _, w in self.host)


def _ragged(ext, B: int, Hp: int, Wp: int, device, what: str) -> Optional[RaggedExt]:
    """ext (None = dense, a list of pairs, or a RaggedExt) checked against a padded [B][.][Hp][Wp] buffer."""
    if ext is None:
        return None
    if not isinstance(ext, RaggedExt):
        ext = RaggedExt(ext, device)
    if len(ext.host) != B or any(h > Hp or w > Wp for h, w in ext.host):
        raise ValueError(f"{what}: {B} extents inside the padded {Hp} x {Wp} are needed (got {ext.host})")
    return ext


def _ext_ptr(ext: Optional[RaggedExt]):
    return None if ext is None else _p(ext.dev)


def _padded_out(out: Optional[torch.Tensor], shape, like: torch.Tensor) -> torch.Tensor:
    if out is None:
        return torch.empty(shape, dtype=torch.float32, device=like.device)
    if tuple(out.shape) != tuple(shape) or out.dtype != torch.float32 or out.device != like.device or not out.is_contiguous():
        raise ValueError(f"out must be contiguous fp32 {tuple(shape)} on {like.device} (got {out.dtype} {tuple(out.shape)} on {out.device})")
    return out


def pack_filter_tables(tab, B: int):
    """tab: one [ks][ks] table or B of them (mixed odd sizes allowed) -> (fp32 numpy [B][ks][ks], ks, the B sizes before padding), each
    checked by blur_kernels.check_filter_table -- finite, sum within 1e-3 of 1, any sign -- and zero-padded, centred, to the largest ks."""
    from . import blur_kernels as bk
    import numpy as np
    if isinstance(tab, torch.Tensor):
        tab = tab.detach().cpu().numpy()
    if isinstance(tab, np.ndarray) and tab.ndim == 2:
        tabs = [bk.check_filter_table(tab)] * B
    else:
        tabs = [bk.check_filter_table(t, f"table[{i}]") for i, t in enumerate(tab)]
    if len(tabs) != B:
        raise ValueError(f"filter tables: one table or one per sample (B={B}; got {len(tabs)})")
    ks = max(t.shape[0] for t in tabs)
    return np.stack([bk.pad_to(t, ks) for t in tabs]), ks, [t.shape[0] for t in tabs]


def filter2d(x: torch.Tensor, tab, ext=None, quant_bits: int = 0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x CUDA fp32 [B,C,Hp,Wp] filtered with one signed ks x ks table or one per sample (csrc/filter2d.hip, srk_filter2d_f32): a
    correlation with a reflect-101 border and no normalisation, cv2.filter2D's default and Real-ESRGAN's filter2D -- the rule sinc
    tables need, and the one every 2-D filter of the second-order chain takes.  ext: None (dense) or the (h, w) of every sample in the
    padded batch; each must exceed the R = ks // 2 of its sample's OWN table (zero-padding a table to the batch's largest ks adds taps
    that multiply in-extent pixels by 0: no bit changes).  A delta table passes its sample through bit for bit.  quant_bits 8 rounds to
    k / 255.  One launch after one small upload.  tab may be `DeviceTables` (one per sample): nothing is checked, packed or uploaded
    then, and the extent check runs on their host list of own sizes."""
    if x.dim() != 4 or not x.is_cuda or x.dtype != torch.float32 or min(x.shape) < 1:
        raise ValueError(f"filter2d takes a non-empty CUDA fp32 [B,C,H,W] batch (got {x.dtype} {tuple(x.shape)} on {x.device})")
    if quant_bits not in (0, 8):
        raise ValueError(f"filter2d: quant_bits must be 0 or 8 (got {quant_bits!r})")
    x = x.contiguous()
    B, Cc, Hp, Wp = x.shape
    if isinstance(tab, DeviceTables):
        tabs, ks, own = None, tab.ks, _device_tables(tab, B, x, "filter2d").own
    else:
        tabs, ks, own = pack_filter_tables(tab, B)
    e = _ragged(ext, B, Hp, Wp, x.device, "filter2d")
    for b, (h, w) in enumerate([(Hp, Wp)] * B if e is None else e.host):
        if min(h, w) <= own[b] // 2:
            raise ValueError(f"filter2d: sample {b} of {h} x {w} does not exceed the R = {own[b] // 2} of its table")
    out = _padded_out(out, x.shape, x)
    k = tab.tab if tabs is None else torch.from_numpy(tabs).to(x.device)
    check(lib().srk_filter2d_f32(_p(x), _p(k), _p(out), _ext_ptr(e), B, Cc, Hp, Wp, ks, int(quant_bits), _stream()))
    return out


def resize_aa_ragged(x: torch.Tensor, ext_in, ext_out, pad_out=None, quant_bits: int = 0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """`resize_aa` with a size per sample (csrc/ragged.hip, srk_resize_aa_ragged_f32): sample b of the padded x [B,C,Hp,Wp] is resized
    from ext_in[b] to ext_out[b] into the top-left of out [B,C,Hop,Wop], bit-identical to `resize_aa` on that sample alone; the rest of
    out keeps its bits.  ext_in / ext_out: None (dense) or B pairs; pad_out = (Hop, Wop), by default the largest output extents.  The
    8x limit of `resize_aa` is checked here, on the host copies of the extents (SrkUnsupported).  One launch."""
    if x.dim() != 4 or not x.is_cuda or x.dtype != torch.float32 or min(x.shape) < 1:
        raise ValueError(f"resize_aa_ragged takes a non-empty CUDA fp32 [B,C,H,W] batch (got {x.dtype} {tuple(x.shape)} on {x.device})")
    if quant_bits not in (0, 8):
        raise ValueError(f"resize_aa_ragged: quant_bits must be 0 or 8 (got {quant_bits!r})")
    x = x.contiguous()
    B, Cc, Hp, Wp = x.shape
    ei = _ragged(ext_in, B, Hp, Wp, x.device, "resize_aa_ragged: ext_in")
    if ext_out is None and pad_out is None:
        raise ValueError("resize_aa_ragged: a dense output needs pad_out = (Hop, Wop)")
    if ext_out is not None and not isinstance(ext_out, RaggedExt):
        ext_out = RaggedExt(ext_out, x.device)
    try:
        Hop, Wop = ext_out.pad() if pad_out is None else (int(v) for v in pad_out)
    except (TypeError, ValueError):
        raise ValueError(f"resize_aa_ragged: pad_out must be (Hop, Wop) (got {pad_out!r})") from None
    if Hop < 1 or Wop < 1:
        raise ValueError(f"resize_aa_ragged: pad_out must be >= 1 (got {(Hop, Wop)})")
    eo = _ragged(ext_out, B, Hop, Wop, x.device, "resize_aa_ragged: ext_out")
    for (h, w), (ho, wo) in zip([(Hp, Wp)] * B if ei is None else ei.host, [(Hop, Wop)] * B if eo is None else eo.host):
        if h > 8 * ho or w > 8 * wo:
            raise _lib.SrkUnsupported(f"resize_aa_ragged: {h} x {w} -> {ho} x {wo} shrinks an axis by more than 8x (more than 33 taps)")
    out = _padded_out(out, (B, Cc, Hop, Wop), x)
    check(lib().srk_resize_aa_ragged_f32(_p(x), _ext_ptr(ei), _p(out), _ext_ptr(eo), B, Cc, Hp, Wp, Hop, Wop, int(quant_bits), _stream()))
    return out


RESIZE_MODES = ("cubic", "bilinear", "area")          # the mode words of srk_resize_ragged_mode_f32


def resize_ragged(x: torch.Tensor, ext_in, ext_out, modes, pad_out=None, quant_bits: int = 0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """`resize_aa_ragged` with a resize rule per sample (csrc/resize_modes.hip, srk_resize_ragged_mode_f32): modes = None or B words,
    0 the antialiased cubic (that sample has the bits of `resize_aa_ragged`), 1 bilinear without antialiasing (F.interpolate,
    align_corners=False), 2 area (adaptive average pooling).  None or all zeros IS `resize_aa_ragged`: the same launch.  The 8x limit
    holds for every mode.  One launch after one small upload."""
    if modes is None:
        return resize_aa_ragged(x, ext_in, ext_out, pad_out, quant_bits, out)
    try:
        ms = [int(m) for m in modes]
    except (TypeError, ValueError):
        raise ValueError(f"resize_ragged: modes must be None or one word in 0..2 per sample (got {modes!r})") from None
    if any(m not in (0, 1, 2) or isinstance(v, bool) for m, v in zip(ms, modes)):
        raise ValueError(f"resize_ragged: a mode is 0 (cubic), 1 (bilinear) or 2 (area) (got {ms})")
    if x.dim() != 4 or len(ms) != x.shape[0]:
        raise ValueError(f"resize_ragged: one mode per sample of a [B,C,H,W] batch (got {len(ms)} for {tuple(x.shape)})")
    if not any(ms):
        return resize_aa_ragged(x, ext_in, ext_out, pad_out, quant_bits, out)
    if not x.is_cuda or x.dtype != torch.float32 or min(x.shape) < 1:
        raise ValueError(f"resize_ragged takes a non-empty CUDA fp32 [B,C,H,W] batch (got {x.dtype} {tuple(x.shape)} on {x.device})")
    if quant_bits not in (0, 8):
        raise ValueError(f"resize_ragged: quant_bits must be 0 or 8 (got {quant_bits!r})")
    x = x.contiguous()
    B, Cc, Hp, Wp = x.shape
    ei = _ragged(ext_in, B, Hp, Wp, x.device, "resize_ragged: ext_in")
    if ext_out is None and pad_out is None:
        raise ValueError("resize_ragged: a dense output needs pad_out = (Hop, Wop)")
    if ext_out is not None and not isinstance(ext_out, RaggedExt):
        ext_out = RaggedExt(ext_out, x.device)
    try:
        Hop, Wop = ext_out.pad() if pad_out is None else (int(v) for v in pad_out)
    except (TypeError, ValueError):
        raise ValueError(f"resize_ragged: pad_out must be (Hop, Wop) (got {pad_out!r})") from None
    if Hop < 1 or Wop < 1:
        raise ValueError(f"resize_ragged: pad_out must be >= 1 (got {(Hop, Wop)})")
    eo = _ragged(ext_out, B, Hop, Wop, x.device, "resize_ragged: ext_out")
    for (h, w), (ho, wo) in zip([(Hp, Wp)] * B if ei is None else ei.host, [(Hop, Wop)] * B if eo is None else eo.host):
        if h > 8 * ho or w > 8 * wo:
            raise _lib.SrkUnsupported(f"resize_ragged: {h} x {w} -> {ho} x {wo} shrinks an axis by more than 8x (the tile staging covers 8x)")
    out = _padded_out(out, (B, Cc, Hop, Wop), x)
    md = torch.tensor(ms, dtype=torch.int32).to(x.device)
    check(lib().srk_resize_ragged_mode_f32(_p(x), _ext_ptr(ei), _p(out), _ext_ptr(eo), _p(md), B, Cc, Hp, Wp, Hop, Wop, int(quant_bits),
                                           _stream()))
    return out


_USM_TAPS: dict = {}


def usm_ks(radius: int) -> int:
    """The tap count of `usm_sharpen` for Real-ESRGAN's `radius`: radius + 1 if it is even, else radius."""
    if isinstance(radius, bool) or not isinstance(radius, numbers.Integral) or not 1 <= radius <= 51:
        raise ValueError(f"usm: radius must be an integer in 1..51 (got {radius!r})")
    return int(radius) + 1 if radius % 2 == 0 else int(radius)


def usm_taps(ks: int, sigma: float, device) -> torch.Tensor:
    """The fp32 taps `blur_kernels.gaussian1d(ks, sigma)` on `device`: uploaded once per (device, ks, sigma) and kept."""
    from . import blur_kernels as bk
    device = torch.device(device)
    key = (device.type, device.index if device.index is not None else torch.cuda.current_device(), int(ks), float(sigma))
    t = _USM_TAPS.get(key)
    if t is None:
        t = _USM_TAPS[key] = torch.from_numpy(bk.gaussian1d(ks, sigma)).to(device)
    return t


def usm_sharpen(x: torch.Tensor, radius: int = 50, sigma: float = 0.0, weight: float = 0.5, threshold: float = 10.0,
                out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Real-ESRGAN's USMSharp on x CUDA fp32 [B,C,H,W] in [0, 1], C 1 or 3 (csrc/usm.hip, srk_usm_sharpen_f32; include/srk.h states the
    arithmetic): blur = G(x), res = x - blur, mask = |res| 255 > threshold, soft = G(mask), out = soft clamp(x + weight res, 0, 1) +
    (1 - soft) x, G the separable Gaussian of ks = radius + 1 (radius even) or radius taps under a reflect-101 border.  sigma <= 0 takes
    OpenCV's rule 0.3 ((ks - 1) / 2 - 1) + 0.8: the defaults are 51 taps at sigma 8.  H and W must exceed (ks - 1) / 2.  Two launches;
    one work buffer of x's size is allocated per call by torch."""
    if x.dim() != 4 or not x.is_cuda or x.dtype != torch.float32 or min(x.shape) < 1 or x.shape[1] not in (1, 3):
        raise ValueError(f"usm_sharpen takes a non-empty CUDA fp32 [B,C,H,W] batch with C 1 or 3 (got {x.dtype} {tuple(x.shape)} on {x.device})")
    ks = usm_ks(radius)
    sigma = float(sigma)
    if not sigma == sigma or sigma == float("inf"):
        raise ValueError(f"usm_sharpen: sigma must be finite (got {sigma!r})")
    if sigma <= 0.0:
        sigma = 0.3 * ((ks - 1) / 2 - 1) + 0.8
    weight, threshold = float(weight), float(threshold)
    if not (weight == weight and threshold == threshold) or abs(weight) == float("inf"):
        raise ValueError(f"usm_sharpen: weight and threshold must be numbers (got {weight!r}, {threshold!r})")
    x = x.contiguous()
    B, Cc, H, W = x.shape
    if min(H, W) <= ks // 2:
        raise _lib.SrkUnsupported(f"usm_sharpen: a {H} x {W} image is not larger than R = {ks // 2} (radius {radius})")
    out = _padded_out(out, x.shape, x)
    work = torch.empty_like(x)
    check(lib().srk_usm_sharpen_f32(_p(x), _p(usm_taps(ks, sigma, x.device)), _p(out), _p(work), B, Cc, H, W, ks, weight, threshold, _stream()))
    return out


def _qualities(quality, B: int, what: str):
    qs = [quality] * B if isinstance(quality, numbers.Real) else list(quality)
    if len(qs) != B:
        raise ValueError(f"{what}: one quality or one per sample (B={B}; got {len(qs)})")
    return [0 if (not isinstance(q, bool) and q == 0) else check_jpeg_quality(q) for q in qs]


def jpeg_roundtrip_ragged(x: torch.Tensor, quality, ext=None, subsample: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """`jpeg_roundtrip` with a size per sample (csrc/ragged.hip, srk_jpeg_roundtrip_ragged_f32): the block grid and the edge replication
    of sample b are those of its own extents ext[b], so it is bit-identical to `jpeg_roundtrip` on that sample alone; quality 0 copies
    the in-extent words.  The padding of out keeps its bits.  One launch after one small upload."""
    if x.dim() != 4 or not x.is_cuda or x.dtype != torch.float32:
        raise ValueError(f"jpeg_roundtrip_ragged takes a CUDA fp32 [B,C,H,W] batch (got {x.dtype} {tuple(x.shape)} on {x.device})")
    B, Cc, Hp, Wp = x.shape
    if Cc not in (1, 3) or min(B, Hp, Wp) < 1:
        raise ValueError(f"jpeg_roundtrip_ragged: C must be 1 or 3 and every extent >= 1 (got {tuple(x.shape)})")
    qs = _qualities(quality, B, "jpeg_roundtrip_ragged")
    x = x.contiguous()
    e = _ragged(ext, B, Hp, Wp, x.device, "jpeg_roundtrip_ragged")
    out = _padded_out(out, x.shape, x)
    qd = torch.tensor(qs, dtype=torch.int32).to(x.device)
    check(lib().srk_jpeg_roundtrip_ragged_f32(_p(x), _p(out), _p(qd), _ext_ptr(e), B, Cc, Hp, Wp, int(bool(subsample)), _stream()))
    return out


class SecondOrder(NamedTuple):
    """The second-order degradation of ONE sample (Real-ESRGAN's chain; sr_datasets.SecondOrderSpec draws it): tables k1 / k2 / k3 for
    the three filters (blur_kernels; a delta = no filter; or `blur_kernels.TableDesc` descriptors, which the device turns into tables), resize factors r1 / r2 of the two intermediate sizes, noise1 / noise2 =
    (sigma_n, gain) with their gray flags, JPEG qualities q1 (stage 1) and q2 (stage 2), `jpeg_last`: False = order A (JPEG 2, final
    resize, final filter), True = order B (final resize, final filter, JPEG 2); the Philox key of noise 1 (noise 2 takes its
    complement).  modes: the rule of resize 1, resize 2 and the final resize (`resize_ragged`: 0 antialiased cubic, 1 bilinear,
    2 area); the default is the cubic of every earlier release."""
    k1: object
    r1: float
    noise1: Tuple[float, float]
    gray1: bool
    q1: int
    k2: object
    r2: float
    noise2: Tuple[float, float]
    gray2: bool
    q2: int
    jpeg_last: bool
    k3: object
    noise_id: int
    modes: Tuple[int, int, int] = (0, 0, 0)


def second_order_sizes(H: int, W: int, scale: int, p: SecondOrder):
    """((h1, w1), (h2, w2), (ho, wo)) of one sample: round-half-up of H r1, of (H / scale) r2, and the dense output H / scale."""
    rnd = lambda v: max(1, int(v + 0.5))          # noqa: E731
    s = int(scale)
    return (rnd(H * p.r1), rnd(W * p.r1)), (rnd(H / s * p.r2), rnd(W / s * p.r2)), (H // s, W // s)


def second_order_noise_ids(p: SecondOrder) -> Tuple[int, int]:
    i = int(p.noise_id) & 0xFFFFFFFFFFFFFFFF
    return i, i ^ 0xFFFFFFFFFFFFFFFF


def _stage_tables(ks_list, bank, device, what: str):
    """One stage's tables of `degrade_second_order`: arrays as they are (filter2d checks, packs and uploads them), descriptors built by
    ONE `kernel_tables` launch."""
    from .blur_kernels import TableDesc
    n = sum(isinstance(k, TableDesc) for k in ks_list)
    if n == 0:
        return ks_list
    if n != len(ks_list):
        raise ValueError(f"degrade_second_order: {what} mixes tables and TableDesc descriptors in one batch ({n} of {len(ks_list)} are descriptors)")
    return kernel_tables(ks_list, bank=bank, device=device)


def _stage_modes(ps):
    """The mode lists of the three resizes of `degrade_second_order`; None for a stage whose samples all take the cubic (the launch of
    `resize_aa_ragged`, and no upload)."""
    if all(p.modes == (0, 0, 0) for p in ps):          # the chain of every earlier release: nothing to check, build or upload
        return None, None, None
    for p in ps:
        if len(p.modes) != 3 or any(isinstance(m, bool) or m not in (0, 1, 2) for m in p.modes):
            raise ValueError(f"degrade_second_order: modes must be three words in 0..2 (got {p.modes!r})")
    return tuple(([p.modes[k] for p in ps] if any(p.modes[k] for p in ps) else None) for k in range(3))


def degrade_second_order(x: torch.Tensor, scale: int, params, subsample: bool = False, pads=None, bufs: Optional[dict] = None,
                         bank=None) -> torch.Tensor:
    """The second-order blind degradation on a batch x CUDA fp32 [B,C,H,W] (C = 1 or 3; H, W multiples of `scale` in 1..4), one
    `SecondOrder` per sample -> the LR batch [B,C,H/scale,W/scale] in 8-bit levels:
        filter k1 -> resize to (H, W) r1 -> noise 1 -> JPEG q1 -> filter k2 -> resize to (H, W) / scale r2 -> noise 2
        -> [order A: JPEG q2] -> resize to (H, W) / scale -> filter k3, rounded to 8 bits -> [order B: JPEG q2]
    Every filter is `filter2d` (reflect border), every intermediate is a ragged batch in a padded buffer, so every sample has its own
    sizes and every stage is ONE launch: eleven launches and their small uploads, no host read, no intermediate copy.  Each sample is
    bit-identical to the composition of the dense ops on that sample alone.  pads = ((Hp1, Wp1), (Hp2, Wp2)) fixes the padded sizes
    (default: the batch's largest); bufs: a dict that keeps the work buffers between calls.
    k1 / k2 / k3 may be `blur_kernels.TableDesc` descriptors in place of tables -- per stage all or none of the batch -- and the
    stage's tables are then built on the device by one `kernel_tables` launch (three more tiny launches, three fewer table uploads);
    bank: the CUDA tensor that kind-5 descriptors index.
    `SecondOrder.modes` picks the rule of each of the three resizes per sample (`resize_ragged`); a stage whose samples all take mode 0
    is the launch of `resize_aa_ragged`, so the default is the chain of every earlier release."""
    if x.dim() != 4 or not x.is_cuda or x.dtype != torch.float32:
        raise ValueError(f"degrade_second_order takes a CUDA fp32 [B,C,H,W] batch (got {x.dtype} {tuple(x.shape)} on {x.device})")
    s = int(scale)
    B, Cc, H, W = x.shape
    if not 1 <= s <= 4 or H % s or W % s or Cc not in (1, 3) or min(B, H // s, W // s) < 1:
        raise ValueError(f"degrade_second_order: scale in 1..4 dividing H and W, C 1 or 3 (got scale {scale!r}, {tuple(x.shape)})")
    ps = list(params)
    if len(ps) != B or not all(isinstance(p, SecondOrder) for p in ps):
        raise ValueError(f"degrade_second_order: one SecondOrder per sample (B={B}; got {len(ps)})")
    sizes = [second_order_sizes(H, W, s, p) for p in ps]
    e1, e2 = RaggedExt([z[0] for z in sizes], x.device), RaggedExt([z[1] for z in sizes], x.device)
    (Hp1, Wp1), (Hp2, Wp2) = (e1.pad(), e2.pad()) if pads is None else pads
    Ho, Wo = H // s, W // s
    bufs = {} if bufs is None else bufs

    def buf(name, *shape):
        t = bufs.get(name)
        if t is None or tuple(t.shape) != shape or t.device != x.device:
            t = bufs[name] = torch.empty(shape, dtype=torch.float32, device=x.device)
        return t

    ids = [second_order_noise_ids(p) for p in ps]
    qa = [0 if p.jpeg_last else p.q2 for p in ps]
    qb = [p.q2 if p.jpeg_last else 0 for p in ps]
    x = x.contiguous()
    t1, t2, t3 = (_stage_tables([getattr(p, k) for p in ps], bank, x.device, k) for k in ("k1", "k2", "k3"))
    a = filter2d(x, t1, out=buf("f1", B, Cc, H, W))
    m1, m2, m3 = _stage_modes(ps)
    a = resize_ragged(a, None, e1, m1, (Hp1, Wp1), out=buf("a1", B, Cc, Hp1, Wp1))
    a = _noise_into(a, [p.noise1 for p in ps], [i[0] for i in ids], [p.gray1 for p in ps], buf("b1", B, Cc, Hp1, Wp1))
    a = jpeg_roundtrip_ragged(a, [p.q1 for p in ps], e1, subsample, out=buf("a1", B, Cc, Hp1, Wp1))
    a = filter2d(a, t2, e1, out=buf("b1", B, Cc, Hp1, Wp1))
    a = resize_ragged(a, e1, e2, m2, (Hp2, Wp2), out=buf("a2", B, Cc, Hp2, Wp2))
    a = _noise_into(a, [p.noise2 for p in ps], [i[1] for i in ids], [p.gray2 for p in ps], buf("b2", B, Cc, Hp2, Wp2))
    a = jpeg_roundtrip_ragged(a, qa, e2, subsample, out=buf("a2", B, Cc, Hp2, Wp2))
    a = resize_ragged(a, e2, None, m3, (Ho, Wo), out=buf("lr0", B, Cc, Ho, Wo))
    a = filter2d(a, t3, quant_bits=8, out=buf("lr1", B, Cc, Ho, Wo))
    return jpeg_roundtrip(a, qb, subsample)


def _noise_into(x: torch.Tensor, amp, noise_ids, gray, out: torch.Tensor) -> torch.Tensor:
    """`noise` into a given buffer: on a padded batch the counter is (x, y, ch) only, so inside a sample's extents the bits are those of
    the dense call on that sample; what lands in the padding is never read."""
    B, Cc, H, W = x.shape
    rows = [pack_restore_params(0, n, i, g) for n, i, g in zip(amp, noise_ids, gray)]
    par = torch.tensor(rows, dtype=torch.int64).to(x.device)
    check(lib().srk_noise_f32(_p(x), _p(out), _p(par), B, Cc, H, W, 0, _stream()))
    return out


LUMA_COEF = (4899, 9617, 1868)          # /16384: full-range BT.601 in 14-bit fixed point, the sum is 16384


def to_gray(x):
    """The integer luma `(4899 R + 9617 G + 1868 B + 8192) >> 14` of stored samples, on the CPU: x uint8 / uint16, a numpy array or a
    CPU tensor, [..., H, W, 3] -> [..., H, W] of the same type and dtype.  What srk_crop_restore_u8 makes of an RGB source at
    out_chans 1, so a validation loader can form the same one-channel HR images."""
    import numpy as np
    is_t = isinstance(x, torch.Tensor)
    a = x.detach().cpu().numpy() if is_t else np.asarray(x)
    if a.dtype not in (np.uint8, np.uint16):
        raise ValueError(f"to_gray takes uint8 or uint16 samples (got {a.dtype})")
    if a.ndim < 3 or a.shape[-1] != 3:
        raise ValueError(f"to_gray takes [..., H, W, 3] samples (got shape {tuple(a.shape)})")
    v = a.astype(np.uint32)          # 16384 * 65535 + 8192 < 2^32
    y = ((LUMA_COEF[0] * v[..., 0] + LUMA_COEF[1] * v[..., 1] + LUMA_COEF[2] * v[..., 2] + 8192) >> 14).astype(a.dtype)
    return torch.from_numpy(y) if is_t else y
