"""Tiled inference: run a model on overlapping tiles of an image batch and merge the outputs (SwinIR's --tile / --tile_overlap, the
tile_size / tile_pad of the HAT and DAT test scripts).

Tile grid, per axis with extent n, tile t (1 <= t <= n) and overlap v (0 <= v < t): stride s = t - v, k = ceil((n - t) / s) + 1 tiles,
origin o_i = min(i s, n - t) -- the SwinIR script's list(range(0, n - t, s)) + [n - t]; the last tile is pulled back to the border.
The 2-D grid is row-major (tile index iy kx + ix), and the tiles are processed in chunks of `tile_batch` consecutive indices.

Blend 'mean' (the script's E / W): a pixel is the sum of the tiles covering it, added in ascending tile index as sequential fp32
adds starting from 0, divided once by their integer count.  Blend 'center': a pixel is copied from one tile -- per axis the
covering tile that maximises min(p - o, o + t - 1 - p), ties to the lower index.  Either way the bits do not depend on tile_batch.

On the device a chunk costs one gather launch and one merge launch (csrc/tile.hip, `srk_tile_gather_f32` / `srk_tile_merge_f32`):
no atomics, no weight image, no zero-fill, and the kernels take the grid as scalars, so the launches are capturable.  CPU tensors
take torch slicing with the same order of operations (the host path of evaluate.py --arch ms_resunet, and of the tests).
"""
from __future__ import annotations

from typing import List, Sequence, Tuple, Union

import torch

BLENDS = ("mean", "center")          # SRK_TILE_MEAN, SRK_TILE_CENTER (include/srk.h)

IntOrPair = Union[int, Sequence[int]]


def tile_origins(n: int, tile: int, overlap: int) -> List[int]:
    """The tile origins along one axis of extent n: o_i = min(i (tile - overlap), n - tile) for i < ceil((n - tile) / stride) + 1."""
    n, tile, overlap = int(n), int(tile), int(overlap)
    if n < 1 or not 1 <= tile <= n:
        raise ValueError(f"a tile is in 1..extent (got tile {tile} for extent {n})")
    if not 0 <= overlap < tile:
        raise ValueError(f"the overlap is in 0..tile-1 (got overlap {overlap} for tile {tile})")
    s = tile - overlap
    k = -(-(n - tile) // s) + 1
    return [min(i * s, n - tile) for i in range(k)]


def _pair(v: IntOrPair, what: str) -> Tuple[int, int]:
    if isinstance(v, (tuple, list)):
        if len(v) != 2:
            raise ValueError(f"{what} is an int or an (h, w) pair (got {v!r})")
        return int(v[0]), int(v[1])
    return int(v), int(v)


def _owners(n: int, t: int, origins: List[int]) -> torch.Tensor:
    """'center': the owner tile of every coordinate of one axis."""
    own = []
    for p in range(n):
        best, best_m = -1, -1
        for i, o in enumerate(origins):
            if o <= p < o + t and min(p - o, o + t - 1 - p) > best_m:
                best, best_m = i, min(p - o, o + t - 1 - p)
        own.append(best)
    return torch.tensor(own)


def _scale_of(y: torch.Tensor, rows: int, th: int, tw: int) -> int:
    if y.dim() != 4 or y.shape[0] != rows:
        raise ValueError(f"the model must map a batch of {rows} tiles to a batch of {rows} 4-D outputs (got {tuple(y.shape)})")
    s = y.shape[-2] // th
    if s < 1 or y.shape[-2] != s * th or y.shape[-1] != s * tw:
        raise ValueError(f"the model must scale both axes by one integer factor (a {th} x {tw} tile came back as "
                         f"{y.shape[-2]} x {y.shape[-1]})")
    return s


def tiled_forward(model, x: torch.Tensor, tile: IntOrPair, overlap: IntOrPair = 32, tile_batch: int = 1,
                  blend: str = "mean") -> torch.Tensor:
    """model(x) [B,C,H,W] -> [B,C',H s,W s] computed on tiles of `tile` (int or (h, w)) LR pixels that overlap by `overlap`, with
    `tile_batch` tiles (a batch of tile_batch * B) per model call, merged by `blend` ('mean' | 'center').

    A tile is clamped to the image; an axis with a single tile ignores its overlap, and a tile at least as large as the image on both
    axes is one plain model call.  The scale s is read off the first chunk's output.  CUDA input runs as fp32 through the kernels;
    CPU input takes torch slicing."""
    th, tw = _pair(tile, "tile")
    vy, vx = _pair(overlap, "overlap")
    tile_batch = int(tile_batch)
    if x.dim() != 4:
        raise ValueError(f"tiled_forward takes [B,C,H,W] (got {tuple(x.shape)})")
    if th < 1 or tw < 1:
        raise ValueError(f"a tile is at least 1 pixel (got {th} x {tw})")
    if not (0 <= vy < th and 0 <= vx < tw):
        raise ValueError(f"the overlap is in 0..tile-1 (got overlap {vy} x {vx} for tile {th} x {tw})")
    if tile_batch < 1:
        raise ValueError(f"tile_batch is at least 1 (got {tile_batch})")
    if blend not in BLENDS:
        raise ValueError(f"blend must be one of {BLENDS} (got {blend!r})")
    B, C, H, W = x.shape
    if min(B, C, H, W) < 1:
        raise ValueError(f"tiled_forward takes a non-empty batch (got {tuple(x.shape)})")
    with torch.no_grad():
        if th >= H and tw >= W:
            return model(x)
        # clamp; a clamped axis holds one tile, whose stride is never used
        (th, sy), (tw, sx) = ((n, n) if t >= n else (t, t - v) for n, t, v in ((H, th, vy), (W, tw, vx)))
        oys, oxs = tile_origins(H, th, th - sy), tile_origins(W, tw, tw - sx)
        kx, N = len(oxs), len(oys) * len(oxs)
        if x.is_cuda:
            return _tiled_device(model, x.float().contiguous(), th, tw, sy, sx, N, tile_batch, BLENDS.index(blend))
        return _tiled_host(model, x, th, tw, oys, oxs, kx, N, tile_batch, blend)


def _tiled_device(model, x, th, tw, sy, sx, N, tile_batch, mode):
    from . import ops as K
    from ._lib import check, lib
    B, C, H, W = x.shape
    out, s = None, 0
    for t0 in range(0, N, tile_batch):
        n = min(tile_batch, N - t0)
        tiles = torch.empty((n * B, C, th, tw), dtype=torch.float32, device=x.device)
        check(lib().srk_tile_gather_f32(K._p(x), K._p(tiles), t0, n, B, C, H, W, th, tw, sy, sx, K._stream()))
        y = model(tiles).float().contiguous()
        if out is None:
            s = _scale_of(y, n * B, th, tw)
            out = torch.empty((B, y.shape[1], H * s, W * s), dtype=torch.float32, device=x.device)
        elif tuple(y.shape) != (n * B, out.shape[1], th * s, tw * s):
            raise ValueError(f"the model returned {tuple(y.shape)} for a chunk of {n * B} tiles (expected {(n * B, out.shape[1], th * s, tw * s)})")
        check(lib().srk_tile_merge_f32(K._p(y), K._p(out), t0, n, B, out.shape[1], H * s, W * s, th * s, tw * s, sy * s, sx * s, mode,
                                       K._stream()))
    return out


def _tiled_host(model, x, th, tw, oys, oxs, kx, N, tile_batch, blend):
    B, C, H, W = x.shape
    out = cnt = own_y = own_x = None
    s = 0
    for t0 in range(0, N, tile_batch):
        idx = range(t0, min(t0 + tile_batch, N))
        n = len(idx)
        crops = [x[:, :, oys[j // kx]:oys[j // kx] + th, oxs[j % kx]:oxs[j % kx] + tw] for j in idx]
        y = model(torch.cat(crops, 0).contiguous())
        if out is None:
            s = _scale_of(y, n * B, th, tw)
            out = torch.zeros((B, y.shape[1], H * s, W * s), dtype=y.dtype)
            if blend == "mean":
                cnt = torch.zeros((H * s, W * s), dtype=torch.int32)
            else:
                own_y, own_x = _owners(H * s, th * s, [o * s for o in oys]), _owners(W * s, tw * s, [o * s for o in oxs])
        elif tuple(y.shape) != (n * B, out.shape[1], th * s, tw * s):
            raise ValueError(f"the model returned {tuple(y.shape)} for a chunk of {n * B} tiles (expected {(n * B, out.shape[1], th * s, tw * s)})")
        for i, j in enumerate(idx):
            iy, ix = j // kx, j % kx
            ys, xs = slice(oys[iy] * s, (oys[iy] + th) * s), slice(oxs[ix] * s, (oxs[ix] + tw) * s)
            yi = y[i * B:(i + 1) * B]
            if blend == "mean":
                out[:, :, ys, xs] += yi
                cnt[ys, xs] += 1
            else:
                mine = (own_y[ys] == iy)[:, None] & (own_x[xs] == ix)[None, :]
                out[:, :, ys, xs] = torch.where(mine, yi, out[:, :, ys, xs])
    return out / cnt.to(out.dtype) if blend == "mean" else out
