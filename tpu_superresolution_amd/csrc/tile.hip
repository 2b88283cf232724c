// Tiled inference on fp32 NCHW batches: crop a chunk of overlapping tiles out of an image batch, and merge a chunk of processed
// tiles back into the output image (include/srk.h: srk_tile_gather_f32, srk_tile_merge_f32).
//
// The tile grid is closed-form per axis (kernels.h: TileAxis): stride s = t - overlap, k = ceil((n - t) / s) + 1 tiles, origin
// o_i = min(i s, n - t) -- the last tile is pulled back to the border.  The origins are non-decreasing, so the tiles covering a
// coordinate p are one index range [lo(p), hi(p)], and the 2-D tiles covering a pixel are a rectangle of tile indices iy kx + ix.
// Both kernels take the scalars (n, t, s, k), not origin arrays: nothing is uploaded and the launches are capturable.
//
//   - gather: one 256-thread workgroup per 64 x 16 block of one (tile, b, c) plane; a wave reads one contiguous 256-B row segment of
//     the image and writes one of the tile.
//   - merge: output-centric, one workgroup per 64 x 16 block of the rectangle of out that the chunk's tiles can cover.  Every thread
//     owns its pixels: it walks the covering tiles of the chunk in ascending index, so there are no atomics, no weight image and no
//     zero-fill.  'mean' starts from 0 when the pixel's first covering tile is in the chunk and from out[p] otherwise (out is read
//     only then), adds in index order and divides once, by the arithmetic count, when the last covering tile is in the chunk: the
//     bits do not depend on the chunking.  'center' copies the pixel from its owner tile in the chunk that holds the owner.
// Edge blocks are predicated per element; offsets are 64-bit; plain vector loads and stores only.
#include "kernels.h"

namespace {

constexpr int TL_COLS = 64;              // one wave along the contiguous axis
constexpr int TL_ROWS = 16;              // rows of a block: 4 per wave
constexpr int TL_PER_WAVE = TL_ROWS / 4;

__device__ __forceinline__ int tl_origin(const TileAxis& a, int i) {
  const int o = i * a.s, last = a.n - a.t;
  return o < last ? o : last;
}
// first / last tile covering p (0 <= p < n): o_i + t > p from lo on, o_i <= p up to hi
__device__ __forceinline__ int tl_lo(const TileAxis& a, int p) { return p < a.t ? 0 : (p - a.t) / a.s + 1; }
__device__ __forceinline__ int tl_hi(const TileAxis& a, int p) { return p >= a.n - a.t ? a.k - 1 : p / a.s; }
// the covering tile whose nearer edge is farthest from p; ties go to the lower index
__device__ __forceinline__ int tl_owner(const TileAxis& a, int p) {
  const int lo = tl_lo(a, p), hi = tl_hi(a, p);
  int best = lo, best_m = -1;
  for (int i = lo; i <= hi; ++i) {
    const int o = tl_origin(a, i);
    const int m = min(p - o, o + a.t - 1 - p);
    if (m > best_m) { best_m = m; best = i; }
  }
  return best;
}

__global__ __launch_bounds__(256) void tile_gather_kernel(const float* __restrict__ x, float* __restrict__ tiles, int t0, int planes,
                                                          TileAxis ay, TileAxis ax, int blocks_h, int blocks_w) {
  int blk = blockIdx.x;
  const int bx = blk % blocks_w; blk /= blocks_w;
  const int by = blk % blocks_h; blk /= blocks_h;
  const int plane = blk % planes, j = blk / planes;
  const int idx = t0 + j, iy = idx / ax.k, ix = idx - iy * ax.k;
  const int oy = tl_origin(ay, iy), ox = tl_origin(ax, ix);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int xt = bx * TL_COLS + lane;
  const bool okx = xt < ax.t;
  const float* src = x + (size_t)plane * (size_t)ay.n * (size_t)ax.n + (size_t)oy * ax.n + ox;
  float* dst = tiles + ((size_t)j * planes + plane) * (size_t)ay.t * (size_t)ax.t;
  float v[TL_PER_WAVE];
#pragma unroll
  for (int i = 0; i < TL_PER_WAVE; ++i) {
    const int yt = by * TL_ROWS + wave + 4 * i;
    v[i] = (okx && yt < ay.t) ? src[(size_t)yt * ax.n + xt] : 0.f;
  }
#pragma unroll
  for (int i = 0; i < TL_PER_WAVE; ++i) {
    const int yt = by * TL_ROWS + wave + 4 * i;
    if (okx && yt < ay.t) dst[(size_t)yt * ax.t + xt] = v[i];
  }
}

template <int MODE>
__global__ __launch_bounds__(256) void tile_merge_kernel(const float* __restrict__ tiles, float* __restrict__ out, int t0, int t1,
                                                         int planes, TileAxis ay, TileAxis ax, int r0, int r1, int c0, int c1,
                                                         int blocks_h, int blocks_w) {
  int blk = blockIdx.x;
  const int bx = blk % blocks_w; blk /= blocks_w;
  const int by = blk % blocks_h;
  const int plane = blk / blocks_h;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int X = c0 + bx * TL_COLS + lane;
  if (X >= c1) return;
  const size_t tile_elems = (size_t)ay.t * (size_t)ax.t;
  const float* src = tiles + (size_t)plane * tile_elems;               // tile j of this plane: + j * planes * tile_elems
  float* dst = out + (size_t)plane * (size_t)ay.n * (size_t)ax.n;
  const int kx = ax.k;
  const int iy_first = t0 / kx, iy_last = (t1 - 1) / kx;                 // tile rows the chunk touches

  if constexpr (MODE == SRK_TILE_CENTER) {
    const int ix = tl_owner(ax, X);
    const int xt = X - tl_origin(ax, ix);
#pragma unroll
    for (int i = 0; i < TL_PER_WAVE; ++i) {
      const int Y = r0 + by * TL_ROWS + wave + 4 * i;
      if (Y >= r1) continue;
      const int iy = tl_owner(ay, Y);
      const int idx = iy * kx + ix;
      if (idx < t0 || idx >= t1) continue;
      const int yt = Y - tl_origin(ay, iy);
      dst[(size_t)Y * ax.n + X] = src[(size_t)(idx - t0) * planes * tile_elems + (size_t)yt * ax.t + xt];
    }
  } else {
    const int lox = tl_lo(ax, X), hix = tl_hi(ax, X);
#pragma unroll
    for (int i = 0; i < TL_PER_WAVE; ++i) {
      const int Y = r0 + by * TL_ROWS + wave + 4 * i;
      if (Y >= r1) continue;
      const int loy = tl_lo(ay, Y), hiy = tl_hi(ay, Y);
      const int first = loy * kx + lox, last = hiy * kx + hix;
      float* p = dst + (size_t)Y * ax.n + X;
      // the covering tiles of row iy that lie in the chunk: columns max(lox, t0 - iy kx) .. min(hix, t1 - 1 - iy kx)
      const int ya = max(loy, iy_first), yb = min(hiy, iy_last);
      bool any = false;
      for (int iy = ya; iy <= yb; ++iy) any |= max(lox, t0 - iy * kx) <= min(hix, t1 - 1 - iy * kx);
      if (!any) continue;
      float acc = first < t0 ? *p : 0.f;                                 // the sum of the earlier chunks: the only read of out
      for (int iy = ya; iy <= yb; ++iy) {
        const size_t yoff = (size_t)(Y - tl_origin(ay, iy)) * ax.t;
        for (int ix = max(lox, t0 - iy * kx); ix <= min(hix, t1 - 1 - iy * kx); ++ix)
          acc += src[(size_t)(iy * kx + ix - t0) * planes * tile_elems + yoff + (X - tl_origin(ax, ix))];
      }
      if (last < t1) acc = acc / (float)((hiy - loy + 1) * (hix - lox + 1));      // IEEE division, once, by the integer count
      *p = acc;
    }
  }
}

}  // namespace

int srk_launch_tile_gather_f32(const float* x, float* tiles, int t0, int n, int planes, TileAxis ay, TileAxis ax, hipStream_t stream) {
  const int blocks_h = cdiv(ay.t, TL_ROWS), blocks_w = cdiv(ax.t, TL_COLS);
  const double blocks = (double)n * planes * blocks_h * blocks_w;      // a double cannot overflow on four int factors
  SRK_REQUIRE(blocks >= 1.0 && blocks <= 2147483647.0, SRK_E_SHAPE, "tile_gather: %.0f blocks do not fit one grid (n=%d planes=%d tile %d x %d)",
              blocks, n, planes, ay.t, ax.t);
  hipLaunchKernelGGL(tile_gather_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, x, tiles, t0, planes, ay, ax, blocks_h, blocks_w);
  return srk_check_launch("tile_gather_f32");
}

int srk_launch_tile_merge_f32(const float* tiles, float* out, int t0, int n, int planes, TileAxis ay, TileAxis ax, int mode,
                              hipStream_t stream) {
  // the rectangle of out the chunk's tiles can cover: the rows of its tile rows; all columns unless it lies inside one tile row
  const int t1 = t0 + n, iy0 = t0 / ax.k, iy1 = (t1 - 1) / ax.k;
  const int r0 = srk_tile_origin(ay, iy0), r1 = srk_tile_origin(ay, iy1) + ay.t;
  int c0 = 0, c1 = ax.n;
  if (iy0 == iy1) {
    c0 = srk_tile_origin(ax, t0 - iy0 * ax.k);
    c1 = srk_tile_origin(ax, t1 - 1 - iy0 * ax.k) + ax.t;
  }
  const int blocks_h = cdiv(r1 - r0, TL_ROWS), blocks_w = cdiv(c1 - c0, TL_COLS);
  const double blocks = (double)planes * blocks_h * blocks_w;
  SRK_REQUIRE(blocks >= 1.0 && blocks <= 2147483647.0, SRK_E_SHAPE, "tile_merge: %.0f blocks do not fit one grid (planes=%d rows %d cols %d)",
              blocks, planes, r1 - r0, c1 - c0);
  const dim3 grid((unsigned)blocks), block(256);
  if (mode == SRK_TILE_CENTER)
    hipLaunchKernelGGL(tile_merge_kernel<SRK_TILE_CENTER>, grid, block, 0, stream, tiles, out, t0, t1, planes, ay, ax, r0, r1, c0, c1,
                       blocks_h, blocks_w);
  else
    hipLaunchKernelGGL(tile_merge_kernel<SRK_TILE_MEAN>, grid, block, 0, stream, tiles, out, t0, t1, planes, ay, ax, r0, r1, c0, c1,
                       blocks_h, blocks_w);
  return srk_check_launch("tile_merge_f32");
}
