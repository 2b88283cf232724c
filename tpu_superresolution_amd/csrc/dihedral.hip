// The eight symmetries of the square (D4) on batches of fp32 NCHW images: the flip / rot90 augmentation of the training batch
// and the forward / inverse transforms of the x8 self-ensemble (include/srk.h: srk_dihedral_f32).
//
// One 256-thread workgroup moves one 64 x 64 tile of one (b, c) plane.  The op code is read once per workgroup (it is
// workgroup-uniform, so the branch on it is too).  T_op = Tr^b2 . V^b1 . H^b0:
//   - without the transpose a tile is 64 row copies with the row and / or column index reversed: a wave reads one contiguous
//     256-B row segment (forwards or backwards) and writes one;
//   - with the transpose the tile goes through LDS at pitch 65 floats: the row writes (bank = lane + const) and the column reads
//     (bank = 65 lane + const = lane + const mod 32) are both conflict-free within their 32-lane groups, and both the global
//     reads and the global writes run along the contiguous axis.
// Edge tiles are predicated per element; offsets are 64-bit; plain vector loads and stores only.
#include "kernels.h"

namespace {

constexpr int D4_TILE = 64;
constexpr int D4_PITCH = 65;
constexpr int D4_ROWS = D4_TILE / 4;     // rows of a tile per wave (4 waves)

enum { D4_COPY = 0, D4_SCALE = 1, D4_ACC = 2 };

template <int MODE>
__device__ __forceinline__ void d4_store(float* p, float v, float alpha) {
  if constexpr (MODE == D4_COPY) *p = v;                 // alpha == 1: a pure permutation, bit patterns (NaN payloads) kept
  else if constexpr (MODE == D4_SCALE) *p = alpha * v;
  else *p += alpha * v;
}

template <int MODE>
__global__ __launch_bounds__(256) void dihedral_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                       const int* __restrict__ ops, int op_all, int C, int H, int W, int tiles_h,
                                                       int tiles_w, float alpha) {
  __shared__ float tile[D4_TILE * D4_PITCH];
  const int tiles = tiles_h * tiles_w;
  const int plane = blockIdx.x / tiles, t = blockIdx.x - plane * tiles;
  const int op = ops ? (ops[plane / C] & 7) : op_all;
  const bool fh = op & 1, fv = op & 2;
  const size_t base = (size_t)plane * (size_t)H * (size_t)W;
  const float* src = in + base;
  float* dst = out + base;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;

  if (!(op & 4)) {
    // out[yo][xo] = in[fv ? H-1-yo : yo][fh ? W-1-xo : xo]
    const int ty = t / tiles_w, tx = t - ty * tiles_w;
    const int xo = tx * D4_TILE + lane;
    const int xi = fh ? W - 1 - xo : xo;
    const bool okx = xo < W;
    float v[D4_ROWS];
#pragma unroll
    for (int i = 0; i < D4_ROWS; ++i) {
      const int yo = ty * D4_TILE + wave + 4 * i;
      const int yi = fv ? H - 1 - yo : yo;
      v[i] = (okx && yo < H) ? src[(size_t)yi * W + xi] : 0.f;
    }
#pragma unroll
    for (int i = 0; i < D4_ROWS; ++i) {
      const int yo = ty * D4_TILE + wave + 4 * i;
      if (okx && yo < H) d4_store<MODE>(dst + (size_t)yo * W + xo, v[i], alpha);
    }
  } else {
    // out is [W][H]: out[yo][xo] = in[fv ? H-1-xo : xo][fh ? W-1-yo : yo]
    const int ty = t / tiles_h, tx = t - ty * tiles_h;          // ty over the W output rows, tx over the H output columns
    const int y0 = ty * D4_TILE, x0 = tx * D4_TILE;
    {  // tile[a][b] = out(y0 + b, x0 + a): input row <-> output column x0 + a, the lane runs along the input row
      const int yo = y0 + lane;
      const int xi = fh ? W - 1 - yo : yo;
      const bool okl = yo < W;
      float v[D4_ROWS];
#pragma unroll
      for (int i = 0; i < D4_ROWS; ++i) {
        const int xo = x0 + wave + 4 * i;
        const int yi = fv ? H - 1 - xo : xo;
        v[i] = (okl && xo < H) ? src[(size_t)yi * W + xi] : 0.f;
      }
#pragma unroll
      for (int i = 0; i < D4_ROWS; ++i) tile[(wave + 4 * i) * D4_PITCH + lane] = v[i];
    }
    __syncthreads();
    const int xo = x0 + lane;
    const bool okx = xo < H;
#pragma unroll
    for (int i = 0; i < D4_ROWS; ++i) {
      const int r = wave + 4 * i, yo = y0 + r;
      if (okx && yo < W) d4_store<MODE>(dst + (size_t)yo * H + xo, tile[lane * D4_PITCH + r], alpha);
    }
  }
}

}  // namespace

int srk_launch_dihedral_f32(const float* in, float* out, const int* ops, int op_all, int B, int C, int H, int W, float alpha,
                            int accumulate, hipStream_t stream) {
  const int tiles_h = cdiv(H, D4_TILE), tiles_w = cdiv(W, D4_TILE);
  const double blocks = (double)B * C * tiles_h * tiles_w;      // a double cannot overflow on four int factors
  SRK_REQUIRE(blocks >= 1.0 && blocks <= 2147483647.0, SRK_E_SHAPE, "dihedral: %.0f tiles do not fit one grid (B=%d C=%d H=%d W=%d)",
              blocks, B, C, H, W);
  const dim3 grid((unsigned)blocks), block(256);
  if (accumulate)
    hipLaunchKernelGGL(dihedral_kernel<D4_ACC>, grid, block, 0, stream, in, out, ops, op_all, C, H, W, tiles_h, tiles_w, alpha);
  else if (alpha == 1.0f)
    hipLaunchKernelGGL(dihedral_kernel<D4_COPY>, grid, block, 0, stream, in, out, ops, op_all, C, H, W, tiles_h, tiles_w, alpha);
  else
    hipLaunchKernelGGL(dihedral_kernel<D4_SCALE>, grid, block, 0, stream, in, out, ops, op_all, C, H, W, tiles_h, tiles_w, alpha);
  return srk_check_launch("dihedral_f32");
}
