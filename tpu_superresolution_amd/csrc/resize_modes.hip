// The ragged resize with a resize rule per sample (include/srk.h: srk_resize_ragged_mode_f32): Real-ESRGAN draws area, bilinear or
// bicubic for every resize of its chain, and the draw is per sample inside the one launch per stage of the ragged design.
//
// The resize kernels are table-driven -- a per-output tap list (resize.h: RsShared wx / wy / lo / cnt) and one filter over it (rs_filter)
// -- so a rule is a table builder.  Mode 0 calls rs_tables itself: the sample has the bits of srk_resize_aa_ragged_f32.  Modes 1 and 2
// fill the same tables:
//   bilinear  src = max(scale (i + 0.5) - 0.5, 0), i0 = min(floor(src), n_in - 1), l = src - i0: taps i0, min(i0 + 1, n_in - 1) with
//             weights 1 - l, l; one tap of weight 1 where both are one pixel
//   area      lo = (i n_in) / n_out, hi = ((i + 1) n_in + n_out - 1) / n_out (64-bit integers): hi - lo taps of weight 1 / (hi - lo)
// in fp64 with one rounding to fp32.  Both keep what rs_filter relies on: at most RS_TAPS taps (2, and ceil(8) + 1 = 9 at the 8x limit),
// lo and hi not decreasing along an axis, and under one tile at most 63 * 8 + 9 columns / 15 * 8 + 9 rows of input.
// The mode is uniform over a workgroup (one sample), so the branch costs nothing and every thread reaches the same barriers.
#include "ragged.h"
#include "resize.h"

#pragma clang fp contract(off)

namespace {

__device__ __forceinline__ int rm_mode(const int* __restrict__ mode, int b) {
  if (!mode) return 0;
  const int m = mode[b];
  return m < 0 ? 0 : (m > 2 ? 2 : m);
}

// taps of output i in [0, n_out) under `mode` 1 | 2: w[0 .. cnt) in fp32, first tap lo; every tap lies in [0, n_in)
__device__ __forceinline__ void rm_weights(int mode, const RsAxis& ax, int i, float* w, int* lo_out, int* cnt_out) {
  if (mode == 1) {
    double src = ax.scale * ((double)i + 0.5) - 0.5;
    src = src > 0.0 ? src : 0.0;
    int i0 = (int)floor(src);
    i0 = i0 > ax.n_in - 1 ? ax.n_in - 1 : i0;
    const double l = src - (double)i0;
    *lo_out = i0;
    if (i0 + 1 > ax.n_in - 1) {
      w[0] = 1.f;
      *cnt_out = 1;
    } else {
      w[0] = (float)(1.0 - l);
      w[1] = (float)l;
      *cnt_out = 2;
    }
  } else {
    const long long lo = ((long long)i * ax.n_in) / ax.n_out;
    long long hi = ((long long)(i + 1) * ax.n_in + ax.n_out - 1) / ax.n_out;
    hi = hi > ax.n_in ? ax.n_in : hi;
    int cnt = (int)(hi - lo);
    cnt = cnt < 1 ? 1 : (cnt > RS_TAPS ? RS_TAPS : cnt);          // beyond 8x (the caller's mistake): taps dropped, in bounds
    const float v = (float)(1.0 / (double)cnt);
    for (int j = 0; j < cnt; ++j) w[j] = v;
    *lo_out = (int)lo;
    *cnt_out = cnt;
  }
}

// rs_tables under mode 1 | 2: the same lanes fill the same slots, and the same barrier ends it
__device__ __forceinline__ void rm_tables(int mode, RsShared& sh, const RsAxis& ay, const RsAxis& ax, int oy0, int ny, int ox0, int nx) {
  const int t = threadIdx.x;
  if (t < nx) rm_weights(mode, ax, ox0 + t, sh.wx + t * RS_TAPS, &sh.lox[t], &sh.cx[t]);
  else if (t >= RS_TOX && t - RS_TOX < ny) rm_weights(mode, ay, oy0 + t - RS_TOX, sh.wy + (t - RS_TOX) * RS_TAPS, &sh.loy[t - RS_TOX], &sh.cy[t - RS_TOX]);
  __syncthreads();
}

__global__ __launch_bounds__(256) void resize_ragged_mode_kernel(const float* __restrict__ in, const int* __restrict__ ext_in,
                                                                 float* __restrict__ out, const int* __restrict__ ext_out,
                                                                 const int* __restrict__ mode, int C, int Hp, int Wp, int Hop, int Wop,
                                                                 int tiles_y, int tiles_x, int quant_bits) {
  __shared__ RsShared sh;
  const int tiles = tiles_y * tiles_x;
  const int plane = blockIdx.x / tiles, t = blockIdx.x - plane * tiles;
  const int ty = t / tiles_x, tx = t - ty * tiles_x;
  const int b = plane / C;
  const int H = rg_extent(ext_in, b, 0, Hp), W = rg_extent(ext_in, b, 1, Wp);
  const int Ho = rg_extent(ext_out, b, 0, Hop), Wo = rg_extent(ext_out, b, 1, Wop);
  const int oy0 = ty * RS_TOY, ox0 = tx * RS_TOX;
  if (oy0 >= Ho || ox0 >= Wo) return;
  const int ny = Ho - oy0 < RS_TOY ? Ho - oy0 : RS_TOY, nx = Wo - ox0 < RS_TOX ? Wo - ox0 : RS_TOX;
  const RsAxis ay = rs_axis(H, Ho), ax = rs_axis(W, Wo);
  const int m = rm_mode(mode, b);
  if (m == 0) rs_tables(sh, ay, ax, oy0, ny, ox0, nx);
  else rm_tables(m, sh, ay, ax, oy0, ny, ox0, nx);
  const float* src = in + (size_t)plane * (size_t)Hp * (size_t)Wp;
  float* dst = out + (size_t)plane * (size_t)Hop * (size_t)Wop;
  rs_filter(sh, [=](int r, int x) { return src[(size_t)r * Wp + x]; },
            [=](int k, int c, float v) { dst[(size_t)(oy0 + k) * Wop + (ox0 + c)] = v; }, ny, nx, quant_bits);
}

}  // namespace

int srk_launch_resize_ragged_mode_f32(const float* x, const int* ext_in, float* out, const int* ext_out, const int* mode, int B, int C, int Hp,
                                      int Wp, int Hop, int Wop, int quant_bits, hipStream_t stream) {
  const int tiles_y = cdiv(Hop, RS_TOY), tiles_x = cdiv(Wop, RS_TOX);
  const double blocks = (double)B * C * tiles_y * tiles_x;
  SRK_REQUIRE(blocks >= 1.0 && blocks <= 2147483647.0, SRK_E_SHAPE, "resize_ragged_mode: %.0f tiles do not fit one grid (B=%d C=%d Hop=%d Wop=%d)",
              blocks, B, C, Hop, Wop);
  hipLaunchKernelGGL(resize_ragged_mode_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, x, ext_in, out, ext_out, mode, C, Hp, Wp, Hop, Wop,
                     tiles_y, tiles_x, quant_bits);
  return srk_check_launch("resize_ragged_mode_f32");
}
