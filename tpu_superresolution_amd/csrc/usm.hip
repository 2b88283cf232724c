// Separable unsharp mask (include/srk.h: srk_usm_sharpen_f32), Real-ESRGAN's USMSharp on the target image:
//   blur = G(x), res = x - blur, mask = |res| 255 > threshold, soft = G(mask), out = soft clamp(x + weight res) + (1 - soft) x
// with G the 1-D table run along rows and then along columns under a reflect-101 border.  The default table has 51 taps, beyond the 21 of
// filter2d.hip / blur2d.hip, and it is separable: 2 * 51 multiply-adds per pixel and pass where the 2-D form has 2601.
//
// G is one device routine (usm_gauss) and both launches run it, so both blurs follow the same chains:
//   launch 1  v = x:     res -> out, mask -> work
//   launch 2  v = mask:  soft = G(work); x, res = out at the thread's own pixel; out <- the blend
// Launch 2 reads out only at the pixel it then writes, from the same thread, so no tile sees another tile's result.
//
// One 256-thread workgroup makes one 32 x 64 tile of one plane:
//   1. v is staged in LDS with a halo of R on every side, element e of a row at e + e / 32 (the skew of blur2d_kernel).  The border rule is
//      applied by the staging -- a halo position holds the reflected pixel -- so the chains have one path and no masks.
//   2. horizontal pass over the 32 + 2R staged rows: a thread forms a strip of four neighbouring outputs with a sliding window, one LDS
//      read per tap and four fmaf; the result goes to hx[row][64] in LDS.
//   3. vertical pass: lane = column, a thread forms four consecutive rows with the same sliding window down hx.
// 82 x 118 + 82 x 65 floats = 60 KB of static LDS: two workgroups per CU.  Plain vector loads and stores, 64-bit offsets.
#include "kernels.h"

#pragma clang fp contract(off)

namespace {

constexpr int US_KMAX = SRK_USM_MAX_KS;
constexpr int US_TY = 32, US_TX = 64;
constexpr int US_TW = US_TX + US_KMAX - 1;                 // 114 staged columns
constexpr int US_PITCH = US_TW + US_TW / 32 + 1;           // 118
constexpr int US_TROWS = US_TY + US_KMAX - 1;              // 82 staged rows
constexpr int US_HP = US_TX + 1;                           // pitch of hx

__device__ __forceinline__ int us_skew(int e) { return e + (e >> 5); }

__device__ __forceinline__ int us_rho(int i, int n) {
  i = i < 0 ? -i : (i >= n ? 2 * (n - 1) - i : i);
  return i < 0 ? 0 : (i > n - 1 ? n - 1 : i);
}

struct UsShared {
  float tile[US_TROWS * US_PITCH];
  float hx[US_TROWS * US_HP];
  float k[US_KMAX + 1];
};

// G(v) on the tile (y0, x0) + nr x nc of an h x w plane `src`: emit(i, j, g) receives G(v)(y0 + i, x0 + j) once per pixel of the tile.
// Every thread of the workgroup calls it (it holds barriers).
template <class Emit>
__device__ __forceinline__ void usm_gauss(UsShared& sh, const float* __restrict__ src, const float* __restrict__ taps, int ks, int h, int w,
                                          int y0, int x0, int nr, int nc, const Emit& emit) {
  const int R = ks >> 1;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (threadIdx.x < ks) sh.k[threadIdx.x] = taps[threadIdx.x];
  // tile[i][j] = v(rho(y0 - R + i, h), rho(x0 - R + j, w)): every staged position is a pixel of the plane
  const int rows = nr + 2 * R, cols = ((nc + 3) & ~3) + 2 * R;
  for (int i = wave; i < rows; i += 4) {
    const float* srow = src + (size_t)us_rho(y0 - R + i, h) * (size_t)w;
    for (int j = lane; j < cols; j += 64) sh.tile[i * US_PITCH + us_skew(j)] = srow[us_rho(x0 - R + j, w)];
  }
  __syncthreads();

  const int strips = (nc + 3) >> 2;
  for (int it = threadIdx.x; it < rows * strips; it += 256) {
    const int i = it / strips, j0 = (it - i * strips) << 2;
    const float* row = sh.tile + i * US_PITCH;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    float v0 = row[us_skew(j0)], v1 = row[us_skew(j0 + 1)], v2 = row[us_skew(j0 + 2)], v3 = row[us_skew(j0 + 3)];
    const int cmax = cols - 1;          // the value read after the last tap is not used: its index is clamped into the staged row, no branch
#pragma unroll 4
    for (int j = 0; j < ks; ++j) {
      const float t = sh.k[j];
      const int c = j0 + j + 4;
      const float nx = row[us_skew(c < cmax ? c : cmax)];
      a0 = fmaf(t, v0, a0);
      a1 = fmaf(t, v1, a1);
      a2 = fmaf(t, v2, a2);
      a3 = fmaf(t, v3, a3);
      v0 = v1;
      v1 = v2;
      v2 = v3;
      v3 = nx;
    }
    float* o = sh.hx + i * US_HP + j0;
    o[0] = a0;
    o[1] = a1;
    o[2] = a2;
    o[3] = a3;
  }
  __syncthreads();

  // groups of four output rows: 8 groups, two per wave; a group past nr forms nothing
  for (int i0 = wave * 4; i0 < nr; i0 += 16) {
    if (lane < nc) {
      const float* col = sh.hx + lane;
      float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
      // rows i0 .. i0 + 3 + 2R are read; those past `rows` (nr not a multiple of 4) feed only accumulators that are not emitted
      const int last = rows - 1;
      auto at = [&](int r) { return col[(r < last ? r : last) * US_HP]; };
      float v0 = at(i0), v1 = at(i0 + 1), v2 = at(i0 + 2), v3 = at(i0 + 3);
#pragma unroll 4
      for (int a = 0; a < ks; ++a) {
        const float t = sh.k[a];
        const float nx = at(i0 + a + 4);          // clamped into the staged rows; the value read after the last tap is not used
        a0 = fmaf(t, v0, a0);
        a1 = fmaf(t, v1, a1);
        a2 = fmaf(t, v2, a2);
        a3 = fmaf(t, v3, a3);
        v0 = v1;
        v1 = v2;
        v2 = v3;
        v3 = nx;
      }
      emit(i0, lane, a0);
      if (i0 + 1 < nr) emit(i0 + 1, lane, a1);
      if (i0 + 2 < nr) emit(i0 + 2, lane, a2);
      if (i0 + 3 < nr) emit(i0 + 3, lane, a3);
    }
  }
}

// PASS 1: res -> out, mask -> work.  PASS 2: the blend -> out.
template <int PASS>
__global__ __launch_bounds__(256) void usm_kernel(const float* __restrict__ x, const float* __restrict__ taps, float* out, float* work, int H,
                                                  int W, int ks, int tiles_y, int tiles_x, float weight, float threshold) {
  __shared__ UsShared sh;
  const int tiles = tiles_y * tiles_x;
  const int plane = blockIdx.x / tiles, t = blockIdx.x - plane * tiles;
  const int ty = t / tiles_x, tx = t - ty * tiles_x;
  const int y0 = ty * US_TY, x0 = tx * US_TX;
  const int nr = H - y0 < US_TY ? H - y0 : US_TY, nc = W - x0 < US_TX ? W - x0 : US_TX;
  const size_t base = (size_t)plane * (size_t)H * (size_t)W;
  const float* xs = x + base;
  float* os = out + base;
  float* ws = work + base;
  if (PASS == 1) {
    usm_gauss(sh, xs, taps, ks, H, W, y0, x0, nr, nc, [=](int i, int j, float blur) {
      const size_t o = (size_t)(y0 + i) * (size_t)W + (size_t)(x0 + j);
      const float res = xs[o] - blur;
      os[o] = res;
      ws[o] = (fabsf(res) * 255.0f > threshold) ? 1.f : 0.f;
    });
  } else {
    usm_gauss(sh, ws, taps, ks, H, W, y0, x0, nr, nc, [=](int i, int j, float soft) {
      const size_t o = (size_t)(y0 + i) * (size_t)W + (size_t)(x0 + j);
      const float xv = xs[o], res = os[o];
      const float sharp = fminf(fmaxf(xv + weight * res, 0.f), 1.f);
      os[o] = soft * sharp + (1.0f - soft) * xv;
    });
  }
}

}  // namespace

int srk_launch_usm_sharpen_f32(const float* x, const float* taps, float* out, float* work, int B, int C, int H, int W, int ks, float weight,
                               float threshold, hipStream_t stream) {
  SRK_REQUIRE(srk_usm_ks_ok(ks) && srk_usm_extent_ok(H, W, ks), SRK_E_SHAPE, "usm_sharpen: ks=%d must be odd, in 1..%d and below 2 min(H, W)", ks,
              SRK_USM_MAX_KS);
  const int tiles_y = cdiv(H, US_TY), tiles_x = cdiv(W, US_TX);
  const double blocks = (double)B * C * tiles_y * tiles_x;
  SRK_REQUIRE(blocks >= 1.0 && blocks <= 2147483647.0, SRK_E_SHAPE, "usm_sharpen: %.0f tiles do not fit one grid (B=%d C=%d H=%d W=%d)", blocks, B, C,
              H, W);
  hipLaunchKernelGGL(usm_kernel<1>, dim3((unsigned)blocks), dim3(256), 0, stream, x, taps, out, work, H, W, ks, tiles_y, tiles_x, weight, threshold);
  int rc = srk_check_launch("usm_sharpen_f32 (mask)");
  if (rc != SRK_OK) return rc;
  hipLaunchKernelGGL(usm_kernel<2>, dim3((unsigned)blocks), dim3(256), 0, stream, x, taps, out, work, H, W, ks, tiles_y, tiles_x, weight, threshold);
  return srk_check_launch("usm_sharpen_f32 (blend)");
}
