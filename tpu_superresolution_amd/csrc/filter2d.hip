// Signed 2-D filter tables on the device (include/srk.h: srk_filter2d_f32): a per-sample ks x ks table -- a sinc (ringing) filter with
// negative lobes, or any table of blur_kernels -- applied as a CORRELATION with a reflect-101 border, cv2.filter2D's default and what
// Real-ESRGAN's filter2D does:
//   out(p, q) = chain over a, b ascending (a outer) of fmaf(K[a][b], x(rho(p + a - R, h), rho(q + b - R, w)), .) from 0
//   rho(i, n) = i < 0 ? -i : (i >= n ? 2 (n - 1) - i : i), then clamped into 0..n-1
// No mass and no division: a signed table has no mass rule (its in-image mass can vanish), which is why blur2d.hip cannot run it.
//
// One workgroup makes one 32 x 64 tile of one plane.  The tile is staged in LDS with a halo of R = KS / 2 on every side; the border rule is
// applied by the STAGING (a halo position holds the reflected pixel), so the chain has one path and no masks.  The layout, the strip of
// four outputs per thread, the rolled row loop around unrolled taps and the e + e / 32 skew are those of blur2d.hip.
// The batch may be ragged (ragged.h): h, w are the sample's extents, rows are Wp apart, a tile outside the extents leaves before any
// barrier, and neither a load nor a store leaves the extents.
// A delta table (centre tap 1, every other tap +-0) is a pass-through: the words of x are copied (with quant_bits 8: rounded), NaN
// payloads and -0 included -- the chain would give x + 0 there.
#include "ragged.h"
#include "resize.h"

#pragma clang fp contract(off)

namespace {

constexpr int F2_KMAX = 21;
constexpr int F2_TY = 32, F2_TX = 64;
constexpr int F2_TW = F2_TX + F2_KMAX - 1;
constexpr int F2_PITCH = F2_TW + F2_TW / 32 + 1;
constexpr int F2_TROWS = F2_TY + F2_KMAX - 1;

__device__ __forceinline__ int f2_skew(int e) { return e + (e >> 5); }

__device__ __forceinline__ int f2_rho(int i, int n) {
  i = i < 0 ? -i : (i >= n ? 2 * (n - 1) - i : i);
  return i < 0 ? 0 : (i > n - 1 ? n - 1 : i);
}

template <int KS>
__global__ __launch_bounds__(256) void filter2d_kernel(const float* __restrict__ in, const float* __restrict__ tab, float* __restrict__ out,
                                                       const int* __restrict__ ext, int C, int Hp, int Wp, int tiles_y, int tiles_x,
                                                       int quant_bits) {
  __shared__ float tile[F2_TROWS * F2_PITCH];
  __shared__ float K[KS * KS];
  constexpr int R = KS >> 1;
  const int tiles = tiles_y * tiles_x;
  const int plane = blockIdx.x / tiles, t = blockIdx.x - plane * tiles;
  const int ty = t / tiles_x, tx = t - ty * tiles_x;
  const int b = plane / C;
  const int h = rg_extent(ext, b, 0, Hp), w = rg_extent(ext, b, 1, Wp);
  const int y0 = ty * F2_TY, x0 = tx * F2_TX;
  if (y0 >= h || x0 >= w) return;                      // uniform over the workgroup, before any barrier
  const int nr = h - y0 < F2_TY ? h - y0 : F2_TY, nc = w - x0 < F2_TX ? w - x0 : F2_TX;
  const float* src = in + (size_t)plane * (size_t)Hp * (size_t)Wp;
  float* dst = out + (size_t)plane * (size_t)Hp * (size_t)Wp;

  int not_delta = 0;
  for (int i = threadIdx.x; i < KS * KS; i += 256) {
    const float v = tab[(size_t)b * (size_t)(KS * KS) + i];
    K[i] = v;
    not_delta |= (i == R * KS + R) ? (v != 1.f) : (v != 0.f);          // a NaN tap compares unequal: not a delta
  }
  // tile[i][j] = x(rho(y0 - R + i, h), rho(x0 - R + j, w)): every staged position is an in-extent pixel
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int rows = nr + 2 * R, cols = ((nc + 3) & ~3) + 2 * R;
  for (int i = wave; i < rows; i += 4) {
    const float* srow = src + (size_t)f2_rho(y0 - R + i, h) * Wp;
    for (int j = lane; j < cols; j += 64) tile[i * F2_PITCH + f2_skew(j)] = srow[f2_rho(x0 - R + j, w)];
  }
  if (!__syncthreads_or(not_delta)) {                  // pass-through, bit for bit
    for (int it = threadIdx.x; it < nr * nc; it += 256) {
      const int i = it / nc, j = it - i * nc;
      const float v = tile[(i + R) * F2_PITCH + f2_skew(j + R)];
      dst[(size_t)(y0 + i) * Wp + (x0 + j)] = quant_bits == 8 ? rs_quant8(v) : v;
    }
    return;
  }

  const int strips = (nc + 3) >> 2;
  for (int it = threadIdx.x; it < nr * strips; it += 256) {
    const int i = it / strips, j0 = (it - i * strips) << 2;
    float n0 = 0.f, n1 = 0.f, n2 = 0.f, n3 = 0.f;
#pragma unroll 1
    for (int a = 0; a < KS; ++a) {
      const float* row = tile + (i + a) * F2_PITCH;
      const float* kr = K + a * KS;
      float v[KS + 3], k[KS];
#pragma unroll
      for (int u = 0; u < KS + 3; ++u) v[u] = row[f2_skew(j0 + u)];
#pragma unroll
      for (int c = 0; c < KS; ++c) k[c] = kr[c];
#pragma unroll
      for (int c = 0; c < KS; ++c) {
        n0 = fmaf(k[c], v[c], n0);
        n1 = fmaf(k[c], v[c + 1], n1);
        n2 = fmaf(k[c], v[c + 2], n2);
        n3 = fmaf(k[c], v[c + 3], n3);
      }
    }
    if (quant_bits == 8) { n0 = rs_quant8(n0); n1 = rs_quant8(n1); n2 = rs_quant8(n2); n3 = rs_quant8(n3); }
    float* o = dst + (size_t)(y0 + i) * Wp + (x0 + j0);
    o[0] = n0;
    if (j0 + 1 < nc) o[1] = n1;
    if (j0 + 2 < nc) o[2] = n2;
    if (j0 + 3 < nc) o[3] = n3;
  }
}

}  // namespace

// ks is odd and in 1..21 here (srk_psf_ks_ok), anything else launches nothing
#define F2_FOR_KS(ks, X) \
  switch (ks) { X(1) X(3) X(5) X(7) X(9) X(11) X(13) X(15) X(17) X(19) X(21) default: break; }

int srk_launch_filter2d_f32(const float* x, const float* tab, float* out, const int* ext, int B, int C, int Hp, int Wp, int ks, int quant_bits,
                            hipStream_t stream) {
  SRK_REQUIRE(srk_psf_ks_ok(ks), SRK_E_SHAPE, "filter2d: ks must be odd and in 1..21 (got %d)", ks);
  const int tiles_y = cdiv(Hp, F2_TY), tiles_x = cdiv(Wp, F2_TX);
  const double blocks = (double)B * C * tiles_y * tiles_x;
  SRK_REQUIRE(blocks >= 1.0 && blocks <= 2147483647.0, SRK_E_SHAPE, "filter2d: %.0f tiles do not fit one grid (B=%d C=%d Hp=%d Wp=%d)", blocks, B,
              C, Hp, Wp);
#define F2_LAUNCH(N)                                                                                                                        \
  case N:                                                                                                                                   \
    hipLaunchKernelGGL(filter2d_kernel<N>, dim3((unsigned)blocks), dim3(256), 0, stream, x, tab, out, ext, C, Hp, Wp, tiles_y, tiles_x, \
                       quant_bits);                                                                                                         \
    break;
  F2_FOR_KS(ks, F2_LAUNCH)
#undef F2_LAUNCH
  return srk_check_launch("filter2d_f32");
}
