// No-reference quality: the device stages of NIQE (Mittal et al., "Making a completely blind image quality analyzer"), in the form of
// BasicSR's calculate_niqe (srk.h "No-reference quality (NIQE)").  Restated from the published algorithm: PARITY UNPINNED.
//   srk_niqe_plane_f32    8-bit quantisation, rounded BT.601 luma, border crop, crop to whole blocks
//   srk_niqe_half_f32     half-size antialiased cubic (MATLAB imresize(., 0.5)), exact in int32
//   srk_niqe_mscn_f32     mean-subtracted contrast-normalised map under a 7 x 7 window, centred form
//   srk_niqe_moments_f32  per block and product map: counts and square sums of both signs, sum of magnitudes
// The AGGD fit, the 36-dimensional Gaussian and the distance are host fp64 (niqe.py).  Every operation order the contract fixes is
// written with fmaf / __f*_rn, and contraction is off for the rest.  Sums are formed in a fixed order, no atomics: two runs give equal bits.
#include <hip/hip_runtime.h>
#include <math.h>

#include "common.h"

#pragma clang fp contract(off)

namespace {

// the shapes the four stages take: the grids fit (B rides in a 16-bit grid axis), a plane indexes below 2^40 elements
inline bool niqe_dims_ok(int B, int H, int W) {
  return B > 0 && B <= 65535 && H > 0 && W > 0 && H <= (1 << 20) && W <= (1 << 20) && 4.0 * B * H * W < 9.0e18;
}
inline size_t niqe_bytes(int B, long long H, long long W) { return sizeof(float) * (size_t)B * (size_t)H * (size_t)W; }

// ---- plane -------------------------------------------------------------------------------------------------------------------
// the quantisation and the luma chain of srk_bench_planes_f32 (metrics.hip), then one rintf of the luma
__device__ __forceinline__ float niqe_q(float x) {
  const float c = x < 0.f ? 0.f : (x > 1.f ? 1.f : x);          // comparisons: a NaN fails both and stays
  return rintf(__fmul_rn(c, 255.0f));
}
__device__ __forceinline__ float niqe_luma(float r, float g, float b) {
  const float t = fmaf(24.966f, b, fmaf(128.553f, g, __fmul_rn(65.481f, r)));
  return rintf(__fadd_rn(16.0f, __fdiv_rn(t, 255.0f)));
}

template <bool Y3>
__global__ __launch_bounds__(256) void niqe_plane_kernel(const float* __restrict__ x, float* __restrict__ plane, int C, int H, int W, int border,
                                                         int Hk, int Wk) {
  const long long per = (long long)Hk * Wk;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= per) return;
  const int b = blockIdx.y;
  const int r = (int)(i / Wk), c = (int)(i - (long long)r * Wk);
  const long long hw = (long long)H * W;
  const float* p = x + (long long)b * C * hw + (long long)(border + r) * W + border + c;
  plane[(long long)b * per + i] = Y3 ? niqe_luma(niqe_q(p[0]), niqe_q(p[hw]), niqe_q(p[2 * hw])) : niqe_q(p[0]);
}

// ---- half size -----------------------------------------------------------------------------------------------------------------
// out[i] = sum_k T[k] in[2 i - 3 + k] / 256 per axis, T = [-3, -9, 29, 111, 111, 29, -9, -3]; symmetric border.  The plane holds
// integers 0..255, so both passes are exact in int32 (|S| <= 304^2 * 255) and the order of the passes does not show.
constexpr int HT = 32;                // output tile
constexpr int HI = 2 * HT + 6;        // input tile 70 x 70
__device__ __forceinline__ int niqe_sym(int g, int n) {
  g = g < 0 ? -1 - g : (g >= n ? 2 * n - 1 - g : g);
  return min(max(g, 0), n - 1);       // only rows / columns that feed no stored output can still be outside
}

__global__ __launch_bounds__(256) void niqe_half_kernel(const float* __restrict__ plane, float* __restrict__ half, int H, int W) {
  __shared__ int tile[HI][HI + 1];
  __shared__ int hz[HI][HT + 1];
  const int T[8] = {-3, -9, 29, 111, 111, 29, -9, -3};
  const int Ho = H >> 1, Wo = W >> 1;
  const int oy0 = blockIdx.y * HT, ox0 = blockIdx.x * HT;
  const float* src = plane + (long long)blockIdx.z * H * W;
  const int tid = threadIdx.x;
  for (int i = tid; i < HI * HI; i += 256) {
    const int r = i / HI, c = i - r * HI;
    const int gy = niqe_sym(2 * oy0 - 3 + r, H), gx = niqe_sym(2 * ox0 - 3 + c, W);
    tile[r][c] = (int)src[(long long)gy * W + gx];
  }
  __syncthreads();
  for (int i = tid; i < HI * HT; i += 256) {
    const int r = i / HT, c = i - r * HT;
    int s = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) s += T[k] * tile[r][2 * c + k];
    hz[r][c] = s;
  }
  __syncthreads();
  for (int i = tid; i < HT * HT; i += 256) {
    const int r = i / HT, c = i - r * HT;
    if (oy0 + r >= Ho || ox0 + c >= Wo) continue;
    int s = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) s += T[k] * hz[2 * r + k][c];
    half[((long long)blockIdx.z * Ho + oy0 + r) * Wo + ox0 + c] = __fmul_rn((float)s, 1.52587890625e-05f);      // one rounding, then 2^-16
  }
}

// ---- MSCN ----------------------------------------------------------------------------------------------------------------------
// d = v - v_centre (exact: integers); a = sum w d, b = sum w d^2 by fmaf over the 49 taps in row-major order;
// sigma = sqrtf(fabsf(b - a a)); m = -a / (sigma + 1).  Replicate border.
constexpr int MT = 32;                // output tile
constexpr int MI = MT + 6;            // input tile 38 x 38

__global__ __launch_bounds__(256) void niqe_mscn_kernel(const float* __restrict__ plane, const float* __restrict__ win, float* __restrict__ mscn,
                                                        float* __restrict__ sigma, int H, int W) {
  __shared__ float tile[MI][MI + 1];
  __shared__ float ws[49];
  const int y0 = blockIdx.y * MT, x0 = blockIdx.x * MT;
  const long long img = (long long)blockIdx.z * H * W;
  const float* src = plane + img;
  const int tid = threadIdx.x;
  if (tid < 49) ws[tid] = win[tid];
  for (int i = tid; i < MI * MI; i += 256) {
    const int r = i / MI, c = i - r * MI;
    const int gy = min(max(y0 - 3 + r, 0), H - 1), gx = min(max(x0 - 3 + c, 0), W - 1);
    tile[r][c] = src[(long long)gy * W + gx];
  }
  __syncthreads();
  float w[49];
#pragma unroll
  for (int k = 0; k < 49; ++k) w[k] = ws[k];
  const int tx = tid & 31, ty = tid >> 5;
#pragma unroll 1
  for (int j = 0; j < MT / 8; ++j) {
    const int r = ty + 8 * j;
    if (y0 + r >= H || x0 + tx >= W) continue;
    const float vc = tile[r + 3][tx + 3];
    float a = 0.f, b = 0.f;
#pragma unroll
    for (int dy = 0; dy < 7; ++dy)
#pragma unroll
      for (int dx = 0; dx < 7; ++dx) {
        const float d = __fsub_rn(tile[r + dy][tx + dx], vc);
        a = fmaf(w[dy * 7 + dx], d, a);
        b = fmaf(w[dy * 7 + dx], __fmul_rn(d, d), b);
      }
    const float sg = __fsqrt_rn(fabsf(__fsub_rn(b, __fmul_rn(a, a))));
    const long long o = img + (long long)(y0 + r) * W + x0 + tx;
    mscn[o] = __fdiv_rn(-a, __fadd_rn(sg, 1.0f));
    if (sigma) sigma[o] = sg;
  }
}

// ---- block moments ---------------------------------------------------------------------------------------------------------------
// One workgroup per (block, image).  Thread t takes the block's pixels t, t + 256, ... in order; per pixel the five maps m, m roll(m, (0,1)),
// (1,0), (1,1), (1,-1) -- the roll circular inside the block -- feed five accumulators each; then an xor butterfly over the wave and the
// four waves added in order.  A NaN product is on neither side and reaches the sum of magnitudes.
__global__ __launch_bounds__(256) void niqe_moments_kernel(const float* __restrict__ mscn, const float* __restrict__ sigma, float* __restrict__ mom,
                                                           float* __restrict__ sharp, int H, int W, int bs, int nbw) {
  __shared__ float red[4][26];
  const int blk = blockIdx.x, b = blockIdx.y, nb = gridDim.x;
  const int by = blk / nbw, bx = blk - by * nbw;
  const long long off = ((long long)b * H + (long long)by * bs) * W + (long long)bx * bs;
  const float* base = mscn + off;
  float acc[26];
#pragma unroll
  for (int k = 0; k < 26; ++k) acc[k] = 0.f;
  const int n = bs * bs;
  for (int i = threadIdx.x; i < n; i += 256) {
    const int r = i / bs, c = i - r * bs;
    const int rm = r == 0 ? bs - 1 : r - 1, cm = c == 0 ? bs - 1 : c - 1, cp = c == bs - 1 ? 0 : c + 1;
    const float* row = base + (long long)r * W;
    const float* up = base + (long long)rm * W;
    const float m = row[c];
    float p[5];
    p[0] = m;
    p[1] = __fmul_rn(m, row[cm]);
    p[2] = __fmul_rn(m, up[c]);
    p[3] = __fmul_rn(m, up[cm]);
    p[4] = __fmul_rn(m, up[cp]);
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      const float v = p[k];
      if (v < 0.f) {
        acc[5 * k + 0] += 1.0f;
        acc[5 * k + 1] = fmaf(v, v, acc[5 * k + 1]);
      }
      if (v > 0.f) {
        acc[5 * k + 2] += 1.0f;
        acc[5 * k + 3] = fmaf(v, v, acc[5 * k + 3]);
      }
      acc[5 * k + 4] += fabsf(v);
    }
    if (sigma) acc[25] += sigma[off + (long long)r * W + c];
  }
#pragma unroll
  for (int k = 0; k < 26; ++k) {
    const float s = wave_sum64(acc[k]);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][k] = s;
  }
  __syncthreads();
  const int t = threadIdx.x;
  if (t < 26) {
    const float s = ((red[0][t] + red[1][t]) + red[2][t]) + red[3][t];
    if (t < 25) mom[((long long)b * nb + blk) * 25 + t] = s;
    else if (sharp) sharp[(long long)b * nb + blk] = __fdiv_rn(s, (float)n);
  }
}

}  // namespace

extern "C" {

int srk_niqe_plane_f32(const float* x, float* plane, int B, int C, int H, int W, int border, int bs, srk_stream_t stream) {
  SRK_REQUIRE(x && plane, SRK_E_NULL, "niqe_plane: null pointer");
  SRK_REQUIRE(niqe_dims_ok(B, H, W) && (C == 1 || C == 3) && border >= 0 && bs >= 8 && (bs & 1) == 0, SRK_E_SHAPE,
              "niqe_plane: B=%d (1..65535) C=%d (1 or 3) H=%d W=%d (1..2^20) border=%d (>= 0) bs=%d (even, >= 8)", B, C, H, W, border, bs);
  const int Hk = border <= (H - 1) / 2 ? (H - 2 * border) / bs * bs : 0, Wk = border <= (W - 1) / 2 ? (W - 2 * border) / bs * bs : 0;
  SRK_REQUIRE(Hk > 0 && Wk > 0, SRK_E_UNSUPPORTED, "niqe_plane: %d x %d with a border of %d holds no block of %d x %d", H, W, border, bs, bs);
  SRK_REQUIRE(((long long)Hk * Wk + 255) / 256 <= 0x7fffffffLL, SRK_E_SHAPE, "niqe_plane: a plane of %d x %d does not fit a grid", Hk, Wk);
  SRK_REQUIRE(!srk_ranges_overlap(plane, niqe_bytes(B, Hk, Wk), x, niqe_bytes(B, (long long)C * H, W)), SRK_E_SHAPE, "niqe_plane: plane overlaps x");
  const dim3 grid((unsigned)(((long long)Hk * Wk + 255) / 256), B);
  if (C == 3)
    hipLaunchKernelGGL(niqe_plane_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, x, plane, C, H, W, border, Hk, Wk);
  else
    hipLaunchKernelGGL(niqe_plane_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, x, plane, C, H, W, border, Hk, Wk);
  return srk_check_launch("niqe_plane");
}

int srk_niqe_half_f32(const float* plane, float* half, int B, int H, int W, srk_stream_t stream) {
  SRK_REQUIRE(plane && half, SRK_E_NULL, "niqe_half: null pointer");
  SRK_REQUIRE(niqe_dims_ok(B, H, W) && H >= 4 && W >= 4 && (H & 1) == 0 && (W & 1) == 0, SRK_E_SHAPE,
              "niqe_half: B=%d (1..65535) H=%d W=%d (even, 4..2^20)", B, H, W);
  SRK_REQUIRE(!srk_ranges_overlap(half, niqe_bytes(B, H / 2, W / 2), plane, niqe_bytes(B, H, W)), SRK_E_SHAPE, "niqe_half: half overlaps plane");
  hipLaunchKernelGGL(niqe_half_kernel, dim3(cdiv(W / 2, HT), cdiv(H / 2, HT), B), dim3(256), 0, (hipStream_t)stream, plane, half, H, W);
  return srk_check_launch("niqe_half");
}

int srk_niqe_mscn_f32(const float* plane, const float* win49, float* mscn, float* sigma, int B, int H, int W, srk_stream_t stream) {
  SRK_REQUIRE(plane && win49 && mscn, SRK_E_NULL, "niqe_mscn: null pointer");
  SRK_REQUIRE(niqe_dims_ok(B, H, W), SRK_E_SHAPE, "niqe_mscn: B=%d (1..65535) H=%d W=%d (1..2^20)", B, H, W);
  const size_t bytes = niqe_bytes(B, H, W);
  SRK_REQUIRE(!srk_ranges_overlap(mscn, bytes, plane, bytes) && !srk_ranges_overlap(mscn, bytes, win49, 49 * sizeof(float)) &&
                  (!sigma || (!srk_ranges_overlap(sigma, bytes, plane, bytes) && !srk_ranges_overlap(sigma, bytes, win49, 49 * sizeof(float)) &&
                              !srk_ranges_overlap(sigma, bytes, mscn, bytes))),
              SRK_E_SHAPE, "niqe_mscn: an output overlaps another buffer");
  hipLaunchKernelGGL(niqe_mscn_kernel, dim3(cdiv(W, MT), cdiv(H, MT), B), dim3(256), 0, (hipStream_t)stream, plane, win49, mscn, sigma, H, W);
  return srk_check_launch("niqe_mscn");
}

int srk_niqe_moments_f32(const float* mscn, const float* sigma, float* mom, float* sharp, int B, int H, int W, int bs, srk_stream_t stream) {
  SRK_REQUIRE(mscn && mom && (sigma != nullptr) == (sharp != nullptr), SRK_E_NULL, "niqe_moments: null pointer (sigma and sharp go together)");
  SRK_REQUIRE(niqe_dims_ok(B, H, W) && bs >= 4 && bs <= 4096, SRK_E_SHAPE, "niqe_moments: B=%d (1..65535) H=%d W=%d (1..2^20) bs=%d (4..4096)", B, H, W, bs);
  SRK_REQUIRE(H >= bs && W >= bs, SRK_E_UNSUPPORTED, "niqe_moments: %d x %d holds no block of %d x %d", H, W, bs, bs);
  SRK_REQUIRE(H % bs == 0 && W % bs == 0, SRK_E_SHAPE, "niqe_moments: H=%d W=%d must be multiples of bs=%d", H, W, bs);
  const long long nb = (long long)(H / bs) * (W / bs);
  SRK_REQUIRE(nb <= 0x7fffffffLL, SRK_E_SHAPE, "niqe_moments: %lld blocks per image do not fit a grid", nb);
  const size_t in_bytes = niqe_bytes(B, H, W), mom_bytes = sizeof(float) * 25 * (size_t)B * (size_t)nb, sharp_bytes = sizeof(float) * (size_t)B * (size_t)nb;
  SRK_REQUIRE(!srk_ranges_overlap(mom, mom_bytes, mscn, in_bytes) && !(sigma && srk_ranges_overlap(mom, mom_bytes, sigma, in_bytes)) &&
                  !(sharp && (srk_ranges_overlap(sharp, sharp_bytes, mscn, in_bytes) || srk_ranges_overlap(sharp, sharp_bytes, sigma, in_bytes) ||
                              srk_ranges_overlap(sharp, sharp_bytes, mom, mom_bytes))),
              SRK_E_SHAPE, "niqe_moments: an output overlaps another buffer");
  hipLaunchKernelGGL(niqe_moments_kernel, dim3((unsigned)nb, B), dim3(256), 0, (hipStream_t)stream, mscn, sigma, mom, sharp, H, W, bs, W / bs);
  return srk_check_launch("niqe_moments");
}

}  // extern "C"
