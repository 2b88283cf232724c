// Device-side evaluation metrics:
//   srk_eval_psnr   evaluate.py:24-29: per image 20 log10(max / sqrt(max(mse, 1e-10))), NO clamp; optionally the batch mean
//   srk_ssim        pytorch_msssim.ssim as the reference calls it (train.py:169, evaluate.py:127,195; package pinned at 1.0.0 in
//                   sr_environment.yml:165 but absent from the reference tree and from this image): Wang et al. 2004 with an
//                   11-tap Gaussian (sigma 1.5) applied separably as a VALID depth-wise filter, K = (0.01, 0.03), per-channel
//                   mean of the SSIM map, then mean over channels.  Restated from the published algorithm: PARITY UNPINNED
//                   (no reference-produced fixture exists); tests compare with the torch-operator form in metrics.py and an
//                   independent scipy evaluation.
// Sums are formed in a fixed order (partials + one finishing workgroup): results are reproducible.
#include <hip/hip_runtime.h>
#include <math.h>

#include "common.h"
#include "kernels.h"

namespace {

__global__ __launch_bounds__(256) void sqerr_partial_kernel(const float* __restrict__ x, const float* __restrict__ y, float* __restrict__ partial,
                                                            long long per_image) {
  __shared__ float red[4];
  const long long base = (long long)blockIdx.y * per_image;
  float sq = 0.f;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < per_image; i += (long long)gridDim.x * blockDim.x) {
    const float d = x[base + i] - y[base + i];
    sq = fmaf(d, d, sq);
  }
  sq = wave_sum64(sq);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = sq;
  __syncthreads();
  if (threadIdx.x == 0) partial[(long long)blockIdx.y * gridDim.x + blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

__global__ void eval_psnr_finish_kernel(const float* __restrict__ partial, int chunks, int B, long long per_image, float max_val,
                                        float* __restrict__ psnr, float* __restrict__ mean_out) {
  __shared__ float sh[1024];
  for (int b = threadIdx.x; b < B; b += blockDim.x) {
    float sq = 0.f;
    for (int c = 0; c < chunks; ++c) sq += partial[(long long)b * chunks + c];
    const float mse = fmaxf(sq / (float)per_image, 1e-10f);
    const float v = 20.0f * log10f(max_val / sqrtf(mse));
    if (psnr) psnr[b] = v;
    sh[b] = v;
  }
  __syncthreads();
  if (threadIdx.x == 0 && mean_out) {
    float s = 0.f;
    for (int b = 0; b < B; ++b) s += sh[b];
    *mean_out = s / (float)B;
  }
}

// ---- SSIM ----------------------------------------------------------------------------------------------------------------
constexpr int ST = 32;            // output tile (valid positions) per workgroup: 32 x 32
constexpr int SI = ST + 10;       // input tile 42 x 42
struct GaussWin { float w[11]; };

__global__ __launch_bounds__(256) void ssim_tile_kernel(const float* __restrict__ X, const float* __restrict__ Y, float* __restrict__ partial,
                                                        int H, int W, int tiles_x, int tiles_y, GaussWin gw, float C1, float C2) {
  __shared__ float xs[SI][SI + 1], ys[SI][SI + 1];
  __shared__ float hb[5][SI][ST + 1];        // horizontally filtered x, y, xx, yy, xy
  __shared__ float red[4];
  const int plane = blockIdx.z;                                 // b * C + c
  const int ty0 = blockIdx.y * ST, tx0 = blockIdx.x * ST;       // first valid output position of the tile
  const int OH = H - 10, OW = W - 10;
  const float* xp = X + (long long)plane * H * W;
  const float* yp = Y + (long long)plane * H * W;
  const int tid = threadIdx.x;
  for (int i = tid; i < SI * SI; i += 256) {
    const int r = i / SI, c = i - r * SI;
    const int gy = ty0 + r, gx = tx0 + c;
    const bool ok = gy < H && gx < W;
    xs[r][c] = ok ? xp[(long long)gy * W + gx] : 0.f;
    ys[r][c] = ok ? yp[(long long)gy * W + gx] : 0.f;
  }
  __syncthreads();
  for (int i = tid; i < SI * ST; i += 256) {
    const int r = i / ST, c = i - r * ST;
    float a = 0.f, b = 0.f, aa = 0.f, bb = 0.f, ab = 0.f;
#pragma unroll
    for (int k = 0; k < 11; ++k) {
      const float xv = xs[r][c + k], yv = ys[r][c + k], wk = gw.w[k];
      a = fmaf(wk, xv, a);
      b = fmaf(wk, yv, b);
      aa = fmaf(wk, xv * xv, aa);
      bb = fmaf(wk, yv * yv, bb);
      ab = fmaf(wk, xv * yv, ab);
    }
    hb[0][r][c] = a; hb[1][r][c] = b; hb[2][r][c] = aa; hb[3][r][c] = bb; hb[4][r][c] = ab;
  }
  __syncthreads();
  float acc = 0.f;
  for (int i = tid; i < ST * ST; i += 256) {
    const int r = i / ST, c = i - r * ST;
    if (ty0 + r >= OH || tx0 + c >= OW) continue;
    float m1 = 0.f, m2 = 0.f, xx = 0.f, yy = 0.f, xy = 0.f;
#pragma unroll
    for (int k = 0; k < 11; ++k) {
      const float wk = gw.w[k];
      m1 = fmaf(wk, hb[0][r + k][c], m1);
      m2 = fmaf(wk, hb[1][r + k][c], m2);
      xx = fmaf(wk, hb[2][r + k][c], xx);
      yy = fmaf(wk, hb[3][r + k][c], yy);
      xy = fmaf(wk, hb[4][r + k][c], xy);
    }
    const float s11 = xx - m1 * m1, s22 = yy - m2 * m2, s12 = xy - m1 * m2;
    const float cs = (2.f * s12 + C2) / (s11 + s22 + C2);
    acc += ((2.f * m1 * m2 + C1) / (m1 * m1 + m2 * m2 + C1)) * cs;
  }
  acc = wave_sum64(acc);
  if ((tid & 63) == 0) red[tid >> 6] = acc;
  __syncthreads();
  if (tid == 0) partial[((long long)plane * tiles_y + blockIdx.y) * tiles_x + blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

__global__ void ssim_finish_kernel(const float* __restrict__ partial, int tiles, int B, int C, float inv_count, float* __restrict__ per_image,
                                   float* __restrict__ mean_out) {
  __shared__ float sh[1024];
  for (int b = threadIdx.x; b < B; b += blockDim.x) {
    float s = 0.f;
    for (int c = 0; c < C; ++c) {
      float pc = 0.f;
      for (int t = 0; t < tiles; ++t) pc += partial[((long long)b * C + c) * tiles + t];
      s += pc * inv_count;                       // per-channel mean of the map
    }
    const float v = s / (float)C;
    if (per_image) per_image[b] = v;
    sh[b] = v;
  }
  __syncthreads();
  if (threadIdx.x == 0 && mean_out) {
    float s = 0.f;
    for (int b = 0; b < B; ++b) s += sh[b];
    *mean_out = s / (float)B;
  }
}

// ---- benchmark-protocol planes and PSNR (srk.h "Benchmark-protocol PSNR / SSIM") ----------------------------------
// A streaming pass: workgroup (chunk, image) takes `rpb` consecutive plane rows of one image -- about BENCH_ELEMS plane elements
// -- and walks them in groups of four input elements that are 16-byte aligned in the input row; a whole group is one dwordx4
// load per tensor and channel, the groups cut by the crop at a row's head and tail are scalar loads of the elements inside the
// crop only (nothing of the cropped-away frame is read).  The plane rows are dense (Wc), so a group's place in the output is
// 16-byte aligned only where crop offset and widths happen to agree: a dwordx4 store there, four dword stores elsewhere.
constexpr int BENCH_ELEMS = 8192;
inline int bench_rows_per_block(int Wc) { return Wc >= BENCH_ELEMS ? 1 : BENCH_ELEMS / Wc; }
inline int bench_chunks(int Cm, int Hc, int Wc) {
  const int rpb = bench_rows_per_block(Wc);
  return (int)(((long long)Cm * Hc + rpb - 1) / rpb);
}

__device__ __forceinline__ float bench_q(float x) {
  const float c = x < 0.f ? 0.f : (x > 1.f ? 1.f : x);          // comparisons: a NaN fails both and stays
  return rintf(__fmul_rn(c, 255.0f));
}
__device__ __forceinline__ float bench_luma(float r, float g, float b) {
  const float t = fmaf(24.966f, b, fmaf(128.553f, g, __fmul_rn(65.481f, r)));
  return __fadd_rn(16.0f, __fdiv_rn(t, 255.0f));
}
// elements j of p[0..4) with bit j of mask set; the others are never addressed
__device__ __forceinline__ void bench_load4(const float* __restrict__ p, unsigned mask, float v[4]) {
  if (mask == 0xFu && (reinterpret_cast<uintptr_t>(p) & 15) == 0) {
    const float4 t = *reinterpret_cast<const float4*>(p);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = ((mask >> j) & 1u) ? p[j] : 0.f;
  }
}
__device__ __forceinline__ void bench_store4(float* __restrict__ p, unsigned mask, const float v[4]) {
  if (mask == 0xFu && (reinterpret_cast<uintptr_t>(p) & 15) == 0) {
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if ((mask >> j) & 1u) p[j] = v[j];
  }
}

// Y3: C == 3 in, one luma plane out (rows = Hc); otherwise plane row R = c * Hc + r of the image is input channel c (rows = C * Hc)
template <bool Y3>
__global__ __launch_bounds__(256) void bench_planes_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                           float* __restrict__ pp, float* __restrict__ pt, float* __restrict__ partial,
                                                           int C, int H, int W, int border, int Hc, int Wc, int rows, int rpb) {
  __shared__ float red[4];
  const int b = blockIdx.y;
  const int R0 = blockIdx.x * rpb;
  const int nr = min(rpb, rows - R0);
  const int S = Wc / 4 + 2;                                     // aligned groups a row can touch, whatever its phase
  const long long plane = (long long)H * W;
  float sq = 0.f;
  for (int i = threadIdx.x; i < nr * S; i += 256) {
    const int rr = i / S, s = i - rr * S;
    const int R = R0 + rr;
    const int c = Y3 ? 0 : R / Hc, r = Y3 ? R : R - c * Hc;
    const long long in0 = (((long long)b * C + c) * H + border + r) * W + border;      // first element of the row inside the crop
    const long long x0 = 4LL * s - (in0 & 3);                   // crop column of the group's first element (-3..Wc+7)
    unsigned mask = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) mask |= (x0 + j >= 0 && x0 + j < Wc) ? (1u << j) : 0u;
    if (!mask) continue;
    float P[4], T[4];
    if (Y3) {
      float pr[4], pg[4], pb[4], tr[4], tg[4], tb[4];
      bench_load4(pred + in0 + x0, mask, pr);
      bench_load4(pred + in0 + x0 + plane, mask, pg);
      bench_load4(pred + in0 + x0 + 2 * plane, mask, pb);
      bench_load4(target + in0 + x0, mask, tr);
      bench_load4(target + in0 + x0 + plane, mask, tg);
      bench_load4(target + in0 + x0 + 2 * plane, mask, tb);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        P[j] = bench_luma(bench_q(pr[j]), bench_q(pg[j]), bench_q(pb[j]));
        T[j] = bench_luma(bench_q(tr[j]), bench_q(tg[j]), bench_q(tb[j]));
      }
    } else {
      bench_load4(pred + in0 + x0, mask, P);
      bench_load4(target + in0 + x0, mask, T);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        P[j] = bench_q(P[j]);
        T[j] = bench_q(T[j]);
      }
    }
    const long long o0 = ((long long)b * rows + R) * Wc + x0;
    if (pp) bench_store4(pp + o0, mask, P);
    if (pt) bench_store4(pt + o0, mask, T);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float d = P[j] - T[j];
      if ((mask >> j) & 1u) sq = fmaf(d, d, sq);
    }
  }
  sq = wave_sum64(sq);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = sq;
  __syncthreads();
  if (threadIdx.x == 0) partial[(long long)blockIdx.y * gridDim.x + blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

// One workgroup of 1024 threads.  A group of L lanes (a power of two <= 64, chosen on the host from the number of partials: a
// full-size image has hundreds, a training patch one) owns an image: lane l adds partials l, l + L, ... in order, then an xor
// butterfly adds the group's lanes -- a fixed order for a given shape.  The batch total is added by thread 0 in image order.
__global__ __launch_bounds__(1024) void bench_psnr_finish_kernel(const float* __restrict__ partial, int chunks, int B, int L, float count,
                                                                 float* __restrict__ sqsum, float* __restrict__ psnr,
                                                                 float* __restrict__ psnr_sum) {
  __shared__ float sh[1024];
  const int groups = 1024 / L, gi = threadIdx.x / L, l = threadIdx.x & (L - 1);
  for (int b0 = 0; b0 < B; b0 += groups) {                      // the same trip count for every thread: the shuffles see whole waves
    const int b = b0 + gi;
    float sq = 0.f;
    if (b < B)
      for (int c = l; c < chunks; c += L) sq += partial[(long long)b * chunks + c];
    for (int o = L >> 1; o > 0; o >>= 1) sq += __shfl_xor(sq, o, 64);
    if (b < B && l == 0) {
      const float mse = sq / count;
      const float v = mse == 0.f ? INFINITY : 10.0f * log10f(65025.0f / mse);      // a NaN mse is not 0: it reaches the result
      if (sqsum) sqsum[b] = sq;
      if (psnr) psnr[b] = v;
      sh[b] = v;
    }
  }
  __syncthreads();
  if (threadIdx.x == 0 && psnr_sum) {
    float s = 0.f;
    for (int b = 0; b < B; ++b) s += sh[b];
    *psnr_sum += s;
  }
}

}  // namespace

extern "C" {

int64_t srk_bench_workspace(int B, int Cm, int Hc, int Wc) {
  if (!srk_bench_plane_dims_ok(B, Cm, Hc, Wc)) return 0;
  return (int64_t)sizeof(float) * B * bench_chunks(Cm, Hc, Wc);
}

int srk_bench_planes_f32(const float* pred, const float* target, float* planes_pred, float* planes_target, void* workspace, int B, int C,
                         int H, int W, int border, int mode, srk_stream_t stream) {
  SRK_REQUIRE(pred && target && workspace, SRK_E_NULL, "bench_planes: null pointer");
  SRK_REQUIRE(srk_bench_planes_shape_ok(B, C, H, W, border, mode), SRK_E_SHAPE,
              "bench_planes: B=%d (1..1024) C=%d H=%d W=%d border=%d (0 <= 2 border < H, W) mode=%d (Y: C 1 or 3; RGB)", B, C, H, W, border, mode);
  const bool y3 = mode == SRK_BENCH_Y && C == 3;
  const int Cm = mode == SRK_BENCH_Y ? 1 : C, Hc = H - 2 * border, Wc = W - 2 * border;
  const size_t in_bytes = sizeof(float) * (size_t)B * C * H * W, out_bytes = sizeof(float) * (size_t)B * Cm * Hc * Wc;
  for (const float* o : {planes_pred, planes_target})
    SRK_REQUIRE(!o || (!srk_ranges_overlap(o, out_bytes, pred, in_bytes) && !srk_ranges_overlap(o, out_bytes, target, in_bytes)), SRK_E_SHAPE,
                "bench_planes: planes overlap an input");
  const int rows = Cm * Hc, rpb = bench_rows_per_block(Wc);
  const dim3 grid(bench_chunks(Cm, Hc, Wc), B);
  if (y3)
    hipLaunchKernelGGL(bench_planes_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, pred, target, planes_pred, planes_target,
                       static_cast<float*>(workspace), C, H, W, border, Hc, Wc, rows, rpb);
  else
    hipLaunchKernelGGL(bench_planes_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, pred, target, planes_pred, planes_target,
                       static_cast<float*>(workspace), C, H, W, border, Hc, Wc, rows, rpb);
  return srk_check_launch("bench_planes");
}

int srk_bench_psnr(const void* workspace, int B, int Cm, int Hc, int Wc, float* sqsum, float* psnr, float* psnr_sum, srk_stream_t stream) {
  SRK_REQUIRE(workspace && (sqsum || psnr || psnr_sum), SRK_E_NULL, "bench_psnr: null workspace, or no output");
  SRK_REQUIRE(srk_bench_plane_dims_ok(B, Cm, Hc, Wc), SRK_E_SHAPE, "bench_psnr: B=%d (1..1024) Cm=%d Hc=%d Wc=%d", B, Cm, Hc, Wc);
  const int chunks = bench_chunks(Cm, Hc, Wc);
  int L = 1;                                                    // lanes per image of the finish step
  while (L < 64 && L < chunks) L <<= 1;
  hipLaunchKernelGGL(bench_psnr_finish_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, static_cast<const float*>(workspace), chunks, B, L,
                     (float)((long long)Cm * Hc * Wc), sqsum, psnr, psnr_sum);
  return srk_check_launch("bench_psnr");
}

int64_t srk_eval_psnr_workspace(int64_t per_image, int B) {
  if (per_image <= 0 || B <= 0) return 0;
  return (int64_t)sizeof(float) * B * srk_batch_psnr_chunks(per_image);
}

int srk_eval_psnr(const float* x, const float* y, void* workspace, int B, int64_t per_image, float max_val, float* psnr, float* mean,
                  srk_stream_t stream) {
  SRK_REQUIRE(x && y && workspace, SRK_E_NULL, "eval_psnr: null pointer");
  SRK_REQUIRE(B > 0 && B <= 1024 && per_image > 0 && max_val > 0.f, SRK_E_SHAPE, "eval_psnr: B=%d (1..1024) per_image=%lld", B, (long long)per_image);
  const int chunks = srk_batch_psnr_chunks(per_image);
  hipLaunchKernelGGL(sqerr_partial_kernel, dim3(chunks, B), dim3(256), 0, (hipStream_t)stream, x, y, static_cast<float*>(workspace), per_image);
  hipLaunchKernelGGL(eval_psnr_finish_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, static_cast<const float*>(workspace), chunks, B,
                     per_image, max_val, psnr, mean);
  return srk_check_launch("eval_psnr");
}

int64_t srk_ssim_workspace(int B, int C, int H, int W) {
  if (B <= 0 || C <= 0 || H < 11 || W < 11) return 0;
  return (int64_t)sizeof(float) * B * C * ((H - 10 + ST - 1) / ST) * ((W - 10 + ST - 1) / ST);
}

int srk_ssim(const float* x, const float* y, void* workspace, int B, int C, int H, int W, float data_range, float* per_image, float* mean,
             srk_stream_t stream) {
  SRK_REQUIRE(x && y && workspace, SRK_E_NULL, "ssim: null pointer");
  SRK_REQUIRE(B > 0 && B <= 1024 && C > 0 && (long long)B * C < 65536, SRK_E_SHAPE, "ssim: B=%d C=%d", B, C);
  SRK_REQUIRE(H >= 11 && W >= 11, SRK_E_UNSUPPORTED, "ssim: the 11-tap window needs H, W >= 11 (got %dx%d)", H, W);
  SRK_REQUIRE(data_range > 0.f, SRK_E_SHAPE, "ssim: data_range=%g", (double)data_range);
  GaussWin gw;
  float sum = 0.f;
  for (int i = 0; i < 11; ++i) {
    const float c = (float)(i - 5);
    gw.w[i] = expf(-(c * c) / (2.0f * 1.5f * 1.5f));
    sum += gw.w[i];
  }
  for (int i = 0; i < 11; ++i) gw.w[i] /= sum;
  const int tx = (W - 10 + ST - 1) / ST, ty = (H - 10 + ST - 1) / ST;
  const float C1 = (0.01f * data_range) * (0.01f * data_range), C2 = (0.03f * data_range) * (0.03f * data_range);
  hipLaunchKernelGGL(ssim_tile_kernel, dim3(tx, ty, B * C), dim3(256), 0, (hipStream_t)stream, x, y, static_cast<float*>(workspace), H, W, tx, ty,
                     gw, C1, C2);
  hipLaunchKernelGGL(ssim_finish_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, static_cast<const float*>(workspace), tx * ty, B, C,
                     1.0f / ((float)(H - 10) * (float)(W - 10)), per_image, mean);
  return srk_check_launch("ssim");
}

}  // extern "C"
