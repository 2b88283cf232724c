// Frequency loss (include/srk.h: srk_fft_loss_fwd_bwd): the L1 distance between the 2-D real FFTs of prediction and
// target, value and gradient from one call, no vendor FFT.
//   d = x - y,  D = rfft2(d) (unnormalised; s = 1, or s = 1 / sqrt(H W) with ortho),  Wh = W / 2 + 1,  N = 2 B C H Wh
//   L = (s / N) sum_{u < H, v < Wh} |Re D| + |Im D|
//   dL/dx[y][x] = (s / N) Re sum_{u < H, v < Wh} G[u][v] exp(+2 pi i (u y / H + v x / W)),  G = sign(Re D) + i sign(Im D), sign(0) = 0
// The gradient is the true adjoint over the HALF spectrum (no Hermitian doubling of the interior columns).  At the up-to-four
// self-conjugate bins (u in {0, H/2}, v in {0, W/2}, the halves only for even extents) Im D is structurally zero and its sign term is
// 0: the twiddles there are exactly 0 / +-1 (below), and the epilogue masks the bins as well.
//
// The DFTs are matrix products on the fp32-input MFMA (v_mfma_f32_32x32x2_f32: bit-for-bit a k-ordered fmaf chain), one kernel
// template for the four products.  Every product reads its data operand k-major ([k][m], the lane index m contiguous), so that no
// stage walks memory across rows; a small kernel writes d transposed for the first one:
//   0  dt[x][y] = x[y][x] - y[y][x]                                         (32 x 32 tiles through LDS)
//   1  T[y][v]  = sum_x dt[x][y] (cw - i sw)(v x)                            chain W        (rows y, lanes v)
//   2  D[u][v]  = sum_y (ch - i sh)(u y) T[y][v]                             chain 2 H      (rows u, lanes v)
//      epilogue: |Re| + |Im| into the workgroup's partial, G = signs into the workspace; D never goes to memory
//   3  Pt[v][y] = sum_u G[u][v] (ch + i sh)(u y)                             chain 2 H      (rows v, lanes y)
//   4  g[y][x]  = sum_v Re Pt[v][y] cw(v x) - Im Pt[v][y] sw(v x)            chain 2 Wh     (rows y, lanes x)
//      epilogue: d_x = or += coef * g, coef = alpha s / N formed in fp64 and rounded once
// Twiddles: tables c[k] = cos(2 pi k / n), s[k] = sin(2 pi k / n) for k < n, n = H and W, built by a kernel of the same call into the
// workspace from fp64 sincospi(2 k / n) rounded once (quarter turns are exactly 0 and +-1); a lane walks the reduced index
// (t k) mod n with one add and one conditional subtract per k step.  No host -> device copy, no host read: the call can be captured.
// The loss sum has a fixed order (a lane's 2 x 16 accumulators, the wave butterfly, then one finishing workgroup over the per-wave
// partials): two calls give the same bits.  No float atomics.
#include <hip/hip_runtime.h>
#include <math.h>

#include "common.h"
#include "kernels.h"

namespace {

using f32x16 = __attribute__((ext_vector_type(16))) float;
constexpr int NT = 2;              // 32 x 32 MFMA tiles of one wave along the twiddle index (fft_stage_kernel)
constexpr int FMAX = 512;          // largest H, W (the twiddle table of a stage sits in LDS)

struct FftWs {                     // offsets into the workspace, in floats
  long long tab_h, tab_w, partial, dt, t, g, total;
  int tiles_u, tiles_v;
};

FftWs fft_ws(int B, int C, int H, int W) {
  FftWs w;
  const long long planes = (long long)B * C, Wh = W / 2 + 1;
  w.tiles_u = cdiv(H, 32 * NT);                // the stage-2 grid: one partial per wave
  w.tiles_v = cdiv((int)Wh, 32);
  w.tab_h = 0;
  w.tab_w = w.tab_h + 2LL * H;
  w.partial = w.tab_w + 2LL * W;
  w.dt = w.partial + planes * w.tiles_u * w.tiles_v;
  w.t = w.dt + planes * H * W;                 // T, later Pt
  w.g = w.t + 2 * planes * H * Wh;
  w.total = w.g + 2 * planes * H * Wh;
  return w;
}

__global__ __launch_bounds__(256) void fft_twiddle_kernel(float* __restrict__ tab_h, int H, float* __restrict__ tab_w, int W) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  double s, c;
  if (i < H) {
    sincospi(2.0 * (double)i / (double)H, &s, &c);
    tab_h[i] = (float)c;
    tab_h[H + i] = (float)s;
  }
  if (i < W) {
    sincospi(2.0 * (double)i / (double)W, &s, &c);
    tab_w[i] = (float)c;
    tab_w[W + i] = (float)s;
  }
}

__global__ __launch_bounds__(256) void fft_diff_t_kernel(const float* __restrict__ X, const float* __restrict__ Y, float* __restrict__ dt,
                                                         int H, int W) {
  __shared__ float tile[32][33];
  const long long base = (long long)blockIdx.z * H * W;
  const int x0 = blockIdx.x * 32, y0 = blockIdx.y * 32, tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int r = ty; r < 32; r += 8) {
    const int y = y0 + r, x = x0 + tx;
    tile[r][tx] = (y < H && x < W) ? X[base + (long long)y * W + x] - Y[base + (long long)y * W + x] : 0.f;
  }
  __syncthreads();
  for (int r = ty; r < 32; r += 8) {
    const int x = x0 + r, y = y0 + tx;
    if (x < W && y < H) dt[base + (long long)x * H + y] = tile[tx][r];
  }
}

__device__ __forceinline__ float sign0(float v) { return v > 0.f ? 1.f : (v < 0.f ? -1.f : 0.f); }

// One of the four products (the file comment).  data: [plane][1 or 2 components][K][M]; the twiddle index t has extent T and modulus
// n.  Stage 2 has the twiddle index on the rows (MFMA operand A) and the data index on the lanes; the others the reverse.
// A workgroup is ONE wave: it owns 32 data indices x NT * 32 twiddle indices, so that every data element it loads feeds NT MFMA
// tiles (the twiddle operand costs an LDS lookup, the data operand L2 bandwidth: with one tile per load the stages were bound by it),
// and the dispatcher balances single waves over the SIMDs.
template <int STAGE>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(3, 8))) void fft_stage_kernel(const float* __restrict__ data, const float* __restrict__ tab, float* __restrict__ out,
                                                       float* __restrict__ partial, int H, int W, float coef, int accumulate) {
  __shared__ float2 tw[FMAX];
  constexpr bool TW_ROWS = STAGE == 2;
  constexpr int NC = STAGE == 1 ? 1 : 2;
  const int Wh = W / 2 + 1;
  const int n = (STAGE == 1 || STAGE == 4) ? W : H;
  const int K = STAGE == 1 ? W : (STAGE == 4 ? Wh : H);
  const int M = (STAGE == 1 || STAGE == 4) ? H : Wh;
  const int T = STAGE == 1 ? Wh : (STAGE == 4 ? W : H);
  const int rows = TW_ROWS ? T : M, cols = TW_ROWS ? M : T;
  const int lane = threadIdx.x, r = lane & 31, h = lane >> 5;
  const long long plane = blockIdx.z;
  for (int i = lane; i < n; i += 64) tw[i] = make_float2(tab[i], tab[n + i]);
  __syncthreads();
  const int row0 = blockIdx.y * (TW_ROWS ? 32 * NT : 32), col0 = blockIdx.x * (TW_ROWS ? 32 : 32 * NT);
  const int m = (TW_ROWS ? col0 : row0) + r, t0 = TW_ROWS ? row0 : col0;
  const bool mok = m < M;
  const long long cs = (long long)K * M;                   // one component of one plane
  const float* dp = data + plane * NC * cs + (mok ? m : M - 1);
  int idx[NT], step[NT];
  f32x16 acc0[NT], acc1[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    const int t = (t0 + 32 * j + r) % n;
    idx[j] = h ? t : 0;                                     // (t k) mod n at k = h
    step[j] = (2 * t) % n;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc0[j][i] = acc1[j][i] = 0.f;
  }
  constexpr int KU = 8;                                     // k steps per group
  // Software pipeline: the data of group g + 1 is requested before the MFMAs of group g and first touched after them.  The
  // scheduling barriers keep the compiler from sinking each load next to its use (it did: every k step then waited a full memory
  // latency).  Rows are clamped to K - 1, so the request past the last group reads valid memory; steps past K multiply zeros.
  float a[KU], b[KU], an[KU], bn[KU];
  auto request = [&](int k0, float (&ra)[KU], float (&rb)[KU]) {
#pragma unroll
    for (int q = 0; q < KU; ++q) {
      const int k = k0 + 2 * q + h;
      const long long off = (long long)(k < K ? k : K - 1) * M;          // clamped: nothing outside the operand is read
      ra[q] = dp[off];
      rb[q] = NC == 2 ? dp[cs + off] : 0.f;
    }
  };
  request(0, a, b);
  for (int k0 = 0; k0 < K; k0 += 2 * KU) {
    float2 w[KU][NT];
    request(k0 + 2 * KU, an, bn);
#pragma unroll
    for (int q = 0; q < KU; ++q) {
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        w[q][j] = tw[idx[j]];
        idx[j] += step[j];
        idx[j] -= idx[j] >= n ? n : 0;
      }
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int q = 0; q < KU; ++q) {
      const bool ok = mok && k0 + 2 * q + h < K;
      a[q] = ok ? a[q] : 0.f;
      b[q] = ok ? b[q] : 0.f;
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        const float2 wv = w[q][j];
        if constexpr (STAGE == 1) {
          acc0[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[q], wv.x, acc0[j], 0, 0, 0);
          acc1[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[q], -wv.y, acc1[j], 0, 0, 0);
        } else if constexpr (STAGE == 2) {                  // (c - i s)(a + i b)
          acc0[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(wv.x, a[q], acc0[j], 0, 0, 0);
          acc1[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(wv.x, b[q], acc1[j], 0, 0, 0);
          acc0[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(wv.y, b[q], acc0[j], 0, 0, 0);
          acc1[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(-wv.y, a[q], acc1[j], 0, 0, 0);
        } else if constexpr (STAGE == 3) {                  // (a + i b)(c + i s)
          acc0[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[q], wv.x, acc0[j], 0, 0, 0);
          acc1[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(b[q], wv.x, acc1[j], 0, 0, 0);
          acc0[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(b[q], -wv.y, acc0[j], 0, 0, 0);
          acc1[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[q], wv.y, acc1[j], 0, 0, 0);
        } else {                                            // Re (a + i b)(c + i s)
          acc0[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[q], wv.x, acc0[j], 0, 0, 0);
          acc0[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(b[q], -wv.y, acc0[j], 0, 0, 0);
        }
      }
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int q = 0; q < KU; ++q) {
      a[q] = an[q];
      b[q] = bn[q];
    }
  }
  // C / D map of the 32 x 32 MFMA: column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
  const long long ocs = (long long)rows * cols;            // one component of one output plane
  float sum = 0.f;
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    const int col = col0 + (TW_ROWS ? 0 : 32 * j) + r;
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
      const int row = row0 + (TW_ROWS ? 32 * j : 0) + (reg & 3) + 8 * (reg >> 2) + 4 * h;
      if (row >= rows || col >= cols) continue;
      if constexpr (STAGE == 1 || STAGE == 3) {
        float* o = out + plane * 2 * ocs + (long long)row * cols + col;
        o[0] = acc0[j][reg];
        o[ocs] = acc1[j][reg];
      } else if constexpr (STAGE == 2) {
        const bool structural = (row == 0 || 2 * row == H) && (col == 0 || 2 * col == W);
        const float re = acc0[j][reg], im = structural ? 0.f : acc1[j][reg];
        sum += fabsf(re) + fabsf(im);
        if (out) {
          float* o = out + plane * 2 * ocs + (long long)row * cols + col;
          o[0] = sign0(re);
          o[ocs] = sign0(im);
        }
      } else {
        // one rounded product, one rounded addition (never contracted into an fma): what is added is exactly what would be stored
        const float v = __fmul_rn(coef, acc0[j][reg]);
        float* o = out + plane * H * W + (long long)row * W + col;
        *o = accumulate ? __fadd_rn(*o, v) : v;
      }
    }
  }
  if constexpr (STAGE == 2) {
    sum = wave_sum64(sum);
    if (lane == 0) partial[(plane * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = sum;
  }
}

__global__ __launch_bounds__(256) void fft_loss_finish_kernel(const float* __restrict__ partial, long long count, float scale, float alpha,
                                                              float* __restrict__ value, float* __restrict__ loss) {
  __shared__ float red[4];
  float s = 0.f;
  for (long long i = threadIdx.x; i < count; i += 256) s += partial[i];
  s = wave_sum64(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    const float L = __fmul_rn((red[0] + red[1]) + (red[2] + red[3]), scale);
    if (value) value[0] = L;
    if (loss) loss[0] = __fadd_rn(loss[0], __fmul_rn(alpha, L));
  }
}

}  // namespace

long long srk_fft_loss_workspace_bytes(int B, int C, int H, int W) {
  if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || H > FMAX || W > FMAX || (long long)B * C >= 65536) return 0;
  return (long long)sizeof(float) * fft_ws(B, C, H, W).total;
}

int srk_launch_fft_loss(const float* x, const float* y, float* ws, int B, int C, int H, int W, int ortho, float alpha, float* d_x,
                        int accumulate, float* value, float* loss, hipStream_t stream) {
  const FftWs o = fft_ws(B, C, H, W);
  const int planes = B * C, Wh = W / 2 + 1;
  const double s = ortho ? 1.0 / sqrt((double)H * (double)W) : 1.0;
  const double count = 2.0 * (double)planes * (double)H * (double)Wh;
  const float coef = (float)((double)alpha * s / count), scale = (float)(s / count);
  float *tab_h = ws + o.tab_h, *tab_w = ws + o.tab_w, *partial = ws + o.partial, *dt = ws + o.dt, *t = ws + o.t, *g = ws + o.g;
  const dim3 block(256), wave(64);
  hipLaunchKernelGGL(fft_twiddle_kernel, dim3(cdiv(H > W ? H : W, 256)), block, 0, stream, tab_h, H, tab_w, W);
  hipLaunchKernelGGL(fft_diff_t_kernel, dim3(cdiv(W, 32), cdiv(H, 32), planes), block, 0, stream, x, y, dt, H, W);
  hipLaunchKernelGGL(fft_stage_kernel<1>, dim3(cdiv(Wh, 32 * NT), cdiv(H, 32), planes), wave, 0, stream, static_cast<const float*>(dt),
                     static_cast<const float*>(tab_w), t, static_cast<float*>(nullptr), H, W, 0.f, 0);
  hipLaunchKernelGGL(fft_stage_kernel<2>, dim3(o.tiles_v, o.tiles_u, planes), wave, 0, stream, static_cast<const float*>(t),
                     static_cast<const float*>(tab_h), d_x ? g : static_cast<float*>(nullptr), partial, H, W, 0.f, 0);
  hipLaunchKernelGGL(fft_loss_finish_kernel, dim3(1), block, 0, stream, static_cast<const float*>(partial),
                     (long long)planes * o.tiles_u * o.tiles_v, scale, alpha, value, loss);
  if (d_x) {
    hipLaunchKernelGGL(fft_stage_kernel<3>, dim3(cdiv(H, 32 * NT), cdiv(Wh, 32), planes), wave, 0, stream, static_cast<const float*>(g),
                       static_cast<const float*>(tab_h), t, static_cast<float*>(nullptr), H, W, 0.f, 0);
    hipLaunchKernelGGL(fft_stage_kernel<4>, dim3(cdiv(W, 32 * NT), cdiv(H, 32), planes), wave, 0, stream, static_cast<const float*>(t),
                       static_cast<const float*>(tab_w), d_x, static_cast<float*>(nullptr), H, W, coef, accumulate);
  }
  return srk_check_launch("fft_loss");
}
