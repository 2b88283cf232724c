// Training objectives next to the L1 kernel of misc.hip (include/srk.h: srk_pixel_loss_fwd_bwd, srk_ssim_loss_fwd_bwd):
//   pixel losses   mean |d|, mean d^2, mean sqrt(d^2 + eps^2) (Charbonnier), d = pred - target: value, d(pred) and the non-finite
//                  counter of the L1 entry from one pass;
//   SSIM term      alpha (1 - S), S = srk_ssim's batch mean (metrics.hip: the 11-tap window, K constants, VALID separable filter), value
//                  and -alpha dS/dx from one fused kernel per 32 x 32 tile of input pixels: no per-pixel intermediate goes to HBM.
//                  Two things are done more carefully than in the metric kernel, because a training term is differentiated and summed
//                  over many steps: the taps are normalised in fp64 (srk_launch_ssim_loss), and the moments are taken of values shifted
//                  by the window's centre pixel (steps 2 and 3 of the kernel), so that flat image regions lose no digits.
// Every sum is formed in a fixed order (per-workgroup partials in the caller's workspace + one finishing workgroup, no float
// atomics): two calls give the same bits.
//
// Gradient of S (per valid position p; mu, sigma from the five filtered moments):
//   B1 = mux^2 + muy^2 + C1,  B2 = sx^2 + sy^2 + C2,  L = (2 mux muy + C1) / B1,  CS = (2 sxy + C2) / B2,  S_p = L CS
//   a_p = 2 CS (muy - L mux) / B1 - 2 L muy / B2 + 2 S_p mux / B2        (through mux, including the -mux^2, -mux muy of the variances)
//   b_p = -2 S_p / B2     (through E[x^2]; the factor 2 x_q is split: 2 here, x_q below)
//   c_p = 2 L / B2        (through E[x y])
//   dS/dx_q = (1 / N) [ (G a)(q) + x_q (G b)(q) + y_q (G c)(q) ],   N = B C (H - 10) (W - 10)
// with G the ADJOINT of the valid filter: (G a)(q) = sum_{i, j} g_i g_j a(q - (i, j)), a taken as zero outside the valid domain.
#include <hip/hip_runtime.h>
#include <math.h>

#include "common.h"
#include "kernels.h"

namespace {

// ---- pixel losses --------------------------------------------------------------------------------------------------------------
// Longest sequential chain of the loss sum (the K of the tests' 2 K u sum|term| / n bound): a thread adds ceil(n / (blocks * 256))
// terms, the wave butterfly 6, the four waves 3, a finishing thread ceil(blocks / 256) <= 8 partials, its butterfly 6, its waves 3,
// then one multiplication by 1/n and one addition onto loss[0].
template <int KIND>
__global__ __launch_bounds__(256) void pixel_loss_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                         float* __restrict__ dpred, float* __restrict__ partial,
                                                         unsigned* __restrict__ nonfinite, long long n, float coef, float eps2,
                                                         int accumulate) {
  __shared__ float red[4];
  float s = 0.f;
  unsigned bad = 0;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const float p = pred[i], d = p - target[i];
    bad += !isfinite(p);
    float g;
    if constexpr (KIND == SRK_LOSS_L1) {
      s += fabsf(d);
      g = d > 0.f ? coef : (d < 0.f ? -coef : 0.f);
    } else if constexpr (KIND == SRK_LOSS_MSE) {
      s = fmaf(d, d, s);
      g = d;                                    // times coef = 2 grad_scale / n below
    } else {
      const float r = sqrtf(fmaf(d, d, eps2));
      s += r;
      g = d / r;
    }
    if (dpred) {
      if constexpr (KIND == SRK_LOSS_L1) dpred[i] = accumulate ? dpred[i] + g : g;
      else dpred[i] = accumulate ? fmaf(g, coef, dpred[i]) : g * coef;
    }
  }
  s = wave_sum64(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  if (bad && nonfinite) atomicAdd(nonfinite, bad);          // an integer count: exact in any order
  __syncthreads();
  if (threadIdx.x == 0) partial[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ __launch_bounds__(256) void pixel_loss_finish_kernel(const float* __restrict__ partial, int blocks, float inv_n,
                                                                float* __restrict__ loss) {
  __shared__ float red[4];
  float s = 0.f;
  for (int i = threadIdx.x; i < blocks; i += 256) s += partial[i];
  s = wave_sum64(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) loss[0] += ((red[0] + red[1]) + (red[2] + red[3])) * inv_n;
}

// ---- SSIM term -----------------------------------------------------------------------------------------------------------------
constexpr int LT = 32;             // tile of input pixels q (= gradient outputs) per workgroup
constexpr int LP = LT + 10;        // 42 x 42 positions p of a, b, c that reach the tile through the adjoint filter
constexpr int LI = LT + 20;        // 52 x 52 inputs that reach those positions through the valid filter
constexpr int XS = LI + 1, HS = LP + 1, TS = LT + 1;          // odd row strides: no LDS bank conflicts on column walks
constexpr int cmax(int a, int b) { return a > b ? a : b; }
// region A: the x / y tiles, later the a / b / c maps; region B: the five horizontally filtered moments, later the horizontally
// adjoint-filtered a / b / c.  5512 + 11180 floats = 66768 bytes (two workgroups per CU).
constexpr int REG_A = cmax(2 * LI * XS, 3 * LP * HS);
constexpr int REG_B = cmax(5 * LI * HS, 3 * LP * TS);
constexpr size_t SSIM_LOSS_LDS = sizeof(float) * (REG_A + REG_B);
struct GaussWin11 {
  float w[11];
  float s1, s2, om;          // sum of the taps, its square (the 2-D window's sum), 1 - s2 (evaluated in fp64)
};

__global__ __launch_bounds__(256) void ssim_loss_tile_kernel(const float* __restrict__ X, const float* __restrict__ Y, float* __restrict__ dX,
                                                             float* __restrict__ partial, int H, int W, int tiles_x, int tiles_y,
                                                             GaussWin11 gw, float C1, float C2, float gscale, int accumulate) {
  extern __shared__ float lds[];
  __shared__ float red[4];
  float* xs = lds;                     // [LI][XS]
  float* ys = lds + LI * XS;           // [LI][XS]
  float* abc = lds;                    // [3][LP][HS]   (aliases xs / ys)
  float* hb = lds + REG_A;             // [5][LI][HS]
  float* tt = hb;                      // [3][LP][TS]   (aliases hb)
  const int plane = blockIdx.z;                                 // b * C + c
  const int qy0 = blockIdx.y * LT, qx0 = blockIdx.x * LT;       // first input pixel of the tile
  const int OH = H - 10, OW = W - 10;
  const float* xp = X + (long long)plane * H * W;
  const float* yp = Y + (long long)plane * H * W;
  const int tid = threadIdx.x;
  // 1. inputs (qy0 - 10 + r, qx0 - 10 + c); zero outside the image (such inputs reach no valid position)
  for (int i = tid; i < LI * LI; i += 256) {
    const int r = i / LI, c = i - r * LI;
    const int gy = qy0 - 10 + r, gx = qx0 - 10 + c;
    const bool ok = gy >= 0 && gy < H && gx >= 0 && gx < W;
    xs[r * XS + c] = ok ? xp[(long long)gy * W + gx] : 0.f;
    ys[r * XS + c] = ok ? yp[(long long)gy * W + gx] : 0.f;
  }
  __syncthreads();
  // 2. the five moments filtered along x, of the values MINUS the window's centre tap (cx, cy) = in[r][pc + 5]:
  //    hb[.][r][pc] = sum_k g_k {x', y', x'^2, y'^2, x' y'}, x' = in[r][pc + k] - cx.  Variances do not depend on the shift, and with it
  //    E[x^2] - mu^2 no longer cancels digits where the image is flat (in fp32 the unshifted form loses them against C2 = 9e-4).
  for (int i = tid; i < LI * LP; i += 256) {
    const int r = i / LP, c = i - r * LP;
    const float cx = xs[r * XS + c + 5], cy = ys[r * XS + c + 5];
    float a = 0.f, b = 0.f, aa = 0.f, bb = 0.f, ab = 0.f;
#pragma unroll
    for (int k = 0; k < 11; ++k) {
      const float xv = xs[r * XS + c + k] - cx, yv = ys[r * XS + c + k] - cy, wk = gw.w[k];
      a = fmaf(wk, xv, a);
      b = fmaf(wk, yv, b);
      aa = fmaf(wk, xv * xv, aa);
      bb = fmaf(wk, yv * yv, bb);
      ab = fmaf(wk, xv * yv, ab);
    }
    float* o = hb + r * HS + c;
    o[0] = a; o[LI * HS] = b; o[2 * LI * HS] = aa; o[3 * LI * HS] = bb; o[4 * LI * HS] = ab;
  }
  float xq[4], yq[4];                  // this thread's four pixels of the tile, kept across the aliasing of xs / ys
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int i = tid + 256 * j, qr = i >> 5, qc = i & 31;
    xq[j] = xs[(qr + 10) * XS + qc + 10];
    yq[j] = ys[(qr + 10) * XS + qc + 10];
  }
  __syncthreads();
  // 3. filter along y, then S_p and a, b, c at position (qy0 - 10 + pr, qx0 - 10 + pc): exactly zero outside the valid domain.
  //    Row k of the window is re-centred from its own shift to the position's (Cx, Cy) = in[pr + 5][pc + 5] (d = row shift - C):
  //    sum g (x - C) = A + d s1,  sum g (x - C)^2 = AA + d (2 A + d s1),  sum g (x - Cx)(y - Cy) = AB + dx B + dy (A + dx s1);
  //    then mu = M' + C s2 and sigma^2 = XX' - M'^2 + (1 - s2)(2 C M' + C^2 s2) with s1 = sum g, s2 = s1^2 (the fp32 taps do not
  //    sum to exactly one; 1 - s2 comes from the host in fp64).  The results stay in registers until every thread has read xs / ys.
  constexpr int PER = (LP * LP + 255) / 256;          // 7 positions per thread
  float ca[PER], cb[PER], cc[PER];
  float acc = 0.f;
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    const int i = tid + 256 * j;
    ca[j] = cb[j] = cc[j] = 0.f;
    if (i >= LP * LP) continue;
    const int pr = i / LP, pc = i - pr * LP;
    const int gy = qy0 - 10 + pr, gx = qx0 - 10 + pc;
    if (gy >= 0 && gy < OH && gx >= 0 && gx < OW) {
      const float Cx = xs[(pr + 5) * XS + pc + 5], Cy = ys[(pr + 5) * XS + pc + 5];
      float m1 = 0.f, m2 = 0.f, xx = 0.f, yy = 0.f, xy = 0.f;
      const float* h = hb + pr * HS + pc;
#pragma unroll
      for (int k = 0; k < 11; ++k) {
        const float wk = gw.w[k];
        const float dx = xs[(pr + k) * XS + pc + 5] - Cx, dy = ys[(pr + k) * XS + pc + 5] - Cy;
        const float A = h[k * HS], Bm = h[LI * HS + k * HS];
        const float Ad = fmaf(dx, gw.s1, A), Bd = fmaf(dy, gw.s1, Bm);          // sum g (x - Cx), sum g (y - Cy) of this row
        m1 = fmaf(wk, Ad, m1);
        m2 = fmaf(wk, Bd, m2);
        xx = fmaf(wk, fmaf(dx, A + Ad, h[2 * LI * HS + k * HS]), xx);
        yy = fmaf(wk, fmaf(dy, Bm + Bd, h[3 * LI * HS + k * HS]), yy);
        xy = fmaf(wk, fmaf(dy, Ad, fmaf(dx, Bm, h[4 * LI * HS + k * HS])), xy);
      }
      const float mu1 = fmaf(Cx, gw.s2, m1), mu2 = fmaf(Cy, gw.s2, m2);
      const float s11 = (xx - m1 * m1) + gw.om * (Cx * fmaf(Cx, gw.s2, 2.f * m1));
      const float s22 = (yy - m2 * m2) + gw.om * (Cy * fmaf(Cy, gw.s2, 2.f * m2));
      const float s12 = (xy - m1 * m2) + gw.om * fmaf(Cx, m2, Cy * fmaf(Cx, gw.s2, m1));
      const float B1 = mu1 * mu1 + mu2 * mu2 + C1, B2 = s11 + s22 + C2;
      const float L = (2.f * mu1 * mu2 + C1) / B1, CS = (2.f * s12 + C2) / B2;
      const float Sp = L * CS;
      ca[j] = 2.f * CS * (mu2 - L * mu1) / B1 - 2.f * L * mu2 / B2 + 2.f * Sp * mu1 / B2;
      cb[j] = -2.f * Sp / B2;
      cc[j] = 2.f * L / B2;
      if (pr >= 10 && pc >= 10) acc += Sp;          // the positions this tile owns: every valid position has one owner
    }
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    const int i = tid + 256 * j;
    if (i >= LP * LP) continue;
    const int pr = i / LP, pc = i - pr * LP;
    float* o = abc + pr * HS + pc;
    o[0] = ca[j]; o[LP * HS] = cb[j]; o[2 * LP * HS] = cc[j];
  }
  acc = wave_sum64(acc);
  if ((tid & 63) == 0) red[tid >> 6] = acc;
  __syncthreads();
  if (tid == 0) partial[((long long)plane * tiles_y + blockIdx.y) * tiles_x + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
  if (!dX) return;
  // 4. adjoint along x: tt[m][pr][qc] = sum_k g_k abc[m][pr][qc + 10 - k]
  for (int i = tid; i < LP * LT; i += 256) {
    const int pr = i >> 5, qc = i & 31;
    const float* s = abc + pr * HS + qc + 10;
    float ta = 0.f, tb = 0.f, tc = 0.f;
#pragma unroll
    for (int k = 0; k < 11; ++k) {
      const float wk = gw.w[k];
      ta = fmaf(wk, s[-k], ta);
      tb = fmaf(wk, s[LP * HS - k], tb);
      tc = fmaf(wk, s[2 * LP * HS - k], tc);
    }
    float* o = tt + pr * TS + qc;
    o[0] = ta; o[LP * TS] = tb; o[2 * LP * TS] = tc;
  }
  __syncthreads();
  // 5. adjoint along y and the combination with x_q, y_q
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int i = tid + 256 * j, qr = i >> 5, qc = i & 31;
    const int gy = qy0 + qr, gx = qx0 + qc;
    if (gy >= H || gx >= W) continue;
    const float* s = tt + (qr + 10) * TS + qc;
    float ga = 0.f, gb = 0.f, gc = 0.f;
#pragma unroll
    for (int k = 0; k < 11; ++k) {
      const float wk = gw.w[k];
      ga = fmaf(wk, s[-k * TS], ga);
      gb = fmaf(wk, s[LP * TS - k * TS], gb);
      gc = fmaf(wk, s[2 * LP * TS - k * TS], gc);
    }
    // one rounded product, one rounded addition (never contracted into an fma): what is added is exactly what would be stored
    const float v = __fmul_rn(gscale, fmaf(yq[j], gc, fmaf(xq[j], gb, ga)));
    float* o = dX + (long long)plane * H * W + (long long)gy * W + gx;
    *o = accumulate ? __fadd_rn(*o, v) : v;
  }
}

// one workgroup; thread b = image b: channel means in channel order, tiles in tile order, then the batch mean in image order
__global__ void ssim_loss_finish_kernel(const float* __restrict__ partial, int tiles, int B, int C, float inv_count, float alpha,
                                        float* __restrict__ ssim_mean, float* __restrict__ loss) {
  __shared__ float sh[1024];
  for (int b = threadIdx.x; b < B; b += blockDim.x) {
    float s = 0.f;
    for (int c = 0; c < C; ++c) {
      float pc = 0.f;
      for (int t = 0; t < tiles; ++t) pc += partial[((long long)b * C + c) * tiles + t];
      s += pc * inv_count;
    }
    sh[b] = s / (float)C;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float s = 0.f;
    for (int b = 0; b < B; ++b) s += sh[b];
    s /= (float)B;
    if (ssim_mean) ssim_mean[0] = s;
    if (loss) loss[0] += alpha * (1.0f - s);
  }
}

}  // namespace

int srk_launch_pixel_loss(const float* pred, const float* target, float* dpred, float* loss, unsigned* nonfinite, long long n, int kind,
                          float eps, float grad_scale, int accumulate, float* partial, hipStream_t stream) {
  const int blocks = srk_pixel_loss_blocks(n);
  const float eps2 = (float)((double)eps * (double)eps);
  const float inv_n = (float)(1.0 / (double)n);
  const dim3 grid(blocks), block(256);
  if (kind == SRK_LOSS_L1)
    hipLaunchKernelGGL(pixel_loss_kernel<SRK_LOSS_L1>, grid, block, 0, stream, pred, target, dpred, partial, nonfinite, n,
                       (float)((double)grad_scale / (double)n), eps2, accumulate);
  else if (kind == SRK_LOSS_MSE)
    hipLaunchKernelGGL(pixel_loss_kernel<SRK_LOSS_MSE>, grid, block, 0, stream, pred, target, dpred, partial, nonfinite, n,
                       (float)(2.0 * (double)grad_scale / (double)n), eps2, accumulate);
  else
    hipLaunchKernelGGL(pixel_loss_kernel<SRK_LOSS_CHARBONNIER>, grid, block, 0, stream, pred, target, dpred, partial, nonfinite, n,
                       (float)((double)grad_scale / (double)n), eps2, accumulate);
  hipLaunchKernelGGL(pixel_loss_finish_kernel, dim3(1), block, 0, stream, static_cast<const float*>(partial), blocks, inv_n, loss);
  return srk_check_launch("pixel_loss");
}

int srk_launch_ssim_loss(const float* x, const float* y, float* partial, int B, int C, int H, int W, float data_range, float alpha, float* d_x,
                         int accumulate, float* ssim_mean, float* loss, hipStream_t stream) {
  static SrkLdsState reserved;      // 66768 bytes of dynamic LDS: above the default 64 KB limit, well inside the CU's 160 KB
  if (const int rc = srk_reserve_lds(&ssim_loss_tile_kernel, SSIM_LOSS_LDS, reserved, false, "ssim_loss: cannot reserve %zu bytes of LDS", SSIM_LOSS_LDS))
    return rc;
  // The 11-tap Gaussian (sigma 1.5) of srk_ssim, but normalised in fp64 and rounded once per tap: its taps sum to 1 within 2e-9.
  // sigma^2 = E[x^2] - mu^2 picks up (s - s^2) mean^2 when the taps sum to s != 1; with the fp32-normalised taps (s - 1 = 4.5e-8)
  // that alone moved S by 4.5e-6 on smooth images against the same formula under torch's fp32 window (s - 1 = -3.1e-8).
  GaussWin11 gw;
  double g[11], sum = 0.0, s1 = 0.0;
  for (int i = 0; i < 11; ++i) {
    const double c = (double)(i - 5);
    g[i] = exp(-(c * c) / (2.0 * 1.5 * 1.5));
    sum += g[i];
  }
  for (int i = 0; i < 11; ++i) {
    gw.w[i] = (float)(g[i] / sum);
    s1 += (double)gw.w[i];
  }
  gw.s1 = (float)s1;
  gw.s2 = (float)(s1 * s1);
  gw.om = (float)(1.0 - s1 * s1);
  const int tx = cdiv(W, LT), ty = cdiv(H, LT);
  const float C1 = (float)((0.01 * data_range) * (0.01 * data_range)), C2 = (float)((0.03 * data_range) * (0.03 * data_range));
  const double count = (double)(H - 10) * (double)(W - 10);
  const float gscale = (float)(-(double)alpha / ((double)B * (double)C * count));
  hipLaunchKernelGGL(ssim_loss_tile_kernel, dim3(tx, ty, B * C), dim3(256), SSIM_LOSS_LDS, stream, x, y, d_x, partial, H, W, tx, ty, gw, C1, C2,
                     gscale, accumulate);
  hipLaunchKernelGGL(ssim_loss_finish_kernel, dim3(1), dim3(256), 0, stream, static_cast<const float*>(partial), tx * ty, B, C,
                     (float)(1.0 / count), alpha, ssim_mean, loss);
  return srk_check_launch("ssim_loss");
}

extern "C" {

int64_t srk_pixel_loss_workspace(int64_t n) {
  if (n <= 0) return 0;
  return (int64_t)sizeof(float) * srk_pixel_loss_blocks(n);
}

int srk_pixel_loss_fwd_bwd(const float* pred, const float* target, float* d_pred, float* loss, uint32_t* nonfinite, int64_t n, int kind,
                           float eps, float grad_scale, int accumulate, void* workspace, srk_stream_t stream) {
  SRK_REQUIRE(pred && target && loss && workspace, SRK_E_NULL, "pixel_loss: null pointer (pred, target, loss and workspace are required)");
  SRK_REQUIRE(n > 0, SRK_E_SHAPE, "pixel_loss: n=%lld", (long long)n);
  SRK_REQUIRE(kind == SRK_LOSS_L1 || kind == SRK_LOSS_MSE || kind == SRK_LOSS_CHARBONNIER, SRK_E_SHAPE, "pixel_loss: unknown kind %d", kind);
  SRK_REQUIRE(kind != SRK_LOSS_CHARBONNIER || eps > 0.f, SRK_E_SHAPE, "pixel_loss: Charbonnier needs eps > 0 (got %g)", (double)eps);
  SRK_REQUIRE(accumulate == 0 || accumulate == 1, SRK_E_SHAPE, "pixel_loss: accumulate must be 0 or 1 (got %d)", accumulate);
  return srk_launch_pixel_loss(pred, target, d_pred, loss, nonfinite, n, kind, eps, grad_scale, accumulate, static_cast<float*>(workspace),
                               (hipStream_t)stream);
}

int64_t srk_ssim_loss_workspace(int B, int C, int H, int W) {
  if (B <= 0 || C <= 0 || H < 11 || W < 11) return 0;
  return (int64_t)sizeof(float) * B * C * cdiv(H, LT) * cdiv(W, LT);
}

int srk_ssim_loss_fwd_bwd(const float* x, const float* y, void* workspace, int B, int C, int H, int W, float data_range, float alpha,
                          float* d_x, int accumulate, float* ssim_mean, float* loss, srk_stream_t stream) {
  SRK_REQUIRE(x && y && workspace, SRK_E_NULL, "ssim_loss: null pointer (x, y and workspace are required)");
  SRK_REQUIRE(B > 0 && B <= 1024 && C > 0 && (long long)B * C < 65536, SRK_E_SHAPE, "ssim_loss: B=%d C=%d", B, C);
  SRK_REQUIRE(H >= 11 && W >= 11, SRK_E_UNSUPPORTED, "ssim_loss: the 11-tap window needs H, W >= 11 (got %dx%d)", H, W);
  SRK_REQUIRE(data_range > 0.f, SRK_E_SHAPE, "ssim_loss: data_range=%g", (double)data_range);
  SRK_REQUIRE(accumulate == 0 || accumulate == 1, SRK_E_SHAPE, "ssim_loss: accumulate must be 0 or 1 (got %d)", accumulate);
  const double bytes = 4.0 * B * C * H * W;
  SRK_REQUIRE(bytes < 9.0e18, SRK_E_SHAPE, "ssim_loss: B=%d C=%d H=%d W=%d is too large", B, C, H, W);
  const size_t n = (size_t)bytes;
  SRK_REQUIRE(!d_x || (!srk_ranges_overlap(d_x, n, x, n) && !srk_ranges_overlap(d_x, n, y, n)), SRK_E_SHAPE, "ssim_loss: d_x overlaps x or y");
  return srk_launch_ssim_loss(x, y, static_cast<float*>(workspace), B, C, H, W, data_range, alpha, d_x, accumulate, ssim_mean, loss,
                              (hipStream_t)stream);
}

}  // extern "C"
