// Full-reference scores on the benchmark-protocol planes (srk.h "Full-reference scores: PSNR-B, MS-SSIM"):
//   srk_psnrb    PSNR-B (Yim & Bovik, "Quality assessment of deblocked images"), in the form of SwinIR's calculate_psnrb
//   srk_msssim   the per-level means of MS-SSIM (Wang, Simoncelli & Bovik 2003), in the form of pytorch_msssim.ms_ssim
// Both restated from the published algorithms: PARITY UNPINNED.  The power product of MS-SSIM is host fp64 (metrics.py).
// Contraction is off: every fused multiply-add is written as fmaf.  Sums are formed in a fixed order, no atomics: two runs give equal bits.
#include <hip/hip_runtime.h>
#include <math.h>

#include "common.h"

#pragma clang fp contract(off)

namespace {

// ---- PSNR-B ------------------------------------------------------------------------------------------------------------------
// A streaming pass: workgroup (chunk, plane) takes `rpb` consecutive rows of one plane -- about PB_ELEMS elements, at most PB_ROWS
// rows -- and reads the one row below its run for the vertical differences, so a plane element is read by at most two workgroups.
// Thread t takes the run's elements t, t + 256, ... in order and feeds five accumulators: the squared error against the target and
// the squared horizontal / vertical differences of the restored plane, each split into block-boundary pairs (x or y = 7 mod 8) and the
// others; then an xor butterfly over the wave and the four waves added in order.
constexpr int PB_ELEMS = 2048;
constexpr int PB_ROWS = 32;
inline int psnrb_rows_per_block(int Wc) { return Wc >= PB_ELEMS ? 1 : (PB_ELEMS / Wc < PB_ROWS ? PB_ELEMS / Wc : PB_ROWS); }
inline int psnrb_chunks(int Hc, int Wc) {
  const int rpb = psnrb_rows_per_block(Wc);
  return (int)(((long long)Hc + rpb - 1) / rpb);
}
// the plane shapes srk_psnrb takes: those of srk_bench_psnr whose planes ride in a 16-bit grid axis (srk_ssim's limit)
inline bool psnrb_dims_ok(int B, int Cm, int Hc, int Wc) { return srk_bench_plane_dims_ok(B, Cm, Hc, Wc) && (long long)B * Cm < 65536; }

__global__ __launch_bounds__(256) void psnrb_partial_kernel(const float* __restrict__ P, const float* __restrict__ T, float* __restrict__ partial,
                                                            int Hc, int Wc, int rpb) {
  __shared__ float red[4][5];
  const int plane = blockIdx.y;
  const int y0 = blockIdx.x * rpb;
  const int nr = min(rpb, Hc - y0);
  const long long base = ((long long)plane * Hc + y0) * Wc;
  const float* p = P + base;
  const float* t = T + base;
  float acc[5] = {0.f, 0.f, 0.f, 0.f, 0.f};       // mse, Dh_b, Dh_n, Dv_b, Dv_n
  for (int i = threadIdx.x; i < nr * Wc; i += 256) {
    const int r = i / Wc, x = i - r * Wc, y = y0 + r;
    const float v = p[i];
    const float d = v - t[i];
    acc[0] = fmaf(d, d, acc[0]);
    if (x < Wc - 1) {
      const float h = v - p[i + 1];
      if ((x & 7) == 7) acc[1] = fmaf(h, h, acc[1]);
      else acc[2] = fmaf(h, h, acc[2]);
    }
    if (y < Hc - 1) {                               // the last row of the run reads the row below it: the next workgroup's first
      const float w = v - p[i + Wc];
      if ((y & 7) == 7) acc[3] = fmaf(w, w, acc[3]);
      else acc[4] = fmaf(w, w, acc[4]);
    }
  }
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    const float s = wave_sum64(acc[k]);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][k] = s;
  }
  __syncthreads();
  const int k = threadIdx.x;
  if (k < 5) partial[((long long)plane * gridDim.x + blockIdx.x) * 5 + k] = ((red[0][k] + red[1][k]) + red[2][k]) + red[3][k];
}

// One workgroup of 1024 threads; a group of L lanes owns an image, as in bench_psnr_finish_kernel (metrics.hip): per plane, lane l adds
// the partials l, l + L, ... in order, an xor butterfly adds the group's lanes, lane 0 forms the plane's score; the image's score is the
// mean over its planes, added in plane order.
__global__ __launch_bounds__(1024) void psnrb_finish_kernel(const float* __restrict__ partial, int chunks, int B, int Cm, int L, float count,
                                                            float n_b, float n_n, float scale, float* __restrict__ sums, float* __restrict__ psnrb) {
  const int groups = 1024 / L, gi = threadIdx.x / L, l = threadIdx.x & (L - 1);
  for (int b0 = 0; b0 < B; b0 += groups) {                      // the same trip counts for every thread: the shuffles see whole waves
    const int b = b0 + gi;
    float total = 0.f;
    for (int c = 0; c < Cm; ++c) {
      float s[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
      if (b < B)
        for (int k = l; k < chunks; k += L) {
          const float* q = partial + (((long long)b * Cm + c) * chunks + k) * 5;
#pragma unroll
          for (int j = 0; j < 5; ++j) s[j] += q[j];
        }
#pragma unroll
      for (int j = 0; j < 5; ++j)
        for (int o = L >> 1; o > 0; o >>= 1) s[j] += __shfl_xor(s[j], o, 64);
      if (b < B && l == 0) {
        if (sums) {
#pragma unroll
          for (int j = 0; j < 5; ++j) sums[((long long)b * Cm + c) * 5 + j] = s[j];
        }
        const float mse = s[0] / count;
        const float d_b = (s[1] + s[3]) / n_b, d_n = (s[2] + s[4]) / n_n;
        const float bef = d_b > d_n ? scale * (d_b - d_n) : 0.f;
        const float den = mse + bef;
        total += den == 0.f ? INFINITY : 10.0f * log10f(65025.0f / den);      // a NaN is not 0: it reaches the result
      }
    }
    if (b < B && l == 0 && psnrb) psnrb[b] = total / (float)Cm;
  }
}

// ---- MS-SSIM -----------------------------------------------------------------------------------------------------------------
// One launch per level: ssim_tile_kernel's (metrics.hip) staging and filters -- a 42 x 42 tile of both images in LDS, 32 x 32 valid map
// positions per workgroup -- with two map sums (SSIM and its contrast-structure factor) and, from the staged tile, the 2 x 2-pooled
// cells of both images for the next level.  Pooled row j covers the input rows a = 2 j - ph and a + 1, ph = H % 2 (an odd extent
// gains a row of zeros in front; the cell is still divided by 4).  The tile in row k of the grid holds the input rows [32 k, 32 k + 42)
// and owns the cells whose first row a lies in [32 k, 32 k + 32) -- tile 0 also the cell of a = -1, the last tile every cell from
// 32 k on -- so each cell is written by exactly one workgroup and both of its rows are in that workgroup's tile.  Columns likewise.
constexpr int ST = 32;            // valid map positions per workgroup: 32 x 32
constexpr int SI = ST + 10;       // input tile 42 x 42
struct GaussWin { float w[11]; };

__device__ __forceinline__ float tile_at(const float (*s)[SI + 1], int r, int c) { return (r < 0 || c < 0) ? 0.f : s[r][c]; }
__device__ __forceinline__ float pool_cell(const float (*s)[SI + 1], int r, int c) {
  return ((tile_at(s, r, c) + tile_at(s, r, c + 1)) + (tile_at(s, r + 1, c) + tile_at(s, r + 1, c + 1))) * 0.25f;
}

__global__ __launch_bounds__(256) void msssim_level_kernel(const float* __restrict__ X, const float* __restrict__ Y, float* __restrict__ partial,
                                                           float* __restrict__ NX, float* __restrict__ NY, int H, int W, int tiles_x, int tiles_y,
                                                           GaussWin gw, float C1, float C2) {
  __shared__ float xs[SI][SI + 1], ys[SI][SI + 1];
  __shared__ float hb[5][SI][ST + 1];        // horizontally filtered x, y, xx, yy, xy
  __shared__ float red[4][2];
  const int plane = blockIdx.z;                                 // b * C + c
  const int ty0 = blockIdx.y * ST, tx0 = blockIdx.x * ST;       // first valid map position of the tile = its first input row / column
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
  if (NX) {                                                     // the next level's planes; absent at the last level
    const int ph = H & 1, pw = W & 1;
    const int Ho = (H + ph) >> 1, Wo = (W + pw) >> 1;
    const int j0 = blockIdx.y == 0 ? 0 : 16 * (int)blockIdx.y + ph, j1 = (int)blockIdx.y == tiles_y - 1 ? Ho : 16 * ((int)blockIdx.y + 1) + ph;
    const int i0 = blockIdx.x == 0 ? 0 : 16 * (int)blockIdx.x + pw, i1 = (int)blockIdx.x == tiles_x - 1 ? Wo : 16 * ((int)blockIdx.x + 1) + pw;
    const int ni = i1 - i0;
    float* nx = NX + (long long)plane * Ho * Wo;
    float* ny = NY + (long long)plane * Ho * Wo;
    for (int i = tid; i < (j1 - j0) * ni; i += 256) {
      const int lj = i / ni, li = i - lj * ni;
      const int r = 2 * (j0 + lj) - ph - ty0, c = 2 * (i0 + li) - pw - tx0;      // -1 for the leading cell of an odd extent, else 0..40
      const long long o = (long long)(j0 + lj) * Wo + i0 + li;
      nx[o] = pool_cell(xs, r, c);
      ny[o] = pool_cell(ys, r, c);
    }
  }
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
  float acc_s = 0.f, acc_cs = 0.f;
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
    const float s11 = fmaf(-m1, m1, xx), s22 = fmaf(-m2, m2, yy), s12 = fmaf(-m1, m2, xy);
    const float cs = fmaf(2.f, s12, C2) / ((s11 + s22) + C2);
    const float m12 = m1 * m2;
    acc_cs += cs;
    acc_s += (fmaf(2.f, m12, C1) / (fmaf(m1, m1, m2 * m2) + C1)) * cs;
  }
  acc_s = wave_sum64(acc_s);
  acc_cs = wave_sum64(acc_cs);
  if ((tid & 63) == 0) {
    red[tid >> 6][0] = acc_s;
    red[tid >> 6][1] = acc_cs;
  }
  __syncthreads();
  if (tid < 2) partial[(((long long)plane * tiles_y + blockIdx.y) * tiles_x + blockIdx.x) * 2 + tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
}

// The pyramid of one call: extents, tiles and the places of the pooled planes and of the partial sums in the workspace (in floats).
constexpr int MS_MAX_LEVELS = 5;
struct MsGeom {
  int H[MS_MAX_LEVELS], W[MS_MAX_LEVELS], tx[MS_MAX_LEVELS], ty[MS_MAX_LEVELS];
  long long plane_off[MS_MAX_LEVELS];       // level s >= 1: x planes at plane_off[s], y planes right behind them
  long long part_off[MS_MAX_LEVELS];
  long long floats;
};
struct MsFinish {
  int tiles[MS_MAX_LEVELS];
  long long off[MS_MAX_LEVELS];
  float inv[MS_MAX_LEVELS];
};
inline bool msssim_args_ok(int B, int C, int H, int W, int levels) {
  return B > 0 && B <= 1024 && C > 0 && (long long)B * C < 65536 && levels >= 1 && levels <= MS_MAX_LEVELS && H > 0 && W > 0 && H <= (1 << 20) &&
         W <= (1 << 20);
}
inline bool msssim_extent_ok(int H, int W, int levels) { return (H < W ? H : W) > (10 << (levels - 1)); }
inline MsGeom msssim_geom(int B, int C, int H, int W, int levels) {
  MsGeom g{};
  long long off = 0;
  for (int s = 0; s < levels; ++s) {
    g.H[s] = H;
    g.W[s] = W;
    g.tx[s] = (W - 10 + ST - 1) / ST;
    g.ty[s] = (H - 10 + ST - 1) / ST;
    if (s > 0) {
      g.plane_off[s] = off;
      off += 2LL * B * C * H * W;
    }
    H = (H + (H & 1)) >> 1;
    W = (W + (W & 1)) >> 1;
  }
  for (int s = 0; s < levels; ++s) {
    g.part_off[s] = off;
    off += 2LL * B * C * g.tx[s] * g.ty[s];
  }
  g.floats = off;
  return g;
}

// Workgroup (plane, level): thread t adds the tiles t, t + 256, ... in order, then the butterfly and the four waves in order.
__global__ __launch_bounds__(256) void msssim_finish_kernel(const float* __restrict__ ws, MsFinish f, int planes, float* __restrict__ means) {
  __shared__ float red[4][2];
  const int plane = blockIdx.x, s = blockIdx.y, tid = threadIdx.x;
  const int tiles = f.tiles[s];
  const float* q = ws + f.off[s] + 2LL * plane * tiles;
  float a = 0.f, b = 0.f;
  for (int t = tid; t < tiles; t += 256) {
    a += q[2 * t];
    b += q[2 * t + 1];
  }
  a = wave_sum64(a);
  b = wave_sum64(b);
  if ((tid & 63) == 0) {
    red[tid >> 6][0] = a;
    red[tid >> 6][1] = b;
  }
  __syncthreads();
  if (tid < 2) means[((long long)s * planes + plane) * 2 + tid] = (((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid]) * f.inv[s];
}

}  // namespace

extern "C" {

int64_t srk_psnrb_workspace(int B, int Cm, int Hc, int Wc) {
  if (!psnrb_dims_ok(B, Cm, Hc, Wc) || Hc < 16 || Wc < 16) return 0;
  return (int64_t)sizeof(float) * 5 * B * Cm * psnrb_chunks(Hc, Wc);
}

int srk_psnrb(const float* planes_pred, const float* planes_target, void* workspace, int B, int Cm, int Hc, int Wc, float* sums, float* psnrb,
              srk_stream_t stream) {
  SRK_REQUIRE(planes_pred && planes_target && workspace && (sums || psnrb), SRK_E_NULL, "psnrb: null planes or workspace, or no output");
  SRK_REQUIRE(psnrb_dims_ok(B, Cm, Hc, Wc), SRK_E_SHAPE, "psnrb: B=%d (1..1024) Cm=%d (B Cm < 65536) Hc=%d Wc=%d", B, Cm, Hc, Wc);
  SRK_REQUIRE(Hc >= 16 && Wc >= 16, SRK_E_UNSUPPORTED, "psnrb: planes of %d x %d hold no 8 x 8 block boundary (Hc, Wc >= 16)", Hc, Wc);
  const size_t in_bytes = sizeof(float) * (size_t)B * Cm * Hc * Wc, ws_bytes = (size_t)srk_psnrb_workspace(B, Cm, Hc, Wc);
  const size_t sums_bytes = sizeof(float) * 5 * (size_t)B * Cm, out_bytes = sizeof(float) * (size_t)B;
  for (const float* in : {planes_pred, planes_target})
    SRK_REQUIRE(!srk_ranges_overlap(workspace, ws_bytes, in, in_bytes) && !(sums && srk_ranges_overlap(sums, sums_bytes, in, in_bytes)) &&
                    !(psnrb && srk_ranges_overlap(psnrb, out_bytes, in, in_bytes)),
                SRK_E_SHAPE, "psnrb: an output or the workspace overlaps an input");
  const int rpb = psnrb_rows_per_block(Wc), chunks = psnrb_chunks(Hc, Wc);
  hipLaunchKernelGGL(psnrb_partial_kernel, dim3(chunks, B * Cm), dim3(256), 0, (hipStream_t)stream, planes_pred, planes_target,
                     static_cast<float*>(workspace), Hc, Wc, rpb);
  int L = 1;                                                    // lanes per image of the finish step
  while (L < 64 && L < chunks) L <<= 1;
  const long long n_bh = (long long)Hc * (Wc / 8 - 1), n_bv = (long long)Wc * (Hc / 8 - 1);      // the published counts
  const long long n_nh = (long long)Hc * (Wc - 1) - n_bh, n_nv = (long long)Wc * (Hc - 1) - n_bv;
  const float scale = (float)(3.0 / log2((double)(Hc < Wc ? Hc : Wc)));
  hipLaunchKernelGGL(psnrb_finish_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, static_cast<const float*>(workspace), chunks, B, Cm, L,
                     (float)((long long)Hc * Wc), (float)(n_bh + n_bv), (float)(n_nh + n_nv), scale, sums, psnrb);
  return srk_check_launch("psnrb");
}

int64_t srk_msssim_workspace(int B, int C, int H, int W, int levels) {
  if (!msssim_args_ok(B, C, H, W, levels) || !msssim_extent_ok(H, W, levels)) return 0;
  return (int64_t)sizeof(float) * msssim_geom(B, C, H, W, levels).floats;
}

int srk_msssim(const float* x, const float* y, void* workspace, int B, int C, int H, int W, int levels, float data_range, float* means,
               srk_stream_t stream) {
  SRK_REQUIRE(x && y && workspace && means, SRK_E_NULL, "msssim: null pointer");
  SRK_REQUIRE(msssim_args_ok(B, C, H, W, levels), SRK_E_SHAPE, "msssim: B=%d (1..1024) C=%d (B C < 65536) H=%d W=%d (1..2^20) levels=%d (1..5)", B, C, H,
              W, levels);
  SRK_REQUIRE(data_range > 0.f, SRK_E_SHAPE, "msssim: data_range=%g", (double)data_range);
  SRK_REQUIRE(msssim_extent_ok(H, W, levels), SRK_E_UNSUPPORTED, "msssim: %d levels need a smaller side above %d (got %d x %d)", levels,
              10 << (levels - 1), H, W);
  const MsGeom g = msssim_geom(B, C, H, W, levels);
  const size_t in_bytes = sizeof(float) * (size_t)B * C * H * W, ws_bytes = sizeof(float) * (size_t)g.floats;
  const size_t means_bytes = sizeof(float) * 2 * (size_t)levels * B * C;
  for (const float* in : {x, y})
    SRK_REQUIRE(!srk_ranges_overlap(workspace, ws_bytes, in, in_bytes) && !srk_ranges_overlap(means, means_bytes, in, in_bytes), SRK_E_SHAPE,
                "msssim: means or the workspace overlaps an input");
  SRK_REQUIRE(!srk_ranges_overlap(means, means_bytes, workspace, ws_bytes), SRK_E_SHAPE, "msssim: means overlaps the workspace");
  GaussWin gw;                                                  // srk_ssim's window
  float sum = 0.f;
  for (int i = 0; i < 11; ++i) {
    const float c = (float)(i - 5);
    gw.w[i] = expf(-(c * c) / (2.0f * 1.5f * 1.5f));
    sum += gw.w[i];
  }
  for (int i = 0; i < 11; ++i) gw.w[i] /= sum;
  const float C1 = (0.01f * data_range) * (0.01f * data_range), C2 = (0.03f * data_range) * (0.03f * data_range);
  float* ws = static_cast<float*>(workspace);
  MsFinish f{};
  const float *cx = x, *cy = y;
  for (int s = 0; s < levels; ++s) {
    const bool last = s == levels - 1;
    float* nx = last ? nullptr : ws + g.plane_off[s + 1];
    float* ny = last ? nullptr : nx + (long long)B * C * g.H[s + 1] * g.W[s + 1];
    hipLaunchKernelGGL(msssim_level_kernel, dim3(g.tx[s], g.ty[s], B * C), dim3(256), 0, (hipStream_t)stream, cx, cy, ws + g.part_off[s], nx, ny,
                       g.H[s], g.W[s], g.tx[s], g.ty[s], gw, C1, C2);
    f.tiles[s] = g.tx[s] * g.ty[s];
    f.off[s] = g.part_off[s];
    f.inv[s] = 1.0f / ((float)(g.H[s] - 10) * (float)(g.W[s] - 10));
    cx = nx;
    cy = ny;
  }
  hipLaunchKernelGGL(msssim_finish_kernel, dim3(B * C, levels), dim3(256), 0, (hipStream_t)stream, static_cast<const float*>(ws), f, B * C, means);
  return srk_check_launch("msssim");
}

}  // extern "C"
