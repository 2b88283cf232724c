// Blind degradation on the device (include/srk.h: srk_degrade_blind_f32, srk_crop_degrade_blind_u8): the antialiased bicubic downscale
// of resize.h behind a per-sample anisotropic Gaussian blur, plus per-sample signal-dependent noise from a counter-based generator.
//
// Blur.  Per axis sigma (HR pixels), R = ceil(3 sigma) clamped to 0..8, g[d] = exp(-d^2 / (2 sigma^2)), d = -R..R, normalised in fp64.
// The blur is composed with the cubic taps (lo_c, w_c[j]) of rs_weights -- the fp64 values before their rounding -- into ONE table per
// output: W[m] = sum_j w_c[j] g[m - lo_c - j] for m in [max(lo_c - R, 0), min(hi_c + R, n_in)), divided by its sum (mass outside the
// image is dropped, the rest renormalised: the border rule of the resize), rounded once to fp32.  At factors 2 / 3 / 4 that is at most
// 8 + 16, 12 + 16 and 16 + 16 taps: they fit the 33-tap rows of RsShared, and rs_filter runs unchanged on the composed tables.  An axis
// with R == 0 (sigma <= 0 or NaN) takes rs_weights itself, so without blur and noise the outputs have the bits of resize.hip's.
//
// Noise.  out = v + sqrtf(sigma_n^2 + gain fmaxf(v, 0)) z on the filtered fp32 value v, before the 8-bit rounding; z is a standard normal
// from Philox4x32-10 with counter (x, y, ch, 0) -- x, y the coordinates in the WHOLE downscaled image, ch the channel or 0 for gray
// noise -- and the key = the two words of the sample's noise_id; Box-Muller on the first two outputs.  Image coordinates make a training
// patch the exact window of the whole-image call.  sigma_n and gain are clamped to [0, 16] (NaN -> 0); both 0: v passes untouched.
//
// Tables, once per workgroup: 17 + 17 threads evaluate the two Gaussians, one thread per axis normalises them, then lane t < 64 composes
// the taps of output column t and lane 64 + t those of output row t, each with 49 doubles of scratch (16 cubic taps, 33 unnormalised
// composed taps) inside RsShared::mid, which the filter only needs afterwards.
#include "degrade.h"

#pragma clang fp contract(off)

namespace {

constexpr int DG_CUBIC = 16;                 // cubic taps per output at factor 4 (8 at 2, 12 at 3)
constexpr int DG_SLOT = DG_CUBIC + RS_TAPS;  // doubles of scratch per table thread
static_assert((RS_TOX + RS_TOY) * DG_SLOT * sizeof(double) <= sizeof(RsShared::mid), "the table scratch must fit mid");
static_assert(DG_CUBIC + 2 * DG_RMAX <= RS_TAPS, "a composed row must fit a weight row");

struct DgShared {
  RsShared rs;
  double g[2][2 * DG_RMAX + 1];              // [0] = y, [1] = x
};

// the composed taps of output i: w[0 .. cnt) in fp32, first tap lo.  g = the normalised Gaussian g[0 .. 2R], R in 1..8; scr = DG_SLOT doubles.
__device__ __forceinline__ void dg_weights(const RsAxis& ax, int i, int R, const double* g, double* scr, float* w, int* lo_out, int* cnt_out) {
  double c;
  int lo_c, cnt_c;
  rs_span(ax, i, &c, &lo_c, &cnt_c);
  cnt_c = cnt_c > DG_CUBIC ? DG_CUBIC : cnt_c;
  double* wc = scr;
  double* wd = scr + DG_CUBIC;
  double s = 0.0;
  for (int j = 0; j < cnt_c; ++j) s += rs_cubic(((double)(j + lo_c) - c + 0.5) * ax.inv);
  for (int j = 0; j < cnt_c; ++j) wc[j] = rs_cubic(((double)(j + lo_c) - c + 0.5) * ax.inv) / s;
  int lo = lo_c - R, hi = lo_c + cnt_c + R;
  lo = lo < 0 ? 0 : lo;
  hi = hi > ax.n_in ? ax.n_in : hi;
  int cnt = hi - lo;
  cnt = (cnt_c <= 0 || cnt < 0) ? 0 : (cnt > RS_TAPS ? RS_TAPS : cnt);
  double sum = 0.0;
  for (int m = 0; m < cnt; ++m) {
    const int o = lo + m - lo_c;             // W[m] = sum over j of w_c[j] g[o - j], |o - j| <= R
    int j0 = o - R, j1 = o + R;
    j0 = j0 < 0 ? 0 : j0;
    j1 = j1 > cnt_c - 1 ? cnt_c - 1 : j1;
    double a = 0.0;
    for (int j = j0; j <= j1; ++j) a += wc[j] * g[o - j + R];
    wd[m] = a;
    sum += a;
  }
  for (int m = 0; m < cnt; ++m) w[m] = (float)(wd[m] / sum);
  *lo_out = lo;
  *cnt_out = cnt;
}

// step 1 of resize.h with the blur folded in.  Every thread of the workgroup calls it (it holds barriers).
__device__ __forceinline__ void dg_tables(DgShared& sh, const DgParams& q, const RsAxis& ay, const RsAxis& ax, int oy0, int ny, int ox0, int nx) {
  const int t = threadIdx.x;
  if (q.Ry && t <= 2 * q.Ry) {
    const double d = (double)(t - q.Ry);
    sh.g[0][t] = exp(-(d * d) / (2.0 * q.sy * q.sy));
  } else if (q.Rx && t >= RS_TOX && t - RS_TOX <= 2 * q.Rx) {
    const double d = (double)(t - RS_TOX - q.Rx);
    sh.g[1][t - RS_TOX] = exp(-(d * d) / (2.0 * q.sx * q.sx));
  }
  __syncthreads();
  if ((t == 0 && q.Ry) || (t == RS_TOX && q.Rx)) {
    double* g = sh.g[t ? 1 : 0];
    const int n = 2 * (t ? q.Rx : q.Ry) + 1;
    double s = 0.0;
    for (int k = 0; k < n; ++k) s += g[k];
    for (int k = 0; k < n; ++k) g[k] = g[k] / s;
  }
  __syncthreads();
  RsShared& rs = sh.rs;
  double* scr = reinterpret_cast<double*>(rs.mid) + t * DG_SLOT;          // t < 80 where it is used
  if (t < nx) {
    if (q.Rx) dg_weights(ax, ox0 + t, q.Rx, sh.g[1], scr, rs.wx + t * RS_TAPS, &rs.lox[t], &rs.cx[t]);
    else rs_weights(ax, ox0 + t, rs.wx + t * RS_TAPS, &rs.lox[t], &rs.cx[t]);
  } else if (t >= RS_TOX && t - RS_TOX < ny) {
    const int k = t - RS_TOX;
    if (q.Ry) dg_weights(ay, oy0 + k, q.Ry, sh.g[0], scr, rs.wy + k * RS_TAPS, &rs.loy[k], &rs.cy[k]);
    else rs_weights(ay, oy0 + k, rs.wy + k * RS_TAPS, &rs.loy[k], &rs.cy[k]);
  }
  __syncthreads();
}

__global__ __launch_bounds__(256) void degrade_blind_kernel(const float* __restrict__ in, float* __restrict__ out, const long long* __restrict__ par,
                                                            int C, int H, int W, int Ho, int Wo, int tiles_y, int tiles_x, int quant_bits) {
  __shared__ DgShared sh;
  const int tiles = tiles_y * tiles_x;
  const int plane = blockIdx.x / tiles, t = blockIdx.x - plane * tiles;
  const int b = plane / C, ch = plane - b * C;
  const int ty = t / tiles_x, tx = t - ty * tiles_x;
  const int oy0 = ty * RS_TOY, ox0 = tx * RS_TOX;
  const int ny = Ho - oy0 < RS_TOY ? Ho - oy0 : RS_TOY, nx = Wo - ox0 < RS_TOX ? Wo - ox0 : RS_TOX;
  const DgParams q = dg_params(par + 4 * (long long)b);
  const RsAxis ay = rs_axis(H, Ho), ax = rs_axis(W, Wo);
  dg_tables(sh, q, ay, ax, oy0, ny, ox0, nx);
  const float* src = in + (size_t)plane * (size_t)H * (size_t)W;
  float* dst = out + (size_t)plane * (size_t)Ho * (size_t)Wo;
  const int nch = (q.gray || C == 1) ? 0 : ch;
  rs_filter(sh.rs, [=](int r, int x) { return src[(size_t)r * W + x]; },
            [=](int k, int c, float v) { dst[(size_t)(oy0 + k) * Wo + (ox0 + c)] = dg_finish(v, q, ox0 + c, oy0 + k, nch, quant_bits); }, ny, nx, 0);
}

// crop_degrade_u8_kernel (resize.hip) with ten-slot descriptors: the same tile, the same HR rectangle, composed tables and noise
__global__ __launch_bounds__(256) void crop_degrade_blind_u8_kernel(const unsigned char* __restrict__ pool, const long long* __restrict__ desc,
                                                                    float* __restrict__ lr_out, float* __restrict__ hr_out, int P, int s,
                                                                    int tiles_x, int quant_bits) {
  __shared__ DgShared sh;
  const long long* d = desc + 10 * (long long)blockIdx.y;
  const CdImage im = cd_image(pool, d);
  const DgParams q = dg_params(d + 6);
  const int H = im.H, W = im.W, C = im.C;
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int py0 = ty * CD_TOY, px0 = tx * RS_TOX;                   // the tile inside the LR patch
  const int ny = P - py0 < CD_TOY ? P - py0 : CD_TOY, nx = P - px0 < RS_TOX ? P - px0 : RS_TOX;
  const int oy0 = im.top / s + py0, ox0 = im.left / s + px0;       // the tile inside the downscaled image
  const RsAxis ay = rs_axis(H - H % s, H / s), ax = rs_axis(W - W % s, W / s);
  dg_tables(sh, q, ay, ax, oy0, ny, ox0, nx);
  const size_t n = (size_t)P * P;
  float* lo = lr_out + (size_t)blockIdx.y * 3 * n;
  for (int c = 0; c < C; ++c) {          // a gray source is filtered once, gets one draw and is written three times
    auto load = [=](int r, int x) { return cd_load(im, r, x, c); };
    if (C == 1)
      rs_filter(sh.rs, load, [=](int k, int t, float v) {
        const size_t i = (size_t)(py0 + k) * P + (px0 + t);
        v = dg_finish(v, q, ox0 + t, oy0 + k, 0, quant_bits);
        lo[i] = v; lo[n + i] = v; lo[2 * n + i] = v;
      }, ny, nx, 0);
    else
      rs_filter(sh.rs, load, [=](int k, int t, float v) {
        lo[c * n + (size_t)(py0 + k) * P + (px0 + t)] = dg_finish(v, q, ox0 + t, oy0 + k, q.gray ? 0 : c, quant_bits);
      }, ny, nx, 0);
  }
  cd_copy_hr(im, hr_out, blockIdx.y, P, s, py0, ny, px0, nx);
}

}  // namespace

int srk_launch_degrade_blind_f32(const float* x, float* out, const long long* par, int B, int C, int H, int W, int scale, int quant_bits,
                                 hipStream_t stream) {
  const int Ho = H / scale, Wo = W / scale;
  const int tiles_y = cdiv(Ho, RS_TOY), tiles_x = cdiv(Wo, RS_TOX);
  const double blocks = (double)B * C * tiles_y * tiles_x;
  SRK_REQUIRE(blocks >= 1.0 && blocks <= 2147483647.0, SRK_E_SHAPE, "degrade_blind: %.0f tiles do not fit one grid (B=%d C=%d Ho=%d Wo=%d)",
              blocks, B, C, Ho, Wo);
  hipLaunchKernelGGL(degrade_blind_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, x, out, par, C, H, W, Ho, Wo, tiles_y, tiles_x,
                     quant_bits);
  return srk_check_launch("degrade_blind_f32");
}

int srk_launch_crop_degrade_blind_u8(const unsigned char* pool, const long long* desc, float* lr_out, float* hr_out, int B, int P, int scale,
                                     int quant_bits, hipStream_t stream) {
  const int tiles_y = cdiv(P, CD_TOY), tiles_x = cdiv(P, RS_TOX);
  hipLaunchKernelGGL(crop_degrade_blind_u8_kernel, dim3(tiles_y * tiles_x, B), dim3(256), 0, stream, pool, desc, lr_out, hr_out, P, scale,
                     tiles_x, quant_bits);
  return srk_check_launch("crop_degrade_blind_u8");
}
