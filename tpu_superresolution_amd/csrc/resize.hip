// Antialiased bicubic resampling (Keys cubic, a = -0.5; the convention of PIL's Image.BICUBIC and of
// F.interpolate(mode='bicubic', antialias=True, align_corners=False)) on the device, and the training degradation built on it
// (include/srk.h: srk_resize_aa_f32, srk_crop_degrade_u8).
// The routines both kernels are made of -- tables, the two LDS passes -- live in resize.h (degrade.hip runs them too).
#include "resize.h"

#pragma clang fp contract(off)

namespace {

__global__ __launch_bounds__(256) void resize_aa_kernel(const float* __restrict__ in, float* __restrict__ out, int H, int W, int Ho, int Wo,
                                                        int tiles_y, int tiles_x, int quant_bits) {
  __shared__ RsShared sh;
  const int tiles = tiles_y * tiles_x;
  const int plane = blockIdx.x / tiles, t = blockIdx.x - plane * tiles;
  const int ty = t / tiles_x, tx = t - ty * tiles_x;
  const int oy0 = ty * RS_TOY, ox0 = tx * RS_TOX;
  const int ny = Ho - oy0 < RS_TOY ? Ho - oy0 : RS_TOY, nx = Wo - ox0 < RS_TOX ? Wo - ox0 : RS_TOX;
  const RsAxis ay = rs_axis(H, Ho), ax = rs_axis(W, Wo);
  rs_tables(sh, ay, ax, oy0, ny, ox0, nx);
  const float* src = in + (size_t)plane * (size_t)H * (size_t)W;
  float* dst = out + (size_t)plane * (size_t)Ho * (size_t)Wo;
  rs_filter(sh, [=](int r, int x) { return src[(size_t)r * W + x]; },
            [=](int k, int c, float v) { dst[(size_t)(oy0 + k) * Wo + (ox0 + c)] = v; }, ny, nx, quant_bits);
}

// The training degradation: workgroup (tile, b) makes one 8 x 64 tile of sample b's LR patch -- the window at (top / s, left / s) of the
// (H / s, W / s) downscale of the image's top-left (H - H % s, W - W % s) region, taps bounded by that region -- and the s-times larger
// rectangle of the HR patch under it, converted as crop_u8_kernel (misc.hip) converts it.
__global__ __launch_bounds__(256) void crop_degrade_u8_kernel(const unsigned char* __restrict__ pool, const long long* __restrict__ desc,
                                                              float* __restrict__ lr_out, float* __restrict__ hr_out, int P, int s,
                                                              int tiles_x, int quant_bits) {
  __shared__ RsShared sh;
  const CdImage im = cd_image(pool, desc + 6 * (long long)blockIdx.y);
  const int H = im.H, W = im.W, C = im.C;
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int py0 = ty * CD_TOY, px0 = tx * RS_TOX;                   // the tile inside the LR patch
  const int ny = P - py0 < CD_TOY ? P - py0 : CD_TOY, nx = P - px0 < RS_TOX ? P - px0 : RS_TOX;
  const RsAxis ay = rs_axis(H - H % s, H / s), ax = rs_axis(W - W % s, W / s);
  rs_tables(sh, ay, ax, im.top / s + py0, ny, im.left / s + px0, nx);
  const size_t n = (size_t)P * P;
  float* lo = lr_out + (size_t)blockIdx.y * 3 * n;
  for (int c = 0; c < C; ++c) {          // a gray source is filtered once and written three times
    auto load = [=](int r, int x) { return cd_load(im, r, x, c); };
    if (C == 1)
      rs_filter(sh, load, [=](int k, int t, float v) {
        const size_t i = (size_t)(py0 + k) * P + (px0 + t);
        lo[i] = v; lo[n + i] = v; lo[2 * n + i] = v;
      }, ny, nx, quant_bits);
    else
      rs_filter(sh, load, [=](int k, int t, float v) { lo[c * n + (size_t)(py0 + k) * P + (px0 + t)] = v; }, ny, nx, quant_bits);
  }
  cd_copy_hr(im, hr_out, blockIdx.y, P, s, py0, ny, px0, nx);
}

}  // namespace

int srk_launch_resize_aa_f32(const float* x, float* out, int planes, int H, int W, int Ho, int Wo, int quant_bits, hipStream_t stream) {
  const int tiles_y = cdiv(Ho, RS_TOY), tiles_x = cdiv(Wo, RS_TOX);
  const double blocks = (double)planes * tiles_y * tiles_x;
  SRK_REQUIRE(blocks >= 1.0 && blocks <= 2147483647.0, SRK_E_SHAPE, "resize_aa: %.0f tiles do not fit one grid (planes=%d Ho=%d Wo=%d)", blocks,
              planes, Ho, Wo);
  hipLaunchKernelGGL(resize_aa_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, x, out, H, W, Ho, Wo, tiles_y, tiles_x, quant_bits);
  return srk_check_launch("resize_aa_f32");
}

int srk_launch_crop_degrade_u8(const unsigned char* pool, const long long* desc, float* lr_out, float* hr_out, int B, int P, int scale,
                               int quant_bits, hipStream_t stream) {
  const int tiles_y = cdiv(P, CD_TOY), tiles_x = cdiv(P, RS_TOX);
  hipLaunchKernelGGL(crop_degrade_u8_kernel, dim3(tiles_y * tiles_x, B), dim3(256), 0, stream, pool, desc, lr_out, hr_out, P, scale, tiles_x,
                     quant_bits);
  return srk_check_launch("crop_degrade_u8");
}
