// The ragged forms of the resize and of the JPEG round trip (include/srk.h "Ragged batches": srk_resize_aa_ragged_f32,
// srk_jpeg_roundtrip_ragged_f32): every sample of a padded batch has its own extents, read from device memory, so a chain of stages
// can give each sample its own intermediate size in one launch per stage and without a host read.
//
// No arithmetic of its own: the kernels below place the tiles of resize.hip / jpeg.hip on sample b's extents and run the shared device
// routines (rs_tables / rs_filter of resize.h, jp_tile of jpeg.h) on them -- the same tile grid from (0, 0), the same values, so sample b
// is bit-identical to the dense entry on that sample alone.  The grid covers the padded extents; a workgroup whose tile lies outside
// its sample's extents leaves before any barrier.  Loads and stores stay inside the extents (ragged.h clamps them into the buffer).
#include "jpeg.h"
#include "ragged.h"
#include "resize.h"

#pragma clang fp contract(off)

namespace {

__global__ __launch_bounds__(256) void resize_aa_ragged_kernel(const float* __restrict__ in, const int* __restrict__ ext_in,
                                                               float* __restrict__ out, const int* __restrict__ ext_out, int C, int Hp, int Wp,
                                                               int Hop, int Wop, int tiles_y, int tiles_x, int quant_bits) {
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
  rs_tables(sh, ay, ax, oy0, ny, ox0, nx);
  const float* src = in + (size_t)plane * (size_t)Hp * (size_t)Wp;
  float* dst = out + (size_t)plane * (size_t)Hop * (size_t)Wop;
  rs_filter(sh, [=](int r, int x) { return src[(size_t)r * Wp + x]; },
            [=](int k, int c, float v) { dst[(size_t)(oy0 + k) * Wop + (ox0 + c)] = v; }, ny, nx, quant_bits);
}

__global__ __launch_bounds__(256) void jpeg_roundtrip_ragged_kernel(const float* __restrict__ x, float* __restrict__ out,
                                                                    const int* __restrict__ quality, const int* __restrict__ ext, int C, int Hp,
                                                                    int Wp, int sub, int tiles_y, int tiles_x) {
  __shared__ JpShared sh;
  const int t = threadIdx.x;
  const int tiles = tiles_y * tiles_x;
  const int b = blockIdx.x / tiles, tile = blockIdx.x - b * tiles;
  const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
  const int H = rg_extent(ext, b, 0, Hp), W = rg_extent(ext, b, 1, Wp);
  const int y0 = ty * JP_TH, x0 = tx * JP_TW;
  if (y0 >= H || x0 >= W) return;                      // a tile is at least one MCU: nothing of it would be kept
  const size_t plane_n = (size_t)Hp * (size_t)Wp;
  const float* src = x + (size_t)b * C * plane_n;
  float* dst = out + (size_t)b * C * plane_n;
  const int q = jp_quality(quality[b]);

  if (q == 0) {          // pass-through of the in-extent words
    const unsigned* s32 = reinterpret_cast<const unsigned*>(src);
    unsigned* d32 = reinterpret_cast<unsigned*>(dst);
    for (int i = t; i < C * JP_TH * JP_TW; i += 256) {
      const int c = i / (JP_TH * JP_TW), r = i - c * (JP_TH * JP_TW);
      const int y = y0 + r / JP_TW, xx = x0 + r % JP_TW;
      if (y < H && xx < W) {
        const size_t o = c * plane_n + (size_t)y * Wp + xx;
        d32[o] = s32[o];
      }
    }
    return;
  }

  // coordinates past the sample's extents replicate its last row / column, as jpeg.hip does at the image's
  jp_tile(
      sh, q, C, sub,
      [=](int r, int c, float* v) {
        int y = y0 + r, xx = x0 + c;
        y = y < H ? y : H - 1;
        xx = xx < W ? xx : W - 1;
        const size_t o = (size_t)y * Wp + xx;
        v[0] = src[o];
        if (C == 3) {
          v[1] = src[plane_n + o];
          v[2] = src[2 * plane_n + o];
        }
      },
      [=](int r, int c) { return y0 + r < H && x0 + c < W; },
      [=](int r, int c, int ch, float v) { dst[ch * plane_n + ((size_t)(y0 + r) * Wp + (x0 + c))] = v; },
      [](const JpBlock&, int, int, float) {});
}

}  // namespace

int srk_launch_resize_aa_ragged_f32(const float* x, const int* ext_in, float* out, const int* ext_out, int B, int C, int Hp, int Wp, int Hop,
                                    int Wop, int quant_bits, hipStream_t stream) {
  const int tiles_y = cdiv(Hop, RS_TOY), tiles_x = cdiv(Wop, RS_TOX);
  const double blocks = (double)B * C * tiles_y * tiles_x;
  SRK_REQUIRE(blocks >= 1.0 && blocks <= 2147483647.0, SRK_E_SHAPE, "resize_aa_ragged: %.0f tiles do not fit one grid (B=%d C=%d Hop=%d Wop=%d)",
              blocks, B, C, Hop, Wop);
  hipLaunchKernelGGL(resize_aa_ragged_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, x, ext_in, out, ext_out, C, Hp, Wp, Hop, Wop, tiles_y,
                     tiles_x, quant_bits);
  return srk_check_launch("resize_aa_ragged_f32");
}

int srk_launch_jpeg_roundtrip_ragged_f32(const float* x, float* out, const int* quality, const int* ext, int B, int C, int Hp, int Wp,
                                         int subsample, hipStream_t stream) {
  const int sub = subsample && C == 3;
  const long long tiles_y = ((long long)Hp + JP_TH - 1) / JP_TH, tiles_x = ((long long)Wp + JP_TW - 1) / JP_TW;
  const double blocks = (double)B * (double)tiles_y * (double)tiles_x;
  SRK_REQUIRE(blocks >= 1.0 && blocks <= 2147483647.0, SRK_E_SHAPE, "jpeg_roundtrip_ragged: %.0f tiles do not fit one grid (B=%d Hp=%d Wp=%d)",
              blocks, B, Hp, Wp);
  hipLaunchKernelGGL(jpeg_roundtrip_ragged_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, x, out, quality, ext, C, Hp, Wp, sub,
                     (int)tiles_y, (int)tiles_x);
  return srk_check_launch("jpeg_roundtrip_ragged_f32");
}
