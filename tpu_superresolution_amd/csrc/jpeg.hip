// JPEG round trip on the device (include/srk.h: srk_jpeg_roundtrip_f32): what a baseline JPEG file of an 8-bit image at quality q
// decodes to, as a closed-form fp32 pipeline -- level, JFIF YCbCr, 8 x 8 DCT, libjpeg-scaled Annex K quantisation, inverse, RGB.
// Entropy coding is lossless and is not done.  The steps and their arithmetic are spelled out in srk.h; tests/jpeg_ref.py restates them.
//
// The tile routine, its constants and its LDS layout are in jpeg.h (shared with restore.hip); this file places the tiles on a whole
// image: the grid is B x tiles -- a batch of 32 patches of 64 x 64 is 256 workgroups -- and rows / columns past the image replicate
// the last.  A sample with quality 0 is copied as 32-bit words, NaNs included.
#include "jpeg.h"

#pragma clang fp contract(off)

namespace {

__global__ __launch_bounds__(256) void jpeg_roundtrip_kernel(const float* __restrict__ x, float* __restrict__ out, const int* __restrict__ quality,
                                                             int C, int H, int W, int Hm, int Wm, int sub, int tiles_y, int tiles_x,
                                                             short* __restrict__ coef) {
  __shared__ JpShared sh;
  const int t = threadIdx.x;
  const int tiles = tiles_y * tiles_x;
  const int b = blockIdx.x / tiles, tile = blockIdx.x - b * tiles;
  const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
  const int y0 = ty * JP_TH, x0 = tx * JP_TW;
  const size_t plane_n = (size_t)H * (size_t)W;
  const float* src = x + (size_t)b * C * plane_n;
  float* dst = out + (size_t)b * C * plane_n;
  const int q = jp_quality(quality[b]);

  if (q == 0) {          // pass-through, bit for bit
    const unsigned* s32 = reinterpret_cast<const unsigned*>(src);
    unsigned* d32 = reinterpret_cast<unsigned*>(dst);
    for (int i = t; i < C * JP_TH * JP_TW; i += 256) {
      const int c = i / (JP_TH * JP_TW), r = i - c * (JP_TH * JP_TW);
      const int y = y0 + r / JP_TW, xx = x0 + r % JP_TW;
      if (y < H && xx < W) {
        const size_t o = c * plane_n + (size_t)y * W + xx;
        d32[o] = s32[o];
      }
    }
    return;
  }

  // coordinates past the image replicate its last row / column (libjpeg's edge expansion)
  jp_tile(
      sh, q, C, sub,
      [=](int r, int c, float* v) {
        int y = y0 + r, xx = x0 + c;
        y = y < H ? y : H - 1;
        xx = xx < W ? xx : W - 1;
        const size_t o = (size_t)y * W + xx;
        v[0] = src[o];
        if (C == 3) {
          v[1] = src[plane_n + o];
          v[2] = src[2 * plane_n + o];
        }
      },
      [=](int r, int c) { return y0 + r < H && x0 + c < W; },
      [=](int r, int c, int ch, float v) { dst[ch * plane_n + ((size_t)(y0 + r) * W + (x0 + c))] = v; },
      [=](const JpBlock& k, int v, int u, float kq) {
        if (coef) {
          const int chroma = sub && k.plane;
          const int row = (chroma ? y0 / 2 : y0) + k.by * 8 + v, col = (chroma ? x0 / 2 : x0) + k.bx * 8 + u;
          if (row < (chroma ? Hm / 2 : Hm) && col < (chroma ? Wm / 2 : Wm))
            coef[((size_t)b * C + k.plane) * ((size_t)Hm * Wm) + (size_t)row * Wm + col] = (short)kq;
        }
      });
}

}  // namespace

int srk_launch_jpeg_roundtrip_f32(const float* x, float* out, const int* quality, int B, int C, int H, int W, int subsample, short* coef_out,
                                  hipStream_t stream) {
  const int sub = subsample && C == 3;
  const int mcu = sub ? 16 : 8;
  const long long Hm = ((long long)H + mcu - 1) / mcu * mcu, Wm = ((long long)W + mcu - 1) / mcu * mcu;
  const long long tiles_y = (Hm + JP_TH - 1) / JP_TH, tiles_x = (Wm + JP_TW - 1) / JP_TW;
  const double blocks = (double)B * (double)tiles_y * (double)tiles_x;
  SRK_REQUIRE(Hm <= 2147483647LL && Wm <= 2147483647LL && blocks >= 1.0 && blocks <= 2147483647.0, SRK_E_SHAPE,
              "jpeg_roundtrip: %.0f tiles do not fit one grid (B=%d H=%d W=%d)", blocks, B, H, W);
  hipLaunchKernelGGL(jpeg_roundtrip_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, x, out, quality, C, H, W, (int)Hm, (int)Wm, sub,
                     (int)tiles_y, (int)tiles_x, coef_out);
  return srk_check_launch("jpeg_roundtrip_f32");
}
