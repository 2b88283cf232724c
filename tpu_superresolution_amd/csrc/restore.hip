// Scale-1 restoration pairs on the device (include/srk.h: srk_noise_f32, srk_crop_restore_u8): the noise stage of degrade.h and the
// JPEG tile routine of jpeg.h, with no resize between the clean target and the degraded input.
//
// srk_noise_f32 is the whole-image noise stage: one thread per element, 1024 consecutive elements of one plane per workgroup.
//
// srk_crop_restore_u8 cuts a P x P training patch at ANY image pixel and makes it the window of the whole-image degradation: the
// 8 x 8 blocks (16 x 16 MCUs at 4:2:0) are anchored at the image's (0, 0), not at the patch, so a batch sees block edges at every phase,
// as crops of compressed files do.  A workgroup of 256 threads owns one 16 x 32 tile of the IMAGE's grid; the launch covers the
// (P + 14) / 16 + 1 by (P + 30) / 32 + 1 tiles a patch can intersect, counted from (top & ~15, left & ~31), and a workgroup whose tile
// misses its sample's patch leaves at once.  A first step reads the pool -- u8 / u16 -> [0, 1], the integer luma, the noise of dg_finish
// on whole-image coordinates, with coordinates past the image clamped to its last row and column (so a replicated pixel carries the
// noise of the pixel it replicates) -- into LDS, where the stage step of jp_tile finds it.  Only pixels inside the patch are stored.
#include "degrade.h"
#include "jpeg.h"

#pragma clang fp contract(off)

namespace {

constexpr int NS_CHUNK = 1024;          // elements of one plane per workgroup of srk_noise_f32

__global__ __launch_bounds__(256) void noise_kernel(const float* __restrict__ x, float* __restrict__ out, const long long* __restrict__ par,
                                                    int C, int H, int W, unsigned chunks, int quant_bits) {
  const unsigned plane = blockIdx.x / chunks, chunk = blockIdx.x - plane * chunks;
  const unsigned b = plane / (unsigned)C;
  const int ch = (int)(plane - b * (unsigned)C);
  const DgParams q = dg_params(par + 4 * (long long)b);          // slot 6 of the row, the sigma pair of the blur, is decoded and never used
  const size_t plane_n = (size_t)H * (size_t)W;
  const float* src = x + (size_t)plane * plane_n;
  float* dst = out + (size_t)plane * plane_n;
  const int nch = (q.gray || C == 1) ? 0 : ch;
#pragma unroll
  for (int k = 0; k < NS_CHUNK / 256; ++k) {
    const size_t i = (size_t)chunk * NS_CHUNK + k * 256 + threadIdx.x;
    if (i >= plane_n) continue;
    const size_t y = plane_n <= 0xffffffffull ? (size_t)((unsigned)i / (unsigned)W) : i / (size_t)W;
    dst[i] = dg_finish(src[i], q, (int)(i - y * (size_t)W), (int)y, nch, quant_bits);
  }
}

// the stored sample (r, x, c) of the image as an integer, u8 or u16
__device__ __forceinline__ unsigned rt_sample(const CdImage& im, int r, int x, int c) {
  const long long e = ((long long)r * im.W + x) * im.C + c;
  return im.wide ? (unsigned)reinterpret_cast<const unsigned short*>(im.img)[e] : (unsigned)im.img[e];
}

// channel ch of the CONVERTED image at (r, x): the stored sample, or the integer luma of an RGB pixel (luma != 0), over 255 / 65535
__device__ __forceinline__ float rt_convert(const CdImage& im, int r, int x, int ch, int luma) {
  if (!luma) return cd_load(im, r, x, ch);
  const unsigned y = (4899u * rt_sample(im, r, x, 0) + 9617u * rt_sample(im, r, x, 1) + 1868u * rt_sample(im, r, x, 2) + 8192u) >> 14;
  return im.wide ? (float)y / 65535.0f : (float)y / 255.0f;
}

__global__ __launch_bounds__(256) void crop_restore_u8_kernel(const unsigned char* __restrict__ pool, const long long* __restrict__ desc,
                                                              float* __restrict__ clean_out, float* __restrict__ degraded_out, int P,
                                                              int out_chans, int subsample, int tiles_x, int quant_bits) {
  __shared__ JpShared sh;
  const long long* d = desc + 10 * (long long)blockIdx.y;
  const CdImage im = cd_image(pool, d);
  const int H = im.H, W = im.W, top = im.top, left = im.left;
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int y0 = (top & ~(JP_TH - 1)) + ty * JP_TH, x0 = (left & ~(JP_TW - 1)) + tx * JP_TW;          // on the image's grid
  if (y0 >= top + P || x0 >= left + P || H < 1 || W < 1) return;          // the tile misses the patch (the same for the whole workgroup)
  // slot 6 is the quality here: the sigma pair dg_params reads from it is never used
  const DgParams q = dg_params(d + 6);
  const int quality = jp_quality((int)(unsigned)(unsigned long long)d[6]);
  const int luma = out_chans == 1 && im.C == 3;
  const int Cc = (out_chans == 3 && im.C == 3) ? 3 : 1;          // planes that are noised and coded; one plane is written out_chans times
  const int sub = subsample && Cc == 3;
  const size_t n = (size_t)P * (size_t)P;
  float* clean = clean_out + (size_t)blockIdx.y * out_chans * n;
  float* degr = degraded_out + (size_t)blockIdx.y * out_chans * n;

  // tile pixel (r, c) -> image coordinates, clamped: every load stays inside the image
  const auto row = [=](int r) { const int y = y0 + r; return y < 0 ? 0 : (y < H ? y : H - 1); };
  const auto col = [=](int c) { const int x = x0 + c; return x < 0 ? 0 : (x < W ? x : W - 1); };
  const auto keep = [=](int r, int c) { return y0 + r >= top && y0 + r < top + P && x0 + c >= left && x0 + c < left + P; };
  // channel ch of a coded pixel goes to output channel ch, the one plane of a gray pixel to every output channel
  const auto put = [=](float* o, int r, int c, int ch, float v) {
    const size_t at = (size_t)(y0 + r - top) * P + (x0 + c - left);
    if (Cc == 3 || out_chans == 1) {
      o[ch * n + at] = v;
    } else {
      o[at] = v;
      o[n + at] = v;
      o[2 * n + at] = v;
    }
  };

  // stage 0, ONE instance of the conversion and the noise: the clean target; the noised plane(s) into b, laid out as jp_tile lays out a
  // (its stage step reads them back before pass 1 writes b); without a JPEG stage the noised values are the degraded input
  float* nb = sh.b;
  for (int i = threadIdx.x; i < Cc * JP_TH * JP_TW; i += 256) {
    const int ch = i / (JP_TH * JP_TW), r = (i / JP_TW) % JP_TH, c = i % JP_TW;
    const bool kept = keep(r, c);
    if (quality == 0 && !kept) continue;
    const int y = row(r), x = col(c);
    const float v = rt_convert(im, y, x, ch, luma);
    const float nv = dg_finish(v, q, x, y, (q.gray || Cc == 1) ? 0 : ch, quant_bits);
    nb[ch * JP_TH * JP_LD + r * JP_LD + c] = nv;
    if (kept) {
      put(clean, r, c, ch, v);
      if (quality == 0) put(degr, r, c, ch, nv);
    }
  }
  if (quality == 0) return;
  __syncthreads();

  jp_tile(
      sh, quality, Cc, sub,
      [=](int r, int c, float* v) {
        const int l = r * JP_LD + c;
        v[0] = nb[l];
        if (Cc == 3) {
          v[1] = nb[JP_TH * JP_LD + l];
          v[2] = nb[2 * JP_TH * JP_LD + l];
        }
      },
      keep, [=](int r, int c, int ch, float v) { put(degr, r, c, ch, v); }, [](const JpBlock&, int, int, float) {});
}

}  // namespace

int srk_launch_noise_f32(const float* x, float* out, const long long* par, int B, int C, int H, int W, int quant_bits, hipStream_t stream) {
  const long long chunks = ((long long)H * W + (NS_CHUNK - 1)) / NS_CHUNK;          // H * W < 2^62
  const double blocks = (double)B * C * (double)chunks;
  SRK_REQUIRE(blocks >= 1.0 && blocks <= 2147483647.0, SRK_E_SHAPE, "noise: %.0f workgroups do not fit one grid (B=%d C=%d H=%d W=%d)", blocks, B, C,
              H, W);
  hipLaunchKernelGGL(noise_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, x, out, par, C, H, W, (unsigned)chunks, quant_bits);
  return srk_check_launch("noise_f32");
}

int srk_launch_crop_restore_u8(const unsigned char* pool, const long long* desc, float* clean_out, float* degraded_out, int B, int P,
                               int out_chans, int subsample, int quant_bits, hipStream_t stream) {
  const int tiles_y = (P + JP_TH - 2) / JP_TH + 1, tiles_x = (P + JP_TW - 2) / JP_TW + 1;          // at the worst phase of top / left
  hipLaunchKernelGGL(crop_restore_u8_kernel, dim3(tiles_y * tiles_x, B), dim3(256), 0, stream, pool, desc, clean_out, degraded_out, P, out_chans,
                     subsample, tiles_x, quant_bits);
  return srk_check_launch("crop_restore_u8");
}
