// The device routines of the closed-form JPEG round trip (include/srk.h: srk_jpeg_roundtrip_f32), shared by jpeg.hip
// (srk_jpeg_roundtrip_f32) and restore.hip (srk_crop_restore_u8): both files run the same code on the same values, so a training patch
// cut at any image pixel is bit-identical to the same window of the whole-image round trip.
//
// One workgroup of 256 threads owns a JP_TH x JP_TW = 16 x 32 pixel tile of one sample: two rows of four blocks per component at
// 4:4:4, two 16 x 16 MCUs at 4:2:0 (eight Y blocks and two blocks of each chroma plane).  The tile lives in two LDS buffers that the
// passes ping-pong between:
//   stage    load -> a     level + colour per pixel, rows of 32 consecutive floats
//   (4:2:0)  a -> a.sub    the 2 x 2 means of the chroma planes, 8 x 16 each
//   pass 1   a -> b        horizontal DCT        pass 2   b -> a   vertical DCT, divide, round (-> coef), multiply back
//   pass 3   a -> b        vertical inverse      pass 4   b -> a   horizontal inverse, + 128, round, clamp
//   finish   a -> store    chroma replicated, RGB
// In passes 1..4 a thread produces ONE output per turn, i = t, t + 256, ..: its frequency / position index is i & 7 = t & 7 for every
// turn, so the row D[t & 7][.] (forward) and the column D[.][t & 7] (inverse) stay in 16 registers.  The 8 lanes that share a row or
// column read the same 8 LDS words (broadcast).  Rows are JP_LD = 36 floats apart: in the column passes a 32-lane group touches
// 8 rows x 4 columns, banks 4 r + c -- all 32 distinct (at the bare 8- or 32-float stride they would be 8- to 32-way conflicts);
// the row passes write 4 rows x 8 columns, banks 4 r + c again, a 2-way conflict on the store only.
#pragma once
#include "kernels.h"

#pragma clang fp contract(off)

namespace {

constexpr int JP_TH = 16, JP_TW = 32, JP_LD = 36;
constexpr int JP_FULL = 3 * JP_TH * JP_LD;             // three full planes
constexpr int JP_SUB = 2 * (JP_TH / 2) * JP_LD;        // two subsampled chroma planes
constexpr int JP_BUF = JP_FULL + JP_SUB;

// D[u][k] = 1/2 c_u cos((2k + 1) u pi / 16), c_0 = 1/sqrt(2): evaluated in fp64, rounded once to fp32
__constant__ float JP_D[64] = {
    0.353553385f, 0.353553385f, 0.353553385f, 0.353553385f, 0.353553385f, 0.353553385f, 0.353553385f, 0.353553385f,
    0.490392625f, 0.415734798f, 0.277785122f, 0.0975451618f, -0.0975451618f, -0.277785122f, -0.415734798f, -0.490392625f,
    0.461939752f, 0.191341713f, -0.191341713f, -0.461939752f, -0.461939752f, -0.191341713f, 0.191341713f, 0.461939752f,
    0.415734798f, -0.0975451618f, -0.490392625f, -0.277785122f, 0.277785122f, 0.490392625f, 0.0975451618f, -0.415734798f,
    0.353553385f, -0.353553385f, -0.353553385f, 0.353553385f, 0.353553385f, -0.353553385f, -0.353553385f, 0.353553385f,
    0.277785122f, -0.490392625f, 0.0975451618f, 0.415734798f, -0.415734798f, -0.0975451618f, 0.490392625f, -0.277785122f,
    0.191341713f, -0.461939752f, 0.461939752f, -0.191341713f, -0.191341713f, 0.461939752f, -0.461939752f, 0.191341713f,
    0.0975451618f, -0.277785122f, 0.415734798f, -0.490392625f, 0.490392625f, -0.415734798f, 0.277785122f, -0.0975451618f};

// ITU-T T.81 Annex K, tables K.1 (luminance) and K.2 (chrominance), natural order
__constant__ unsigned char JP_BASE[2][64] = {
    {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
     18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};

struct JpShared {
  float a[JP_BUF], b[JP_BUF];
  float q[2][64];
};

// a quality word as the kernels take it: any bit pattern into 0..100 (0 = no JPEG stage)
__device__ __forceinline__ int jp_quality(int q) { return q < 0 ? 0 : (q > 100 ? 100 : q); }

__device__ __forceinline__ float jp_round8(float v) { return fminf(fmaxf(rintf(v), 0.f), 255.f); }

// block j of the tile: its offset in a buffer, its plane, and its block row / column inside the plane's part of the tile
struct JpBlock {
  int off, plane, by, bx;
};

__device__ __forceinline__ JpBlock jp_block(int j, int sub) {
  JpBlock k;
  if (sub && j >= 8) {          // 4:2:0: blocks 8, 9 = Cb, 10, 11 = Cr
    k.plane = 1 + ((j - 8) >> 1);
    k.by = 0;
    k.bx = (j - 8) & 1;
    k.off = JP_FULL + (k.plane - 1) * (JP_TH / 2) * JP_LD + k.bx * 8;
  } else {
    k.plane = j >> 3;
    k.by = (j >> 2) & 1;
    k.bx = j & 3;
    k.off = k.plane * JP_TH * JP_LD + k.by * 8 * JP_LD + k.bx * 8;
  }
  return k;
}

// One tile at quality q in 1..100, C = 1 or 3 coded planes, sub = 4:2:0 (C == 3 only).  Every thread of the workgroup calls it (it holds
// barriers).  r, c below are the row and column of a pixel INSIDE the tile; the tile's place on the image's block grid is the caller's.
//   load(r, c, v)           -> v[0 .. C): the pixel's fp32 values in image units; the caller replicates the image's last row / column
//   keep(r, c)              -> whether the pixel is stored at all (inside the image, inside the patch)
//   store(r, c, ch, v)      <- the decoded value of channel ch < C, level / 255
//   coef(k, v, u, kq)       <- the quantised coefficient (v, u) of block k: the test port of srk_jpeg_roundtrip_f32
template <class Load, class Keep, class Store, class Coef>
__device__ __forceinline__ void jp_tile(JpShared& sh, int q, int C, int sub, const Load& load, const Keep& keep, const Store& store,
                                        const Coef& coef) {
  const int t = threadIdx.x;
  if (t < 128) {          // the two tables, libjpeg's jpeg_quality_scaling and jpeg_add_quant_table
    const int s = q < 50 ? 5000 / q : 200 - 2 * q;
    int v = ((int)JP_BASE[t >> 6][t & 63] * s + 50) / 100;
    v = v < 1 ? 1 : (v > 255 ? 255 : v);
    sh.q[t >> 6][t & 63] = (float)v;
  }
  float d[8], dt[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    d[k] = JP_D[(t & 7) * 8 + k];
    dt[k] = JP_D[k * 8 + (t & 7)];
  }

  // stage: level, colour
  for (int i = t; i < JP_TH * JP_TW; i += 256) {
    const int r = i / JP_TW, c = i - r * JP_TW;
    const int l = r * JP_LD + c;
    float v[3];
    load(r, c, v);
    const float R = rintf(fminf(fmaxf(v[0], 0.f), 1.f) * 255.f);
    if (C == 3) {
      const float G = rintf(fminf(fmaxf(v[1], 0.f), 1.f) * 255.f);
      const float Bl = rintf(fminf(fmaxf(v[2], 0.f), 1.f) * 255.f);
      sh.a[l] = jp_round8(fmaf(0.114f, Bl, fmaf(0.587f, G, 0.299f * R)));
      sh.a[JP_TH * JP_LD + l] = jp_round8(fmaf(0.5f, Bl, fmaf(-0.331264108f, G, fmaf(-0.168735892f, R, 128.f))));
      sh.a[2 * JP_TH * JP_LD + l] = jp_round8(fmaf(-0.081312411f, Bl, fmaf(-0.418687589f, G, fmaf(0.5f, R, 128.f))));
    } else {
      sh.a[l] = R;
    }
  }
  __syncthreads();
  if (sub) {          // the 2 x 2 means: 2 planes x 8 x 16 = 256 values, exact in fp32
    const int p = t >> 7, r = (t >> 4) & 7, c = t & 15;
    const float* f = sh.a + (1 + p) * JP_TH * JP_LD + 2 * r * JP_LD + 2 * c;
    sh.a[JP_FULL + p * (JP_TH / 2) * JP_LD + r * JP_LD + c] = (f[0] + f[1] + f[JP_LD] + f[JP_LD + 1]) * 0.25f;
    __syncthreads();
  }

  const int nblk = sub ? 12 : C * 8;
  const int n = nblk * 64;
  const int lo = t & 7;          // = i & 7 on every turn
  // pass 1, horizontal: b[r][u] = sum_k D[u][k] (a[r][k] - 128), u = lo
  for (int i = t; i < n; i += 256) {
    const JpBlock k = jp_block(i >> 6, sub);
    const int o = k.off + ((i >> 3) & 7) * JP_LD;
    float acc = 0.f;
#pragma unroll
    for (int m = 0; m < 8; ++m) acc = fmaf(d[m], sh.a[o + m] - 128.f, acc);
    sh.b[o + lo] = acc;
  }
  __syncthreads();
  // pass 2, vertical: c[v][u] = sum_k D[v][k] b[k][u], v = lo; k = rintf(c / Q); a[v][u] = k Q
  for (int i = t; i < n; i += 256) {
    const JpBlock k = jp_block(i >> 6, sub);
    const int u = (i >> 3) & 7;
    const int o = k.off + u;
    float acc = 0.f;
#pragma unroll
    for (int m = 0; m < 8; ++m) acc = fmaf(d[m], sh.b[o + m * JP_LD], acc);
    const float Q = sh.q[k.plane ? 1 : 0][lo * 8 + u];
    const float kq = rintf(acc / Q);
    sh.a[o + lo * JP_LD] = kq * Q;
    coef(k, lo, u, kq);
  }
  __syncthreads();
  // pass 3, vertical inverse: b[y][u] = sum_v D[v][y] a[v][u], y = lo
  for (int i = t; i < n; i += 256) {
    const JpBlock k = jp_block(i >> 6, sub);
    const int o = k.off + ((i >> 3) & 7);
    float acc = 0.f;
#pragma unroll
    for (int m = 0; m < 8; ++m) acc = fmaf(dt[m], sh.a[o + m * JP_LD], acc);
    sh.b[o + lo * JP_LD] = acc;
  }
  __syncthreads();
  // pass 4, horizontal inverse: a[y][x] = round8(sum_u D[u][x] b[y][u] + 128), x = lo
  for (int i = t; i < n; i += 256) {
    const JpBlock k = jp_block(i >> 6, sub);
    const int o = k.off + ((i >> 3) & 7) * JP_LD;
    float acc = 0.f;
#pragma unroll
    for (int m = 0; m < 8; ++m) acc = fmaf(dt[m], sh.b[o + m], acc);
    sh.a[o + lo] = jp_round8(acc + 128.f);
  }
  __syncthreads();
  // finish: chroma by replication, RGB, level / 255
  for (int i = t; i < JP_TH * JP_TW; i += 256) {
    const int r = i / JP_TW, c = i - r * JP_TW;
    if (!keep(r, c)) continue;
    const float Y = sh.a[r * JP_LD + c];
    float v0 = Y;          // channel 0: R, or the one plane
    if (C == 3) {
      const int l = sub ? JP_FULL + (r >> 1) * JP_LD + (c >> 1) : JP_TH * JP_LD + r * JP_LD + c;
      const float cb = sh.a[l] - 128.f, cr = sh.a[l + (sub ? JP_TH / 2 : JP_TH) * JP_LD] - 128.f;
      v0 = jp_round8(fmaf(1.402f, cr, Y));
      store(r, c, 1, jp_round8(fmaf(-0.714136286f, cr, fmaf(-0.344136286f, cb, Y))) / 255.0f);
      store(r, c, 2, jp_round8(fmaf(1.772f, cb, Y)) / 255.0f);
    }
    store(r, c, 0, v0 / 255.0f);
  }
}

}  // namespace
