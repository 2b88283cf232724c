// The device routines of the antialiased bicubic resampler, shared by resize.hip (srk_resize_aa_f32, srk_crop_degrade_u8) and degrade.hip
// (srk_degrade_blind_f32, srk_crop_degrade_blind_u8): both files run the same code on the same values.
//
// Per axis n_in -> n_out, scale = n_in / n_out in fp64: support = 2 max(scale, 1), centre c = scale (i + 0.5), taps
// [lo, hi) = [max(int(c - support + .5), 0), min(int(c + support + .5), n_in)), w_j = k((j + lo - c + .5) / max(scale, 1)) / sum:
// taps outside the image are dropped and the rest renormalised.  The weights are evaluated and normalised in fp64 (contraction off)
// and rounded once to fp32; the horizontal pass runs first, then the vertical pass, each an ascending-tap chain of fmaf from 0.
//
// One 256-thread workgroup makes one tile of 16 x 64 outputs of one plane (8 x 64 of one training patch):
//   1. tables: lane t < 64 computes the taps of output column t, lane 64 + t < 80 those of output row t (once per workgroup; for an
//      integer factor every interior output gets the same bits because lo - c does not depend on i).  Weight rows have a pitch of 33
//      floats, so the 64 lanes of the horizontal pass (same tap, neighbouring outputs) fall into distinct banks.
//   2. horizontal pass, up to four input rows per wave and round: the wave copies the row segments [lo(first column), hi(last column))
//      into LDS with coalesced loads (the u8 / u16 -> [0, 1] conversion of the pool happens here), element e at e + e / 32 -- the skew
//      keeps the stride-2 and stride-4 reads of the /2 and /4 factors conflict-free -- and each lane forms one output column.  The
//      result goes to mid[row][64] in LDS and never to HBM.
//   3. vertical pass: lane = column, wave = output row (mod 4); mid is read along rows (conflict-free), the weight is a broadcast.
// Both entry points run the SAME three routines on the same fp32 values, which makes a training patch bit-identical to the window
// of the whole-image resize.  Shrinking by more than 8x needs more than 33 taps and is refused by the host.
#pragma once
#include "kernels.h"

#pragma clang fp contract(off)     // the fp64 weights: no fused multiply-add the formula does not spell

namespace {

constexpr int RS_TOX = 64;          // output columns per tile (one per lane)
constexpr int RS_TOY = 16;          // output rows per tile of srk_resize_aa_f32
constexpr int CD_TOY = 8;           // output rows per tile of srk_crop_degrade_u8: twice the workgroups for a batch of small patches
constexpr int RS_TAPS = 33;         // int(c + 16.5) - int(c - 15.5) at scale 8; also the (odd) pitch of a weight row
constexpr int RS_ROWS = 160;        // input rows under 16 output rows: <= 15 * 8 + 33 = 153
constexpr int RS_SEG = 576;         // input columns under 64 output columns: <= 63 * 8 + 33 = 537, + 16 of skew

struct RsAxis {
  int n_in, n_out;
  double scale, support, inv;
};

struct RsShared {
  float mid[RS_ROWS * RS_TOX];
  float wx[RS_TOX * RS_TAPS];
  float wy[RS_TOY * RS_TAPS];
  float stage[4 * RS_SEG];
  int lox[RS_TOX], cx[RS_TOX], loy[RS_TOY], cy[RS_TOY];
};

__device__ __forceinline__ RsAxis rs_axis(int n_in, int n_out) {
  RsAxis a;
  a.n_in = n_in;
  a.n_out = n_out;
  a.scale = (double)n_in / (double)n_out;
  const double m = a.scale > 1.0 ? a.scale : 1.0;
  a.support = 2.0 * m;
  a.inv = 1.0 / m;
  return a;
}

__device__ __forceinline__ double rs_cubic(double x) {
  const double a = -0.5;
  x = fabs(x);
  if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * (x * x) + 1.0;
  if (x < 2.0) return (((x - 5.0) * x + 8.0) * x - 4.0) * a;
  return 0.0;
}

// centre c and taps [lo, lo + cnt) of output i (an index into the whole axis).  i outside [0, n_out) (a caller's mistake) gives no taps.
__device__ __forceinline__ void rs_span(const RsAxis& ax, int i, double* c_out, int* lo_out, int* cnt_out) {
  const double c = ax.scale * ((double)i + 0.5);
  int lo = (int)(c - ax.support + 0.5), hi = (int)(c + ax.support + 0.5);
  lo = lo < 0 ? 0 : lo;
  hi = hi > ax.n_in ? ax.n_in : hi;
  int cnt = hi - lo;
  cnt = (i < 0 || i >= ax.n_out || cnt < 0) ? 0 : (cnt > RS_TAPS ? RS_TAPS : cnt);
  *c_out = c;
  *lo_out = lo;
  *cnt_out = cnt;
}

// taps of output i (an index into the whole axis): w[0 .. cnt) in fp32, first tap lo.
__device__ __forceinline__ void rs_weights(const RsAxis& ax, int i, float* w, int* lo_out, int* cnt_out) {
  double c;
  int lo, cnt;
  rs_span(ax, i, &c, &lo, &cnt);
  double s = 0.0;
  for (int j = 0; j < cnt; ++j) s += rs_cubic(((double)(j + lo) - c + 0.5) * ax.inv);
  for (int j = 0; j < cnt; ++j) w[j] = (float)(rs_cubic(((double)(j + lo) - c + 0.5) * ax.inv) / s);
  *lo_out = lo;
  *cnt_out = cnt;
}

// step 1: the tables of the tile whose first output is (oy0, ox0); ny <= 16 rows and nx <= 64 columns of it exist
__device__ __forceinline__ void rs_tables(RsShared& sh, const RsAxis& ay, const RsAxis& ax, int oy0, int ny, int ox0, int nx) {
  const int t = threadIdx.x;
  if (t < nx) rs_weights(ax, ox0 + t, sh.wx + t * RS_TAPS, &sh.lox[t], &sh.cx[t]);
  else if (t >= RS_TOX && t - RS_TOX < ny) rs_weights(ay, oy0 + t - RS_TOX, sh.wy + (t - RS_TOX) * RS_TAPS, &sh.loy[t - RS_TOX], &sh.cy[t - RS_TOX]);
  __syncthreads();
}

__device__ __forceinline__ float rs_quant8(float v) { return rintf(fminf(fmaxf(v, 0.f), 1.f) * 255.0f) / 255.0f; }

// steps 2 and 3 for one plane: load(row, col) -> the fp32 input value, store(k, t, v) <- output (oy0 + k, ox0 + t).
// Every thread of the workgroup calls it (it holds barriers); it ends with one, so mid can be reused at once.
template <class Load, class Store>
__device__ __forceinline__ void rs_filter(RsShared& sh, const Load& load, const Store& store, int ny, int nx, int quant_bits) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r0 = sh.loy[0], x0 = sh.lox[0];                     // lo and hi do not decrease along an axis
  int nrows = sh.loy[ny - 1] + sh.cy[ny - 1] - r0, seg = sh.lox[nx - 1] + sh.cx[nx - 1] - x0;
  nrows = nrows > RS_ROWS ? RS_ROWS : nrows;
  seg = seg > RS_SEG - RS_SEG / 32 ? RS_SEG - RS_SEG / 32 : seg;
  // a wave takes `rpw` (1..4) consecutive input rows per round -- as many as fit its 576 staging floats -- and issues the loads of all of
  // them before the first LDS write: fewer rounds, each of which exposes one global-load latency and two barriers
  const int pitch = seg + (seg >> 5) + 1;
  int rpw = pitch > 0 ? RS_SEG / pitch : 1;
  rpw = rpw > 4 ? 4 : (rpw < 1 ? 1 : rpw);
  float* st = sh.stage + wave * RS_SEG;
  for (int rb = 0; rb < nrows; rb += 4 * rpw) {
    const int rw = rb + wave * rpw;
    for (int e = lane; e < seg; e += 64) {
      float v[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) v[k] = (k < rpw && rw + k < nrows) ? load(r0 + rw + k, x0 + e) : 0.f;
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (k < rpw && rw + k < nrows) st[k * pitch + e + (e >> 5)] = v[k];
    }
    __syncthreads();
    if (lane < nx) {
      const float* w = sh.wx + lane * RS_TAPS;
      const int b = sh.lox[lane] - x0, cnt = sh.cx[lane];
      for (int k = 0; k < rpw && rw + k < nrows; ++k) {
        const float* row = st + k * pitch;
        float acc = 0.f;
        for (int j = 0; j < cnt; ++j) acc = fmaf(w[j], row[(b + j) + ((b + j) >> 5)], acc);
        sh.mid[(rw + k) * RS_TOX + lane] = acc;
      }
    }
    __syncthreads();
  }
  for (int k = wave; k < ny; k += 4) {
    if (lane < nx) {
      const float* w = sh.wy + k * RS_TAPS;
      const int b = sh.loy[k] - r0, cnt = sh.cy[k];
      float acc = 0.f;
      for (int j = 0; j < cnt && b + j < RS_ROWS; ++j) acc = fmaf(w[j], sh.mid[(b + j) * RS_TOX + lane], acc);
      store(k, lane, quant_bits == 8 ? rs_quant8(acc) : acc);
    }
  }
  __syncthreads();
}

// One pool descriptor {byte offset, H, W, C | wide << 8, top, left} (include/srk.h: srk_paired_crop_u8).
struct CdImage {
  const unsigned char* img;
  int H, W, C, wide, top, left;
};

__device__ __forceinline__ CdImage cd_image(const unsigned char* pool, const long long* d) {
  return CdImage{pool + d[0], (int)d[1], (int)d[2], (int)(d[3] & 0xff), (int)((d[3] >> 8) & 1), (int)d[4], (int)d[5]};
}

// element (r, x, c) of the image in [0, 1], converted as crop_u8_kernel (misc.hip) converts it
__device__ __forceinline__ float cd_load(const CdImage& im, int r, int x, int c) {
  const long long e = ((long long)r * im.W + x) * im.C + c;
  return im.wide ? (float)reinterpret_cast<const unsigned short*>(im.img)[e] / 65535.0f : (float)im.img[e] / 255.0f;
}

// the HR rectangle under the LR tile (py0, px0) + ny x nx of a P x P patch: rows [py0 * s, (py0 + ny) * s) x columns
// [px0 * s, (px0 + nx) * s) of the P*s square, into sample b of hr_out = [B][3][P*s][P*s]
__device__ __forceinline__ void cd_copy_hr(const CdImage& im, float* hr_out, unsigned b, int P, int s, int py0, int ny, int px0, int nx) {
  const unsigned char* img = im.img;
  const int H = im.H, W = im.W, C = im.C, wide = im.wide, top = im.top, left = im.left;
  const int Ph = P * s, hw = nx * s, hn = ny * s * hw;
  const size_t nh = (size_t)Ph * Ph;
  float* ho = hr_out + (size_t)b * 3 * nh;
  for (int i = threadIdx.x; i < hn; i += 256) {
    const int yy = i / hw, y = py0 * s + yy, x = px0 * s + (i - yy * hw);
    float c0 = 0.f, c1 = 0.f, c2 = 0.f;
    if (top + y < H && left + x < W) {   // a descriptor outside its image reads nothing (the caller checks; this only keeps the loads in)
      const long long e = ((long long)(top + y) * W + (left + x)) * C;
      if (wide) {
        const unsigned short* px = reinterpret_cast<const unsigned short*>(img) + e;
        c0 = (float)px[0] / 65535.0f;
        c1 = C == 1 ? c0 : (float)px[1] / 65535.0f;
        c2 = C == 1 ? c0 : (float)px[2] / 65535.0f;
      } else {
        const unsigned char* px = img + e;
        c0 = (float)px[0] / 255.0f;
        c1 = C == 1 ? c0 : (float)px[1] / 255.0f;
        c2 = C == 1 ? c0 : (float)px[2] / 255.0f;
      }
    }
    const size_t o = (size_t)y * Ph + x;
    ho[o] = c0;
    ho[nh + o] = c1;
    ho[2 * nh + o] = c2;
  }
}

}  // namespace
