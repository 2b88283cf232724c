// General 2-D blur kernels on the device (include/srk.h: srk_blur2d_f32, srk_crop_degrade_psf_u8): a per-sample ks x ks table (a rotated,
// generalized or plateau Gaussian, a measured point-spread function) applied as a CORRELATION with the border rule of the resize per
// blurred pixel -- taps outside the image are dropped and the rest renormalised:
//   num(p, q)  = chain over a, b ascending (a outer) of fmaf(K[a][b], x(p + a - R, q + b - R), .) from 0, taps inside the image only
//   mass(p, q) = the same chain with x == 1;  blurred = num / mass (IEEE, in the interior too)
//
// One routine, bl_blur_tile_ks<KS>, makes the values of both entries.  It reads a tile staged in LDS with a halo of R = KS / 2 on every
// side, in which positions outside the image hold +0: fmaf(k, 0, acc) == acc for a finite k (acc starts at +0 and a chain of
// round-to-nearest fmaf never reaches -0 from there), so a dropped tap and a zero operand give the same bits, and only the mass chain needs
// the mask.  A thread makes a strip of four horizontal neighbours: the KS + 3 image values of a window row and the KS taps of the table
// row are read from LDS once and feed 4 KS fmaf.  The table side is a template argument (11 instantiations of either kernel, picked by
// the launcher), so the taps of a row are unrolled.  Element e of a staged row lies at e + e / 32 (the skew of resize.h), which spreads
// the stride-4 reads of 32 neighbouring strips over all banks.  A strip whose 4 + 2R window columns and 1 + 2R rows all lie inside the
// image takes `full`, the mass chain over the whole table that one thread ran once for the workgroup: the same chain, the same bits.
//
// srk_blur2d_f32: one workgroup per 32 x 64 tile of one plane.
// srk_crop_degrade_psf_u8: the 8 x 64 LR tile of crop_degrade_blind_u8_kernel.  After rs_tables the tile's cubic footprint is known
// (at most 44 rows x 268 columns at factor 4); the source under it plus the halo is staged in row bands into RsShared::mid (free until
// the filter runs), blurred into a footprint buffer `fp`, and rs_filter runs unchanged with a load() that reads fp.  Noise and rounding
// are dg_finish of degrade.h.  A gray source is blurred and filtered once and written three times.
#include "degrade.h"

#pragma clang fp contract(off)

namespace {

constexpr int BL_KMAX = 21;                       // the largest table side; R <= 10
constexpr int BL_TY = 32, BL_TX = 64;             // outputs per workgroup of srk_blur2d_f32
constexpr int BL_TW = BL_TX + BL_KMAX - 1;        // staged columns of that tile
constexpr int BL_PITCH = BL_TW + BL_TW / 32 + 1;
constexpr int BL_TROWS = BL_TY + BL_KMAX - 1;
constexpr int FP_ROWS = 48, FP_W = 272;           // the cubic footprint of an 8 x 64 LR tile at factor 4: 7 * 4 + 16 rows, 63 * 4 + 16 columns
constexpr int MID_FLOATS = RS_ROWS * RS_TOX;

struct PsfShared {
  RsShared rs;
  float fp[FP_ROWS * FP_W];
  float K[BL_KMAX * BL_KMAX];
  float full;
};
static_assert(sizeof(PsfShared) <= 160 * 1024, "the patch kernel must fit one CU's LDS");
static_assert(MID_FLOATS / (FP_W + BL_KMAX - 1 + (FP_W + BL_KMAX - 1) / 32 + 1) > BL_KMAX - 1, "a band must hold the halo and one row");

__device__ __forceinline__ int bl_skew(int e) { return e + (e >> 5); }

// A workgroup-uniform value kept in a vector register: the patch kernel holds more uniform state across the blur than there are scalar
// registers, and what only the store of an output needs can wait in a VGPR (one wave per SIMD: there are plenty).
__device__ __forceinline__ int bl_vreg(int v) {
  asm volatile("" : "+v"(v));
  return v;
}
__device__ __forceinline__ unsigned bl_vreg(unsigned v) { return (unsigned)bl_vreg((int)v); }
__device__ __forceinline__ float bl_vreg(float v) { return __int_as_float(bl_vreg(__float_as_int(v))); }

// the table of one sample into LDS, and the interior mass chain on it by thread 0.  Neither ends with a barrier: the callers' next
// barrier publishes K before bl_full_mass reads it, and the one before the blur publishes *full.
__device__ __forceinline__ void bl_load_table(const float* __restrict__ psf, int ks, float* K) {
  for (int i = threadIdx.x; i < ks * ks; i += 256) K[i] = psf[i];
}
__device__ __forceinline__ void bl_full_mass(const float* K, int ks, float* full) {
  if (threadIdx.x == 0) {
    float m = 0.f;
    for (int i = 0; i < ks * ks; ++i) m = fmaf(K[i], 1.f, m);
    *full = m;
  }
}

// Blurs nr x nc pixels whose first one is (y0, x0) of an Hr x Wr image.  tile[i * pitch + bl_skew(j)] = x(y0 - R + i, x0 - R + j), +0
// outside the image, for i < nr + 2R and j < 4 ceil(nc / 4) + 2R.  store(i, j, v) gets pixel (y0 + i, x0 + j).
// The table side is a template argument: the taps of a row are unrolled, so the KS + 3 image values and the KS taps of the row are all
// requested from LDS before the first fmaf waits for one (a workgroup of the patch kernel has the CU to itself -- one wave per SIMD --
// and a loop that waits for two reads per tap spends its time on their latency).  The order of every chain is unchanged.
template <int KS, class Store>
__device__ __forceinline__ void bl_blur_tile_ks(const float* tile, int pitch, const float* K, float full, int y0, int x0, int nr, int nc, int Hr,
                                                int Wr, const Store& store) {
  constexpr int R = KS >> 1;
  const int strips = (nc + 3) >> 2;
  for (int it = threadIdx.x; it < nr * strips; it += 256) {
    const int i = it / strips, j0 = (it - i * strips) << 2;
    const int p = y0 + i, q = x0 + j0;
    float n0 = 0.f, n1 = 0.f, n2 = 0.f, n3 = 0.f;
#pragma unroll 1
    for (int a = 0; a < KS; ++a) {
      const float* row = tile + (i + a) * pitch;
      const float* kr = K + a * KS;
      float v[KS + 3], k[KS];
#pragma unroll
      for (int t = 0; t < KS + 3; ++t) v[t] = row[bl_skew(j0 + t)];
#pragma unroll
      for (int b = 0; b < KS; ++b) k[b] = kr[b];
#pragma unroll
      for (int b = 0; b < KS; ++b) {
        n0 = fmaf(k[b], v[b], n0);
        n1 = fmaf(k[b], v[b + 1], n1);
        n2 = fmaf(k[b], v[b + 2], n2);
        n3 = fmaf(k[b], v[b + 3], n3);
      }
    }
    float m0 = full, m1 = full, m2 = full, m3 = full;
    if (p - R < 0 || p + R >= Hr || q - R < 0 || q + 3 + R >= Wr) {
      m0 = m1 = m2 = m3 = 0.f;
#pragma unroll 1                             // the border path: rolled, its compare masks would fill the scalar registers
      for (int a = 0; a < KS; ++a) {
        if ((unsigned)(p + a - R) >= (unsigned)Hr) continue;
        const float* kr = K + a * KS;
#pragma unroll 1
        for (int b = 0; b < KS; ++b) {
          const float kk = kr[b];
          const int c = q + b - R;
          if ((unsigned)c < (unsigned)Wr) m0 = fmaf(kk, 1.f, m0);
          if ((unsigned)(c + 1) < (unsigned)Wr) m1 = fmaf(kk, 1.f, m1);
          if ((unsigned)(c + 2) < (unsigned)Wr) m2 = fmaf(kk, 1.f, m2);
          if ((unsigned)(c + 3) < (unsigned)Wr) m3 = fmaf(kk, 1.f, m3);
        }
      }
    }
    store(i, j0, n0 / m0);
    if (j0 + 1 < nc) store(i, j0 + 1, n1 / m1);
    if (j0 + 2 < nc) store(i, j0 + 2, n2 / m2);
    if (j0 + 3 < nc) store(i, j0 + 3, n3 / m3);
  }
}

// stages rows [ya, ya + rows) x columns [xa, xa + cols) of an Hr x Wr image into tile (see bl_blur_tile); load(y, x) is only called inside
template <class Load>
__device__ __forceinline__ void bl_stage(float* tile, int pitch, int ya, int xa, int rows, int cols, int Hr, int Wr, const Load& load) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int i = wave; i < rows; i += 4) {
    const int y = ya + i;
    const bool rok = (unsigned)y < (unsigned)Hr;
    for (int j = lane; j < cols; j += 64) {
      const int x = xa + j;
      tile[i * pitch + bl_skew(j)] = (rok && (unsigned)x < (unsigned)Wr) ? load(y, x) : 0.f;
    }
  }
}

template <int KS>
__global__ __launch_bounds__(256) void blur2d_kernel(const float* __restrict__ in, const float* __restrict__ psf, float* __restrict__ out, int C,
                                                     int H, int W, int tiles_y, int tiles_x) {
  __shared__ float tile[BL_TROWS * BL_PITCH];
  __shared__ float K[BL_KMAX * BL_KMAX];
  __shared__ float full;
  constexpr int ks = KS, R = KS >> 1;
  const int tiles = tiles_y * tiles_x;
  const int plane = blockIdx.x / tiles, t = blockIdx.x - plane * tiles;
  const int ty = t / tiles_x, tx = t - ty * tiles_x;
  const int y0 = ty * BL_TY, x0 = tx * BL_TX;
  const int nr = H - y0 < BL_TY ? H - y0 : BL_TY, nc = W - x0 < BL_TX ? W - x0 : BL_TX;
  const float* src = in + (size_t)plane * (size_t)H * (size_t)W;
  float* dst = out + (size_t)plane * (size_t)H * (size_t)W;
  bl_load_table(psf + (size_t)(plane / C) * (size_t)(KS * KS), ks, K);
  bl_stage(tile, BL_PITCH, y0 - R, x0 - R, nr + 2 * R, ((nc + 3) & ~3) + 2 * R, H, W, [=](int y, int x) { return src[(size_t)y * W + x]; });
  __syncthreads();
  bl_full_mass(K, ks, &full);
  __syncthreads();
  bl_blur_tile_ks<KS>(tile, BL_PITCH, K, full, y0, x0, nr, nc, H, W, [=](int i, int j, float v) { dst[(size_t)(y0 + i) * W + (x0 + j)] = v; });
}

// the blurred footprint of one channel of the tile: rows [r0, r0 + nrows) x columns [x0, x0 + seg) of the region into sh.fp
template <int KS, class Load>
__device__ __forceinline__ void psf_footprint(PsfShared& sh, int r0, int nrows, int x0, int seg, int Hr, int Wr, const Load& load) {
  if (nrows <= 0 || seg <= 0) return;                           // a descriptor's mistake (uniform over the workgroup): nothing to blur
  constexpr int R = KS >> 1;
  const int cols = ((seg + 3) & ~3) + 2 * R, pitch = cols + (cols >> 5) + 1;
  const int nb = MID_FLOATS / pitch - 2 * R;                    // >= 13 blurred rows per band (static_assert above)
  float* fp = sh.fp;
  for (int i0 = 0; i0 < nrows; i0 += nb) {
    const int nbr = nrows - i0 < nb ? nrows - i0 : nb;
    bl_stage(sh.rs.mid, pitch, r0 + i0 - R, x0 - R, nbr + 2 * R, cols, Hr, Wr, load);
    __syncthreads();
    bl_blur_tile_ks<KS>(sh.rs.mid, pitch, sh.K, sh.full, r0 + i0, x0, nbr, seg, Hr, Wr, [=](int i, int j, float v) { fp[(i0 + i) * FP_W + j] = v; });
    __syncthreads();
  }
}

template <int KS>
__global__ __launch_bounds__(256) void crop_degrade_psf_u8_kernel(const unsigned char* __restrict__ pool, const long long* __restrict__ desc,
                                                                  const float* __restrict__ psf, float* __restrict__ lr_out,
                                                                  float* __restrict__ hr_out, int P, int s, int tiles_x, int quant_bits) {
  extern __shared__ __attribute__((aligned(16))) unsigned char psf_lds[];
  PsfShared& sh = *reinterpret_cast<PsfShared*>(psf_lds);
  constexpr int ks = KS;
  const long long* d = desc + 10 * (long long)blockIdx.y;
  const CdImage im = cd_image(pool, d);
  const DgParams q = dg_params(d + 6);                             // slot 6 (the sigma pair) is decoded and not used
  const int H = im.H, W = im.W, C = im.C;
  const int Hr = H - H % s > 0 ? H - H % s : 0, Wr = W - W % s > 0 ? W - W % s : 0;       // a descriptor's mistake reads nothing
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int py0 = ty * CD_TOY, px0 = tx * RS_TOX;                   // the tile inside the LR patch
  const int ny = P - py0 < CD_TOY ? P - py0 : CD_TOY, nx = P - px0 < RS_TOX ? P - px0 : RS_TOX;
  const int oy0 = im.top / s + py0, ox0 = im.left / s + px0;       // the tile inside the downscaled image
  const RsAxis ay = rs_axis(Hr, H / s), ax = rs_axis(Wr, W / s);
  cd_copy_hr(im, hr_out, blockIdx.y, P, s, py0, ny, px0, nx);       // first: what only the HR copy needs is not kept alive across the blur
  bl_load_table(psf + (size_t)blockIdx.y * (size_t)(KS * KS), ks, sh.K);
  rs_tables(sh.rs, ay, ax, oy0, ny, ox0, nx);                        // ends with a barrier: K is visible
  bl_full_mass(sh.K, ks, &sh.full);                                 // published by the staging barrier of the first band
  const int r0 = sh.rs.loy[0], x0 = sh.rs.lox[0];
  int nrows = sh.rs.loy[ny - 1] + sh.rs.cy[ny - 1] - r0, seg = sh.rs.lox[nx - 1] + sh.rs.cx[nx - 1] - x0;
  nrows = nrows > FP_ROWS ? FP_ROWS : nrows;
  seg = seg > FP_W ? FP_W : seg;
  const float* fp = sh.fp;
  auto load = [=](int r, int x) {                                  // rs_filter asks for rows r0.. and columns x0.. of the footprint
    const int i = r - r0, j = x - x0;
    return ((unsigned)i < (unsigned)FP_ROWS && (unsigned)j < (unsigned)FP_W) ? fp[i * FP_W + j] : 0.f;
  };
  const size_t n = (size_t)P * P;
  float* lo = lr_out + (size_t)blockIdx.y * 3 * n;
  DgParams qv = q;                                                  // the store's operands: see bl_vreg
  qv.sn = bl_vreg(q.sn); qv.gain = bl_vreg(q.gain); qv.k0 = bl_vreg(q.k0); qv.k1 = bl_vreg(q.k1); qv.noisy = bl_vreg(q.noisy);
  const int Pv = bl_vreg(P), pyv = bl_vreg(py0), pxv = bl_vreg(px0), oyv = bl_vreg(oy0), oxv = bl_vreg(ox0), qbv = bl_vreg(quant_bits);
  for (int c = 0; c < C; ++c) {          // a gray source is blurred and filtered once, gets one draw and is written three times
    psf_footprint<KS>(sh, r0, nrows, x0, seg, Hr, Wr, [=](int y, int x) { return cd_load(im, y, x, c); });
    const int nch = bl_vreg((q.gray || C == 1) ? 0 : c), cv = bl_vreg(C == 1 ? -1 : c);
    rs_filter(sh.rs, load, [=](int k, int t, float v) {
      const size_t nv = (size_t)Pv * Pv, i = (size_t)(pyv + k) * Pv + (pxv + t);
      v = dg_finish(v, qv, oxv + t, oyv + k, nch, qbv);
      if (cv < 0) { lo[i] = v; lo[nv + i] = v; lo[2 * nv + i] = v; }
      else lo[cv * nv + i] = v;
    }, ny, nx, 0);
  }
}

}  // namespace

// the instantiation of a table side; ks is odd and in 1..21 here (srk_psf_ks_ok), anything else launches nothing
#define BL_FOR_KS(ks, X) \
  switch (ks) { X(1) X(3) X(5) X(7) X(9) X(11) X(13) X(15) X(17) X(19) X(21) default: break; }

int srk_launch_blur2d_f32(const float* x, const float* psf, float* out, int B, int C, int H, int W, int ks, hipStream_t stream) {
  SRK_REQUIRE(srk_psf_ks_ok(ks), SRK_E_SHAPE, "blur2d: ks must be odd and in 1..21 (got %d)", ks);
  const int tiles_y = cdiv(H, BL_TY), tiles_x = cdiv(W, BL_TX);
  const double blocks = (double)B * C * tiles_y * tiles_x;
  SRK_REQUIRE(blocks >= 1.0 && blocks <= 2147483647.0, SRK_E_SHAPE, "blur2d: %.0f tiles do not fit one grid (B=%d C=%d H=%d W=%d)", blocks, B, C,
              H, W);
#define BL_LAUNCH(N) \
  case N: hipLaunchKernelGGL(blur2d_kernel<N>, dim3((unsigned)blocks), dim3(256), 0, stream, x, psf, out, C, H, W, tiles_y, tiles_x); break;
  BL_FOR_KS(ks, BL_LAUNCH)
#undef BL_LAUNCH
  return srk_check_launch("blur2d_f32");
}

int srk_launch_crop_degrade_psf_u8(const unsigned char* pool, const long long* desc, const float* psf, int ks, float* lr_out, float* hr_out,
                                   int B, int P, int scale, int quant_bits, hipStream_t stream) {
  SRK_REQUIRE(srk_psf_ks_ok(ks), SRK_E_SHAPE, "crop_degrade_psf: ks must be odd and in 1..21 (got %d)", ks);
  // rs tables and staging + the 52 KB footprint + the table: above the default 64 KB limit.  One reservation state per instantiation
  static SrkLdsState reserved[BL_KMAX / 2 + 1];
  const void* fn = nullptr;
#define BL_FN(N) case N: fn = reinterpret_cast<const void*>(&crop_degrade_psf_u8_kernel<N>); break;
  BL_FOR_KS(ks, BL_FN)
#undef BL_FN
  if (const int rc = srk_reserve_lds_fn(fn, (int)sizeof(PsfShared), reserved[ks / 2], false, "crop_degrade_psf: cannot reserve %zu bytes of LDS",
                                        sizeof(PsfShared)))
    return rc;
  const int tiles_y = cdiv(P, CD_TOY), tiles_x = cdiv(P, RS_TOX);
#define BL_LAUNCH(N)                                                                                                                          \
  case N:                                                                                                                                     \
    hipLaunchKernelGGL(crop_degrade_psf_u8_kernel<N>, dim3(tiles_y * tiles_x, B), dim3(256), sizeof(PsfShared), stream, pool, desc, psf, lr_out, \
                       hr_out, P, scale, tiles_x, quant_bits);                                                                                \
    break;
  BL_FOR_KS(ks, BL_LAUNCH)
#undef BL_LAUNCH
  return srk_check_launch("crop_degrade_psf_u8");
}
