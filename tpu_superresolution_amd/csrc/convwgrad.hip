// All-taps weight gradient of a 3x3 / stride 1 / pad 1 conv on NHWC bf16 (gfx950, v_mfma_f32_16x16x32_bf16):
//
//   dW[n][tap][k] += sum_{b,y,x} Y[b][y][x][n] * X[b][y+dy][x+dx][k]      db[n] += sum Y[b][y][x][n]
//
// wgrad.hip treats the nine taps as nine independent GEMM tiles: every tap re-reads the whole Y tile and a
// shifted copy of the same X rows, and a workgroup gets 16-32 MFMAs per 24 KB it stages -- the kernel is bound
// by staging latency at a few percent of either roofline.  Here a workgroup owns 64 output channels x 64 input
// channels for ALL nine taps: per 64-pixel run of an image row it stages the Y rows once (8 KB) and the X halo
// (3 rows x 66 pixels, 25 KB) once, and issues 288 MFMAs on them (each wave: all four n-fragments x nine of
// the 36 (tap, k-fragment) column groups; 144 accumulator registers).  Operands are m-major in memory, so the
// fragments come from the transposing LDS read, with the same row padding as wgrad.hip.
//
// Three stagings of that tile, selected by the options conv_wgrad_taps / conv_wgrad_roll:
//   conv_wgrad_taps_kernel             register-staged, one run ahead (conv_wgrad_taps = 1)
//   conv_wgrad_taps_dma_staged_kernel  LDS-DMA ring of whole runs: dY + a fresh 3 x 66-pixel halo per run (conv_wgrad_roll = 0,
//                                      and every width the rolling window does not cover)
//   conv_wgrad_taps_dma_kernel         LDS-DMA with a rolling X-row window (default at W = 64 and W = 128): a run fetches its dY
//                                      and ONE new X row, 16 KB instead of 33.5 KB; loop per run and wave: 72 MFMA, 13 VALU,
//                                      52 LDS reads, 4 DMAs (the whole-run ring: 72 + 8, 306 of which 160 register-file copies,
//                                      52, 9).  cfg3: 125.0 -> 76.0 us per launch (profiles/conv_wgrad_roll_kernel_stats.md).
// All three sum in the same order (runs in order per split, ks -> q -> i inside a run).
#include <type_traits>

#include "wgrad.h"

#ifndef SRK_NT_TAPS
#define SRK_NT_TAPS 0
#endif

namespace {

constexpr int CT = 64;                 // pixels per chunk: one run inside an image row (needs W % 64 == 0)
constexpr int SP = 64 + 16;            // LDS row stride in elements: 32 B x odd -> conflict-free transposing reads
constexpr int HALO = CT + 2;           // pixels per halo row
constexpr int XROWS = 3 * HALO;
constexpr int YPIECES = CT * 8 / 256;                 // 16-byte pieces per thread
constexpr int XPIECES = (XROWS * 8 + 255) / 256;

template <bool SHUF>
__global__ __launch_bounds__(256) void conv_wgrad_taps_kernel(const WgradParams p, int ntiles, int chunks_per) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  bf16_t* Ys = reinterpret_cast<bf16_t*>(smem);      // [2][CT][SP]
  bf16_t* Xs = Ys + 2 * CT * SP;                     // [2][XROWS][SP]

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r16 = lane & 15, g = lane >> 4;
  // 1-D grid, (m-split, tile) with the tiles of one m-split contiguous on one XCD: they re-read the same rows
  const int logical = xcd_remap(blockIdx.x, gridDim.x);
  const int bsplit = logical / ntiles, btile = logical - bsplit * ntiles;
  const int ntn = p.N / 64;
  const int tn = btile % ntn, tk = btile / ntn;
  const int n0 = tn * 64, k0 = tk * 64;
  const int c_begin = bsplit * chunks_per;
  const int c_end = min(p.M / CT, c_begin + chunks_per);
  if (c_begin >= c_end) return;
  const int hw = p.H * p.W;

  uint4 ry[YPIECES], rx[XPIECES];
  auto load_stage = [&](int ch) {
    const int m0 = ch * CT;
    const int b = m0 / hw, rem = m0 - b * hw;
    const int y = rem / p.W, x0 = rem - y * p.W;
#pragma unroll
    for (int t = 0; t < YPIECES; ++t) {
      const int pid = tid + 256 * t;
      const int row = pid >> 3, c8 = pid & 7;
      if constexpr (SHUF) {
        // Y lives pixel-shuffled: channel n = (si*r + sj)*Cs + c of pixel (y, x) is stored at [r*y+si][r*x+sj][c]
        const int nn = n0 + c8 * 8;
        const int ij = nn / p.Cs, c = nn - ij * p.Cs;
        const int si = ij / p.r, sj = ij - si * p.r;
        ry[t] = *reinterpret_cast<const uint4*>(
            p.Y + (((long long)(b * p.H * p.r + y * p.r + si)) * (p.W * p.r) + (x0 + row) * p.r + sj) * p.Cs + c);
      } else {
        ry[t] = *reinterpret_cast<const uint4*>(p.Y + (long long)(m0 + row) * p.ldy + n0 + c8 * 8);
      }
    }
#pragma unroll
    for (int t = 0; t < XPIECES; ++t) {
      const int pid = tid + 256 * t;
      const int hr = pid >> 3, c8 = pid & 7;
      const int rr = hr / HALO, px = hr - rr * HALO;
      const int yy = y + rr - 1, xx = x0 + px - 1;
      uint4 v = make_uint4(0, 0, 0, 0);
      if (hr < XROWS && (unsigned)yy < (unsigned)p.H && (unsigned)xx < (unsigned)p.W)
        v = *reinterpret_cast<const uint4*>(p.X + ((long long)(b * p.H + yy) * p.W + xx) * p.ldx + k0 + c8 * 8);
      rx[t] = v;
    }
  };
  auto store_stage = [&](int buf) {
    bf16_t* ys = Ys + buf * CT * SP;
    bf16_t* xs = Xs + buf * XROWS * SP;
#pragma unroll
    for (int t = 0; t < YPIECES; ++t) {
      const int pid = tid + 256 * t;
      *reinterpret_cast<uint4*>(ys + (pid >> 3) * SP + (pid & 7) * 8) = ry[t];
    }
#pragma unroll
    for (int t = 0; t < XPIECES; ++t) {
      const int pid = tid + 256 * t;
      if (pid < XROWS * 8) *reinterpret_cast<uint4*>(xs + (pid >> 3) * SP + (pid & 7) * 8) = rx[t];
    }
  };

  f32x4_t acc[4][9], accb[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    accb[i] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int q = 0; q < 9; ++q) acc[i][q] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  }
  const bool do_bias = p.db != nullptr && tk == 0 && wave == 0;
  const bf16x8_t ones = bf16x8_t{0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80};
  // this wave's nine column groups: cg = 9 wave + q -> (tap = cg / 4, k-fragment = cg % 4)

  load_stage(c_begin);
  store_stage(0);
  __syncthreads();
  for (int ch = c_begin; ch < c_end; ++ch) {
    const int buf = (ch - c_begin) & 1;
    if (ch + 1 < c_end) load_stage(ch + 1);
    const bf16_t* ys = Ys + buf * CT * SP;
    const bf16_t* xs = Xs + buf * XROWS * SP;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      // k order inside a fragment: jj < 4 -> pixel 32ks + 4g + jj, jj >= 4 -> pixel 32ks + 16 + 4g + jj - 4 (same for Y and X)
      bf16x8_t yf[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const bf16x4_t lo = lds_tr_read(tr_addr(ys, SP, 32 * ks + 4 * g, 16 * i, lane));
        const bf16x4_t hi = lds_tr_read(tr_addr(ys, SP, 32 * ks + 16 + 4 * g, 16 * i, lane));
        yf[i] = bf16x8_t{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
      }
#pragma unroll
      for (int q = 0; q < 9; ++q) {
        const int cg = 9 * wave + q;
        const int tap = cg >> 2;
        const int xb = (tap / 3) * HALO + (tap % 3);        // halo row of pixel x0 shifted by this tap's (dy, dx)
        const bf16x4_t lo = lds_tr_read(tr_addr(xs, SP, xb + 32 * ks + 4 * g, 16 * (cg & 3), lane));
        const bf16x4_t hi = lds_tr_read(tr_addr(xs, SP, xb + 32 * ks + 16 + 4 * g, 16 * (cg & 3), lane));
        const bf16x8_t xf = bf16x8_t{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i][q] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(yf[i], xf, acc[i][q], 0, 0, 0);
      }
      if (do_bias) {
#pragma unroll
        for (int i = 0; i < 4; ++i) accb[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(yf[i], ones, accb[i], 0, 0, 0);
      }
    }
    if (ch + 1 < c_end) store_stage(buf ^ 1);
    __syncthreads();
  }

  // acc[i][q][e] = dW[n = n0 + 16i + 4g + e][tap][k = k0 + 16kf + r16]
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int n = n0 + 16 * i + 4 * g;
#pragma unroll
    for (int q = 0; q < 9; ++q) {
      const int cg = 9 * wave + q;
      const long long col = (long long)(cg >> 2) * p.K + k0 + 16 * (cg & 3) + r16;
#pragma unroll
      for (int e = 0; e < 4; ++e) atomicAdd(p.dW + (long long)(n + e) * p.ldw + col, acc[i][q][e]);
    }
    if (do_bias && r16 == 0) {
#pragma unroll
      for (int e = 0; e < 4; ++e) atomicAdd(p.db + n + e, accb[i][e]);
    }
  }
}

SrkOpt g_taps_enabled{OPT_TAPS_ENABLED, 1};

template <bool SHUF>
int launch_taps(const WgradParams& p, hipStream_t stream) {
  constexpr size_t lds = (size_t)2 * (CT + XROWS) * SP * sizeof(bf16_t);
  static SrkLdsState reserved;
  if (const int rc = srk_reserve_lds(&conv_wgrad_taps_kernel<SHUF>, lds, reserved, false, "conv wgrad: cannot reserve %zu bytes of LDS", lds)) return rc;
  const int tiles = (p.N / 64) * (p.K / 64);
  const int nchunks = p.M / CT;
  // one workgroup per CU (LDS-limited): ~256 workgroups; every m-split costs one pass of fp32 atomics over the tile
  int splits = 256 / tiles;
  if (splits < 1) splits = 1;
  if (splits > nchunks) splits = nchunks;
  const int chunks_per = cdiv(nchunks, splits);
  splits = cdiv(nchunks, chunks_per);
  srk_probe_pre(FAM_WGRAD_CONV, stream, p.flops, p.bytes);
  hipLaunchKernelGGL((conv_wgrad_taps_kernel<SHUF>), dim3(tiles * splits), dim3(256), lds, stream, p, tiles, chunks_per);
  srk_probe_post(FAM_WGRAD_CONV, stream);
  return srk_check_launch("conv wgrad (all taps)");
}

// ---- LDS-DMA ring variant of the all-taps kernel: whole runs (conv_wgrad_taps_dma_staged_kernel) -----------------------
// Same tile and MFMA schedule as conv_wgrad_taps_kernel, but the dY rows and the X halo of a 64-pixel run arrive by
// LDS-DMA into a 4-deep ring (33.5 KB per stage, three runs in flight) instead of one register-staged run: the
// register-staged loop was bound by its load latency (2.4 us per run for 0.5 us of MFMA work).  Out-of-image halo
// pixels are DMA'd from a zero page (the source address is per lane), rows are unpadded 128-byte pixel rows whose
// 32-byte column pairs are XOR-swizzled with (row >> 1) & 3 on the source address (conflict-free transposing reads for
// any 8 consecutive rows), no wave stores inside the loop (exact counted vmcnt), one raw barrier per run.
__device__ uint4 g_zero_page[8];     // 128 zero bytes: DMA source for out-of-image pixels

constexpr int TD_YROWS = CT, TD_STAGE_ROWS = CT + XROWS;       // 64 + 198 rows of 64 bf16
constexpr int TD_STAGE_BYTES = TD_STAGE_ROWS * 128;
constexpr int TD_RING = 4;
constexpr int TD_PIECES = TD_STAGE_ROWS * 8;                   // 16-byte pieces per stage (2096)
constexpr int TD_PPW = TD_PIECES / 4;                          // per wave (524)
constexpr int TD_NI = (TD_PPW + 63) / 64;                      // DMA instructions per wave per run (9)

__device__ __forceinline__ const bf16_t* tr_addr_swz64(const bf16_t* tile, int rbase, int c0, int lane) {
  const int ll = lane & 15;
  const int row = rbase + (ll >> 2);
  return tile + row * 64 + (((c0 >> 4) ^ ((row >> 1) & 3)) << 4) + ((ll & 3) << 2);
}

// accumulators -> the split's slab (or fp32 atomics into dW), bias sums -> db; shared by both stagings of the kernel
__device__ __forceinline__ void taps_store(const WgradParams& p, const f32x4_t (&acc)[4][9], const f32x4_t (&accb)[4], float* partial,
                                           int nsplit, int btile, int bsplit, int wave, int lane, int n0, int k0, bool do_bias) {
  const int r16 = lane & 15, g = lane >> 4;
  if (partial != nullptr) {
    // partial tile in accumulator order, summed over the splits by conv_wgrad_taps_reduce_kernel (see wgrad.hip)
    f32x4_t* slab = reinterpret_cast<f32x4_t*>(partial) + ((size_t)btile * nsplit + bsplit) * WS_SLAB_VEC + (size_t)wave * 36 * 64 + lane;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int q = 0; q < 9; ++q) slab[(i * 9 + q) * 64] = acc[i][q];
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int n = n0 + 16 * i + 4 * g;
    if (partial == nullptr) {
#pragma unroll
      for (int q = 0; q < 9; ++q) {
        const int cg = 9 * wave + q;
        const long long col = (long long)(cg >> 2) * p.K + k0 + 16 * (cg & 3) + r16;
#pragma unroll
        for (int e = 0; e < 4; ++e) atomicAdd(p.dW + (long long)(n + e) * p.ldw + col, acc[i][q][e]);
      }
    }
    if (do_bias && r16 == 0) {
#pragma unroll
      for (int e = 0; e < 4; ++e) atomicAdd(p.db + n + e, accb[i][e]);
    }
  }
}

// the per-run staging (conv_wgrad_roll = 0, and every width the rolling window below does not cover)
template <bool SHUF>
__device__ __forceinline__ void taps_dma_staged(const WgradParams& p, int ntiles, int chunks_per, float* partial, int nsplit,
                                                unsigned char* smem) {
  const unsigned ring_base = (unsigned)(size_t)smem;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r16 = lane & 15, g = lane >> 4;
  const int logical = xcd_remap(blockIdx.x, gridDim.x);
  const int bsplit = logical / ntiles, btile = logical - bsplit * ntiles;
  const int ntn = p.N / 64;
  const int tn = btile % ntn, tk = btile / ntn;
  const int n0 = tn * 64, k0 = tk * 64;
  const int c_begin = bsplit * chunks_per;
  const int c_end = min(p.M / CT, c_begin + chunks_per);
  if (c_begin >= c_end) return;
  const int hw = p.H * p.W;
  const bf16_t* zero = reinterpret_cast<const bf16_t*>(g_zero_page);

  // stage image: rows 0..63 = dY of the run's pixels, rows 64.. = X halo (3 rows x 66 pixels); this wave moves pieces
  // [wave * TD_PPW, (wave + 1) * TD_PPW).  Which piece a lane moves in DMA instruction i never changes, so everything
  // that depends on the lane only is computed once: the element offset relative to the run's first pixel and, for halo
  // pieces, (halo row, halo pixel) for the per-run bounds test.  Per run and instruction this leaves two compares, a
  // select and a 64-bit add (the address math otherwise costs more issue slots than the 72 MFMAs of the run).
  int loff[TD_NI];          // element offset of the piece relative to the run base (dY or X)
  int lrp[TD_NI];           // dY piece: -1; halo piece: (rr << 8) | px
#pragma unroll
  for (int i = 0; i < TD_NI; ++i) {
    const int qq = wave * TD_PPW + i * 64 + lane;
    const int row = qq >> 3, pos = qq & 7;
    const int c = (((pos >> 1) ^ ((row >> 1) & 3)) << 1) | (pos & 1);           // logical 16-byte piece of this LDS position
    if (row < TD_YROWS) {
      lrp[i] = -1;
      if constexpr (SHUF) {
        const int nn = n0 + c * 8;
        const int ij = nn / p.Cs, cc = nn - ij * p.Cs;
        const int si = ij / p.r, sj = ij - si * p.r;
        loff[i] = (si * (p.W * p.r) + row * p.r + sj) * p.Cs + cc;
      } else {
        loff[i] = row * p.ldy + n0 + c * 8;
      }
    } else {
      const int hr = row - TD_YROWS;
      const int rr = hr / HALO, px = hr - rr * HALO;
      lrp[i] = (rr << 8) | px;
      loff[i] = ((rr - 1) * p.W + (px - 1)) * p.ldx + k0 + c * 8;
    }
  }
  auto issue = [&](int ch) {
    const int m0 = ch * CT;
    const int b = m0 / hw, rem = m0 - b * hw;
    const int y = rem / p.W, x0 = rem - y * p.W;
    const bf16_t* ybase = SHUF ? p.Y + (((long long)(b * p.H * p.r + y * p.r)) * (p.W * p.r) + (long long)x0 * p.r) * p.Cs
                               : p.Y + (long long)m0 * p.ldy;
    const bf16_t* xbase = p.X + (long long)m0 * p.ldx;
    const unsigned dst = ring_base + (unsigned)(((ch - c_begin) % TD_RING) * TD_STAGE_BYTES);
#pragma unroll
    for (int i = 0; i < TD_NI; ++i) {
      if (i * 64 + lane < TD_PPW) {
        const bf16_t* src;
        if (lrp[i] < 0) {
          src = ybase + loff[i];
        } else {
          const int yy = y + (lrp[i] >> 8) - 1, xx = x0 + (lrp[i] & 255) - 1;
          src = ((unsigned)yy < (unsigned)p.H && (unsigned)xx < (unsigned)p.W) ? xbase + loff[i] : zero;
        }
        srk_glds16<SRK_NT_TAPS != 0>(src, __builtin_amdgcn_readfirstlane(dst + (wave * TD_PPW + i * 64) * 16));
      }
    }
  };

  f32x4_t acc[4][9], accb[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    accb[i] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int q = 0; q < 9; ++q) acc[i][q] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  }
  const bool do_bias = p.db != nullptr && tk == 0 && wave == 0;
  const bf16x8_t ones = bf16x8_t{0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80};

  const int nrun = c_end - c_begin;
  for (int s = 0; s < TD_RING - 1 && s < nrun; ++s) issue(c_begin + s);
  for (int it = 0; it < nrun; ++it) {
    // run `it` has landed once at most the (TD_RING - 2) runs issued after it are outstanding
    if (it + TD_RING - 2 < nrun) srk_wait_vmcnt<TD_NI*(TD_RING - 2)>(); else srk_wait_vmcnt<0>();
    srk_lds_barrier();
    if (it + TD_RING - 1 < nrun) issue(c_begin + it + TD_RING - 1);
    const bf16_t* ys = reinterpret_cast<const bf16_t*>(smem + (it % TD_RING) * TD_STAGE_BYTES);
    const bf16_t* xs = ys + TD_YROWS * 64;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      bf16x8_t yf[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const bf16x4_t lo = lds_tr_read(tr_addr_swz64(ys, 32 * ks + 4 * g, 16 * i, lane));
        const bf16x4_t hi = lds_tr_read(tr_addr_swz64(ys, 32 * ks + 16 + 4 * g, 16 * i, lane));
        yf[i] = bf16x8_t{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
      }
#pragma unroll
      for (int q = 0; q < 9; ++q) {
        const int cg = 9 * wave + q;
        const int tap = cg >> 2;
        const int xb = (tap / 3) * HALO + (tap % 3);
        // NOTE the swizzle is a function of the row inside the STAGE image (dY rows first), so the halo rows are offset
        const bf16x4_t lo = lds_tr_read(tr_addr_swz64(ys, TD_YROWS + xb + 32 * ks + 4 * g, 16 * (cg & 3), lane));
        const bf16x4_t hi = lds_tr_read(tr_addr_swz64(ys, TD_YROWS + xb + 32 * ks + 16 + 4 * g, 16 * (cg & 3), lane));
        const bf16x8_t xf = bf16x8_t{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i][q] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(yf[i], xf, acc[i][q], 0, 0, 0);
      }
      if (do_bias) {
#pragma unroll
        for (int i = 0; i < 4; ++i) accb[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(yf[i], ones, accb[i], 0, 0, 0);
      }
    }
    (void)xs;
  }

  taps_store(p, acc, accb, partial, nsplit, btile, bsplit, wave, lane, n0, k0, do_bias);
}

// ---- rolling X-row window (conv_wgrad_roll = 1; W = 64 and W = 128) ---------------------------------------------------------------
// Consecutive runs of a workgroup are consecutive image rows (W = 64) or the two halves of one (W = 128), so two of the three halo
// rows of a run were already staged for the run before it.  Here LDS holds
//   a dY ring     RL::NY stages of 64 rows x 128 B,
//   an X row ring RL::NR slots of one image row of the workgroup's 64 input channels: (W + 2) pixels x 128 B, pixel x at row x + 1;
//                 the two pad pixels are zeroed once and no DMA ever writes them,
//   a zero row    66 pixels.
// The rows G0 - 1, G0, G0 + 1, ... of the split (G = b H + y, clamped into the tensor: a clamped row only lands in a slot that
// no tap selects) are streamed in order, in units of 64 pixels (2 DMA instructions per wave); group k = {dY of run k, unit k + PRO}
// is issued RL::A runs ahead: four full DMA instructions per wave and run, 16 KB instead of 33.5 KB.  The three X rows of a run
// are three slots; for a tap whose row lies outside the image the base is the zero row -- a scalar select per run, no per-lane
// bounds test and no zero page.  The swizzle is the same function of the row inside the slot (stage) on the DMA source side and on
// the read side, so the per-lane read offsets (one per n-fragment, one per (tap, k-fragment) group) are loop-invariant: a read is
// slot base (scalar) + lane offset + immediate.  Same run order, same MFMA order ks -> q -> i as the per-run staging: at W = 64
// and equal chunks_per the two give the same bits.
template <int RPR>
struct RL {
  static constexpr int A = RPR == 1 ? 4 : 3;                    // runs in flight
  static constexpr int PRO = 3 * RPR - 1;                       // units ahead of group 0: run `it` needs the units <= it + PRO
  static constexpr int NY = A + 1;
  static constexpr int NR = (A + PRO + RPR - 1) / RPR + 1;      // the unit issued in run `it` never lands in a row of a run >= it
  static constexpr int ROWB = (RPR * CT + 2) * 128;
  static constexpr int X_OFF = NY * CT * 128, Z_OFF = X_OFF + NR * ROWB, LDS = Z_OFF + HALO * 128;
};

// Two LDS-DMAs of one wave (8 + 8 rows of 128 B) with wave-uniform 64-bit bases and one per-lane 32-bit byte offset: no 64-bit
// vector add per instruction; M0 is written in the statement that reads it and restored once.
template <bool NT = false>
__device__ __forceinline__ void srk_glds16_s2(const void* sb0, const void* sb1, unsigned voff, unsigned dst0, unsigned dst1) {
  unsigned keep;
  if constexpr (NT)
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %4 nt\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\t"
                 "global_load_lds_dwordx4 %1, %5 nt\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(voff), "s"(dst0), "s"(dst1), "s"(sb0), "s"(sb1)
                 : "memory");
  else
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %4\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\t"
                 "global_load_lds_dwordx4 %1, %5\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(voff), "s"(dst0), "s"(dst1), "s"(sb0), "s"(sb1)
                 : "memory");
}

__device__ __forceinline__ bf16x4_t lds_tr_read_at(unsigned addr) {
  typedef __attribute__((ext_vector_type(4))) short s4;
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((s4 __attribute__((address_space(3)))*)(addr));
}

template <bool SHUF, int RPR>
__device__ __forceinline__ void taps_dma_roll(const WgradParams& p, int ntiles, int chunks_per, float* partial, int nsplit,
                                              unsigned char* smem) {
  using C = RL<RPR>;
  const unsigned lds0 = (unsigned)(size_t)smem;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int logical = xcd_remap(blockIdx.x, gridDim.x);
  const int bsplit = logical / ntiles, btile = logical - bsplit * ntiles;
  const int ntn = p.N / 64;
  const int tn = btile % ntn, tk = btile / ntn;
  const int n0 = tn * 64, k0 = tk * 64;
  const int c_begin = bsplit * chunks_per;                       // whole image rows: chunks_per % RPR == 0
  const int c_end = min(p.M / CT, c_begin + chunks_per);
  if (c_begin >= c_end) return;
  const int nrun = c_end - c_begin;
  const int BH = p.B * p.H;
  const int G0 = c_begin / RPR;                                  // global row b H + y of the first run
  int y = G0 % p.H;

  // the zero row and the pad pixels of every slot (plain stores, complete at the first barrier of the loop)
  for (int i = tid; i < HALO * 8; i += 256) *reinterpret_cast<uint4*>(smem + C::Z_OFF + i * 16) = make_uint4(0, 0, 0, 0);
  for (int i = tid; i < C::NR * 16; i += 256)
    *reinterpret_cast<uint4*>(smem + C::X_OFF + (i >> 4) * C::ROWB + ((i >> 3) & 1) * (RPR * CT + 1) * 128 + (i & 7) * 16) =
        make_uint4(0, 0, 0, 0);

  // DMA: a wave instruction fills 8 consecutive 128-byte rows; lane -> (row l8 of the 8, 16-byte position pos), which holds the
  // logical piece pos ^ swizzle(row); the rows start at a multiple of 8 (dY) or at 8 j + 1 (X, behind the pad pixel)
  const int l8 = lane >> 3, pos = lane & 7;
  const int cy = (((pos >> 1) ^ ((l8 >> 1) & 3)) << 1) | (pos & 1);
  const int cx = (((pos >> 1) ^ (((l8 + 1) >> 1) & 3)) << 1) | (pos & 1);
  unsigned voffy;
  int ypix;                                                      // elements of Y between two pixels of an image row
  if constexpr (SHUF) {
    // Y lives pixel-shuffled: channel n = (si*r + sj)*Cs + c of pixel (y, x) is stored at [r*y+si][r*x+sj][c]
    const int nn = n0 + cy * 8;
    const int ij = nn / p.Cs, cc = nn - ij * p.Cs;
    const int si = ij / p.r, sj = ij - si * p.r;
    voffy = 2u * (unsigned)((si * (p.W * p.r) + l8 * p.r + sj) * p.Cs + cc);
    ypix = p.r * p.Cs;
  } else {
    voffy = 2u * (unsigned)(l8 * p.ldy + n0 + cy * 8);
    ypix = p.ldy;
  }
  const unsigned voffx = 2u * (unsigned)(l8 * p.ldx + k0 + cx * 8);

  // The two streams advance by increments (all wave-uniform): dY run by run, X in units of 64 pixels, row by row.  The row index
  // of the X stream is clamped into [0, B H): the pointer stands still outside.
  const long long y8 = (long long)8 * ypix * 2, x8 = (long long)8 * p.ldx * 2;            // bytes between the two DMAs of a pair
  const long long ystep_in = (long long)CT * ypix * 2;                                     // next run of the same image row
  const long long ystep_row = SHUF ? ((long long)p.r * (p.W * p.r) - (long long)(RPR - 1) * CT * p.r) * p.Cs * 2 : ystep_in;
  const long long xstep_in = (long long)CT * p.ldx * 2, xstep_row = (long long)p.W * p.ldx * 2;
  const unsigned ydst0 = lds0 + (unsigned)(wave * 2048), ydst_end = ydst0 + C::NY * (CT * 128);
  const unsigned xdst0 = lds0 + (unsigned)(C::X_OFF + (1 + wave * 16) * 128), xdst_end = xdst0 + C::NR * C::ROWB;
  const char* ysrc = reinterpret_cast<const char*>(
      p.Y + (SHUF ? (long long)G0 * p.r * (p.W * p.r) * p.Cs : (long long)c_begin * CT * p.ldy) + (long long)(wave * 16) * ypix);
  int xj = G0 - 1;
  const char* xsrc = reinterpret_cast<const char*>(p.X + ((long long)max(xj, 0) * p.W + wave * 16) * p.ldx);
  unsigned ydst = ydst0, xdst = xdst0;
  int yh = 0, xh = 0;
  auto issue_y = [&]() {
    srk_glds16_s2<SRK_NT_TAPS != 0>(ysrc, ysrc + y8, voffy, ydst, ydst + 1024);
    ydst = ydst + CT * 128 == ydst_end ? ydst0 : ydst + CT * 128;
    if (RPR == 1 || ++yh == RPR) {
      yh = 0;
      ysrc += ystep_row;
    } else {
      ysrc += ystep_in;
    }
  };
  auto issue_x = [&]() {
    const char* s = RPR == 1 ? xsrc : xsrc + xh * xstep_in;
    const unsigned d = RPR == 1 ? xdst : xdst + (unsigned)(xh * (CT * 128));
    srk_glds16_s2<SRK_NT_TAPS != 0>(s, s + x8, voffx, d, d + 1024);
    if (RPR == 1 || ++xh == RPR) {
      xh = 0;
      xdst = xdst + C::ROWB == xdst_end ? xdst0 : xdst + C::ROWB;
      ++xj;
      if (xj > 0 && xj < BH) xsrc += xstep_row;
    }
  };

  // reads: lane -> row 4 g + (ll >> 2) of a 16-row group, 8 bytes at (ll & 3) of the 32-byte column (fragment ^ swizzle(row)).
  // A wave's nine (tap, k-fragment) groups cover at most two values of dy: the first nsel groups have dy = dA, the others dB.
  const int g = lane >> 4, ll = lane & 15;
  const int lrow = 4 * g + (ll >> 2);
  unsigned yoff[4], xoff[9];
#pragma unroll
  for (int i = 0; i < 4; ++i) yoff[i] = (unsigned)(lrow * 128 + ((i ^ ((lrow >> 1) & 3)) << 5) + ((ll & 3) << 3));
  const int dA = ((9 * wave) >> 2) / 3, dB = ((9 * wave + 8) >> 2) / 3;
  int nsel = 0;
#pragma unroll
  for (int q = 0; q < 9; ++q) {
    const int cg = 9 * wave + q;
    const int tap = cg >> 2, kf = cg & 3;
    const int px = tap % 3 + lrow;                               // pixel x0 - 1 + dx + lrow sits at row dx + lrow of the slot
    nsel += tap / 3 == dA ? 1 : 0;
    xoff[q] = (unsigned)(px * 128 + ((kf ^ ((px >> 1) & 3)) << 5) + ((ll & 3) << 3));
  }

  f32x4_t acc[4][9], accb[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    accb[i] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int q = 0; q < 9; ++q) acc[i][q] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  }
  const bool do_bias = p.db != nullptr && tk == 0 && wave == 0;
  const bf16x8_t ones = bf16x8_t{0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80};

  // group k = {dY of run k, X unit k + PRO}: run `it` needs the groups <= it (the rows r .. r + 2 of its image row r end with
  // unit RPR (r + 2) + RPR - 1 <= it + PRO)
  for (int uu = 0; uu < C::PRO; ++uu) issue_x();
  for (int k = 0; k < C::A && k < nrun; ++k) {
    issue_y();
    issue_x();
  }
  const unsigned xbeg = lds0 + C::X_OFF, xend = xbeg + C::NR * C::ROWB, zrow = lds0 + C::Z_OFF;
  unsigned ys = lds0, xs0 = xbeg, xs1 = xbeg + C::ROWB, xs2 = xbeg + 2 * C::ROWB;     // dY stage of the run; slots of rows r, r + 1, r + 2
  int u = 0;                                                                          // run inside the image row
  // The bias sums ride on wave 0 of the k-tile-0 workgroups only: that wave runs its own copy of the loop, the others carry neither
  // the four extra MFMAs per k-step nor their accumulators (the branch is wave-uniform; the barrier counts arrivals).
  auto run_loop = [&](auto bias) {
  constexpr bool BIAS = decltype(bias)::value;
  for (int it = 0; it < nrun; ++it) {
    // group `it` has landed once at most the (A - 1) groups issued after it are outstanding
    if (it + C::A - 1 < nrun) srk_wait_vmcnt<4 * (C::A - 1)>(); else srk_wait_vmcnt<0>();
    srk_lds_barrier();
    if (it + C::A < nrun) {
      issue_y();
      issue_x();
    }
    const unsigned xu = (unsigned)(u * (CT * 128));
    const unsigned rb0 = y > 0 ? xs0 + xu : zrow;
    const unsigned rb1 = xs1 + xu;
    const unsigned rb2 = y + 1 < p.H ? xs2 + xu : zrow;
    const unsigned rbA = dA == 0 ? rb0 : (dA == 1 ? rb1 : rb2);
    const unsigned rbB = dB == 0 ? rb0 : (dB == 1 ? rb1 : rb2);
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      bf16x8_t yf[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const bf16x4_t lo = lds_tr_read_at(ys + yoff[i] + (32 * ks) * 128);
        const bf16x4_t hi = lds_tr_read_at(ys + yoff[i] + (32 * ks + 16) * 128);
        yf[i] = bf16x8_t{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
      }
#pragma unroll
      for (int q = 0; q < 9; ++q) {
        const unsigned rb = q < nsel ? rbA : rbB;
        const bf16x4_t lo = lds_tr_read_at(rb + xoff[q] + (32 * ks) * 128);
        const bf16x4_t hi = lds_tr_read_at(rb + xoff[q] + (32 * ks + 16) * 128);
        const bf16x8_t xf = bf16x8_t{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i][q] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(yf[i], xf, acc[i][q], 0, 0, 0);
      }
      if constexpr (BIAS) {
#pragma unroll
        for (int i = 0; i < 4; ++i) accb[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(yf[i], ones, accb[i], 0, 0, 0);
      }
    }
    ys = ys + CT * 128 == xbeg ? lds0 : ys + CT * 128;
    if (RPR == 1 || ++u == RPR) {
      u = 0;
      xs0 = xs1;
      xs1 = xs2;
      xs2 = xs2 + C::ROWB == xend ? xbeg : xs2 + C::ROWB;
      y = y + 1 == p.H ? 0 : y + 1;
    }
  }
  };
  if (do_bias) run_loop(std::true_type{});
  else run_loop(std::false_type{});

  taps_store(p, acc, accb, partial, nsplit, btile, bsplit, wave, lane, n0, k0, do_bias);
}

// The rolling window keeps the kernel's name; the per-run staging lives in a kernel of its own, so that each is register-allocated
// alone: (256, 2) caps the rolling kernel at 256 registers, where the MFMAs accumulate in place (with the 512-register budget of
// one wave per SIMD the scheduler hoists LDS reads until the accumulators are copied to and from the upper half of the file).
// rpr: 64-pixel runs per image row (1 or 2)
template <bool SHUF>
__global__ __launch_bounds__(256, 2) void conv_wgrad_taps_dma_kernel(const WgradParams p, int ntiles, int chunks_per, float* partial,
                                                                     int nsplit, int rpr) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  if (rpr == 1) taps_dma_roll<SHUF, 1>(p, ntiles, chunks_per, partial, nsplit, smem);
  else taps_dma_roll<SHUF, 2>(p, ntiles, chunks_per, partial, nsplit, smem);
}

template <bool SHUF>
__global__ __launch_bounds__(256) void conv_wgrad_taps_dma_staged_kernel(const WgradParams p, int ntiles, int chunks_per, float* partial,
                                                                         int nsplit) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  taps_dma_staged<SHUF>(p, ntiles, chunks_per, partial, nsplit, smem);
}

// sum of the nsplit partial tiles of conv_wgrad_taps_dma_kernel, added to dW (36 workgroups per 64 x 64 x 9-tap tile)
__global__ __launch_bounds__(256) void conv_wgrad_taps_reduce_kernel(const WgradParams p, const float* __restrict__ partial, int nsplit) {
  const int btile = blockIdx.x / 36;
  const int v = (blockIdx.x - btile * 36) * 256 + threadIdx.x;
  const int ntn = p.N / 64;
  const int tn = btile % ntn, tk = btile / ntn;
  const f32x4_t* src = reinterpret_cast<const f32x4_t*>(partial) + (size_t)btile * nsplit * WS_SLAB_VEC + v;
  f32x4_t sum = f32x4_t{0.f, 0.f, 0.f, 0.f};
  int s = 0;
  for (; s + 8 <= nsplit; s += 8) {
    f32x4_t t[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) t[u] = src[(size_t)(s + u) * WS_SLAB_VEC];
#pragma unroll
    for (int u = 0; u < 8; ++u) sum += t[u];
  }
  for (; s < nsplit; ++s) sum += src[(size_t)s * WS_SLAB_VEC];
  const int lane = v & 63, t = v >> 6;
  const int q = t % 9, i = (t / 9) % 4, wave = t / 36;
  const int r16 = lane & 15, g = lane >> 4;
  const int n = tn * 64 + 16 * i + 4 * g;
  const int cg = 9 * wave + q;
  const long long col = (long long)(cg >> 2) * p.K + tk * 64 + 16 * (cg & 3) + r16;
#pragma unroll
  for (int e = 0; e < 4; ++e) atomicAdd(p.dW + (long long)(n + e) * p.ldw + col, sum[e]);
}

SrkOpt g_taps_dma{OPT_TAPS_DMA, 1};
SrkOpt g_taps_roll{OPT_TAPS_ROLL, 1};

template <bool SHUF>
int launch_taps_dma(const WgradParams& p, hipStream_t stream) {
  constexpr int lds_staged = TD_RING * TD_STAGE_BYTES;
  constexpr int lds_roll = RL<2>::LDS > RL<1>::LDS ? RL<2>::LDS : RL<1>::LDS;
  static_assert(lds_roll <= 160 * 1024 && lds_staged <= 160 * 1024, "LDS budget");
  // rolling X-row window: one or two runs per image row; the M-splits are whole image rows (at W = 64 a run IS a row: same splits)
  const int rpr = g_taps_roll && (p.W == CT || p.W == 2 * CT) && p.M % p.W == 0 ? p.W / CT : 0;
  static SrkLdsState reserved[2];                       // [staged, rolling]: the kernel this launch runs
  constexpr const char* err = "conv wgrad (dma): cannot reserve %d bytes of LDS";
  constexpr int lds_max = lds_roll > lds_staged ? lds_roll : lds_staged;
  if (const int rc = rpr ? srk_reserve_lds(&conv_wgrad_taps_dma_kernel<SHUF>, lds_roll, reserved[1], false, err, lds_max)
                         : srk_reserve_lds(&conv_wgrad_taps_dma_staged_kernel<SHUF>, lds_staged, reserved[0], false, err, lds_max))
    return rc;
  const int lds = rpr == 1 ? RL<1>::LDS : (rpr == 2 ? RL<2>::LDS : lds_staged);
  const int unit = rpr ? rpr : 1;
  const int tiles = (p.N / 64) * (p.K / 64);
  const int nchunks = p.M / CT / unit;                  // rows (rolling) or runs
  int splits = 256 / tiles;
  if (splits < 1) splits = 1;
  if (splits > nchunks) splits = nchunks;
  const int chunks_per = cdiv(nchunks, splits);
  splits = cdiv(nchunks, chunks_per);
  float* partial =
      srk_wgrad_partials_enabled() && splits > 1 ? srk_wgrad_scratch(stream, (size_t)tiles * splits * WS_SLAB_VEC * 16) : nullptr;
  srk_probe_pre(FAM_WGRAD_CONV, stream, p.flops, p.bytes);
  if (rpr)
    hipLaunchKernelGGL((conv_wgrad_taps_dma_kernel<SHUF>), dim3(tiles * splits), dim3(256), lds, stream, p, tiles, chunks_per * unit,
                       partial, splits, rpr);
  else
    hipLaunchKernelGGL((conv_wgrad_taps_dma_staged_kernel<SHUF>), dim3(tiles * splits), dim3(256), lds, stream, p, tiles, chunks_per,
                       partial, splits);
  if (partial) hipLaunchKernelGGL(conv_wgrad_taps_reduce_kernel, dim3(tiles * 36), dim3(256), 0, stream, p, partial, splits);
  srk_probe_post(FAM_WGRAD_CONV, stream);
  return srk_check_launch("conv wgrad (all taps, dma)");
}

__device__ __forceinline__ void split_bf16x8(const float (&v)[8], bf16x8_t& hi, bf16x8_t& lo) {
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const bf16_t h = f2bf(v[i]);
    hi[i] = (short)h;
    lo[i] = (short)f2bf(v[i] - bf2f(h));
  }
}

// ---- image-head kernel with the rolling row window (conv_wgrad_roll = 1) -------------------------------------------------------------
// Same walk (down a 64-pixel column, consecutive chunks), same MFMAs in the same order as the staged kernel below, but nothing is staged
// through registers: the X rows arrive by LDS-DMA in a ring of SR::NR slots, one new row of 66 pixels per run, SR::A runs ahead, and the
// fp32 dY of a run (1 KB at COP = 4) arrives by LDS-DMA as it lies; every wave splits its dY fragment into bf16 hi + lo in registers
// (the same two roundings as the staged kernel), so a run has one barrier and no LDS stores (cfg3: 223.9 -> 198.8 us; the run loop
// was not this kernel's limit).  Slot layout: rows 0..63 = pixels
// x0..x0+63, row 64 = pixel x0+64, row 65 = pixel x0-1 (the two halo pixels are one 256-byte DMA; outside the image they come from the
// zero page); 128-byte rows with the 32-byte column pairs swizzled by (row >> 1) & 3, on the DMA source side and on the read side.
template <int COP>
struct SR {
  static constexpr int A = 3, NY = A + 1, NR = A + 3;
  static constexpr int GYB = CT * COP * 4;                     // bytes of a dY stage
  static constexpr int ROWB = HALO * 128;
  static constexpr int X_OFF = NY * GYB, Z_OFF = X_OFF + NR * ROWB, LDS = Z_OFF + ROWB;
};

template <bool NT = false>
__device__ __forceinline__ void srk_glds16_s1(const void* sb, unsigned voff, unsigned dst) {
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %3\n\ts_mov_b32 m0, %0"
               : "=&s"(keep)
               : "v"(voff), "s"(dst), "s"(sb)
               : "memory");
}

__device__ __forceinline__ float lds_read_f32(unsigned addr) {
  return *reinterpret_cast<const float __attribute__((address_space(3)))*>(addr);
}

template <int COP>
__global__ __launch_bounds__(256, 2) void smallconv_wgrad_mfma_kernel(const bf16_t* __restrict__ x, const float* __restrict__ gy,
                                                                      float* __restrict__ dW, float* __restrict__ db, int B, int H, int W,
                                                                      int Cin, int CinP, int Co, int ntiles, int chunks_per) {
  using C = SR<COP>;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const unsigned lds0 = (unsigned)(size_t)smem;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int logical = xcd_remap(blockIdx.x, gridDim.x);
  const int bsplit = logical / ntiles, tk = logical - bsplit * ntiles;
  const int k0 = tk * 64;
  const int NCH = (int)(((long long)B * H * W) / CT);
  const int c_begin = bsplit * chunks_per;
  const int c_end = min(NCH, c_begin + chunks_per);
  if (c_begin >= c_end) return;
  const int nrun = c_end - c_begin;
  const int nxb = W / CT;
  for (int i = tid; i < HALO * 8; i += 256) *reinterpret_cast<uint4*>(smem + C::Z_OFF + i * 16) = make_uint4(0, 0, 0, 0);

  // chunk -> (image, column block, row): consecutive chunks walk DOWN a CT-pixel column.  A cursor is (row, column block) plus a
  // byte pointer to the chunk's first pixel; `step` moves it to the next chunk.
  auto locate = [&](int ch, int& cy, int& cxb) -> long long {
    const int b = ch / (H * nxb), r = ch - b * (H * nxb);
    cxb = r / H;
    cy = r - cxb * H;
    return ((long long)(b * H + cy)) * W + cxb * CT;             // pixel index
  };
  auto step = [&](int& cy, int& cxb, const char*& ptr, long long ebytes) {
    if (++cy == H) {
      cy = 0;
      if (++cxb == nxb) {
        cxb = 0;
        ptr += CT * ebytes;                                      // last column of an image -> first column of the next
      } else {
        ptr += ((long long)CT - (long long)(H - 1) * W) * ebytes;
      }
    } else {
      ptr += (long long)W * ebytes;
    }
  };
  const long long xe = (long long)CinP * 2, ge = (long long)COP * 4;          // bytes per pixel
  int xj = c_begin - 1, xy, xxb, gyy, gxb, y;
  const char* xptr = reinterpret_cast<const char*>(x + k0) + locate(max(xj, 0), xy, xxb) * xe;
  const char* gptr = reinterpret_cast<const char*>(gy) + locate(c_begin, gyy, gxb) * ge;
  y = gyy;
  const char* zero = reinterpret_cast<const char*>(g_zero_page);

  constexpr int LA = CT * COP / 16;                              // lanes of a wave that move dY (16 or 64 pieces of 16 B)
  const int l8 = lane >> 3, pos = lane & 7;
  const unsigned voffx = 2u * (unsigned)(l8 * CinP + ((((pos >> 1) ^ ((l8 >> 1) & 3)) << 1) | (pos & 1)) * 8);
  const unsigned voffh = (unsigned)(((wave & 1) * 4 + (lane & 3)) * 16);       // rows 64 / 65: swizzle 0
  const unsigned voffg = (unsigned)((lane & (LA - 1)) * 16);
  const unsigned gdst0 = lds0 + (unsigned)(wave * LA * 16), gdst_end = gdst0 + C::NY * C::GYB;
  const unsigned xdst0 = lds0 + C::X_OFF, xdst_end = xdst0 + C::NR * C::ROWB;
  unsigned gdst = gdst0, xdst = xdst0;
  auto issue_y = [&]() {
    if (LA == 64 || lane < LA) srk_glds16_s1(gptr + wave * LA * 16, voffg, gdst);
    gdst = gdst + C::GYB == gdst_end ? gdst0 : gdst + C::GYB;
    step(gyy, gxb, gptr, ge);
  };
  auto issue_x = [&]() {
    const char* s = xptr + (long long)(wave * 16) * xe;
    const unsigned d = xdst + (unsigned)(wave * 2048);
    srk_glds16_s2(s, s + 8 * xe, voffx, d, d + 1024);
    const bool ok = wave < 2 ? xxb + 1 < nxb : xxb > 0;          // waves 0, 1: pixel x0 + 64 (row 64); waves 2, 3: pixel x0 - 1 (row 65)
    const char* hb = ok ? (wave < 2 ? xptr + CT * xe : xptr - xe) : zero;
    if (lane < 4) srk_glds16_s1(hb, voffh, xdst + (unsigned)(CT * 128 + wave * 64));
    xdst = xdst + C::ROWB == xdst_end ? xdst0 : xdst + C::ROWB;
    ++xj;
    if (xj > 0 && xj < NCH) step(xy, xxb, xptr, xe);
  };

  const int g = lane >> 4, ll = lane & 15;
  const int lrow = 4 * g + (ll >> 2);
  const unsigned goff = (unsigned)((4 * g) * COP * 4 + (ll < COP ? ll : 0) * 4);
  unsigned xoff0[9];                                             // reads of rows lrow + dx - 1 (row -1 is the slot's row 65)
  int xoff[9];                                                   // the same rows + 16 m, m = 1..3, relative to the slot (>= -128)
  const int dA = ((9 * wave) >> 2) / 3, dB = ((9 * wave + 8) >> 2) / 3;
  int nsel = 0;
#pragma unroll
  for (int q = 0; q < 9; ++q) {
    const int cg = 9 * wave + q;
    const int tap = cg >> 2, kf = cg & 3;
    const int pr = lrow + tap % 3 - 1;
    const int p0 = pr < 0 ? HALO - 1 : pr, p1 = pr + 16;
    nsel += tap / 3 == dA ? 1 : 0;
    xoff0[q] = (unsigned)(p0 * 128 + ((kf ^ ((p0 >> 1) & 3)) << 5) + ((ll & 3) << 3));
    xoff[q] = p1 * 128 + ((kf ^ ((p1 >> 1) & 3)) << 5) + ((ll & 3) << 3) - 16 * 128;
  }

  f32x4_t acc[9], accb = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int q = 0; q < 9; ++q) acc[q] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  const bool do_bias = db != nullptr && tk == 0 && wave == 0;
  const bf16x8_t ones = bf16x8_t{0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80};

  // group k = {dY of run k, X row k + 2}: four DMA instructions per wave; run `it` needs the groups <= it
  issue_x();
  issue_x();
  for (int k = 0; k < C::A && k < nrun; ++k) {
    issue_y();
    issue_x();
  }
  const unsigned zrow = lds0 + C::Z_OFF;
  unsigned gs = lds0, xs0 = xdst0, xs1 = xdst0 + C::ROWB, xs2 = xdst0 + 2 * C::ROWB;
  auto run_loop = [&](auto bias) {
  constexpr bool BIAS = decltype(bias)::value;
  for (int it = 0; it < nrun; ++it) {
    if (it + C::A - 1 < nrun) srk_wait_vmcnt<4 * (C::A - 1)>(); else srk_wait_vmcnt<0>();
    srk_lds_barrier();
    if (it + C::A < nrun) {
      issue_y();
      issue_x();
    }
    const unsigned rb0 = y > 0 ? xs0 : zrow;
    const unsigned rb2 = y + 1 < H ? xs2 : zrow;
    const unsigned rbA = dA == 0 ? rb0 : (dA == 1 ? xs1 : rb2);
    const unsigned rbB = dB == 0 ? rb0 : (dB == 1 ? xs1 : rb2);
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      // k order inside a fragment: jj < 4 -> pixel 32ks + 4g + jj, jj >= 4 -> pixel 32ks + 16 + 4g + jj - 4 (same for dY and X)
      float v[8];
#pragma unroll
      for (int jj = 0; jj < 8; ++jj) {
        const float t = lds_read_f32(gs + goff + (unsigned)((32 * ks + 16 * (jj >> 2) + (jj & 3)) * COP * 4));
        v[jj] = ll < COP ? t : 0.f;
      }
      bf16x8_t yfh, yfl;
      split_bf16x8(v, yfh, yfl);
#pragma unroll
      for (int q = 0; q < 9; ++q) {
        const unsigned rb = q < nsel ? rbA : rbB;
        const bf16x4_t lo = lds_tr_read_at(ks == 0 ? rb + xoff0[q] : rb + (unsigned)xoff[q] + 32 * 128);
        const bf16x4_t hi = lds_tr_read_at(rb + (unsigned)xoff[q] + (32 * ks + 16) * 128);
        const bf16x8_t xf = bf16x8_t{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        acc[q] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(yfh, xf, acc[q], 0, 0, 0);
        acc[q] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(yfl, xf, acc[q], 0, 0, 0);
      }
      if constexpr (BIAS) {
        accb = __builtin_amdgcn_mfma_f32_16x16x32_bf16(yfh, ones, accb, 0, 0, 0);
        accb = __builtin_amdgcn_mfma_f32_16x16x32_bf16(yfl, ones, accb, 0, 0, 0);
      }
    }
    gs = gs + C::GYB == lds0 + C::X_OFF ? lds0 : gs + C::GYB;
    xs0 = xs1;
    xs1 = xs2;
    xs2 = xs2 + C::ROWB == xdst_end ? xdst0 : xs2 + C::ROWB;
    y = y + 1 == H ? 0 : y + 1;
  }
  };
  if (do_bias) run_loop(std::true_type{});
  else run_loop(std::false_type{});

  // acc[q][e] = dW[n = 4g + e][k = k0 + 16 kf + r16][tap]   (state_dict layout [Cout][Cin][3][3])
#pragma unroll
  for (int q = 0; q < 9; ++q) {
    const int cg = 9 * wave + q;
    const int tap = cg >> 2, k = k0 + 16 * (cg & 3) + ll;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int n = 4 * g + e;
      if (n < Co && k < Cin) atomicAdd(dW + ((long long)(n * Cin) + k) * 9 + tap, acc[q][e]);
    }
  }
  if (do_bias && ll == 0) {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (4 * g + e < Co) atomicAdd(db + 4 * g + e, accb[e]);
  }
}

// ---- image-head variant, staged through registers (conv_wgrad_roll = 0): Cout <= 16, dY in fp32 ------------------------------------------------------------------
// Weight gradient of the convs that produce the image (conv_last 64 -> 3 at HR resolution, UpsampleOneStep): same
// all-taps structure with ONE 16-row n-fragment.  dY arrives as fp32 [pixels][COP] (the L1-loss gradient) and is split
// into bf16 hi + lo on the way into LDS (two MFMAs per fragment pair, ~2^-17 relative), so this path keeps fp32-grade
// precision while the 2 M-pixel reduction runs on the matrix cores instead of the VALU (0.9 ms -> see profiles/).
template <int COP>
__global__ __launch_bounds__(256) void smallconv_wgrad_mfma_staged_kernel(const bf16_t* __restrict__ x, const float* __restrict__ gy,
                                                                   float* __restrict__ dW, float* __restrict__ db, int B, int H, int W,
                                                                   int Cin, int CinP, int Co, int ntiles, int chunks_per) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  bf16_t* Yh = reinterpret_cast<bf16_t*>(smem);      // [2][CT][16]
  bf16_t* Yl = Yh + 2 * CT * 16;                     // [2][CT][16]
  bf16_t* Xs = Yl + 2 * CT * 16;                     // [2][XROWS][SP]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r16 = lane & 15, g = lane >> 4;
  const int logical = xcd_remap(blockIdx.x, gridDim.x);
  const int bsplit = logical / ntiles, tk = logical - bsplit * ntiles;
  const int k0 = tk * 64;
  const int M = B * H * W;
  const int c_begin = bsplit * chunks_per;
  const int c_end = min(M / CT, c_begin + chunks_per);
  if (c_begin >= c_end) return;
  const int hw = H * W;
  for (int i = tid; i < 2 * 2 * CT * 16 / 2; i += 256) reinterpret_cast<unsigned*>(Yh)[i] = 0u;   // columns >= COP stay zero

  constexpr int YP = CT * COP / 4;          // float4 pieces of dY per chunk (64 or 256)
  float4 ry = make_float4(0.f, 0.f, 0.f, 0.f);
  uint4 rx[XPIECES];
  // chunk -> (image, column block, row): consecutive chunks of a workgroup walk DOWN a CT-pixel column, so two of the three
  // halo rows of a chunk were read by the previous one (a row-major walk re-read them W / CT chunks later, after they had left
  // the L2: 0.79 GB of fetches per launch for a 268 MB input)
  const int nxb = W / CT;
  auto load_stage = [&](int ch) {
    const int b = ch / (H * nxb), r = ch - b * (H * nxb);
    const int xb = r / H, y = r - xb * H, x0 = xb * CT;
    const int m0 = b * hw + y * W + x0;
    if (tid < YP) ry = *reinterpret_cast<const float4*>(gy + (long long)m0 * COP + tid * 4);
#pragma unroll
    for (int t = 0; t < XPIECES; ++t) {
      const int pid = tid + 256 * t;
      const int hr = pid >> 3, c8 = pid & 7;
      const int rr = hr / HALO, px = hr - rr * HALO;
      const int yy = y + rr - 1, xx = x0 + px - 1;
      uint4 v = make_uint4(0, 0, 0, 0);
      if (hr < XROWS && (unsigned)yy < (unsigned)H && (unsigned)xx < (unsigned)W)
        v = *reinterpret_cast<const uint4*>(x + ((long long)(b * H + yy) * W + xx) * CinP + k0 + c8 * 8);
      rx[t] = v;
    }
  };
  auto store_stage = [&](int buf) {
    if (tid < YP) {
      const int row = tid / (COP / 4), f4 = tid % (COP / 4);
      const float gv[4] = {ry.x, ry.y, ry.z, ry.w};
      float hi[4], lo[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        hi[e] = bf2f(f2bf(gv[e]));
        lo[e] = gv[e] - hi[e];
      }
      *reinterpret_cast<uint2*>(Yh + (buf * CT + row) * 16 + f4 * 4) = pack_bf4(hi[0], hi[1], hi[2], hi[3]);
      *reinterpret_cast<uint2*>(Yl + (buf * CT + row) * 16 + f4 * 4) = pack_bf4(lo[0], lo[1], lo[2], lo[3]);
    }
    bf16_t* xs = Xs + buf * XROWS * SP;
#pragma unroll
    for (int t = 0; t < XPIECES; ++t) {
      const int pid = tid + 256 * t;
      if (pid < XROWS * 8) *reinterpret_cast<uint4*>(xs + (pid >> 3) * SP + (pid & 7) * 8) = rx[t];
    }
  };

  f32x4_t acc[9], accb = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int q = 0; q < 9; ++q) acc[q] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  const bool do_bias = db != nullptr && tk == 0 && wave == 0;
  const bf16x8_t ones = bf16x8_t{0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80};

  load_stage(c_begin);
  __syncthreads();                                   // the zero fill above is complete
  store_stage(0);
  __syncthreads();
  for (int ch = c_begin; ch < c_end; ++ch) {
    const int buf = (ch - c_begin) & 1;
    if (ch + 1 < c_end) load_stage(ch + 1);
    const bf16_t* yh = Yh + buf * CT * 16;
    const bf16_t* yl = Yl + buf * CT * 16;
    const bf16_t* xs = Xs + buf * XROWS * SP;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      bf16x8_t yfh, yfl;
      {
        const bf16x4_t lo = lds_tr_read(tr_addr(yh, 16, 32 * ks + 4 * g, 0, lane));
        const bf16x4_t hi = lds_tr_read(tr_addr(yh, 16, 32 * ks + 16 + 4 * g, 0, lane));
        yfh = bf16x8_t{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        const bf16x4_t lo2 = lds_tr_read(tr_addr(yl, 16, 32 * ks + 4 * g, 0, lane));
        const bf16x4_t hi2 = lds_tr_read(tr_addr(yl, 16, 32 * ks + 16 + 4 * g, 0, lane));
        yfl = bf16x8_t{lo2[0], lo2[1], lo2[2], lo2[3], hi2[0], hi2[1], hi2[2], hi2[3]};
      }
#pragma unroll
      for (int q = 0; q < 9; ++q) {
        const int cg = 9 * wave + q;
        const int tap = cg >> 2, kf = cg & 3;
        const int xb = (tap / 3) * HALO + (tap % 3);
        const bf16x4_t lo = lds_tr_read(tr_addr(xs, SP, xb + 32 * ks + 4 * g, 16 * kf, lane));
        const bf16x4_t hi = lds_tr_read(tr_addr(xs, SP, xb + 32 * ks + 16 + 4 * g, 16 * kf, lane));
        const bf16x8_t xf = bf16x8_t{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        acc[q] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(yfh, xf, acc[q], 0, 0, 0);
        acc[q] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(yfl, xf, acc[q], 0, 0, 0);
      }
      if (do_bias) {
        accb = __builtin_amdgcn_mfma_f32_16x16x32_bf16(yfh, ones, accb, 0, 0, 0);
        accb = __builtin_amdgcn_mfma_f32_16x16x32_bf16(yfl, ones, accb, 0, 0, 0);
      }
    }
    if (ch + 1 < c_end) store_stage(buf ^ 1);
    __syncthreads();
  }

  // acc[q][e] = dW[n = 4g + e][k = k0 + 16 kf + r16][tap]   (state_dict layout [Cout][Cin][3][3])
#pragma unroll
  for (int q = 0; q < 9; ++q) {
    const int cg = 9 * wave + q;
    const int tap = cg >> 2, k = k0 + 16 * (cg & 3) + r16;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int n = 4 * g + e;
      if (n < Co && k < Cin) atomicAdd(dW + ((long long)(n * Cin) + k) * 9 + tap, acc[q][e]);
    }
  }
  if (do_bias && r16 == 0) {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (4 * g + e < Co) atomicAdd(db + 4 * g + e, accb[e]);
  }
}

template <int COP>
int launch_smallconv_mfma(const bf16_t* x, const float* gy, float* dW, float* db, int B, int H, int W, int Cin, int CinP, int Co,
                          hipStream_t stream) {
  constexpr int lds_staged = (int)((2 * 2 * CT * 16 + 2 * XROWS * SP) * sizeof(bf16_t));
  static_assert(2 * SR<COP>::LDS <= 160 * 1024, "two workgroups per CU");
  static SrkLdsState reserved[2];                       // [staged, rolling]: the kernel this launch runs
  constexpr const char* err = "smallconv wgrad: cannot reserve %d bytes of LDS";
  constexpr int lds_max = SR<COP>::LDS > lds_staged ? SR<COP>::LDS : lds_staged;
  const bool roll = g_taps_roll;
  if (const int rc = roll ? srk_reserve_lds(&smallconv_wgrad_mfma_kernel<COP>, SR<COP>::LDS, reserved[1], false, err, lds_max)
                          : srk_reserve_lds(&smallconv_wgrad_mfma_staged_kernel<COP>, lds_staged, reserved[0], false, err, lds_max))
    return rc;
  const int tiles = CinP / 64;
  const int nchunks = (int)(((long long)B * H * W) / CT);
  int splits = 512 / tiles;                       // two workgroups per CU
  if (splits > nchunks) splits = nchunks;
  const int chunks_per = cdiv(nchunks, splits);
  splits = cdiv(nchunks, chunks_per);
  if (roll)
    hipLaunchKernelGGL((smallconv_wgrad_mfma_kernel<COP>), dim3(tiles * splits), dim3(256), SR<COP>::LDS, stream, x, gy, dW, db, B, H, W,
                       Cin, CinP, Co, tiles, chunks_per);
  else
    hipLaunchKernelGGL((smallconv_wgrad_mfma_staged_kernel<COP>), dim3(tiles * splits), dim3(256), lds_staged, stream, x, gy, dW, db, B, H,
                       W, Cin, CinP, Co, tiles, chunks_per);
  return srk_check_launch("smallconv wgrad (mfma)");
}

// ---- image-head dgrad on the matrix cores ---------------------------------------------------------------------------
//   dX[pix][ci] = sum_{tap,co} gy[pix - off(tap)][co] * W[co][ci][tap]      (Cout <= 4, Cin <= 64; conv_last of the x2/x4 heads)
// A GEMM with K = 9 taps x 4 channels = 36 (padded to 64): the A fragment of a pixel is gathered straight from the fp32
// dY (two taps = 8 consecutive k per lane), W sits in registers, both operands are split into bf16 hi + lo (hi*hi + lo*hi
// + hi*lo, ~2^-16 relative: the result is then rounded to bf16 once, like the fp32 VALU kernel it replaces), and the
// 64 x 64 output tile goes through LDS so that every store is a full 128-byte pixel row.
__global__ __launch_bounds__(256) void imghead_dgrad_mfma_kernel(const float* __restrict__ gy, const float* __restrict__ wgt,
                                                                 bf16_t* __restrict__ dx, int B, int H, int W, int Cin, int Co, int nchunks) {
  constexpr int TP = 64 + 8;
  __shared__ __attribute__((aligned(16))) bf16_t T[64 * TP];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r16 = lane & 15, g = lane >> 4;

  // W fragments: row n = ci = 16 j + r16, k = 32 ks + 8 g + jj  ->  (tap, co) = (k / 4, k % 4)
  bf16x8_t wh[4][2], wl[4][2];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      float v[8];
#pragma unroll
      for (int jj = 0; jj < 8; ++jj) {
        const int k = 32 * ks + 8 * g + jj;
        const int tap = k >> 2, co = k & 3, ci = 16 * j + r16;
        v[jj] = (tap < 9 && co < Co && ci < Cin) ? wgt[((co * Cin) + ci) * 9 + tap] : 0.f;
      }
      split_bf16x8(v, wh[j][ks], wl[j][ks]);
    }

  const int hw = H * W;
  for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
    const int pix = c * 64 + 16 * wave + r16;
    const int b = pix / hw, rem = pix - b * hw;
    const int y = rem / W, x = rem - y * W;
    f32x4_t acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      float v[8];
#pragma unroll
      for (int half = 0; half < 2; ++half) {
        const int tap = 8 * ks + 2 * g + half;
        float4 gv = make_float4(0.f, 0.f, 0.f, 0.f);
        if (tap < 9) {
          // output pixel that used input pixel (y, x) through tap (ky, kx) is (y - (ky - 1), x - (kx - 1))
          const int yy = y - (tap / 3 - 1), xs = x - (tap % 3 - 1);
          if ((unsigned)yy < (unsigned)H && (unsigned)xs < (unsigned)W)
            gv = *reinterpret_cast<const float4*>(gy + ((long long)(b * H + yy) * W + xs) * 4);
        }
        v[4 * half] = gv.x; v[4 * half + 1] = gv.y; v[4 * half + 2] = gv.z; v[4 * half + 3] = gv.w;
      }
      bf16x8_t xh, xl;
      split_bf16x8(v, xh, xl);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh[j][ks], xh, acc[j], 0, 0, 0);
        acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wl[j][ks], xh, acc[j], 0, 0, 0);
        acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh[j][ks], xl, acc[j], 0, 0, 0);
      }
    }
    // acc[j][e] = dX[pixel 16 wave + r16][ci = 16 j + 4 g + e]
#pragma unroll
    for (int j = 0; j < 4; ++j)
      *reinterpret_cast<uint2*>(T + (16 * wave + r16) * TP + 16 * j + 4 * g) = pack_bf4(acc[j][0], acc[j][1], acc[j][2], acc[j][3]);
    srk_lds_barrier();
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int pid = tid + 256 * t;
      const int row = pid >> 3, c8 = pid & 7;
      *reinterpret_cast<uint4*>(dx + ((long long)c * 64 + row) * 64 + c8 * 8) = *reinterpret_cast<const uint4*>(T + row * TP + c8 * 8);
    }
    srk_lds_barrier();
  }
}

}  // namespace

void srk_conv_wgrad_taps_enable(int on) {
  g_taps_enabled = on ? 1 : 0;    // 0: per-tap tiles / VALU image head; 1: all-taps register-staged; 2: all-taps LDS-DMA ring (default)
  g_taps_dma = on >= 2 ? 1 : 0;
}
int srk_conv_wgrad_taps_mode() { return g_taps_enabled ? (g_taps_dma ? 2 : 1) : 0; }
void srk_conv_wgrad_roll_enable(int on) { g_taps_roll = on ? 1 : 0; }   // 1 (default): rolling X-row window where it applies
int srk_conv_wgrad_roll_enabled() { return g_taps_roll; }

// SRK_WGRAD_NOT_COVERED when the all-taps kernel does not apply (the caller then uses the per-tap tiles of wgrad.hip)
int srk_launch_conv_wgrad_taps(const WgradParams& p, hipStream_t stream) {
  if (!g_taps_enabled || !p.conv || p.W % CT != 0 || p.N % 64 != 0 || p.K % 64 != 0 || p.ldx % 8 != 0) return SRK_WGRAD_NOT_COVERED;
  if (p.r > 1) {
    if (p.Cs % 8 != 0 || p.N != p.r * p.r * p.Cs) return SRK_WGRAD_NOT_COVERED;
    return g_taps_dma ? launch_taps_dma<true>(p, stream) : launch_taps<true>(p, stream);
  }
  if (p.ldy % 8 != 0) return SRK_WGRAD_NOT_COVERED;
  return g_taps_dma ? launch_taps_dma<false>(p, stream) : launch_taps<false>(p, stream);
}

// image-head convs (Cout <= 16, fp32 dY): SRK_WGRAD_NOT_COVERED -> the VALU kernel of misc.hip
int srk_launch_smallconv_wgrad_mfma(const bf16_t* x, const float* gy, float* dW, float* db, int B, int H, int W, int Cin, int CinP,
                                    int Co, int CoP, hipStream_t stream) {
  if (!g_taps_enabled || W % CT != 0 || CinP % 64 != 0 || Co > CoP || ((long long)B * H * W) % CT != 0) return SRK_WGRAD_NOT_COVERED;
  if (CoP == 4) return launch_smallconv_mfma<4>(x, gy, dW, db, B, H, W, Cin, CinP, Co, stream);
  if (CoP == 16) return launch_smallconv_mfma<16>(x, gy, dW, db, B, H, W, Cin, CinP, Co, stream);
  return SRK_WGRAD_NOT_COVERED;
}

int srk_launch_imghead_dgrad_mfma(const float* gy, const float* wgt, bf16_t* dx, int B, int H, int W, int Cin, int CinP, int Co, int CoP,
                                  hipStream_t stream) {
  const long long npix = (long long)B * H * W;
  if (!g_taps_enabled || CoP != 4 || CinP != 64 || Co > 4 || Cin > 64 || npix % 64 != 0 || npix > (1ll << 30)) return SRK_WGRAD_NOT_COVERED;
  const int nchunks = (int)(npix / 64);
  const int grid = nchunks < 2048 ? nchunks : 2048;
  hipLaunchKernelGGL(imghead_dgrad_mfma_kernel, dim3(grid), dim3(256), 0, stream, gy, wgt, dx, B, H, W, Cin, Co, nchunks);
  return srk_check_launch("image-head dgrad (mfma)");
}
