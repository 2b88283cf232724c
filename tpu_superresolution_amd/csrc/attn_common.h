// Device helpers shared by the window-attention kernels (attn*.hip).  gfx950 only.
#pragma once
#include "common.h"

// exp(x - m) = exp2(x log2e - m log2e): one fma + v_exp_f32 per score
constexpr float SRK_L2E = 1.4426950408889634f;

// Softmax numerators of one 16-query x 64-key score tile held as four MFMA accumulators (s[jt][e] = S[query r16][key
// 16 jt + 4 g + e], bias and mask already added).  Returns exp(s - rowmax) -- in [0, 1], UNNORMALISED -- as the two bf16
// B-operand fragments of P (k = key) and 1 / row sum: the caller scales its 8 outputs instead of the 64 probabilities.
// exp(x - m) = exp2(x log2e - m log2e): one packed fma per two scores + v_exp_f32, v_rcp_f32 for the sum (the phase is
// VALU-issue-bound: 4 cycles per wave-instruction, 8 for a transcendental).
__device__ __forceinline__ float softmax_numerators(const f32x4_t (&s)[4], bf16x8_t (&pf)[2]) {
  float mx = fmaxf(fmaxf(s[0][0], s[0][1]), fmaxf(s[0][2], s[0][3]));
#pragma unroll
  for (int jt = 1; jt < 4; ++jt) mx = fmaxf(fmaxf(mx, s[jt][0]), fmaxf(fmaxf(s[jt][1], s[jt][2]), s[jt][3]));
  mx = xrow_max4(mx);
  const float mxl = mx * SRK_L2E;
  f32x4_t e[4];
#pragma unroll
  for (int jt = 0; jt < 4; ++jt) {
    const f32x4_t t = s[jt] * SRK_L2E - mxl;
#pragma unroll
    for (int k = 0; k < 4; ++k) e[jt][k] = __builtin_amdgcn_exp2f(t[k]);
  }
  const f32x4_t a = (e[0] + e[1]) + (e[2] + e[3]);
  const float sum = xrow_sum4((a[0] + a[1]) + (a[2] + a[3]));
#pragma unroll
  for (int ss = 0; ss < 2; ++ss) {
    const uint2 lo = pack_bf4(e[2 * ss][0], e[2 * ss][1], e[2 * ss][2], e[2 * ss][3]);
    const uint2 hi = pack_bf4(e[2 * ss + 1][0], e[2 * ss + 1][1], e[2 * ss + 1][2], e[2 * ss + 1][3]);
    pf[ss] = __builtin_bit_cast(bf16x8_t, make_uint4(lo.x, lo.y, hi.x, hi.y));
  }
  return __builtin_amdgcn_rcpf(sum);
}

// two transposed 4-element reads side by side: one 8-element MFMA operand fragment
__device__ __forceinline__ bf16x8_t cat4(bf16x4_t lo, bf16x4_t hi) {
  return bf16x8_t{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}

// shift-mask region (0, 1, 2) of coordinate v on an axis of n positions, window w, shift s (network_swinir.py:219-230 for any
// window / shift; a token's label is region3(y) * 3 + region3(x))
__device__ __forceinline__ int region3(int v, int n, int w, int s) { return v < n - w ? 0 : (v < n - s ? 1 : 2); }

// [rows][32] bf16 tiles without padding (64-byte rows): the 16-byte chunk index (0..3) of row r is XOR-ed with tfs(r), a function
// of row bits 1..3.  With it the three ways these kernels read a tile each touch every LDS bank once: the row-per-lane fragment
// ds_read_b128 (16 consecutive rows x one chunk per 16-lane group) and both k orders of the transposing ds_read_b64_tr_b16 (4
// consecutive rows x 16 columns per 16-lane group, two row blocks 16 apart).  A 40-element pitch does the same with 25% more LDS.
__device__ __forceinline__ int tfs(int r) { return ((((r >> 2) ^ (r >> 3)) & 1) << 1) | (((r >> 3) ^ (r >> 1)) & 1); }
// element offset of 16-byte chunk c of row r
__device__ __forceinline__ int chunk_off(int r, int c) { return r * 32 + ((c ^ tfs(r)) << 3); }
