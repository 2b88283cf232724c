// The per-sample parameters and the noise stage of the blind degradation, shared by degrade.hip (srk_degrade_blind_f32,
// srk_crop_degrade_blind_u8) and blur2d.hip (srk_crop_degrade_psf_u8): both files decode slots 6..9 of a descriptor and finish an
// output with the same code on the same values, so a draw depends on (noise_id, x, y, ch) alone and not on the entry that made it.
#pragma once
#include "resize.h"

#pragma clang fp contract(off)

namespace {

constexpr int DG_RMAX = 8;                   // ceil(3 * 2.5): the widest Gaussian radius

// slots 6..9 of a descriptor / one row of par4, decoded and made safe: any bit pattern gives R in 0..8 and finite noise amplitudes
struct DgParams {
  double sy, sx;
  int Ry, Rx;
  float sn, gain;
  unsigned k0, k1;
  int gray, noisy;
};

__device__ __forceinline__ int dg_radius(float sigma) {
  if (!(sigma > 0.f)) return 0;              // 0, negative, NaN: no blur on this axis
  const double r = ceil(3.0 * (double)sigma);
  return r > (double)DG_RMAX ? DG_RMAX : (int)r;
}

__device__ __forceinline__ float dg_amplitude(float a) { return a > 0.f ? fminf(a, 16.f) : 0.f; }

__device__ __forceinline__ DgParams dg_params(const long long* p) {
  const unsigned long long b = (unsigned long long)p[0], n = (unsigned long long)p[1], id = (unsigned long long)p[2];
  DgParams q;
  const float sy = __uint_as_float((unsigned)b), sx = __uint_as_float((unsigned)(b >> 32));
  q.sy = (double)sy;
  q.sx = (double)sx;
  q.Ry = dg_radius(sy);
  q.Rx = dg_radius(sx);
  q.sn = dg_amplitude(__uint_as_float((unsigned)n));
  q.gain = dg_amplitude(__uint_as_float((unsigned)(n >> 32)));
  q.k0 = (unsigned)id;
  q.k1 = (unsigned)(id >> 32);
  q.gray = (int)(p[3] & 1);
  q.noisy = q.sn > 0.f || q.gain > 0.f;
  return q;
}

// Philox4x32-10 (Salmon et al., SC'11): the first two words of the block of counter (c0, c1, c2, 0) under key (k0, k1)
__device__ __forceinline__ void dg_philox(unsigned c0, unsigned c1, unsigned c2, unsigned k0, unsigned k1, unsigned* r0, unsigned* r1) {
  unsigned c3 = 0u;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0, h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
    c0 = h1 ^ c1 ^ k0;
    c1 = l1;
    c2 = h0 ^ c3 ^ k1;
    c3 = l0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  *r0 = c0;
  *r1 = c1;
}

// the filtered value v of output (x, y) of the whole downscaled image, channel ch -> the stored value
__device__ __forceinline__ float dg_finish(float v, const DgParams& q, int x, int y, int ch, int quant_bits) {
  if (q.noisy) {
    unsigned r0, r1;
    dg_philox((unsigned)x, (unsigned)y, (unsigned)ch, q.k0, q.k1, &r0, &r1);
    const float u1 = (float)((r0 >> 8) + 1u) * 5.9604644775390625e-8f, u2 = (float)(r1 >> 8) * 5.9604644775390625e-8f;          // 2^-24
    const float z = sqrtf(-2.0f * logf(u1)) * cospif(2.0f * u2);
    v = v + sqrtf(q.sn * q.sn + q.gain * fmaxf(v, 0.f)) * z;
  }
  return quant_bits == 8 ? rs_quant8(v) : v;
}

}  // namespace
