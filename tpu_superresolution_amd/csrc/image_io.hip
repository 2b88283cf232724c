// Image files to and from the device: interleaved 8- / 16-bit samples [B][H][W][ch] <-> planar fp32 [B][C][H][W] in [0, 1]
// (include/srk.h: srk_image_unpack, srk_image_pack; arguments checked there).
//
// An image is P = H * W pixels; both its interleaved samples and each of its planes are contiguous, so the kernels walk pixels, not
// rows.  A thread owns GROUPS of four consecutive pixels: 4 * ch * (bits / 8) interleaved bytes -- always whole dwords -- and one
// float4 of every plane; consecutive lanes own consecutive groups, so a wave touches one contiguous interleaved span and one
// contiguous 1-KiB span per plane.  blockIdx.y is the image, blockIdx.x strides over its groups (at most ~2048 workgroups in all).
//
//   - interleaved loads (unpack): the image may start at any byte (a PIL buffer, an odd-sized image behind another).  The start is
//     rounded DOWN to a dword, the thread loads the dwords that hold its bytes (one more when the phase is not 0) and shifts them into
//     place with v_alignbyte; the phase is the same for every thread of an image.  A dword is loaded only if it holds a byte of the image.
//   - interleaved stores (pack): whole dwords when the image starts on a dword and the group is complete; else sample by sample (a
//     dword two threads share cannot be stored without a race).
//   - planar side: float4 when the plane starts on 16 bytes and P % 4 == 0 (then every group is complete), else one float per pixel.
// Offsets are 64-bit; plain vector loads and stores; the two counters of pack are integer sums: per thread, then per workgroup
// through 32 bytes of LDS, then one integer vector atomic per counter and workgroup (none when the sum is 0) -- exact in any order.
#include "kernels.h"

namespace {

constexpr int IO_THREADS = 256;
constexpr int IO_MAX_BLOCKS = 2048;           // 8 per CU: the grid-stride cap of a memory-bound launch

struct __attribute__((packed, aligned(4))) IoWords2 { unsigned w[2]; };
struct __attribute__((packed, aligned(4))) IoWords3 { unsigned w[3]; };
struct __attribute__((packed, aligned(4))) IoWords4 { unsigned w[4]; };

__device__ __forceinline__ unsigned io_luma(unsigned r, unsigned g, unsigned b) {      // ops.to_gray: 16384 * 65535 + 8192 < 2^32
  return (4899u * r + 9617u * g + 1868u * b + 8192u) >> 14;
}

// sample j of a group held as little-endian dwords
template <int BITS, int ND>
__device__ __forceinline__ unsigned io_sample(const unsigned (&v)[ND], int j) {
  if constexpr (BITS == 8) return (v[j >> 2] >> (8 * (j & 3))) & 0xffu;
  else return (v[j >> 1] >> (16 * (j & 1))) & 0xffffu;
}

__device__ __forceinline__ void io_store4(float* plane, long long p0, long long P, bool vec, const float (&v)[4]) {
  if (vec) {
    *reinterpret_cast<float4*>(plane + p0) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (p0 + i < P) plane[p0 + i] = v[i];
  }
}

__device__ __forceinline__ void io_load4(const float* plane, long long p0, long long P, bool vec, float (&v)[4]) {
  if (vec) {
    const float4 t = *reinterpret_cast<const float4*>(plane + p0);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = p0 + i < P ? plane[p0 + i] : 0.f;      // 0: quantises to 0, counts nothing, is never stored
  }
}

template <int IC, int BITS, int OC>
__global__ __launch_bounds__(IO_THREADS) void image_unpack_kernel(const unsigned char* __restrict__ src, float* __restrict__ dst,
                                                                  float* __restrict__ alpha, long long P, int vec, int avec) {
  constexpr int SB = BITS / 8, NB = 4 * IC * SB, ND = NB / 4;
  constexpr float MAXV = BITS == 8 ? 255.0f : 65535.0f;
  const size_t img_bytes = (size_t)P * (IC * SB);
  const unsigned char* img = src + (size_t)blockIdx.y * img_bytes;
  const unsigned phase = (unsigned)(reinterpret_cast<uintptr_t>(img) & 3u);           // the same in every thread
  const unsigned* base = reinterpret_cast<const unsigned*>(img - phase);
  const size_t end = img_bytes + phase;                                                // the image's bytes, counted from base
  float* out = dst + (size_t)blockIdx.y * OC * (size_t)P;
  float* aout = alpha ? alpha + (size_t)blockIdx.y * (size_t)P : nullptr;
  const long long G = (P + 3) >> 2;
  for (long long g = (long long)blockIdx.x * IO_THREADS + threadIdx.x; g < G; g += (long long)gridDim.x * IO_THREADS) {
    const size_t d0 = (size_t)g * ND;
    unsigned w[ND + 1];
#pragma unroll
    for (int k = 0; k < ND; ++k) w[k] = (d0 + k) * 4 < end ? base[d0 + k] : 0u;
    w[ND] = (phase != 0 && (d0 + ND) * 4 < end) ? base[d0 + ND] : 0u;
    unsigned v[ND];
#pragma unroll
    for (int k = 0; k < ND; ++k) v[k] = __builtin_amdgcn_alignbyte(w[k + 1], w[k], phase);
    float c[OC][4], a[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      unsigned s[IC];
#pragma unroll
      for (int j = 0; j < IC; ++j) s[j] = io_sample<BITS, ND>(v, i * IC + j);
      if constexpr (IC <= 2) {
#pragma unroll
        for (int ch = 0; ch < OC; ++ch) c[ch][i] = (float)s[0] / MAXV;
      } else if constexpr (OC == 3) {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) c[ch][i] = (float)s[ch] / MAXV;
      } else {
        c[0][i] = (float)io_luma(s[0], s[1], s[2]) / MAXV;
      }
      a[i] = (IC & 1) ? 0.f : (float)s[IC - 1] / MAXV;
    }
    const long long p0 = g << 2;
#pragma unroll
    for (int ch = 0; ch < OC; ++ch) io_store4(out + (size_t)ch * (size_t)P, p0, P, vec != 0, c[ch]);
    if constexpr ((IC & 1) == 0)
      if (aout) io_store4(aout, p0, P, avec != 0, a);
  }
}

// q(v): NaN -> 0, v <= 0 -> 0, v >= 1 -> max, else rint(v * max) (one fp32 product, round-half-to-even); the counts of the input
template <int BITS>
__device__ __forceinline__ unsigned io_quant(float v, unsigned& nonfinite, unsigned& clipped) {
  constexpr float MAXV = BITS == 8 ? 255.0f : 65535.0f;
  const bool fin = __builtin_fabsf(v) < __builtin_inff();          // false for NaN and +-Inf
  nonfinite += fin ? 0u : 1u;
  clipped += (fin && (v < 0.f || v > 1.f)) ? 1u : 0u;
  if (!(v > 0.f)) return 0u;                                         // NaN, -0.0, negatives, -Inf
  if (v >= 1.f) return (unsigned)MAXV;
  return (unsigned)__builtin_rintf(v * MAXV);
}

template <int C, int OC, int BITS>
__global__ __launch_bounds__(IO_THREADS) void image_pack_kernel(const float* __restrict__ y, const float* __restrict__ alpha,
                                                                unsigned char* __restrict__ dst, unsigned* __restrict__ counters,
                                                                long long P, int vec, int avec) {
  constexpr int SB = BITS / 8, NS = 4 * OC, NB = NS * SB, ND = NB / 4;
  constexpr bool HAS_A = (OC & 1) == 0;
  const float* in = y + (size_t)blockIdx.y * C * (size_t)P;
  const float* ain = HAS_A ? alpha + (size_t)blockIdx.y * (size_t)P : nullptr;
  unsigned char* img = dst + (size_t)blockIdx.y * (size_t)P * (OC * SB);
  const bool aligned = (reinterpret_cast<uintptr_t>(img) & 3u) == 0;                   // the same in every thread
  const long long G = (P + 3) >> 2;
  unsigned nonfinite = 0, clipped = 0;
  for (long long g = (long long)blockIdx.x * IO_THREADS + threadIdx.x; g < G; g += (long long)gridDim.x * IO_THREADS) {
    const long long p0 = g << 2;
    float c[C][4], a[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ch = 0; ch < C; ++ch) io_load4(in + (size_t)ch * (size_t)P, p0, P, vec != 0, c[ch]);
    if constexpr (HAS_A) io_load4(ain, p0, P, avec != 0, a);
    unsigned s[NS];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      unsigned q[C];
#pragma unroll
      for (int ch = 0; ch < C; ++ch) q[ch] = io_quant<BITS>(c[ch][i], nonfinite, clipped);
      if constexpr (OC <= 2) {
        if constexpr (C == 3) s[i * OC] = io_luma(q[0], q[1], q[2]);       // the luma of the QUANTISED samples
        else s[i * OC] = q[0];
      } else {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) s[i * OC + ch] = q[C == 3 ? ch : 0];
      }
      if constexpr (HAS_A) s[i * OC + OC - 1] = io_quant<BITS>(a[i], nonfinite, clipped);
    }
    if (aligned && p0 + 3 < P) {
      unsigned v[ND];
#pragma unroll
      for (int k = 0; k < ND; ++k) {
        if constexpr (BITS == 8) v[k] = s[4 * k] | (s[4 * k + 1] << 8) | (s[4 * k + 2] << 16) | (s[4 * k + 3] << 24);
        else v[k] = s[2 * k] | (s[2 * k + 1] << 16);
      }
      unsigned char* at = img + (size_t)g * NB;
      if constexpr (ND % 4 == 0) {          // 4, 8
#pragma unroll
        for (int k = 0; k < ND; k += 4) *reinterpret_cast<IoWords4*>(at + 4 * k) = IoWords4{{v[k], v[k + 1], v[k + 2], v[k + 3]}};
      } else if constexpr (ND == 3) {
        *reinterpret_cast<IoWords3*>(at) = IoWords3{{v[0], v[1], v[2]}};
      } else if constexpr (ND % 2 == 0) {   // 2, 6
#pragma unroll
        for (int k = 0; k < ND; k += 2) *reinterpret_cast<IoWords2*>(at + 4 * k) = IoWords2{{v[k], v[k + 1]}};
      } else {
        *reinterpret_cast<unsigned*>(at) = v[0];
      }
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (p0 + i >= P) continue;
#pragma unroll
        for (int j = 0; j < OC; ++j) {
          const size_t at = ((size_t)(p0 + i) * OC + j);
          if constexpr (BITS == 8) img[at] = (unsigned char)s[i * OC + j];
          else reinterpret_cast<unsigned short*>(img)[at] = (unsigned short)s[i * OC + j];
        }
      }
    }
  }
  if (counters) {          // the same in every thread: the barrier below is reached by all or none
    __shared__ unsigned red[2][IO_THREADS / 64];
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      nonfinite += __shfl_xor(nonfinite, o, 64);
      clipped += __shfl_xor(clipped, o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
      red[0][threadIdx.x >> 6] = nonfinite;
      red[1][threadIdx.x >> 6] = clipped;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
      unsigned t = 0;
#pragma unroll
      for (int k = 0; k < IO_THREADS / 64; ++k) t += red[threadIdx.x][k];
      if (t) atomicAdd(counters + threadIdx.x, t);
    }
  }
}

dim3 io_grid(int B, long long P) {
  const long long G = (P + 3) >> 2;
  long long gx = (G + IO_THREADS - 1) / IO_THREADS;
  const long long cap = (IO_MAX_BLOCKS + B - 1) / B;
  if (gx > cap) gx = cap;
  return dim3((unsigned)gx, (unsigned)B);
}

template <int IC, int BITS>
void unpack_launch(const void* src, float* dst, float* alpha, int B, long long P, int out_chans, int vec, int avec, hipStream_t stream) {
  const dim3 grid = io_grid(B, P), block(IO_THREADS);
  const unsigned char* s = static_cast<const unsigned char*>(src);
  if (out_chans == 1) hipLaunchKernelGGL((image_unpack_kernel<IC, BITS, 1>), grid, block, 0, stream, s, dst, alpha, P, vec, avec);
  else hipLaunchKernelGGL((image_unpack_kernel<IC, BITS, 3>), grid, block, 0, stream, s, dst, alpha, P, vec, avec);
}

template <int C, int BITS>
void pack_launch(const float* y, const float* alpha, void* dst, unsigned* counters, int B, long long P, int out_chans, int vec, int avec,
                 hipStream_t stream) {
  const dim3 grid = io_grid(B, P), block(IO_THREADS);
  unsigned char* d = static_cast<unsigned char*>(dst);
  switch (out_chans) {
    case 1: hipLaunchKernelGGL((image_pack_kernel<C, 1, BITS>), grid, block, 0, stream, y, alpha, d, counters, P, vec, avec); break;
    case 2: hipLaunchKernelGGL((image_pack_kernel<C, 2, BITS>), grid, block, 0, stream, y, alpha, d, counters, P, vec, avec); break;
    case 3: hipLaunchKernelGGL((image_pack_kernel<C, 3, BITS>), grid, block, 0, stream, y, alpha, d, counters, P, vec, avec); break;
    default: hipLaunchKernelGGL((image_pack_kernel<C, 4, BITS>), grid, block, 0, stream, y, alpha, d, counters, P, vec, avec); break;
  }
}

// float4 on a plane: every plane of every image starts on 16 bytes and no group is partial
int io_vec(const float* p, long long P) { return p != nullptr && srk_aligned(p, 16) && (P & 3) == 0; }

}  // namespace

int srk_launch_image_unpack(const void* src, float* dst, float* alpha, int B, int H, int W, int in_chans, int bits, int out_chans,
                            hipStream_t stream) {
  const long long P = (long long)H * W;
  const int vec = io_vec(dst, P), avec = io_vec(alpha, P);
#define IO_UNPACK(IC)                                                                                       \
  case IC:                                                                                                  \
    if (bits == 8) unpack_launch<IC, 8>(src, dst, alpha, B, P, out_chans, vec, avec, stream);               \
    else unpack_launch<IC, 16>(src, dst, alpha, B, P, out_chans, vec, avec, stream);                        \
    break;
  switch (in_chans) {
    IO_UNPACK(1)
    IO_UNPACK(2)
    IO_UNPACK(3)
    IO_UNPACK(4)
  }
#undef IO_UNPACK
  return srk_check_launch("image_unpack");
}

int srk_launch_image_pack(const float* y, const float* alpha, void* dst, unsigned* counters, int B, int H, int W, int chans, int out_chans,
                          int bits, hipStream_t stream) {
  const long long P = (long long)H * W;
  const int vec = io_vec(y, P), avec = io_vec(alpha, P);
  if (chans == 1) {
    if (bits == 8) pack_launch<1, 8>(y, alpha, dst, counters, B, P, out_chans, vec, avec, stream);
    else pack_launch<1, 16>(y, alpha, dst, counters, B, P, out_chans, vec, avec, stream);
  } else {
    if (bits == 8) pack_launch<3, 8>(y, alpha, dst, counters, B, P, out_chans, vec, avec, stream);
    else pack_launch<3, 16>(y, alpha, dst, counters, B, P, out_chans, vec, avec, stream);
  }
  return srk_check_launch("image_pack");
}
