// Blur and sinc tables built on the device (include/srk.h: srk_kernel_tables_f32): the fp32 [n][ks][ks] tables that blur2d.hip,
// degrade.hip and filter2d.hip consume, from eight doubles each, so that the host of a training step draws variates and uploads no
// table.  What blur_kernels evaluates in fp64 numpy is evaluated here in fp64 VALU, in the order srk.h fixes:
//   q = (A x^2 + B2 x y) + C y^2, the integer products exact, A / B2 / C formed by the host: the host's bits
//   e = exp(-0.5 q) | exp(-0.5 pow(q, beta)) | 1 / (pow(q, beta) + 1) | cutoff J1(cutoff r) / (2 pi r)
//   S = the sum of e over the own taps, sequential, row-major; tap = (float)(e / S)
// J1 is the 512-interval trapezoid rule of blur_kernels.j1 on Bessel's integral; it is evaluated once per DISTINCT x^2 + y^2 of the grid
// (a 21 x 21 grid has 61 of them, not 441) and looked up by that integer.
//
// One workgroup of 256 threads makes one table.  LDS: sin(t_j), j = 0..512, once per workgroup (4104 B); J1 by x^2 + y^2 in 0..200 and
// the flags of the values the grid holds (1608 + 804 B); the fp64 taps (3528 B); S.  Thread d evaluates J1 for x^2 + y^2 = d -- 513
// cosines summed in ascending order, the chain the contract fixes -- and thread 0 sums the taps.  No MFMA, static LDS only.
// Every index is formed from CLAMPED integers (tb_kind / tb_own / tb_bank_index): for any descriptor bits the kernel stays inside desc
// [8 n], bank [n_bank kb kb] and tab [n ks ks].
#include "tables.h"

#pragma clang fp contract(off)

namespace {

constexpr int TB_KMAX = 21;
constexpr int TB_D2MAX = 2 * (TB_KMAX / 2) * (TB_KMAX / 2);          // 200: the largest x^2 + y^2 of a 21 x 21 grid
constexpr int TB_J1N = 512;                                         // intervals of the trapezoid rule (blur_kernels._J1_N)
constexpr double TB_PI = 3.141592653589793;                         // math.pi

// the three integers of a descriptor, from ANY bit pattern: comparisons with a NaN are false
__device__ __forceinline__ int tb_kind(double v, bool has_bank) {
  const int k = (v >= 0.0 && v < 6.0) ? (int)v : 0;
  return (k == 5 && !has_bank) ? 0 : k;
}
__device__ __forceinline__ int tb_own(double v, int ks) {          // odd, in 1..ks (ks is odd)
  const int o = v >= 1.0 ? (v <= (double)ks ? (int)v : ks) : 1;
  return (o - 1) | 1;
}
__device__ __forceinline__ int tb_bank_index(double v, int n_bank) {
  return v >= 0.0 ? (v <= (double)(n_bank - 1) ? (int)v : n_bank - 1) : 0;
}

__global__ __launch_bounds__(256) void kernel_tables_kernel(const double* __restrict__ desc, const unsigned* __restrict__ bank, int n_bank, int kb,
                                                            unsigned* __restrict__ tab, int ks) {
  __shared__ double sin_t[TB_J1N + 1];
  __shared__ double j1v[TB_D2MAX + 1];
  __shared__ double e[TB_KMAX * TB_KMAX];
  __shared__ int used[TB_D2MAX + 1];
  __shared__ double S;
  const int tid = threadIdx.x;
  const double* d = desc + (size_t)blockIdx.x * 8;
  unsigned* out = tab + (size_t)blockIdx.x * (size_t)(ks * ks);
  const int kind = tb_kind(d[0], bank != nullptr && n_bank >= 1);
  const int own = kind == 5 ? kb : tb_own(d[1], ks);                // the host requires kb odd in 1..ks (srk_tables_shape_ok)
  const int R = own >> 1, pad = (ks - own) >> 1, taps = own * own;

  if (kind == 0 || kind == 5) {                                     // words, no arithmetic; uniform over the workgroup
    const unsigned* src = kind == 5 ? bank + (size_t)tb_bank_index(d[7], n_bank) * (size_t)(kb * kb) : nullptr;
    for (int i = tid; i < ks * ks; i += 256) {
      const int a = i / ks - pad, b = i % ks - pad;
      const bool in = a >= 0 && a < own && b >= 0 && b < own;
      out[i] = !in ? 0u : (kind == 5 ? src[a * own + b] : ((a == R && b == R) ? 0x3f800000u : 0u));
    }
    return;
  }

  if (kind == 4) {
    const double cutoff = d[6];
    for (int j = tid; j <= TB_J1N; j += 256) sin_t[j] = sin(j == TB_J1N ? TB_PI : (double)j * (TB_PI / TB_J1N));
    for (int i = tid; i <= TB_D2MAX; i += 256) used[i] = 0;
    __syncthreads();
    for (int i = tid; i < taps; i += 256) {
      const int y = i / own - R, x = i % own - R;
      used[x * x + y * y] = 1;                                      // every writer stores the same value
    }
    __syncthreads();
    if (tid >= 1 && tid <= TB_D2MAX && used[tid]) {
      const double z = cutoff * sqrt((double)tid);
      double acc = 0.0;
      for (int j = 1; j < TB_J1N; ++j) acc += cos((double)j * (TB_PI / TB_J1N) - z * sin_t[j]);
      const double ends = cos(0.0 - z * sin_t[0]) + cos(TB_PI - z * sin_t[TB_J1N]);
      j1v[tid] = (acc + 0.5 * ends) / (double)TB_J1N;
    }
    __syncthreads();
    for (int i = tid; i < taps; i += 256) {
      const int y = i / own - R, x = i % own - R, d2 = x * x + y * y;
      const double r = sqrt((double)d2);
      e[i] = d2 == 0 ? cutoff * cutoff / (4.0 * TB_PI) : cutoff * j1v[d2] / (2.0 * TB_PI * r);
    }
  } else {
    const double A = d[2], B2 = d[3], Cq = d[4], beta = d[5];
    for (int i = tid; i < taps; i += 256) {
      const int y = i / own - R, x = i % own - R;
      const double q = (A * (double)(x * x) + B2 * (double)(x * y)) + Cq * (double)(y * y);
      e[i] = kind == 1 ? exp(-0.5 * q) : (kind == 2 ? exp(-0.5 * pow(q, beta)) : 1.0 / (pow(q, beta) + 1.0));
    }
  }
  __syncthreads();
  if (tid == 0) {
    double s = 0.0;
    for (int i = 0; i < taps; ++i) s += e[i];
    S = s;
  }
  __syncthreads();
  const double s = S;
  for (int i = tid; i < ks * ks; i += 256) {
    const int a = i / ks - pad, b = i % ks - pad;
    const bool in = a >= 0 && a < own && b >= 0 && b < own;
    out[i] = in ? __float_as_uint((float)(e[a * own + b] / s)) : 0u;
  }
}

}  // namespace

int srk_launch_kernel_tables_f32(const double* desc, const float* bank, int n_bank, int kb, float* tab, int n, int ks, hipStream_t stream) {
  SRK_REQUIRE(srk_tables_shape_ok(n, ks, bank != nullptr, n_bank, kb), SRK_E_SHAPE,
              "kernel_tables: n=%d must be >= 1, ks=%d odd in 1..21, and the bank (n_bank=%d, kb=%d) absent or with kb odd in 1..ks", n, ks, n_bank, kb);
  hipLaunchKernelGGL(kernel_tables_kernel, dim3((unsigned)n), dim3(256), 0, stream, desc, reinterpret_cast<const unsigned*>(bank), n_bank, kb,
                     reinterpret_cast<unsigned*>(tab), ks);
  return srk_check_launch("kernel_tables_f32");
}
