// Multi-tensor global-norm clip + AdamW for gfx950: the optimizer step of a model whose parameters are ordinary separate
// allocations (HAT, DAT: several hundred fp32 tensors, most of them 180 or 180 x 180 elements), in the multi-tensor-apply form.
// Semantics = srk_grad_sumsq / srk_adamw_clip_step (misc.hip) over a LIST: the gate, the clip coefficient and the per-element update
// are the functions of adamw.h that the flat-range kernel calls, so the two paths agree bit for bit.
//
// A launch covers a CHUNK of the list.  The chunk's table (pointers, element counts, first block of every tensor) travels BY VALUE
// in the kernel arguments (< 4 KB): nothing is uploaded, nothing is allocated and the host does not wait, so a step is capturable into
// a hipGraph as it is -- the captured node keeps its own copy of the table.  Launches per call = ceil(n_tensors / chunk).
//
// Work is split by (tensor, block of BLOCK elements): block b of the grid finds its tensor by a binary search of the block prefix
// (wave-uniform, scalar loads from the kernel-argument segment) and covers elements [c * BLOCK, min(n, (c + 1) * BLOCK)) of it, so a
// 180-element bias costs one workgroup and a 180 x 180 x 9 conv weight 72.  BLOCK is a multiple of 4, so a tensor whose base pointers
// are 16-byte aligned is walked with 16-byte loads and stores and a scalar tail of < 4 elements; a tensor with a pointer that is only
// 4-byte aligned (a view at an odd storage offset) takes the scalar loop.  Plain C++ / vector stores only.
//
// EMA of the weights (srk_multi_adamw_clip_ema_step): the same body with a compile-time flag and a table of its own that carries a
// fifth pointer per tensor (52 B instead of 44 B), so its chunk is 72 tensors; the table, the chunk and the launch count of the call
// without EMA are what they were.
#include <hip/hip_runtime.h>

#include "adamw.h"
#include "kernels.h"

namespace {

constexpr int THREADS = 256;
constexpr int STEP_TENSORS = 80;          // 80 * 44 B + 4 B = 3524 B of table, + 64 B of scalars
constexpr int STEP_BLOCK = 4096;          // elements per workgroup: 4 float4 per thread and array
constexpr int SUMSQ_TENSORS = 160;        // 160 * 20 B + 4 B = 3204 B
constexpr int SUMSQ_BLOCK = 16384;        // one atomic per workgroup: larger blocks, fewer adds on the one destination

struct StepTable {
  float* p[STEP_TENSORS];
  const float* g[STEP_TENSORS];
  float* m[STEP_TENSORS];
  float* v[STEP_TENSORS];
  long long n[STEP_TENSORS];
  int start[STEP_TENSORS + 1];            // first block of tensor t; start[nt] = grid size
};

constexpr int EMA_TENSORS = 72;           // 72 * 52 B + 4 B = 3748 B of table, + 80 B of scalars and pointers

struct EmaStepTable {
  float* p[EMA_TENSORS];
  const float* g[EMA_TENSORS];
  float* m[EMA_TENSORS];
  float* v[EMA_TENSORS];
  float* e[EMA_TENSORS];
  long long n[EMA_TENSORS];
  int start[EMA_TENSORS + 1];
};

struct SumsqTable {
  const float* g[SUMSQ_TENSORS];
  long long n[SUMSQ_TENSORS];
  int start[SUMSQ_TENSORS + 1];
};

static_assert(sizeof(StepTable) + 64 <= 4096 && sizeof(SumsqTable) + 64 <= 4096, "kernel arguments must stay below 4 KB");
static_assert(sizeof(EmaStepTable) + 96 <= 4096, "kernel arguments must stay below 4 KB");

struct AdamwScalars {
  float max_norm, grad_div, lr, beta1, beta2, omb1, omb2, eps, wd, bc1, bc2_sqrt;          // omb = adamw_one_minus(beta)
};

// largest t in [0, nt) with start[t] <= b; tensors of 0 elements own no block (start[t] == start[t + 1]) and are never returned
template <int N>
__device__ __forceinline__ int find_tensor(const int (&start)[N], int nt, int b) {
  int lo = 0, hi = nt;                     // invariant: start[lo] <= b < start[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (start[mid] <= b) lo = mid; else hi = mid;
  }
  return lo;
}

__device__ __forceinline__ bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

__global__ __launch_bounds__(THREADS) void multi_sumsq_kernel(const SumsqTable tab, int nt, float* __restrict__ out) {
  __shared__ float red[THREADS / 64];
  const int t = find_tensor(tab.start, nt, (int)blockIdx.x);
  const long long off = (long long)((int)blockIdx.x - tab.start[t]) * SUMSQ_BLOCK;
  const float* __restrict__ g = tab.g[t] + off;
  const long long rest = tab.n[t] - off;
  const int len = rest < SUMSQ_BLOCK ? (int)rest : SUMSQ_BLOCK;
  float s = 0.f;
  if (aligned16(g)) {
    const int nvec = len >> 2;
    const float4* __restrict__ g4 = reinterpret_cast<const float4*>(g);
    for (int i = threadIdx.x; i < nvec; i += THREADS) {
      const float4 x = g4[i];
      s += x.x * x.x + x.y * x.y + x.z * x.z + x.w * x.w;
    }
    for (int i = (nvec << 2) + threadIdx.x; i < len; i += THREADS) s += g[i] * g[i];
  } else {
    for (int i = threadIdx.x; i < len; i += THREADS) s += g[i] * g[i];
  }
  s = wave_sum64(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) atomicAdd(out, red[0] + red[1] + red[2] + red[3]);
}

// hyper: optional DEVICE {lr, bc1, bc2_sqrt}; when given it replaces the three host scalars, so that a captured launch follows a
// learning-rate schedule and the step count (the host rewrites the three floats before every replay).
// One body for both tables; EMA = true also advances tab.e (adamw_ema_elem) with the weight the step has just produced.
template <bool EMA, class Table>
__device__ __forceinline__ void multi_adamw_body(const Table& tab, int nt, const float* __restrict__ sumsq,
                                                 const int* __restrict__ nonfinite, const float* __restrict__ hyper, AdamwScalars a,
                                                 float decay, float omd) {
  float coef;
  if (!adamw_gate_coef(sumsq, nonfinite, a.max_norm, a.grad_div, coef)) return;
  if (hyper != nullptr) {
    a.lr = hyper[0];
    a.bc1 = hyper[1];
    a.bc2_sqrt = hyper[2];
  }
  const int t = find_tensor(tab.start, nt, (int)blockIdx.x);
  const long long off = (long long)((int)blockIdx.x - tab.start[t]) * STEP_BLOCK;
  float* __restrict__ p = tab.p[t] + off;
  const float* __restrict__ g = tab.g[t] + off;
  float* __restrict__ m = tab.m[t] + off;
  float* __restrict__ v = tab.v[t] + off;
  float* __restrict__ e = nullptr;
  if constexpr (EMA) e = tab.e[t] + off;
  const long long rest = tab.n[t] - off;
  const int len = rest < STEP_BLOCK ? (int)rest : STEP_BLOCK;
  int done = 0;
  bool vec = aligned16(p) && aligned16(g) && aligned16(m) && aligned16(v);
  if constexpr (EMA) vec = vec && aligned16(e);
  if (vec) {
    const int nvec = len >> 2;
    float4* __restrict__ p4 = reinterpret_cast<float4*>(p);
    const float4* __restrict__ g4 = reinterpret_cast<const float4*>(g);
    float4* __restrict__ m4 = reinterpret_cast<float4*>(m);
    float4* __restrict__ v4 = reinterpret_cast<float4*>(v);
    for (int i = threadIdx.x; i < nvec; i += THREADS) {
      float4 pi = p4[i], mi = m4[i], vi = v4[i];
      const float4 gi = g4[i];
      adamw_elem(pi.x, gi.x, mi.x, vi.x, coef, a.lr, a.beta1, a.beta2, a.omb1, a.omb2, a.eps, a.wd, a.bc1, a.bc2_sqrt);
      adamw_elem(pi.y, gi.y, mi.y, vi.y, coef, a.lr, a.beta1, a.beta2, a.omb1, a.omb2, a.eps, a.wd, a.bc1, a.bc2_sqrt);
      adamw_elem(pi.z, gi.z, mi.z, vi.z, coef, a.lr, a.beta1, a.beta2, a.omb1, a.omb2, a.eps, a.wd, a.bc1, a.bc2_sqrt);
      adamw_elem(pi.w, gi.w, mi.w, vi.w, coef, a.lr, a.beta1, a.beta2, a.omb1, a.omb2, a.eps, a.wd, a.bc1, a.bc2_sqrt);
      p4[i] = pi;
      m4[i] = mi;
      v4[i] = vi;
      if constexpr (EMA) {
        float4* __restrict__ e4 = reinterpret_cast<float4*>(e);
        float4 ei = e4[i];
        adamw_ema_elem(ei.x, pi.x, decay, omd);
        adamw_ema_elem(ei.y, pi.y, decay, omd);
        adamw_ema_elem(ei.z, pi.z, decay, omd);
        adamw_ema_elem(ei.w, pi.w, decay, omd);
        e4[i] = ei;
      }
    }
    done = nvec << 2;
  }
  for (int i = done + threadIdx.x; i < len; i += THREADS) {          // scalar tail, or the whole block of an unaligned tensor
    float pi = p[i], mi = m[i], vi = v[i];
    adamw_elem(pi, g[i], mi, vi, coef, a.lr, a.beta1, a.beta2, a.omb1, a.omb2, a.eps, a.wd, a.bc1, a.bc2_sqrt);
    p[i] = pi;
    m[i] = mi;
    v[i] = vi;
    if constexpr (EMA) {
      float ei = e[i];
      adamw_ema_elem(ei, pi, decay, omd);
      e[i] = ei;
    }
  }
}

__global__ __launch_bounds__(THREADS) void multi_adamw_kernel(const StepTable tab, int nt, const float* __restrict__ sumsq,
                                                              const int* __restrict__ nonfinite, const float* __restrict__ hyper,
                                                              AdamwScalars a) {
  multi_adamw_body<false>(tab, nt, sumsq, nonfinite, hyper, a, 0.f, 0.f);
}

__global__ __launch_bounds__(THREADS) void multi_adamw_ema_kernel(const EmaStepTable tab, int nt, const float* __restrict__ sumsq,
                                                                  const int* __restrict__ nonfinite, const float* __restrict__ hyper,
                                                                  AdamwScalars a, float decay, float omd) {
  multi_adamw_body<true>(tab, nt, sumsq, nonfinite, hyper, a, decay, omd);
}

inline long long blocks_of(long long n, int block) { return (n + block - 1) / block; }

}  // namespace

// Callers (api.hip) have validated the lists: non-null entries, 0 <= numel <= 2^34 (so the blocks of a chunk fit an int grid).
int srk_launch_multi_sumsq(const float* const* grads, const long long* numel, int n_tensors, float* out, hipStream_t stream) {
  for (int base = 0; base < n_tensors; base += SUMSQ_TENSORS) {
    const int nt = n_tensors - base < SUMSQ_TENSORS ? n_tensors - base : SUMSQ_TENSORS;
    SumsqTable tab = {};
    long long blocks = 0;
    for (int t = 0; t < nt; ++t) {
      tab.g[t] = grads[base + t];
      tab.n[t] = numel[base + t];
      tab.start[t] = (int)blocks;
      blocks += blocks_of(tab.n[t], SUMSQ_BLOCK);
    }
    tab.start[nt] = (int)blocks;
    if (blocks == 0) continue;
    hipLaunchKernelGGL(multi_sumsq_kernel, dim3((unsigned)blocks), dim3(THREADS), 0, stream, tab, nt, out);
    const int rc = srk_check_launch("multi_sumsq");
    if (rc != SRK_OK) return rc;
  }
  return SRK_OK;
}

int srk_launch_multi_adamw(float* const* p, const float* const* g, float* const* m, float* const* v, const long long* numel, int n_tensors,
                           const float* sumsq, const int* nonfinite, const float* hyper, float max_norm, float grad_div, float lr,
                           float beta1, float beta2, float eps, float wd, int step, hipStream_t stream) {
  AdamwScalars a = {max_norm, grad_div, lr, beta1, beta2, adamw_one_minus(beta1), adamw_one_minus(beta2), eps, wd, 1.f, 1.f};
  adamw_bias_corrections(beta1, beta2, step, &a.bc1, &a.bc2_sqrt);
  for (int base = 0; base < n_tensors; base += STEP_TENSORS) {
    const int nt = n_tensors - base < STEP_TENSORS ? n_tensors - base : STEP_TENSORS;
    StepTable tab = {};
    long long blocks = 0;
    for (int t = 0; t < nt; ++t) {
      tab.p[t] = p[base + t];
      tab.g[t] = g[base + t];
      tab.m[t] = m[base + t];
      tab.v[t] = v[base + t];
      tab.n[t] = numel[base + t];
      tab.start[t] = (int)blocks;
      blocks += blocks_of(tab.n[t], STEP_BLOCK);
    }
    tab.start[nt] = (int)blocks;
    if (blocks == 0) continue;
    hipLaunchKernelGGL(multi_adamw_kernel, dim3((unsigned)blocks), dim3(THREADS), 0, stream, tab, nt, sumsq, nonfinite, hyper, a);
    const int rc = srk_check_launch("multi_adamw");
    if (rc != SRK_OK) return rc;
  }
  return SRK_OK;
}

int srk_launch_multi_adamw_ema(float* const* p, const float* const* g, float* const* m, float* const* v, float* const* e,
                               const long long* numel, int n_tensors, const float* sumsq, const int* nonfinite, const float* hyper,
                               float max_norm, float grad_div, float lr, float beta1, float beta2, float eps, float wd, int step,
                               float ema_decay, hipStream_t stream) {
  AdamwScalars a = {max_norm, grad_div, lr, beta1, beta2, adamw_one_minus(beta1), adamw_one_minus(beta2), eps, wd, 1.f, 1.f};
  adamw_bias_corrections(beta1, beta2, step, &a.bc1, &a.bc2_sqrt);
  const float omd = adamw_one_minus(ema_decay);
  for (int base = 0; base < n_tensors; base += EMA_TENSORS) {
    const int nt = n_tensors - base < EMA_TENSORS ? n_tensors - base : EMA_TENSORS;
    EmaStepTable tab = {};
    long long blocks = 0;
    for (int t = 0; t < nt; ++t) {
      tab.p[t] = p[base + t];
      tab.g[t] = g[base + t];
      tab.m[t] = m[base + t];
      tab.v[t] = v[base + t];
      tab.e[t] = e[base + t];
      tab.n[t] = numel[base + t];
      tab.start[t] = (int)blocks;
      blocks += blocks_of(tab.n[t], STEP_BLOCK);
    }
    tab.start[nt] = (int)blocks;
    if (blocks == 0) continue;
    hipLaunchKernelGGL(multi_adamw_ema_kernel, dim3((unsigned)blocks), dim3(THREADS), 0, stream, tab, nt, sumsq, nonfinite, hyper, a,
                       ema_decay, omd);
    const int rc = srk_check_launch("multi_adamw_ema");
    if (rc != SRK_OK) return rc;
  }
  return SRK_OK;
}
