// global-norm clip + AdamW: the gate, the clip coefficient and the per-element update, shared by the flat-range kernel
// (misc.hip: adamw_kernel, SwinIR's flat fp32 buffer) and the multi-tensor kernel (optim_multi.hip: lists of separate tensors),
// so that the two paths cannot drift.  Both functions pin floating-point contraction OFF: whether a * b + c becomes one fma is otherwise
// the optimizer's choice per call site, and the flat and the multi-tensor kernel must round alike (their results are compared bit for
// bit).  The one fused operation is written out (the decay factor).  Division and sqrtf are
// the correctly rounded forms in both.  Semantics: torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW
// (finetune_swinir.py:168-171, :303).
#pragma once
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include "common.h"

// Host: a beta that crossed the C ABI as fp32, as the decimal the caller wrote.  The betas are short decimals (0.9, 0.999) and fp32
// cannot hold them: fp32(0.999) = 0.99900001287, so 1.0f - beta = 0.00099998713, 1.3e-5 below 0.001 in relative terms (2.4e-7 for
// 0.9); every element of a moment carried that offset, and so did the bias corrections.  torch forms 1 - beta and 1 - beta^step in
// fp64 from the decimal and rounds once.  So does this: the shortest decimal that rounds to the given float is recovered, and the
// host-side factors below are computed from it in fp64.  (beta itself multiplies the old moment as the fp32 it is, as in torch.)
inline double adamw_decimal(float beta) {
  char buf[32];
  for (int prec = 1; prec <= 9; ++prec) {
    snprintf(buf, sizeof(buf), "%.*g", prec, (double)beta);
    if (strtof(buf, nullptr) == beta) break;          // 9 significant digits always round-trip an fp32
  }
  return strtod(buf, nullptr);
}

inline float adamw_one_minus(float beta) { return (float)(1.0 - adamw_decimal(beta)); }

// Host: bias corrections of the 1-based step, as the kernels take them (bc1 = 1 - beta1^step, bc2_sqrt = sqrt(1 - beta2^step)).
inline void adamw_bias_corrections(float beta1, float beta2, int step, float* bc1, float* bc2_sqrt) {
  *bc1 = (float)(1.0 - pow(adamw_decimal(beta1), (double)step));
  *bc2_sqrt = (float)sqrt(1.0 - pow(adamw_decimal(beta2), (double)step));
}

// false: the step is gated off and params and both moments stay untouched -- a non-finite forward (counter of the loss kernel) or a
// non-finite gradient norm; the reference raises before backward/step (finetune_swinir.py:159-165), so the model must survive for
// that raise.  true: coef = (1 / grad_div) * min(1, max_norm / (norm + 1e-6)) multiplies every gradient element.
__device__ __forceinline__ bool adamw_gate_coef(const float* __restrict__ sumsq, const int* __restrict__ nonfinite, float max_norm,
                                                float grad_div, float& coef) {
#pragma clang fp contract(off)
  if (nonfinite != nullptr && *nonfinite != 0) return false;
  coef = 1.0f / grad_div;
  if (sumsq != nullptr) {
    const float ss = *sumsq;
    if (!(ss == ss) || ss > 3.0e38f) return false;
    if (max_norm > 0.f) {
      const float total = sqrtf(ss) / grad_div;
      const float c = max_norm / (total + 1e-6f);
      coef *= c < 1.0f ? c : 1.0f;
    }
  }
  return true;
}

__device__ __forceinline__ void adamw_elem(float& p, float g, float& m, float& v, float coef, float lr, float beta1, float beta2,
                                           float omb1, float omb2, float eps, float wd, float bc1, float bc2_sqrt) {
#pragma clang fp contract(off)
  const float gi = g * coef;
  float pi = p * __builtin_fmaf(-lr, wd, 1.0f);          // 1 - lr * wd in one rounding: the form the flat kernel has always computed
  const float mi = beta1 * m + omb1 * gi;          // omb = adamw_one_minus(beta), from the host
  const float vi = beta2 * v + omb2 * gi * gi;
  const float denom = sqrtf(vi) / bc2_sqrt + eps;
  pi -= (lr / bc1) * (mi / denom);
  p = pi;
  m = mi;
  v = vi;
}

// Exponential moving average of the weights, folded into the step: p_new is the value adamw_elem has just produced (still in a
// register).  omd = adamw_one_minus(decay), from the host, as for the betas: fp32(0.999) puts 1 - decay 1.3e-5 off.  decay itself
// multiplies the old average as the fp32 it is.  Two products and one sum, each rounded on its own.
__device__ __forceinline__ void adamw_ema_elem(float& e, float p_new, float decay, float omd) {
#pragma clang fp contract(off)
  e = decay * e + omd * p_new;
}
