// The ragged batch of include/srk.h ("Ragged batches"): one padded fp32 buffer [B][C][Hp][Wp], sample b in the top-left h_b x w_b of each
// of its planes at row pitch Wp, ext = DEVICE int32 [B][2] = (h_b, w_b) or NULL for a dense batch.  Shared by filter2d.hip and ragged.hip.
#pragma once
#include "kernels.h"

namespace {

// extent k (0 = rows, 1 = columns) of sample b: any bit pattern is clamped into 1..n, so a kernel stays inside its buffers whatever ext holds
__device__ __forceinline__ int rg_extent(const int* __restrict__ ext, int b, int k, int n) {
  if (!ext) return n;
  const int v = ext[2 * b + k];
  return v < 1 ? 1 : (v > n ? n : v);
}

}  // namespace
