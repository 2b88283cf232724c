// Edge values for the host argument predicates of srk_usm_sharpen_f32 / srk_resize_ragged_mode_f32 (csrc/common.h: srk_usm_ks_ok,
// srk_usm_shape_ok, srk_usm_extent_ok, srk_resize_ragged_shape_ok, srk_resize_factor_ok, srk_quant_bits_ok, and srk_ranges_overlap on the
// byte counts those entries form), as a stand-alone program for a sanitizer build; needs no GPU:
//   hipcc --offload-arch=gfx950 --cuda-host-only -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined tools/usm_predicates_check.hip -o /tmp/usm_predicates_check && /tmp/usm_predicates_check
#include <limits.h>
#include <stdio.h>

#include <vector>

#include "../tpu_superresolution_amd/csrc/common.h"

static int failures = 0;
#define EXPECT(cond)                                      \
  do {                                                    \
    const bool ok_ = (cond);                              \
    printf("%s  %s\n", ok_ ? "ok  " : "FAIL", #cond);     \
    failures += !ok_;                                     \
  } while (0)

// the byte counts the entries form AFTER their shape checks passed: they must not wrap
static size_t image_bytes(int B, int C, int H, int W) { return (size_t)(4.0 * B * C * H * W); }
static size_t ext_bytes(int B) { return sizeof(int) * 2 * (size_t)B; }
static size_t mode_bytes(int B) { return ext_bytes(B) / 2; }

int main() {
  // the taps: odd, 1..51
  EXPECT(srk_usm_ks_ok(1) && srk_usm_ks_ok(3) && srk_usm_ks_ok(21) && srk_usm_ks_ok(51) && SRK_USM_MAX_KS == 51);
  for (int ks = 0; ks <= 52; ks += 2) EXPECT(!srk_usm_ks_ok(ks));
  EXPECT(!srk_usm_ks_ok(53) && !srk_usm_ks_ok(-1) && !srk_usm_ks_ok(-51) && !srk_usm_ks_ok(INT_MIN) && !srk_usm_ks_ok(INT_MAX));
  // the shapes: those of the noise stage, C 1 or 3
  EXPECT(srk_usm_shape_ok(2, 3, 26, 27, 51) && srk_usm_shape_ok(2, 1, 26, 27, 51) && srk_usm_shape_ok(1, 1, 1, 1, 1) && srk_usm_shape_ok(65535, 3, 2048, 2048, 51));
  EXPECT(!srk_usm_shape_ok(2, 2, 26, 27, 51) && !srk_usm_shape_ok(2, 4, 26, 27, 51) && !srk_usm_shape_ok(2, 0, 26, 27, 51));
  EXPECT(!srk_usm_shape_ok(0, 3, 26, 27, 51) && !srk_usm_shape_ok(2, 3, 0, 27, 51) && !srk_usm_shape_ok(2, 3, 26, 0, 51) && !srk_usm_shape_ok(-1, 3, 26, 27, 51));
  EXPECT(!srk_usm_shape_ok(2, 3, INT_MIN, 27, 51) && !srk_usm_shape_ok(2, 3, 26, INT_MIN, 51) && !srk_usm_shape_ok(2, 3, 26, 27, 50) && !srk_usm_shape_ok(2, 3, 26, 27, 53));
  EXPECT(srk_usm_shape_ok(INT_MAX, 1, 1, 1, 1) && !srk_usm_shape_ok(INT_MAX, 3, 1, 1, 1) && srk_usm_shape_ok(1, 1, INT_MAX, 1000000000, 51));
  EXPECT(!srk_usm_shape_ok(1, 1, INT_MAX, 1100000000, 51) && !srk_usm_shape_ok(INT_MAX, 1, INT_MAX, INT_MAX, 1));
  // both extents above R = ks / 2
  EXPECT(srk_usm_extent_ok(26, 26, 51) && !srk_usm_extent_ok(25, 26, 51) && !srk_usm_extent_ok(26, 25, 51) && srk_usm_extent_ok(1, 1, 1));
  EXPECT(srk_usm_extent_ok(2, 2, 3) && !srk_usm_extent_ok(1, 2, 3) && !srk_usm_extent_ok(2, 1, 3) && srk_usm_extent_ok(INT_MAX, INT_MAX, 51));
  EXPECT(!srk_usm_extent_ok(0, 0, 1) && !srk_usm_extent_ok(INT_MIN, 26, 51));
  // the ragged resize with modes: the shapes and the 8x limit of srk_resize_aa_ragged_f32
  EXPECT(srk_resize_ragged_shape_ok(4, 3, 40, 72, 60, 108) && srk_resize_ragged_shape_ok(1, 1, 1, 1, 1, 1) && !srk_resize_ragged_shape_ok(0, 3, 40, 72, 60, 108));
  EXPECT(!srk_resize_ragged_shape_ok(4, 3, 40, 72, 0, 108) && !srk_resize_ragged_shape_ok(4, 3, 40, 72, 60, -1) && !srk_resize_ragged_shape_ok(INT_MAX, 2, 1, 1, 1, 1));
  EXPECT(srk_resize_factor_ok(8, 1) && !srk_resize_factor_ok(9, 1) && srk_resize_factor_ok(72, 9) && !srk_resize_factor_ok(73, 9) && srk_resize_factor_ok(1, INT_MAX));
  EXPECT(srk_resize_factor_ok(INT_MAX, 268435456) && !srk_resize_factor_ok(INT_MAX, 268435455) && !srk_resize_factor_ok(0, 1) && !srk_resize_factor_ok(INT_MIN, 1));
  EXPECT(srk_quant_bits_ok(0) && srk_quant_bits_ok(8) && !srk_quant_bits_ok(4) && !srk_quant_bits_ok(-8) && !srk_quant_bits_ok(INT_MIN));
  // what passes gives byte counts that fit a size_t
  EXPECT(image_bytes(2, 3, 26, 27) == 4u * 2 * 3 * 26 * 27 && image_bytes(INT_MAX, 1, 1, 1) == 4ull * INT_MAX && mode_bytes(INT_MAX) == 4ull * INT_MAX);
  EXPECT(SRK_USM_WORK_FLOATS(2, 3, 26, 27) == 2u * 3 * 26 * 27 && SRK_USM_WORK_FLOATS(INT_MAX, 1, INT_MAX, 1) == (size_t)INT_MAX * INT_MAX);
  // overlap of the operands as api.hip asks: x, out, work pairwise, taps against out and work, mode against out; real storage
  std::vector<float> buf(8192);
  const float* x = buf.data();
  const size_t n = image_bytes(1, 3, 16, 24), kb = sizeof(float) * 51, mb = mode_bytes(2);
  EXPECT(srk_ranges_overlap(x, n, x, n) && srk_ranges_overlap(x, n, x + 3 * 16 * 24 - 1, n) && !srk_ranges_overlap(x, n, x + 3 * 16 * 24, n));
  EXPECT(srk_ranges_overlap(x + 50, n, x, kb) && !srk_ranges_overlap(x + 51, n, x, kb) && srk_ranges_overlap(x, kb, x + 50, n) && !srk_ranges_overlap(x, kb, x + 51, n));
  EXPECT(srk_ranges_overlap(x + 1, n, x, mb) && !srk_ranges_overlap(x + 2, n, x, mb) && !srk_ranges_overlap(nullptr, 0, x, n));          // a null mode has no bytes
  EXPECT(!srk_ranges_overlap(x, 0, x, n) && !srk_ranges_overlap(x, n, x, 0));
  printf("%d failure(s)\n", failures);
  return failures != 0;
}
