// Edge values for the host argument predicates of srk_filter2d_f32 / srk_resize_aa_ragged_f32 / srk_jpeg_roundtrip_ragged_f32 / srk_crop_u8
// (csrc/common.h: srk_filter2d_shape_ok, srk_resize_ragged_shape_ok, srk_ragged_extent_ok, srk_resize_factor_ok, and srk_ranges_overlap on
// the byte counts those entries form), as a stand-alone program for a sanitizer build; needs no GPU:
//   hipcc --offload-arch=gfx950 --cuda-host-only -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined tools/degrade2_predicates_check.hip -o /tmp/degrade2_predicates_check && /tmp/degrade2_predicates_check
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

int main() {
  // the filter: the shapes of the blur, and both padded extents above R = ks / 2
  EXPECT(srk_filter2d_shape_ok(1, 1, 1, 1, 1) && srk_filter2d_shape_ok(4, 3, 40, 72, 21) && srk_filter2d_shape_ok(65535, 3, 2048, 2048, 21));
  EXPECT(srk_filter2d_shape_ok(1, 1, 11, 11, 21) && !srk_filter2d_shape_ok(1, 1, 10, 11, 21) && !srk_filter2d_shape_ok(1, 1, 11, 10, 21));
  EXPECT(srk_filter2d_shape_ok(1, 1, 2, 2, 3) && !srk_filter2d_shape_ok(1, 1, 1, 2, 3) && !srk_filter2d_shape_ok(1, 1, 2, 1, 3));
  for (int ks = 0; ks <= 22; ks += 2) EXPECT(!srk_filter2d_shape_ok(1, 1, 64, 64, ks));
  EXPECT(!srk_filter2d_shape_ok(1, 1, 64, 64, 23) && !srk_filter2d_shape_ok(1, 1, 64, 64, -1) && !srk_filter2d_shape_ok(1, 1, 64, 64, INT_MIN) && !srk_filter2d_shape_ok(1, 1, 64, 64, INT_MAX));
  EXPECT(!srk_filter2d_shape_ok(0, 1, 64, 64, 7) && !srk_filter2d_shape_ok(1, 0, 64, 64, 7) && !srk_filter2d_shape_ok(1, 1, 0, 64, 7) && !srk_filter2d_shape_ok(1, 1, 64, 0, 7));
  EXPECT(!srk_filter2d_shape_ok(-1, 1, 64, 64, 7) && !srk_filter2d_shape_ok(1, 1, INT_MIN, 64, 7) && !srk_filter2d_shape_ok(1, 1, 64, INT_MIN, 1));
  EXPECT(srk_filter2d_shape_ok(INT_MAX, 1, 1, 1, 1) && !srk_filter2d_shape_ok(INT_MAX, 2, 1, 1, 1) && srk_filter2d_shape_ok(1, 1, INT_MAX, 1000000000, 21));
  EXPECT(!srk_filter2d_shape_ok(1, 1, INT_MAX, 1100000000, 21) && !srk_filter2d_shape_ok(INT_MAX, 1, INT_MAX, INT_MAX, 1));
  // the ragged resize: both padded shapes
  EXPECT(srk_resize_ragged_shape_ok(4, 3, 40, 72, 60, 108) && srk_resize_ragged_shape_ok(1, 1, 1, 1, 1, 1) && srk_resize_ragged_shape_ok(1, 1, INT_MAX, 1, 1, INT_MAX));
  EXPECT(!srk_resize_ragged_shape_ok(0, 3, 40, 72, 60, 108) && !srk_resize_ragged_shape_ok(4, 0, 40, 72, 60, 108) && !srk_resize_ragged_shape_ok(4, 3, 0, 72, 60, 108));
  EXPECT(!srk_resize_ragged_shape_ok(4, 3, 40, 0, 60, 108) && !srk_resize_ragged_shape_ok(4, 3, 40, 72, 0, 108) && !srk_resize_ragged_shape_ok(4, 3, 40, 72, 60, 0));
  EXPECT(!srk_resize_ragged_shape_ok(4, 3, 40, 72, -60, 108) && !srk_resize_ragged_shape_ok(4, 3, INT_MIN, 72, 60, 108) && !srk_resize_ragged_shape_ok(1, 1, 1, 1, INT_MAX, 1100000000));
  EXPECT(!srk_resize_ragged_shape_ok(1, 1, INT_MAX, 1100000000, 1, 1) && !srk_resize_ragged_shape_ok(INT_MAX, 2, 1, 1, 1, 1));
  // one sample's extents, and its resize against the 33-tap rows (8x)
  EXPECT(srk_ragged_extent_ok(1, 1, 1, 1) && srk_ragged_extent_ok(40, 72, 40, 72) && srk_ragged_extent_ok(12, 11, 40, 72));
  EXPECT(!srk_ragged_extent_ok(0, 1, 40, 72) && !srk_ragged_extent_ok(1, 0, 40, 72) && !srk_ragged_extent_ok(41, 72, 40, 72) && !srk_ragged_extent_ok(40, 73, 40, 72));
  EXPECT(!srk_ragged_extent_ok(-1, 1, 40, 72) && !srk_ragged_extent_ok(INT_MIN, INT_MIN, 40, 72) && !srk_ragged_extent_ok(INT_MAX, INT_MAX, 40, 72));
  EXPECT(srk_resize_factor_ok(8, 1) && !srk_resize_factor_ok(9, 1) && srk_resize_factor_ok(1, INT_MAX) && srk_resize_factor_ok(INT_MAX, INT_MAX));
  EXPECT(srk_resize_factor_ok(INT_MAX, 268435456) && !srk_resize_factor_ok(INT_MAX, 268435455));          // 8 n_out is formed in 64 bits
  EXPECT(!srk_resize_factor_ok(0, 1) && !srk_resize_factor_ok(1, 0) && !srk_resize_factor_ok(-8, -1) && !srk_resize_factor_ok(INT_MIN, 1));
  // the JPEG stage takes the shapes of the noise stage
  EXPECT(srk_noise_shape_ok(4, 3, 40, 72) && srk_noise_shape_ok(4, 1, 40, 72) && !srk_noise_shape_ok(4, 2, 40, 72) && srk_flag01_ok(1) && !srk_flag01_ok(2));
  // what passes gives byte counts that fit a size_t
  EXPECT(image_bytes(4, 3, 40, 72) == 4u * 4 * 3 * 40 * 72 && image_bytes(INT_MAX, 1, 1, 1) == 4ull * INT_MAX && ext_bytes(INT_MAX) == 8ull * INT_MAX);
  // overlap of the operands as api.hip asks: out against x, against the tables, against ext; real storage, every offset in range
  std::vector<float> buf(8192);
  const float* x = buf.data();
  const size_t n = image_bytes(1, 2, 16, 24), kb = sizeof(float) * 1 * 21 * 21, eb = ext_bytes(1);
  EXPECT(srk_ranges_overlap(x, n, x, n) && srk_ranges_overlap(x, n, x + 2 * 16 * 24 - 1, n) && !srk_ranges_overlap(x, n, x + 2 * 16 * 24, n));
  EXPECT(srk_ranges_overlap(x + 440, n, x, kb) && !srk_ranges_overlap(x + 441, n, x, kb));
  EXPECT(srk_ranges_overlap(x + 1, n, x, eb) && !srk_ranges_overlap(x + 2, n, x, eb) && !srk_ranges_overlap(nullptr, 0, x, n));          // a null ext has no bytes
  const size_t nb = image_bytes(1, 2, 8, 12);          // the two sides of a resize have different sizes
  EXPECT(srk_ranges_overlap(x, n, x + 2 * 16 * 24 - 1, nb) && !srk_ranges_overlap(x, n, x + 2 * 16 * 24, nb) && srk_ranges_overlap(x + 2 * 8 * 12 - 1, n, x, nb) &&
         !srk_ranges_overlap(x + 2 * 8 * 12, n, x, nb));
  printf("%d failure(s)\n", failures);
  return failures != 0;
}
