// Edge values for the host argument predicates of srk_blur2d_f32 / srk_crop_degrade_psf_u8 (csrc/common.h: srk_psf_ks_ok,
// srk_blur2d_shape_ok, srk_crop_degrade_shape_ok, and srk_ranges_overlap on the byte counts those entries form), as a stand-alone program
// for a sanitizer build; needs no GPU:
//   hipcc --offload-arch=gfx950 --cuda-host-only -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined tools/psf_predicates_check.hip -o /tmp/psf_predicates_check && /tmp/psf_predicates_check
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

// the byte counts srk_blur2d_f32 forms AFTER its shape checks passed: they must not wrap
static size_t image_bytes(int B, int C, int H, int W) { return (size_t)(4.0 * B * C * H * W); }
static size_t table_bytes(int B, int ks) { return sizeof(float) * (size_t)B * ks * ks; }

int main() {
  // the table side: odd, 1..21
  for (int ks = 1; ks <= 21; ks += 2) EXPECT(srk_psf_ks_ok(ks));
  for (int ks = 0; ks <= 22; ks += 2) EXPECT(!srk_psf_ks_ok(ks));
  EXPECT(!srk_psf_ks_ok(23) && !srk_psf_ks_ok(-1) && !srk_psf_ks_ok(-21) && !srk_psf_ks_ok(INT_MAX) && !srk_psf_ks_ok(INT_MIN) && !srk_psf_ks_ok(INT_MIN + 1));
  // image shapes: every extent >= 1, the planes index an int, the bytes stay below 2^63
  EXPECT(srk_blur2d_shape_ok(1, 1, 1, 1) && srk_blur2d_shape_ok(2, 3, 45, 61) && srk_blur2d_shape_ok(65535, 3, 2048, 2048));
  EXPECT(!srk_blur2d_shape_ok(0, 1, 1, 1) && !srk_blur2d_shape_ok(1, 0, 1, 1) && !srk_blur2d_shape_ok(1, 1, 0, 1) && !srk_blur2d_shape_ok(1, 1, 1, 0));
  EXPECT(!srk_blur2d_shape_ok(-1, 1, 1, 1) && !srk_blur2d_shape_ok(1, 1, INT_MIN, 1) && !srk_blur2d_shape_ok(1, -3, -3, 1));
  EXPECT(srk_blur2d_shape_ok(INT_MAX, 1, 1, 1) && srk_blur2d_shape_ok(1, INT_MAX, 1, 1) && !srk_blur2d_shape_ok(INT_MAX, 2, 1, 1) && !srk_blur2d_shape_ok(65536, 32768, 1, 1));
  EXPECT(srk_blur2d_shape_ok(1, 1, INT_MAX, 1) && srk_blur2d_shape_ok(1, 1, INT_MAX, 1000000000));          // 8.59e18 bytes: below 9.0e18 < 2^63
  EXPECT(!srk_blur2d_shape_ok(1, 1, INT_MAX, 1100000000) && !srk_blur2d_shape_ok(1, 1, INT_MAX, INT_MAX) && !srk_blur2d_shape_ok(INT_MAX, 1, INT_MAX, INT_MAX));
  // what passes gives byte counts that fit a size_t, with room for the address arithmetic of srk_ranges_overlap
  EXPECT(image_bytes(1, 1, 1, 1) == 4 && image_bytes(2, 3, 45, 61) == 4u * 2 * 3 * 45 * 61 && image_bytes(INT_MAX, 1, 1, 1) == 4ull * INT_MAX);
  EXPECT(table_bytes(1, 1) == 4 && table_bytes(65535, 21) == 4ull * 65535 * 441 && table_bytes(INT_MAX, 21) == 4ull * INT_MAX * 441);
  // overlap of the operands of srk_blur2d_f32 as api.hip asks: out against x, out against psf; real storage, every offset in range
  std::vector<float> buf(4096);
  const float* x = buf.data();
  const size_t n = image_bytes(1, 2, 16, 24), kb = table_bytes(1, 21);
  EXPECT(srk_ranges_overlap(x, n, x, n) && srk_ranges_overlap(x, n, x + 2 * 16 * 24 - 1, n) && !srk_ranges_overlap(x, n, x + 2 * 16 * 24, n));
  EXPECT(srk_ranges_overlap(x + 2 * 16 * 24 - 1, kb, x, n) && !srk_ranges_overlap(x + 2 * 16 * 24, kb, x, n) && !srk_ranges_overlap(x, kb, x + 441, n));
  EXPECT(srk_ranges_overlap(x + 440, n, x, kb) && !srk_ranges_overlap(x + 441, n, x, kb));
  // the batch shapes of the crop + degrade entries
  EXPECT(srk_crop_degrade_shape_ok(1, 1, 2) && srk_crop_degrade_shape_ok(65535, 2048, 4) && srk_crop_degrade_shape_ok(5, 72, 3));
  EXPECT(!srk_crop_degrade_shape_ok(0, 72, 2) && !srk_crop_degrade_shape_ok(65536, 72, 2) && !srk_crop_degrade_shape_ok(-1, 72, 2) && !srk_crop_degrade_shape_ok(INT_MIN, 72, 2));
  EXPECT(!srk_crop_degrade_shape_ok(5, 0, 2) && !srk_crop_degrade_shape_ok(5, 2049, 2) && !srk_crop_degrade_shape_ok(5, -72, 2) && !srk_crop_degrade_shape_ok(5, INT_MAX, 2));
  EXPECT(!srk_crop_degrade_shape_ok(5, 72, 1) && !srk_crop_degrade_shape_ok(5, 72, 5) && !srk_crop_degrade_shape_ok(5, 72, 0) && !srk_crop_degrade_shape_ok(5, 72, -2) && !srk_crop_degrade_shape_ok(5, 72, INT_MAX));
  printf("%d failure(s)\n", failures);
  return failures != 0;
}
