// Edge values for the host argument predicates of srk_noise_f32 / srk_crop_restore_u8 (csrc/common.h: srk_noise_shape_ok,
// srk_crop_restore_shape_ok, srk_flag01_ok, srk_quant_bits_ok, and srk_ranges_overlap on the byte counts those entries form), as a
// stand-alone program for a sanitizer build; needs no GPU:
//   hipcc --offload-arch=gfx950 --cuda-host-only -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined tools/restore_predicates_check.hip -o /tmp/restore_predicates_check && /tmp/restore_predicates_check
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

// the byte counts the two entries form AFTER their shape checks passed: they must not wrap
static size_t image_bytes(int B, int C, int H, int W) { return (size_t)(4.0 * B * C * H * W); }
static size_t patch_bytes(int B, int out_chans, int patch) { return sizeof(float) * (size_t)B * out_chans * patch * patch; }
// the grid of srk_crop_restore_u8's launcher: tiles at the worst phase of (top, left), one grid row per sample
static long long restore_tiles(int P) { return (long long)((P + 14) / 16 + 1) * ((P + 30) / 32 + 1); }

int main() {
  // srk_noise_f32: every extent >= 1, C in {1, 3}, the planes index an int, the bytes stay below 2^63
  EXPECT(srk_noise_shape_ok(1, 1, 1, 1) && srk_noise_shape_ok(5, 3, 45, 61) && srk_noise_shape_ok(65535, 3, 2048, 2048));
  EXPECT(!srk_noise_shape_ok(0, 1, 1, 1) && !srk_noise_shape_ok(1, 1, 0, 1) && !srk_noise_shape_ok(1, 1, 1, 0) && !srk_noise_shape_ok(-1, 3, 4, 4));
  EXPECT(!srk_noise_shape_ok(1, 0, 1, 1) && !srk_noise_shape_ok(1, 2, 1, 1) && !srk_noise_shape_ok(1, 4, 1, 1) && !srk_noise_shape_ok(1, -3, 1, 1) && !srk_noise_shape_ok(1, INT_MAX, 1, 1));
  EXPECT(!srk_noise_shape_ok(1, 1, INT_MIN, 1) && !srk_noise_shape_ok(INT_MIN, 1, 1, 1) && !srk_noise_shape_ok(1, 3, -3, -3));
  EXPECT(srk_noise_shape_ok(INT_MAX, 1, 1, 1) && !srk_noise_shape_ok(INT_MAX, 3, 1, 1) && srk_noise_shape_ok(715827882, 3, 1, 1) && !srk_noise_shape_ok(715827883, 3, 1, 1));
  EXPECT(srk_noise_shape_ok(1, 1, INT_MAX, 1000000000) && !srk_noise_shape_ok(1, 1, INT_MAX, 1100000000) && !srk_noise_shape_ok(1, 3, INT_MAX, INT_MAX));
  EXPECT(image_bytes(1, 1, 1, 1) == 4 && image_bytes(5, 3, 45, 61) == 4u * 5 * 3 * 45 * 61 && image_bytes(INT_MAX, 1, 1, 1) == 4ull * INT_MAX);
  EXPECT(image_bytes(1, 1, INT_MAX, 1000000000) < (size_t)1 << 63);
  // srk_crop_restore_u8: B 1..65535, patch 1..2048, out_chans 1 | 3
  EXPECT(srk_crop_restore_shape_ok(1, 1, 1) && srk_crop_restore_shape_ok(65535, 2048, 3) && srk_crop_restore_shape_ok(5, 32, 1));
  EXPECT(!srk_crop_restore_shape_ok(0, 32, 3) && !srk_crop_restore_shape_ok(65536, 32, 3) && !srk_crop_restore_shape_ok(-1, 32, 3) && !srk_crop_restore_shape_ok(INT_MIN, 32, 3) && !srk_crop_restore_shape_ok(INT_MAX, 32, 3));
  EXPECT(!srk_crop_restore_shape_ok(5, 0, 3) && !srk_crop_restore_shape_ok(5, 2049, 3) && !srk_crop_restore_shape_ok(5, -32, 3) && !srk_crop_restore_shape_ok(5, INT_MAX, 3) && !srk_crop_restore_shape_ok(5, INT_MIN, 3));
  EXPECT(!srk_crop_restore_shape_ok(5, 32, 0) && !srk_crop_restore_shape_ok(5, 32, 2) && !srk_crop_restore_shape_ok(5, 32, 4) && !srk_crop_restore_shape_ok(5, 32, -1) && !srk_crop_restore_shape_ok(5, 32, INT_MAX) && !srk_crop_restore_shape_ok(5, 32, INT_MIN));
  EXPECT(srk_flag01_ok(0) && srk_flag01_ok(1) && !srk_flag01_ok(2) && !srk_flag01_ok(-1) && !srk_flag01_ok(INT_MAX) && !srk_flag01_ok(INT_MIN));
  EXPECT(srk_quant_bits_ok(0) && srk_quant_bits_ok(8) && !srk_quant_bits_ok(1) && !srk_quant_bits_ok(7) && !srk_quant_bits_ok(16) && !srk_quant_bits_ok(-8) && !srk_quant_bits_ok(INT_MAX) && !srk_quant_bits_ok(INT_MIN));
  // what passes gives byte counts and a grid that fit: the largest batch is 4 * 65535 * 3 * 2048^2 bytes and 129 * 65 tiles per sample
  EXPECT(patch_bytes(1, 1, 1) == 4 && patch_bytes(65535, 3, 2048) == 4ull * 65535 * 3 * 2048 * 2048 && patch_bytes(65535, 3, 2048) < (size_t)1 << 42);
  EXPECT(restore_tiles(1) == 1 && restore_tiles(2) == 4 && restore_tiles(16) == 2 * 2 && restore_tiles(17) == 2 * 2 && restore_tiles(18) == 3 * 2 && restore_tiles(34) == 4 * 3);
  EXPECT(restore_tiles(2048) == 129ll * 65 && restore_tiles(2048) <= INT_MAX);
  // overlap of the operands as api.hip asks: out against x (noise), clean_out against degraded_out (crop_restore); real storage
  std::vector<float> buf(8192);
  const float* x = buf.data();
  const size_t n = image_bytes(1, 3, 16, 24);
  EXPECT(srk_ranges_overlap(x, n, x, n) && srk_ranges_overlap(x, n, x + 3 * 16 * 24 - 1, n) && !srk_ranges_overlap(x, n, x + 3 * 16 * 24, n));
  const size_t p = patch_bytes(2, 3, 20);
  EXPECT(srk_ranges_overlap(x, p, x + 1, p) && srk_ranges_overlap(x + 2 * 3 * 400 - 1, p, x, p) && !srk_ranges_overlap(x + 2 * 3 * 400, p, x, p));
  printf("%d failure(s)\n", failures);
  return failures != 0;
}
