// Edge values for the host argument predicates of srk_kernel_tables_f32 (csrc/common.h: srk_tables_shape_ok, srk_tables_bytes, and
// srk_ranges_overlap on the byte counts the entry forms), as a stand-alone program for a sanitizer build; needs no GPU:
//   hipcc --offload-arch=gfx950 --cuda-host-only -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined tools/tables_predicates_check.hip -o /tmp/tables_predicates_check && /tmp/tables_predicates_check
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

int main() {
  // n tables of side ks, no bank
  EXPECT(srk_tables_shape_ok(1, 1, false, 0, 0) && srk_tables_shape_ok(32, 21, false, 0, 0) && srk_tables_shape_ok(INT_MAX, 21, false, 0, 0));
  EXPECT(!srk_tables_shape_ok(0, 7, false, 0, 0) && !srk_tables_shape_ok(-1, 7, false, 0, 0) && !srk_tables_shape_ok(INT_MIN, 7, false, 0, 0));
  for (int ks = 0; ks <= 22; ks += 2) EXPECT(!srk_tables_shape_ok(1, ks, false, 0, 0));
  for (int ks = 1; ks <= 21; ks += 2) EXPECT(srk_tables_shape_ok(1, ks, false, 0, 0));
  EXPECT(!srk_tables_shape_ok(1, 23, false, 0, 0) && !srk_tables_shape_ok(1, -1, false, 0, 0) && !srk_tables_shape_ok(1, -7, false, 0, 0) &&
         !srk_tables_shape_ok(1, INT_MIN, false, 0, 0) && !srk_tables_shape_ok(1, INT_MAX, false, 0, 0));
  // the bank triple: all absent, or a pointer with n_bank >= 1 and kb odd in 1..ks
  EXPECT(!srk_tables_shape_ok(1, 7, false, 1, 5) && !srk_tables_shape_ok(1, 7, false, 0, 5) && !srk_tables_shape_ok(1, 7, false, 1, 0) &&
         !srk_tables_shape_ok(1, 7, false, -1, 0) && !srk_tables_shape_ok(1, 7, false, 0, -1));
  EXPECT(srk_tables_shape_ok(1, 7, true, 1, 1) && srk_tables_shape_ok(1, 7, true, 1, 7) && srk_tables_shape_ok(4, 21, true, INT_MAX, 21) &&
         srk_tables_shape_ok(1, 1, true, 1, 1));
  EXPECT(!srk_tables_shape_ok(1, 7, true, 0, 5) && !srk_tables_shape_ok(1, 7, true, -1, 5) && !srk_tables_shape_ok(1, 7, true, INT_MIN, 5));
  EXPECT(!srk_tables_shape_ok(1, 7, true, 1, 9) && !srk_tables_shape_ok(1, 7, true, 1, 4) && !srk_tables_shape_ok(1, 7, true, 1, 0) &&
         !srk_tables_shape_ok(1, 7, true, 1, -5) && !srk_tables_shape_ok(1, 7, true, 1, INT_MAX) && !srk_tables_shape_ok(1, 7, true, 1, INT_MIN) &&
         !srk_tables_shape_ok(1, 21, true, 1, 23));
  // what passes gives byte counts that fit a size_t: the largest of each
  EXPECT(srk_tables_bytes(1, 1, 4) == 4u && srk_tables_bytes(32, 21, 4) == 4u * 32 * 441 && srk_tables_bytes(INT_MAX, 21, 4) == 4ull * INT_MAX * 441);
  EXPECT(srk_tables_bytes(INT_MAX, 21, 8) == 8ull * INT_MAX * 441 && srk_tables_bytes(INT_MAX, 21, 8) / 8 / 441 == (size_t)INT_MAX);
  EXPECT(sizeof(double) * 8 * (size_t)INT_MAX == 64ull * INT_MAX);
  // overlap of the operands as api.hip asks: tab against desc and against the bank; real storage, every offset in range
  std::vector<double> buf(4096);
  const double* desc = buf.data();
  const float* f = reinterpret_cast<const float*>(buf.data());
  const size_t db = sizeof(double) * 8 * 3, tb = srk_tables_bytes(3, 7, sizeof(float)), bb = srk_tables_bytes(2, 5, sizeof(float));
  EXPECT(srk_ranges_overlap(desc, db, desc, tb) && srk_ranges_overlap(desc, db, desc + 23, tb) && !srk_ranges_overlap(desc, db, desc + 24, tb));
  EXPECT(srk_ranges_overlap(f + 146, db, f, tb) && !srk_ranges_overlap(f + 147, db, f, tb));
  EXPECT(srk_ranges_overlap(f + 49, bb, f, tb) && srk_ranges_overlap(f, bb, f + 49, tb) && !srk_ranges_overlap(f, bb, f + 50, tb) &&
         !srk_ranges_overlap(f + 147, bb, f, tb));
  EXPECT(!srk_ranges_overlap(nullptr, 0, f, tb));          // no bank: no bytes
  printf("%d failure(s)\n", failures);
  return failures != 0;
}
