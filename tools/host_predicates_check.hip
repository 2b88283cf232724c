// Edge values for the host argument predicates of csrc/common.h (srk_aligned, srk_ranges_overlap, srk_qkv_layout_ok, the benchmark-plane shapes,
// the wide-head shapes srk_widehead_cop_ok / _prep_shape_ok / _conv_shape_ok), as a stand-alone program for a sanitizer build; needs no GPU:
//   hipcc --offload-arch=gfx950 --cuda-host-only -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined tools/host_predicates_check.hip -o /tmp/host_predicates_check && /tmp/host_predicates_check
#include <stdio.h>

#include "../tpu_superresolution_amd/csrc/common.h"

static int failures = 0;
#define EXPECT(cond)                                      \
  do {                                                    \
    const bool ok_ = (cond);                              \
    printf("%s  %s\n", ok_ ? "ok  " : "FAIL", #cond);     \
    failures += !ok_;                                     \
  } while (0)

int main() {
  const auto ptr = [](uintptr_t v) { return reinterpret_cast<const void*>(v); };
  const uintptr_t top = ~(uintptr_t)0;
  // alignment: null is aligned to everything; the last addresses of the range
  EXPECT(srk_aligned(nullptr, 16) && srk_aligned(nullptr, 4));
  EXPECT(srk_aligned(ptr(64), 16) && !srk_aligned(ptr(72), 16) && srk_aligned(ptr(72), 8) && !srk_aligned(ptr(68), 8) && srk_aligned(ptr(68), 4));
  EXPECT(srk_aligned(ptr(top - 15), 16) && !srk_aligned(ptr(top), 4) && !srk_aligned(ptr(top - 7), 16) && srk_aligned(ptr(top - 7), 8));
  // overlap: empty ranges overlap nothing, not even themselves
  EXPECT(!srk_ranges_overlap(ptr(100), 0, ptr(100), 0) && !srk_ranges_overlap(ptr(100), 0, ptr(100), 8) && !srk_ranges_overlap(ptr(100), 8, ptr(104), 0));
  EXPECT(!srk_ranges_overlap(nullptr, 0, nullptr, 0) && srk_ranges_overlap(nullptr, 1, nullptr, 1));
  // ranges that touch do not overlap; one shared byte does; either order
  EXPECT(!srk_ranges_overlap(ptr(100), 8, ptr(108), 8) && !srk_ranges_overlap(ptr(108), 8, ptr(100), 8));
  EXPECT(srk_ranges_overlap(ptr(100), 9, ptr(108), 8) && srk_ranges_overlap(ptr(108), 8, ptr(100), 9));
  EXPECT(srk_ranges_overlap(ptr(100), 100, ptr(150), 1) && srk_ranges_overlap(ptr(150), 1, ptr(100), 100) && srk_ranges_overlap(ptr(100), 4, ptr(100), 4));
  // the top of the address range: a + n would wrap to 0 here
  EXPECT(!srk_ranges_overlap(ptr(top - 15), 8, ptr(top - 7), 8) && srk_ranges_overlap(ptr(top - 15), 9, ptr(top - 7), 8));
  EXPECT(!srk_ranges_overlap(ptr(16), 16, ptr(top - 15), 16) && !srk_ranges_overlap(ptr(top - 15), 16, ptr(16), 16));
  EXPECT(srk_ranges_overlap(ptr(0), (size_t)top, ptr(top - 1), 1) && !srk_ranges_overlap(ptr(0), (size_t)top, ptr(top), 1));
  // q/k/v layout: the smallest valid one, then each clause broken in turn
  EXPECT(srk_qkv_layout_ok(1, 32, 96, 32, 8) && srk_qkv_layout_ok(6, 192, 576, 192, 8) && srk_qkv_layout_ok(6, 192, 584, 196, 4));
  EXPECT(!srk_qkv_layout_ok(0, 32, 96, 32, 8) && !srk_qkv_layout_ok(-1, 32, 96, 32, 8) && !srk_qkv_layout_ok(2, 32, 96, 64, 8));
  EXPECT(!srk_qkv_layout_ok(1, 48, 144, 32, 8) && !srk_qkv_layout_ok(1, 32, 95, 32, 8) && !srk_qkv_layout_ok(1, 32, 100, 32, 8));
  EXPECT(!srk_qkv_layout_ok(1, 32, 96, 31, 8) && !srk_qkv_layout_ok(1, 32, 96, 36, 8) && srk_qkv_layout_ok(1, 32, 96, 36, 4));
  // benchmark-protocol planes: the smallest valid shapes, then each clause broken in turn, then the ends of the int range
  EXPECT(srk_bench_planes_shape_ok(1, 3, 9, 10, 4, SRK_BENCH_Y) && srk_bench_planes_shape_ok(1024, 1, 1, 1, 0, SRK_BENCH_Y));
  EXPECT(srk_bench_planes_shape_ok(2, 5, 12, 12, 5, SRK_BENCH_RGB) && !srk_bench_planes_shape_ok(2, 5, 12, 12, 5, SRK_BENCH_Y));
  EXPECT(!srk_bench_planes_shape_ok(0, 3, 9, 10, 4, 0) && !srk_bench_planes_shape_ok(1025, 3, 9, 10, 4, 0) && !srk_bench_planes_shape_ok(-1, 3, 9, 10, 4, 0));
  EXPECT(!srk_bench_planes_shape_ok(1, 0, 9, 10, 4, 1) && !srk_bench_planes_shape_ok(1, 2, 9, 10, 4, 0) && !srk_bench_planes_shape_ok(1, 4, 9, 10, 4, 0));
  EXPECT(!srk_bench_planes_shape_ok(1, 3, 9, 10, 5, 0) && !srk_bench_planes_shape_ok(1, 3, 10, 9, 5, 0) && !srk_bench_planes_shape_ok(1, 3, 8, 10, 4, 0));
  EXPECT(!srk_bench_planes_shape_ok(1, 3, 9, 10, -1, 0) && !srk_bench_planes_shape_ok(1, 3, 9, 10, 0, 2) && !srk_bench_planes_shape_ok(1, 3, 9, 10, 0, -1));
  EXPECT(!srk_bench_planes_shape_ok(1, 3, 0, 10, 0, 1) && !srk_bench_planes_shape_ok(1, 3, 9, 0, 0, 1) && !srk_bench_planes_shape_ok(1, 3, -9, -10, 0, 1));
  EXPECT(srk_bench_planes_shape_ok(1, 1, 0x7fffffff, 0x7fffffff, 0x3fffffff, 0) && !srk_bench_planes_shape_ok(1, 1, 0x7fffffff, 0x7fffffff, 0x40000000, 0));
  EXPECT(!srk_bench_planes_shape_ok(1, 3, 0x7fffffff, 3, 0x7fffffff, 0) && !srk_bench_planes_shape_ok(1, 2, 0x40000000, 1, 0, 1));
  EXPECT(srk_bench_planes_shape_ok(1, 1, 0x7fffffff, 1, 0, 1) && !srk_bench_planes_shape_ok(1, 0x7fffffff, 0x7fffffff, 1, 0, 1));
  EXPECT(srk_bench_plane_dims_ok(1, 1, 1, 1) && srk_bench_plane_dims_ok(1024, 3, 11, 11) && !srk_bench_plane_dims_ok(1025, 3, 11, 11));
  EXPECT(!srk_bench_plane_dims_ok(0, 1, 1, 1) && !srk_bench_plane_dims_ok(1, 0, 1, 1) && !srk_bench_plane_dims_ok(1, 1, 0, 1) && !srk_bench_plane_dims_ok(1, 1, 1, 0));
  EXPECT(srk_bench_plane_dims_ok(1, 1, 0x7fffffff, 0x7fffffff) && !srk_bench_plane_dims_ok(1, 2, 0x40000000, 1) && !srk_bench_plane_dims_ok(1, 0x7fffffff, 0x7fffffff, 1));
  // wide one-step head backward: the three padded widths and nothing beside them
  EXPECT(srk_widehead_cop_ok(32) && srk_widehead_cop_ok(48) && srk_widehead_cop_ok(64) && !srk_widehead_cop_ok(16) && !srk_widehead_cop_ok(4));
  EXPECT(!srk_widehead_cop_ok(0) && !srk_widehead_cop_ok(-32) && !srk_widehead_cop_ok(40) && !srk_widehead_cop_ok(80) && !srk_widehead_cop_ok(0x7fffffff));
  // gradient prep: the smallest and the widest valid shapes, each clause broken in turn, then the ends of the int range (no product wraps)
  EXPECT(srk_widehead_prep_shape_ok(1, 1, 1, 1, 1, 1, 1, 32) && srk_widehead_prep_shape_ok(2, 3, 16, 32, 4, 8, 4, 48) && srk_widehead_prep_shape_ok(1, 1, 8, 8, 1, 1, 8, 64));
  EXPECT(srk_widehead_prep_shape_ok(2, 3, 15, 29, 4, 8, 4, 48) && !srk_widehead_prep_shape_ok(2, 3, 17, 32, 4, 8, 4, 48) && !srk_widehead_prep_shape_ok(2, 3, 16, 33, 4, 8, 4, 48));
  EXPECT(!srk_widehead_prep_shape_ok(0, 3, 16, 32, 4, 8, 4, 48) && !srk_widehead_prep_shape_ok(2, 0, 16, 32, 4, 8, 4, 48) && !srk_widehead_prep_shape_ok(2, 3, 0, 32, 4, 8, 4, 48));
  EXPECT(!srk_widehead_prep_shape_ok(2, 3, 16, 0, 4, 8, 4, 48) && !srk_widehead_prep_shape_ok(2, 3, 16, 32, 0, 8, 4, 48) && !srk_widehead_prep_shape_ok(2, 3, 16, 32, 4, -8, 4, 48));
  EXPECT(!srk_widehead_prep_shape_ok(2, 3, 16, 32, 4, 8, 0, 48) && !srk_widehead_prep_shape_ok(2, 3, 16, 32, 4, 8, 9, 48) && !srk_widehead_prep_shape_ok(2, 4, 16, 32, 4, 8, 4, 48));
  EXPECT(!srk_widehead_prep_shape_ok(2, 3, 16, 32, 4, 8, 4, 16) && !srk_widehead_prep_shape_ok(2, 3, 16, 32, 4, 8, 4, 56) && !srk_widehead_prep_shape_ok(2, 3, 16, 32, 4, 8, 5, 64));
  EXPECT(!srk_widehead_prep_shape_ok(2, 0x7fffffff, 16, 32, 4, 8, 4, 48) && !srk_widehead_prep_shape_ok(2, 3, 16, 32, 4, 8, 0x7fffffff, 48));
  EXPECT(!srk_widehead_prep_shape_ok(0x7fffffff, 3, 16, 32, 4, 8, 4, 48) && !srk_widehead_prep_shape_ok(1, 1, 1, 1, 0x7fffffff, 0x7fffffff, 1, 32));
  EXPECT(srk_widehead_prep_shape_ok(1, 1, 0x7fffffff, 1, 0x7fffffff, 1, 1, 32) && !srk_widehead_prep_shape_ok(1, 1, 1, 1, 0x40000000, 1, 2, 32));
  EXPECT(srk_widehead_prep_shape_ok(1, 1, 0x7ffffff8, 1, 0x0fffffff, 1, 8, 64) && !srk_widehead_prep_shape_ok(1, 1, 1, 1, 0x10000000, 1, 8, 64));
  // the two conv gradients: the narrow family's predicates at the wide widths
  EXPECT(srk_widehead_conv_shape_ok(1, 1, 1, 1, 64, 1, 32) && srk_widehead_conv_shape_ok(32, 64, 64, 60, 64, 48, 48) && srk_widehead_conv_shape_ok(1, 4, 8, 256, 256, 64, 64));
  EXPECT(!srk_widehead_conv_shape_ok(0, 4, 8, 60, 64, 48, 48) && !srk_widehead_conv_shape_ok(1, 0, 8, 60, 64, 48, 48) && !srk_widehead_conv_shape_ok(1, 4, -8, 60, 64, 48, 48));
  EXPECT(!srk_widehead_conv_shape_ok(1, 4, 8, 0, 64, 48, 48) && !srk_widehead_conv_shape_ok(1, 4, 8, 65, 64, 48, 48) && !srk_widehead_conv_shape_ok(1, 4, 8, 60, 60, 48, 48));
  EXPECT(!srk_widehead_conv_shape_ok(1, 4, 8, 60, 0, 48, 48) && !srk_widehead_conv_shape_ok(1, 4, 8, 60, 320, 48, 48) && !srk_widehead_conv_shape_ok(1, 4, 8, 60, 64, 0, 48));
  EXPECT(!srk_widehead_conv_shape_ok(1, 4, 8, 60, 64, 49, 48) && !srk_widehead_conv_shape_ok(1, 4, 8, 60, 64, 12, 16) && !srk_widehead_conv_shape_ok(1, 4, 8, 60, 64, 3, 4));
  EXPECT(!srk_widehead_conv_shape_ok(1, 4, 8, 60, 64, 48, 56) && !srk_widehead_conv_shape_ok(1, 4, 8, 60, 64, 48, 128) && !srk_widehead_conv_shape_ok(1, 4, 8, 60, 64, 48, -48));
  EXPECT(srk_widehead_conv_shape_ok(1, 0x7fffffff, 1, 60, 64, 48, 48) && !srk_widehead_conv_shape_ok(2, 0x40000000, 1, 60, 64, 48, 48));
  EXPECT(!srk_widehead_conv_shape_ok(0x7fffffff, 0x7fffffff, 0x7fffffff, 60, 64, 48, 48) && !srk_widehead_conv_shape_ok(1, 4, 8, 0x7fffffff, 64, 48, 48));
  printf("%d failure(s)\n", failures);
  return failures != 0;
}
