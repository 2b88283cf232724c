// tables.hip: the launcher behind srk_kernel_tables_f32 (arguments checked there and by srk_tables_shape_ok).
#pragma once
#include "common.h"

int srk_launch_kernel_tables_f32(const double* desc, const float* bank, int n_bank, int kb, float* tab, int n, int ks, hipStream_t stream);
