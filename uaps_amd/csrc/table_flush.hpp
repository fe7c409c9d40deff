// The per-image table flush shared by shapes.hip (uaps_shape_descriptors) and skeleton.hip (uaps_skeleton_stats): a table of
// int64 [B][M][COLS] rows, one row per component of an image, every column a sum except ONE maximum column.
//   table_zero          zeroes the whole table (the body of the first launch of both entry points)
//   LDS form            a workgroup (rows of ONE image) zeroes a copy of the image's table in LDS (table_lds_zero), the runs' first
//                       lanes add into it, and table_lds_flush sends the non-zero words to the table with 64-bit atomics
//   direct form         above kLdsRows rows the first lanes send to the table themselves
// atomicAdd, and atomicMax for the maximum column, on non-negative integers only: two runs and both forms give the same bits.
// Builds on call_common.hpp alone (kThreads, u64 of the enclosing namespace): nothing of the loss scaffold comes with this header.
#pragma once
#include "call_common.hpp"

namespace uaps {
namespace table {
constexpr int kLdsRows = UAPS_SHAPE_LDS_ROWS;
constexpr int kMaxGrid = 1 << 24;

// the body of a user's zeroing kernel (each keeps a kernel of its own name: shape_zero_kernel, skeleton_zero_kernel)
__device__ __forceinline__ void table_zero(u64* table, long n) {
    for (long i = (long)blockIdx.x * kThreads + threadIdx.x; i < n; i += (long)gridDim.x * kThreads) table[i] = 0ull;
}

__device__ __forceinline__ void table_lds_zero(u64* acc, int words) {
    for (int i = threadIdx.x; i < words; i += kThreads) acc[i] = 0ull;
    __syncthreads();
}

// COLS words a row, column MAXCOL a maximum
template <int COLS, int MAXCOL>
__device__ __forceinline__ void table_lds_flush(const u64* acc, u64* out, int words) {
    __syncthreads();
    for (int i = threadIdx.x; i < words; i += kThreads) {
        const u64 v = acc[i];
        if (v == 0ull) continue;
        if (i % COLS == MAXCOL) atomicMax(out + i, v);
        else atomicAdd(out + i, v);
    }
}

}  // namespace table
}  // namespace uaps
