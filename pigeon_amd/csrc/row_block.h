// row_block.h -- what the row kernels share: one workgroup of 256 threads owns one row of C geocells (head_row_kernel and
// head_margin_kernel in head.hip, guess_spread_kernel, ht_row_kernel, gb_weights_kernel).
//
// THE SUMMATION ORDER.  Thread t adds its cells t, t + 256, ... in ascending order (the caller's loop); block_sum combines the 64 lanes
// of a wave in the butterfly v += v(lane xor o), o = 32 .. 1, and the four waves as (w0 + w1) + (w2 + w3).  The sequence of additions
// depends on C only -- no atomics, nothing of the batch, the row's position or its alignment -- which is why a row is the same bits
// alone and inside any batch.  Every term of a masked sum is a weight or +0.0, and x + (+0.0) = x for every x >= +0.0, so a masked cell
// leaves each partial sum as it was: a sum whose mask lets every cell through equals the unmasked sum bit for bit.
// block_sum holds additions, shuffles and one barrier: nothing in it can be contracted, whatever the including file's setting.
//
// WHERE A ROW'S CELLS LIVE.  In dynamic LDS while they fit ROW_LDS_BUDGET (GLOBAL = false), in a stream-ordered device scratch above
// (GLOBAL = true): the same kernel body, the same arithmetic in the same order, the same bits.  row_cells_launch decides and launches.
#pragma once
#include "common.h"
#include "pigeon_internal.h"

#define ROW_LDS_BUDGET (150 * 1024)                  // bytes of the CU's 160 KB of LDS that a row's cells may take

constexpr int row_lds_cells(int bytes_per_cell) { return ROW_LDS_BUDGET / bytes_per_cell; }
static_assert(row_lds_cells(16) == 9600, "pg_guess_spread: (key, weight) pairs of doubles");
static_assert(row_lds_cells(8) == 19200, "pg_head_train_loss: one double a cell");
static_assert(row_lds_cells(4) == 38400, "pg_head_forward: one float a cell");

// v[0..N) of every thread -> the block's sums, identical in every thread.  One barrier: the caller separates two uses of the same
// `red` (a barrier of its own, or two alternating buffers).
template <typename T, int N>
__device__ __forceinline__ void block_sum(T (&v)[N], T (*red)[N]) {
#pragma unroll
    for (int j = 0; j < N; ++j) {
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) v[j] += __shfl_xor(v[j], o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int j = 0; j < N; ++j) red[threadIdx.x >> 6][j] = v[j];
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < N; ++j) v[j] = (red[0][j] + red[1][j]) + (red[2][j] + red[3][j]);
}
template <typename T>
__device__ __forceinline__ void block_sum(T& v, T* red /*[4]*/) {
    block_sum(reinterpret_cast<T(&)[1]>(v), reinterpret_cast<T(*)[1]>(red));
}

// the row maximum and the OR of a flag, identical in every thread; one barrier
__device__ __forceinline__ void block_max_flag(float& mx, int& bad, float* redmax /*[4]*/, int* redbad /*[4]*/) {
    mx = wave_max(mx);
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) bad |= __shfl_xor(bad, o, 64);
    if ((threadIdx.x & 63) == 0) { redmax[threadIdx.x >> 6] = mx; redbad[threadIdx.x >> 6] = bad; }
    __syncthreads();
    mx = fmaxf(fmaxf(redmax[0], redmax[1]), fmaxf(redmax[2], redmax[3]));
    bad = redbad[0] | redbad[1] | redbad[2] | redbad[3];
}

// ---------------------------------------------------------------------------------------------------------------------------- host
// out[0..3] of a row kernel's plan: form (1 = scratch), dynamic LDS bytes, the cell limit, threads
static int row_cells_plan(const char* who, int C, int cells, size_t bytes_per_cell, int threads, int32_t out[4]) {
    if (!out) { pg_set_error("%s: null argument out", who); return PG_EINVAL; }
    if (C < 1) { pg_set_error("%s: C must be at least 1 (got %d)", who, C); return PG_EINVAL; }
    out[0] = C > cells ? 1 : 0;
    out[1] = C > cells ? 0 : (int32_t)((size_t)C * bytes_per_cell);
    out[2] = cells;
    out[3] = threads;
    return PG_OK;
}

// One launch of `blocks` rows of C cells: IN_LDS with C * bytes_per_cell of dynamic LDS up to `cells` cells, IN_SCRATCH with a
// stream-ordered scratch of that many bytes per block above.  launch(kernel, lds_bytes, scratch) does the hipLaunchKernelGGL.
template <auto IN_LDS, auto IN_SCRATCH, typename Launch>
static int row_cells_launch(const char* what, const char* what_large, int64_t blocks, int C, int cells, size_t bytes_per_cell,
                            hipStream_t s, Launch launch) {
    const size_t row_bytes = (size_t)C * bytes_per_cell;
    if (C > cells) {
        void* scratch = nullptr;
        PG_HIP(hipMallocAsync(&scratch, (size_t)blocks * row_bytes, s));
        launch(IN_SCRATCH, (size_t)0, scratch);
        const int rc = pg_check_launch(what_large);
        (void)hipFreeAsync(scratch, s);
        return rc;
    }
    static bool attr_set = false;                      // once per kernel: the most any launch of it asks for
    if (!attr_set) {
        PG_HIP(hipFuncSetAttribute((const void*)IN_LDS, hipFuncAttributeMaxDynamicSharedMemorySize, (int)((size_t)cells * bytes_per_cell)));
        attr_set = true;
    }
    launch(IN_LDS, row_bytes, (void*)nullptr);
    return pg_check_launch(what);
}
