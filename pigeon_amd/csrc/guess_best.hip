// guess_best.hip -- the guess that maximises the expected score: pg_score_table, pg_guess_best, pg_guess_best_plan (contract:
// include/pigeon_hip.h, restated in tests/_bestref.py).
//
// The head leaves the (B, C) fp32 logits behind.  Over a candidate set shared by the batch the expectation of a candidate j under
// row b's softmax is a matrix product, all in float64:
//   w[b,c] = exp(l[b,c] - max_c l[b,c])    Z[b] = sum_c w[b,c]                         -- pg_guess_spread's weights and its Z
//   E[b,j] = (sum_c w[b,c] * table[j,c]) / Z[b]
// where table (M, C) depends on the model alone (candidates x cell centroids: km or score, pg_score_table) and is built once.
//
// pg_guess_best, three kernels on one stream:
//   1. gb_weights_kernel, one workgroup of 256 threads per row: the row maximum, the NaN / +inf test, w[b,:] and Z[b] into a
//      stream-ordered scratch.  Z is spread.hip's sum, in row_block.h's summation order.  A row the contract answers with NaN (a NaN
//      or +inf logit, -inf only) gets w = 0 and Z = NaN: every E of that row is then NaN with no branch in the product, and no other
//      row sees it.
//   2. gb_product_kernel<T>, one workgroup of 256 threads per (row tile, candidate tile) of 32T x 32T, T = 1 or 2; each of the four
//      waves owns a 16T x 16T corner as T x T accumulators of v_mfma_f64_16x16x4_f64.  Both operands are contiguous along c and
//      staged [row][k] in LDS, GB_KC cells per step, the next step's loads in flight in registers.  One element's sum is ONE
//      accumulator that walks c = 0, 4, 8, ... ascending through the same instruction whatever T, the tile, the wave or the lane:
//      E[b,j] is the same bits for a row alone, inside any batch, at any row position, with any M and at any candidate position, in
//      either form.  Cells past C are staged as zeros on both sides (fma(0, 0, acc) = acc, and acc is never -0); rows past B and
//      candidates past M are staged as zeros too and never stored.  The tile's E go to `expected` when asked for and, through
//      LDS, to one (value, index) partial per (row, candidate tile): thread r scans its row's candidates in ascending order.
//   3. gb_pick_kernel, one thread per row: the partials in ascending tile order.  Strict comparisons in both scans: the smallest j
//      among equals wins; a NaN never wins; a row with nothing but NaN gives -1 / NaN.
// No atomics, no split over c, and no input value forms an address or bounds a loop.
#include "common.h"
#include "pigeon_internal.h"
#include "haversine.h"
#include "row_block.h"

#include <cmath>

#define GB_THREADS 256
#define GB_KC 32                                     // cells staged per K step
#define GB_LDK (GB_KC + 2)                           // 34 doubles a row: the 16 rows x 2 k of a half wave's read fall on 32 distinct bank pairs
#define GB_FILL_WGS 256                              // the 64 x 64 form is taken when it alone gives every CU a workgroup

typedef __attribute__((ext_vector_type(4))) double f64x4;

// ------------------------------------------------------------------------------------------------ the table
__global__ __launch_bounds__(256) void score_table_kernel(const double* __restrict__ cand, const double* __restrict__ cen, int C,
                                                          int64_t n, int kind, double* __restrict__ table) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;       // j * C + c
    if (i >= n) return;
    const int64_t j = i / C, c = i - j * C;
    const double d = pg_haversine_km<double>(cand[2 * j], cand[2 * j + 1], cen[2 * c], cen[2 * c + 1]);
    table[i] = kind == 0 ? d : PG_SCORE_MAX * exp(-d / PG_SCORE_DECAY_KM);
}

extern "C" int pg_score_table(const double* candidates, int M, const double* centroids, int C, int kind, double* table, void* stream) {
    if (M < 0) { pg_set_error("score_table: M = %d", M); return PG_EINVAL; }
    if (C < 1) { pg_set_error("score_table: C must be at least 1 (got %d)", C); return PG_EINVAL; }
    if (kind != 0 && kind != 1) { pg_set_error("score_table: kind must be 0 (km) or 1 (score), got %d", kind); return PG_EINVAL; }
    if (M == 0) return PG_OK;
    PG_NEED("score_table", candidates);
    PG_NEED("score_table", centroids);
    PG_NEED("score_table", table);
    const int64_t n = (int64_t)M * C, blocks = (n + 255) / 256;
    if (blocks > 0x7fffffffLL) { pg_set_error("score_table: M * C = %lld is more than one launch holds", (long long)n); return PG_EINVAL; }
    hipLaunchKernelGGL(score_table_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, candidates, centroids, C, n, kind, table);
    return pg_check_launch("score_table");
}

// ------------------------------------------------------------------------------------------------ 1. weights
__global__ __launch_bounds__(GB_THREADS) void gb_weights_kernel(const float* __restrict__ logits, int C, double* __restrict__ w,
                                                                double* __restrict__ Z) {
    __shared__ float redmax[4];
    __shared__ int redbad[4];
    __shared__ double red[4];
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x;
    const float* row = logits + b * (int64_t)C;
    double* wrow = w + b * (int64_t)C;
    float mx = -INFINITY;
    int bad = 0;
    for (int c = tid; c < C; c += GB_THREADS) {
        const float v = row[c];
        bad |= (v != v || v == INFINITY); mx = v > mx ? v : mx;
    }
    block_max_flag(mx, bad, redmax, redbad);
    bad |= !(mx > -INFINITY);                          // a row of -inf only
    const double m = (double)mx;
    double acc = 0.0;
    for (int c = tid; c < C; c += GB_THREADS) {        // `bad` is uniform: exp(l - m) needs a finite m
        const double e = bad ? 0.0 : exp((double)row[c] - m);
        wrow[c] = e;
        acc += e;
    }
    block_sum(acc, red);
    if (tid == 0) Z[b] = bad ? (double)NAN : acc;
}

// ------------------------------------------------------------------------------------------------ 2. product and tile partials
__device__ __forceinline__ bool gb_better(double v, double best, int best_idx, int maximize) {
    return best_idx < 0 ? v == v : (maximize ? v > best : v < best);
}

template <int T>
__global__ __launch_bounds__(GB_THREADS) void gb_product_kernel(const double* __restrict__ w, const double* __restrict__ Z,
                                                                const double* __restrict__ table, int B, int C, int M, int maximize,
                                                                double* __restrict__ expected, double* __restrict__ part_val,
                                                                int32_t* __restrict__ part_idx, int ntiles) {
    constexpr int TILE = 32 * T;
    constexpr int LDE = TILE + 1;
    static_assert(TILE * LDE <= 2 * TILE * GB_LDK, "the tile of E reuses the staging buffers");
    __shared__ double lds[2 * TILE * GB_LDK];
    double (*Ws)[GB_LDK] = (double (*)[GB_LDK])lds;
    double (*Ts)[GB_LDK] = (double (*)[GB_LDK])(lds + TILE * GB_LDK);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j0 = blockIdx.x * TILE, b0 = blockIdx.y * TILE;
    const int wb = (wave & 1) * 16 * T, wj = (wave >> 1) * 16 * T;
    f64x4 acc[T][T];
#pragma unroll
    for (int i = 0; i < T; ++i)
#pragma unroll
        for (int j = 0; j < T; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[i][j][r] = 0.0;
    const int sk = tid & 31, sr = tid >> 5;             // staging: 32 consecutive cells of one row per half wave
    double pw[4 * T], pt[4 * T];
#pragma unroll
    for (int i = 0; i < 4 * T; ++i) {
        const int r = sr + 8 * i;
        const bool k_in = sk < C;
        pw[i] = (k_in && b0 + r < B) ? w[(int64_t)(b0 + r) * C + sk] : 0.0;
        pt[i] = (k_in && j0 + r < M) ? table[(int64_t)(j0 + r) * C + sk] : 0.0;
    }
    for (int k0 = 0; k0 < C; k0 += GB_KC) {
#pragma unroll
        for (int i = 0; i < 4 * T; ++i) {
            Ws[sr + 8 * i][sk] = pw[i];
            Ts[sr + 8 * i][sk] = pt[i];
        }
        __syncthreads();
        if (k0 + GB_KC < C) {
            const int k = k0 + GB_KC + sk;
            const bool k_in = k < C;
#pragma unroll
            for (int i = 0; i < 4 * T; ++i) {
                const int r = sr + 8 * i;
                pw[i] = (k_in && b0 + r < B) ? w[(int64_t)(b0 + r) * C + k] : 0.0;
                pt[i] = (k_in && j0 + r < M) ? table[(int64_t)(j0 + r) * C + k] : 0.0;
            }
        }
#pragma unroll
        for (int kk = 0; kk < GB_KC / 4; ++kk) {
            const int k = 4 * kk + (lane >> 4);
            double a[T], t[T];
#pragma unroll
            for (int i = 0; i < T; ++i) a[i] = Ws[wb + 16 * i + (lane & 15)][k];
#pragma unroll
            for (int j = 0; j < T; ++j) t[j] = Ts[wj + 16 * j + (lane & 15)][k];
#pragma unroll
            for (int i = 0; i < T; ++i)
#pragma unroll
                for (int j = 0; j < T; ++j) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i], t[j], acc[i][j], 0, 0, 0);
        }
        __syncthreads();
    }
    // E = acc / Z: to `expected`, and into LDS for the row scans (the K loop's last barrier has released the staging buffers)
    double (*Es)[LDE] = (double (*)[LDE])lds;
#pragma unroll
    for (int i = 0; i < T; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int rb = wb + 16 * i + (lane >> 4) + 4 * r;          // the f64 form's C/D map: row = (lane >> 4) + 4 reg, col = lane & 15
            const int b = b0 + rb;
            const double z = b < B ? Z[b] : 1.0;
#pragma unroll
            for (int j = 0; j < T; ++j) {
                const int cj = wj + 16 * j + (lane & 15);
                const double e = acc[i][j][r] / z;
                Es[rb][cj] = e;
                if (expected && b < B && j0 + cj < M) expected[(int64_t)b * M + j0 + cj] = e;
            }
        }
    __syncthreads();
    if (tid < TILE && b0 + tid < B) {
        double best = NAN;
        int best_idx = -1;
        const int n = M - j0 < TILE ? M - j0 : TILE;
        for (int j = 0; j < n; ++j) {
            const double v = Es[tid][j];
            if (gb_better(v, best, best_idx, maximize)) { best = v; best_idx = j0 + j; }
        }
        part_val[(int64_t)(b0 + tid) * ntiles + blockIdx.x] = best;
        part_idx[(int64_t)(b0 + tid) * ntiles + blockIdx.x] = best_idx;
    }
}

// ------------------------------------------------------------------------------------------------ 3. the pick
__global__ __launch_bounds__(GB_THREADS) void gb_pick_kernel(const double* __restrict__ part_val, const int32_t* __restrict__ part_idx, int B,
                                                             int ntiles, int maximize, int32_t* __restrict__ best_idx,
                                                             double* __restrict__ best_value) {
    const int b = blockIdx.x * GB_THREADS + threadIdx.x;
    if (b >= B) return;
    double best = NAN;
    int idx = -1;
    for (int t = 0; t < ntiles; ++t) {
        const double v = part_val[(int64_t)b * ntiles + t];
        const int32_t i = part_idx[(int64_t)b * ntiles + t];
        if (i >= 0 && gb_better(v, best, idx, maximize)) { best = v; idx = i; }
    }
    best_idx[b] = idx;
    best_value[b] = best;
}

// ------------------------------------------------------------------------------------------------ host
struct GbPlan { int form, tile, row_tiles, cand_tiles; size_t w_bytes, z_bytes, val_bytes, idx_bytes; };

static GbPlan gb_plan(int B, int C, int M) {
    GbPlan p;
    const int64_t big = (int64_t)((B + 63) / 64) * ((M + 63) / 64);
    p.form = big >= GB_FILL_WGS ? 1 : 0;
    p.tile = p.form ? 64 : 32;
    p.row_tiles = (B + p.tile - 1) / p.tile;
    p.cand_tiles = (M + p.tile - 1) / p.tile;
    auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    p.w_bytes = up((size_t)B * (size_t)C * sizeof(double));
    p.z_bytes = up((size_t)B * sizeof(double));
    p.val_bytes = up((size_t)B * (size_t)p.cand_tiles * sizeof(double));
    p.idx_bytes = up((size_t)B * (size_t)p.cand_tiles * sizeof(int32_t));
    return p;
}

static int gb_check_shape(const char* who, int B, int C, int M) {
    if (B < 0) { pg_set_error("%s: B = %d", who, B); return PG_EINVAL; }
    if (M < 0) { pg_set_error("%s: M = %d", who, M); return PG_EINVAL; }
    if (C < 1) { pg_set_error("%s: C must be at least 1 (got %d)", who, C); return PG_EINVAL; }
    if ((int64_t)B * M > 0x7fffffffLL) { pg_set_error("%s: B * M = %lld exceeds 2^31 - 1", who, (long long)B * M); return PG_EINVAL; }
    return PG_OK;
}

extern "C" int pg_guess_best_plan(int B, int C, int M, int32_t out[8]) {
    PG_NEED("guess_best_plan", out);
    const int rc = gb_check_shape("guess_best_plan", B, C, M);
    if (rc != PG_OK) return rc;
    const GbPlan p = gb_plan(B, C, M);
    const size_t scratch = p.w_bytes + p.z_bytes + p.val_bytes + p.idx_bytes;
    const int64_t wgs = (int64_t)p.row_tiles * p.cand_tiles;
    out[0] = p.form;
    out[1] = p.tile;
    out[2] = p.tile;
    out[3] = GB_KC;
    out[4] = (int32_t)(wgs > 0x7fffffffLL ? 0x7fffffffLL : wgs);
    out[5] = (B == 0 || M == 0) ? 0 : (int32_t)(scratch > 0x7fffffffULL ? 0x7fffffffULL : scratch);
    out[6] = GB_THREADS;
    out[7] = p.cand_tiles;
    return PG_OK;
}

extern "C" int pg_guess_best(const float* logits, int B, int C, const double* table, int M, int maximize, int32_t* best_idx,
                             double* best_value, double* expected, void* stream) {
    const int rc0 = gb_check_shape("guess_best", B, C, M);
    if (rc0 != PG_OK) return rc0;
    if (B == 0 || M == 0) return PG_OK;                    // nothing to do: the (empty) buffers may be NULL
    PG_NEED("guess_best", logits);
    PG_NEED("guess_best", table);
    PG_NEED("guess_best", best_idx);
    PG_NEED("guess_best", best_value);
    const GbPlan p = gb_plan(B, C, M);
    if (p.row_tiles > 65535) { pg_set_error("guess_best: B = %d is more than one launch holds", B); return PG_EINVAL; }
    hipStream_t s = (hipStream_t)stream;
    char* scratch = nullptr;
    PG_HIP(hipMallocAsync((void**)&scratch, p.w_bytes + p.z_bytes + p.val_bytes + p.idx_bytes, s));
    double* w = (double*)scratch;
    double* Z = (double*)(scratch + p.w_bytes);
    double* part_val = (double*)(scratch + p.w_bytes + p.z_bytes);
    int32_t* part_idx = (int32_t*)(scratch + p.w_bytes + p.z_bytes + p.val_bytes);
    const int mx = maximize != 0;
    hipLaunchKernelGGL(gb_weights_kernel, dim3((unsigned)B), dim3(GB_THREADS), 0, s, logits, C, w, Z);
    int rc = pg_check_launch("guess_best (weights)");
    if (rc == PG_OK) {
        const dim3 grid((unsigned)p.cand_tiles, (unsigned)p.row_tiles);
        if (p.form)
            hipLaunchKernelGGL(gb_product_kernel<2>, grid, dim3(GB_THREADS), 0, s, w, Z, table, B, C, M, mx, expected, part_val, part_idx,
                               p.cand_tiles);
        else
            hipLaunchKernelGGL(gb_product_kernel<1>, grid, dim3(GB_THREADS), 0, s, w, Z, table, B, C, M, mx, expected, part_val, part_idx,
                               p.cand_tiles);
        rc = pg_check_launch("guess_best (product)");
    }
    if (rc == PG_OK) {
        hipLaunchKernelGGL(gb_pick_kernel, dim3((unsigned)((B + GB_THREADS - 1) / GB_THREADS)), dim3(GB_THREADS), 0, s, part_val, part_idx, B,
                           p.cand_tiles, mx, best_idx, best_value);
        rc = pg_check_launch("guess_best (pick)");
    }
    (void)hipFreeAsync(scratch, s);
    return rc;
}
