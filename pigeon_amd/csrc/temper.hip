// temper.hip -- one scalar that calibrates the head's softmax: pg_temper_stats, pg_temper_logits, pg_temper_plan (contract:
// include/pigeon_hip.h, restated in tests/_tempref.py).
//
// With beta = 1 / T the calibrated probabilities are softmax(beta * l).  Per row n, label y and beta_k, all in float64, with
// m = max_c l_c and x_c = (double)l_c - (double)m:
//   w_c = exp(beta_k * x_c)        Z = sum w_c        A = sum w_c * x_c        Q = sum (w_c * x_c) * x_c
//   row_stats[n,k,:] = { log(Z) - beta_k * x_y,  A / Z - x_y,  max(0, Q / Z - (A / Z) * (A / Z)) }      conf[n,k] = 1 / Z
// the negative log-likelihood of the label and its first and second derivative in beta (the total is convex in beta), and the
// probability of the argmax.  pigeon_amd/temperature.py minimises the total over beta with these three numbers.
//
// temper_row_kernel: one workgroup of 256 threads per row.  The row is read from global memory 1 + ceil(K / TEMPER_GROUP) times -- a
// 10 000-cell row is 40 KB and stays in L2, so there is no LDS staging and no scratch form: once for the maximum, the first index
// that attains it (torch.argmax's order), the label's logit and the NaN / +inf test, then once per group of TEMPER_GROUP betas with
// three accumulators per beta.  A slot of a group runs the same operations whatever its index, and every sum over cells is
// row_block.h's one summation order, so a row's outputs are the same bits alone, inside any batch, at any position and at any
// position of its beta inside betas (this file is compiled with -ffp-contract=off: no product is fused into a sum).
// A -inf logit is a cell of weight +0.0 and of x = +0.0 in the products: it adds +0.0 to every sum, never 0 * inf.
// The label's logit is picked by the comparison c == labels[n]: no input value forms an address or bounds a loop.
//
// temper_totals_kernel: 3 K workgroups, one per (k, j), and one more for the two counts.  Thread t adds rows t, t + 256, ... in
// ascending order, an invalid row as +0.0, then block_sum: the order depends on N only, no atomics.
#include "common.h"
#include "pigeon_internal.h"
#include "row_block.h"

#include <cmath>

#define TEMPER_THREADS 256
#define TEMPER_MAX_K 16
#define TEMPER_GROUP 4                               // betas per pass over a row: 12 fp64 accumulators a thread
#define TEMPER_NO_INDEX 0x7fffffff

struct TemperBetas { double b[TEMPER_MAX_K]; };

__global__ __launch_bounds__(TEMPER_THREADS) void temper_row_kernel(const float* __restrict__ logits, int C,
                                                                    const int64_t* __restrict__ labels, TemperBetas B, int K,
                                                                    double* __restrict__ row_stats, double* __restrict__ conf,
                                                                    uint8_t* __restrict__ state) {
    // block_sum alternates between the two slots, so its one barrier per call is enough
    __shared__ double red[2][4][3 * TEMPER_GROUP];
    __shared__ double sbeta[TEMPER_MAX_K];             // TEMPER_MAX_K is a multiple of TEMPER_GROUP: a group never reads past it
    __shared__ float redmax[4];
    __shared__ int redbad[4];
    __shared__ int redidx[4];
    __shared__ float label_logit;
    const int tid = threadIdx.x;
    const int64_t n = blockIdx.x;
    const float* row = logits + n * (int64_t)C;
    const int64_t y = labels[n];

    // the betas into LDS with constant indices into the argument; a slot past K computes with 1.0 and is never written out
#pragma unroll
    for (int i = 0; i < TEMPER_MAX_K; ++i)
        if (tid == i) sbeta[i] = i < K ? B.b[i] : 1.0;
    if (tid == 0) label_logit = NAN;
    __syncthreads();

    // 1. the maximum, its first index, the label's logit, the NaN / +inf test
    float mx = -INFINITY;
    int first = TEMPER_NO_INDEX;
    int bad = !(y >= 0 && y < (int64_t)C);
    for (int c = tid; c < C; c += TEMPER_THREADS) {
        const float v = row[c];
        bad |= (v != v || v == INFINITY);
        if (v > mx) { mx = v; first = c; }
        if ((int64_t)c == y) label_logit = v;
    }
    const float mine = mx;
    block_max_flag(mx, bad, redmax, redbad);           // its barrier also publishes label_logit
    int a = (first != TEMPER_NO_INDEX && mine == mx) ? first : TEMPER_NO_INDEX;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) { const int other = __shfl_xor(a, o, 64); a = other < a ? other : a; }
    if ((tid & 63) == 0) redidx[tid >> 6] = a;
    __syncthreads();
    a = min(min(redidx[0], redidx[1]), min(redidx[2], redidx[3]));
    const float ly = label_logit;
    bad |= !(mx > -INFINITY);                          // a row of -inf only
    bad |= !(ly > -INFINITY);                          // the label on a masked cell (NaN: the label is outside [0, C))
    if (bad) {                                         // uniform
        for (int i = tid; i < K; i += TEMPER_THREADS) {
            if (row_stats) {
                row_stats[(n * K + i) * 3 + 0] = NAN; row_stats[(n * K + i) * 3 + 1] = NAN; row_stats[(n * K + i) * 3 + 2] = NAN;
            }
            if (conf) conf[n * K + i] = NAN;
        }
        if (tid == 0) state[n] = 2;
        return;
    }
    if (tid == 0) state[n] = (int64_t)a == y ? 1 : 0;
    const double m = (double)mx;
    const double xy = (double)ly - m;

    // 2. per group of betas: Z, A, Q of each
    for (int g0 = 0, pass = 0; g0 < K; g0 += TEMPER_GROUP, ++pass) {
        double beta[TEMPER_GROUP], acc[3 * TEMPER_GROUP];
#pragma unroll
        for (int j = 0; j < TEMPER_GROUP; ++j) { beta[j] = sbeta[g0 + j]; acc[3 * j] = 0.0; acc[3 * j + 1] = 0.0; acc[3 * j + 2] = 0.0; }
        for (int c = tid; c < C; c += TEMPER_THREADS) {
            const float v = row[c];
            const bool masked = v == -INFINITY;
            const double x = masked ? 0.0 : (double)v - m;
#pragma unroll
            for (int j = 0; j < TEMPER_GROUP; ++j) {
                const double w = masked ? 0.0 : exp(beta[j] * x);
                const double wx = w * x;
                acc[3 * j] += w;
                acc[3 * j + 1] += wx;
                acc[3 * j + 2] += wx * x;
            }
        }
        block_sum(acc, red[pass & 1]);
        if (tid < TEMPER_GROUP && g0 + tid < K) {
            double Z = 0.0, A = 0.0, Q = 0.0;
#pragma unroll
            for (int j = 0; j < TEMPER_GROUP; ++j)
                if (tid == j) { Z = acc[3 * j]; A = acc[3 * j + 1]; Q = acc[3 * j + 2]; }
            const double bk = sbeta[g0 + tid];
            const double mean = A / Z;
            const int64_t o = n * K + g0 + tid;
            if (row_stats) {
                row_stats[o * 3 + 0] = log(Z) - bk * xy;
                row_stats[o * 3 + 1] = mean - xy;
                row_stats[o * 3 + 2] = fmax(0.0, Q / Z - mean * mean);
            }
            if (conf) conf[o] = 1.0 / Z;
        }
    }
}

__global__ __launch_bounds__(TEMPER_THREADS) void temper_totals_kernel(const double* __restrict__ row_stats,
                                                                       const uint8_t* __restrict__ state, int64_t N, int K,
                                                                       double* __restrict__ totals, int64_t* __restrict__ counts) {
    __shared__ double red[4];
    __shared__ long long redc[4][2];
    const int tid = threadIdx.x;
    const int slot = blockIdx.x;                       // k * 3 + j, or 3 K: the counts
    if (slot == 3 * K) {
        long long c[2] = {0, 0};
        for (int64_t n = tid; n < N; n += TEMPER_THREADS) {
            const int st = state[n];
            c[0] += st != 2;
            c[1] += st == 1;
        }
        block_sum(c, redc);
        if (tid == 0) { counts[0] = c[0]; counts[1] = c[1]; }
        return;
    }
    double acc = 0.0;
    for (int64_t n = tid; n < N; n += TEMPER_THREADS) acc += state[n] != 2 ? row_stats[n * 3 * K + slot] : 0.0;
    block_sum(acc, red);
    if (tid == 0) totals[slot] = acc;
}

__global__ __launch_bounds__(TEMPER_THREADS) void temper_logits_kernel(const float* logits, int64_t total, float beta, float* out) {
    const int64_t stride = (int64_t)gridDim.x * TEMPER_THREADS;
    for (int64_t i = (int64_t)blockIdx.x * TEMPER_THREADS + threadIdx.x; i < total; i += stride) out[i] = logits[i] * beta;
}

static bool temper_beta_ok(double b) { return b > 0.0 && b < INFINITY; }

// stream-ordered scratch of a call that is given neither row_stats nor state
static size_t temper_scratch_bytes(int64_t N, int K, bool need_stats, bool need_state) {
    size_t stats = need_stats ? (size_t)N * K * 3 * sizeof(double) : 0;
    size_t st = need_state ? (((size_t)N + 15) & ~(size_t)15) : 0;
    return stats + st;
}

static int temper_sizes(const char* who, int64_t N, int C, int K) {
    if (N < 0) { pg_set_error("%s: N = %lld", who, (long long)N); return PG_EINVAL; }
    if (N > 0x7fffffffLL) { pg_set_error("%s: N = %lld exceeds 2^31 - 1", who, (long long)N); return PG_EINVAL; }
    if (C < 1) { pg_set_error("%s: C must be at least 1 (got %d)", who, C); return PG_EINVAL; }
    if (K < 1 || K > TEMPER_MAX_K) { pg_set_error("%s: K must be 1 .. %d (got %d)", who, TEMPER_MAX_K, K); return PG_EINVAL; }
    return PG_OK;
}

extern "C" int pg_temper_plan(int64_t N, int C, int K, int32_t out[4]) {
    if (!out) { pg_set_error("temper_plan: null argument out"); return PG_EINVAL; }
    const int rc = temper_sizes("temper_plan", N, C, K);
    if (rc != PG_OK) return rc;
    const size_t bytes = temper_scratch_bytes(N, K, true, true);
    out[0] = TEMPER_THREADS;
    out[1] = TEMPER_GROUP;
    out[2] = 3 * K + 1;
    out[3] = bytes > 0x7fffffffull ? 0x7fffffff : (int32_t)bytes;
    return PG_OK;
}

extern "C" int pg_temper_stats(const float* logits, int64_t N, int C, const int64_t* labels, const double* betas, int K,
                               double* row_stats, double* conf, uint8_t* state, double* totals, int64_t* counts, void* stream) {
    const int rc = temper_sizes("temper_stats", N, C, K);
    if (rc != PG_OK) return rc;
    PG_NEED("temper_stats", betas);
    TemperBetas B;
    for (int k = 0; k < TEMPER_MAX_K; ++k) B.b[k] = 1.0;
    for (int k = 0; k < K; ++k) {
        if (!temper_beta_ok(betas[k])) {
            pg_set_error("temper_stats: betas[%d] = %g is not a finite positive number", k, betas[k]); return PG_EINVAL;
        }
        B.b[k] = betas[k];
    }
    PG_NEED("temper_stats", totals);
    PG_NEED("temper_stats", counts);
    if (N > 0) {
        PG_NEED("temper_stats", logits);
        PG_NEED("temper_stats", labels);
    }
    hipStream_t s = (hipStream_t)stream;
    if (N == 0) {
        PG_HIP(hipMemsetAsync(totals, 0, (size_t)K * 3 * sizeof(double), s));
        PG_HIP(hipMemsetAsync(counts, 0, 2 * sizeof(int64_t), s));
        return PG_OK;
    }
    char* scratch = nullptr;
    const size_t bytes = temper_scratch_bytes(N, K, !row_stats, !state);
    if (bytes) PG_HIP(hipMallocAsync((void**)&scratch, bytes, s));
    uint8_t* st = state ? state : (uint8_t*)scratch;                               // the state first: both parts stay 16-byte aligned
    double* rs = row_stats ? row_stats : (double*)(scratch + temper_scratch_bytes(N, K, false, !state));
    hipLaunchKernelGGL(temper_row_kernel, dim3((unsigned)N), dim3(TEMPER_THREADS), 0, s, logits, C, labels, B, K, rs, conf, st);
    int out = pg_check_launch("temper_stats");
    if (out == PG_OK) {
        hipLaunchKernelGGL(temper_totals_kernel, dim3((unsigned)(3 * K + 1)), dim3(TEMPER_THREADS), 0, s, rs, st, N, K, totals, counts);
        out = pg_check_launch("temper_stats (totals)");
    }
    if (scratch) (void)hipFreeAsync(scratch, s);
    return out;
}

extern "C" int pg_temper_logits(const float* logits, int64_t N, int C, double beta, float* out, void* stream) {
    if (N < 0) { pg_set_error("temper_logits: N = %lld", (long long)N); return PG_EINVAL; }
    if (C < 1) { pg_set_error("temper_logits: C must be at least 1 (got %d)", C); return PG_EINVAL; }
    if (!temper_beta_ok(beta)) { pg_set_error("temper_logits: beta = %g is not a finite positive number", beta); return PG_EINVAL; }
    if (N == 0) return PG_OK;
    PG_NEED("temper_logits", logits);
    PG_NEED("temper_logits", out);
    const int64_t total = N * (int64_t)C;
    const int64_t want = (total + TEMPER_THREADS - 1) / TEMPER_THREADS;
    const unsigned blocks = (unsigned)(want < (1 << 20) ? want : (1 << 20));
    hipLaunchKernelGGL(temper_logits_kernel, dim3(blocks), dim3(TEMPER_THREADS), 0, (hipStream_t)stream, logits, total, (float)beta, out);
    return pg_check_launch("temper_logits");
}
