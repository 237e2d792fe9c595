// spread.hip -- how far off a guess may be: pg_guess_spread (contract: include/pigeon_hip.h, restated in tests/_spreadref.py).
//
// The head leaves the (B, C) fp32 logits behind; per batch row b and query point g (G points per row, float64 [lng, lat]) this file
// computes, all in float64 and with the softmax weights w_c = exp(l[b,c] - max_c l[b,c]), Z = sum_c w_c:
//   expected_km     (sum_c w_c d_c) / Z,  d_c = pg_haversine_km(point, centroid c) -- haversine.h, the function pg_haversine_matrix runs
//   expected_score  (sum_c w_c 5000 exp(-d_c / 1492.7)) / Z: the GeoGuessr score before its rounding
//   radius[j]       min { key_c : M(key_c) >= q_j Z },  key_c = d_c + extent_c,  M(t) = sum over { c : key_c <= t } of w_c
// The reference has no code for this (layers/hedge.py opens with a TODO); the contract is this project's own.
//
// One workgroup of 256 threads per (row, point):
//   1. the logits row is read once, with 16-byte loads from the first 16-byte boundary on (up to 3 scalar elements on either side),
//      into the weight slots as doubles (exact); the row maximum and the NaN / +inf test ride along.
//   2. thread t owns cells t, t + 256, ...: weight, distance and key of each, in place; three sums.
//   3. the quantile is a SELECTION, not a sort: keys are non-negative doubles, so their bit patterns order like integers, and M(t) is
//      a monotone step function of that integer (every addition of a fixed-order sum of non-negative terms is monotone).  All nq
//      quantiles bisect [0, bits(+inf)] together, one masked sum per quantile and step, at most 63 steps; the smallest pattern with
//      M >= q Z is a key.
// Every sum over cells -- Z, the two numerators, every M -- is row_block.h's one summation order: it depends on C only, not on B, G,
// the row's position or its alignment (step 1 decides where a load goes, never what is added to what).  A masked cell adds +0.0, so
// M(+inf) is Z bit for bit and q = 1 needs no tolerance.  The (key, weight) pairs are the cells that row_block.h keeps in LDS or in
// scratch.
// No input value forms an address or bounds a loop: a NaN or +inf logit, a row of -inf only, a non-finite point, and a key that is
// not a finite non-negative number (non-finite centroid or extent) give NaN in every output of that (row, point) and nothing else.
#include "common.h"
#include "pigeon_internal.h"
#include "haversine.h"
#include "row_block.h"

#include <cmath>

#define SPREAD_THREADS 256
#define SPREAD_CELL_BYTES (2 * sizeof(double))       // key and weight
#define SPREAD_LDS_CELLS row_lds_cells(SPREAD_CELL_BYTES)
#define SPREAD_MAX_Q 4
#define SPREAD_INF_BITS 0x7ff0000000000000ull

struct SpreadQuantiles { double q[SPREAD_MAX_Q]; };

template <bool GLOBAL>
__global__ __launch_bounds__(SPREAD_THREADS) void guess_spread_kernel(const float* __restrict__ logits, int C,
                                                                      const double* __restrict__ centroids,
                                                                      const double* __restrict__ extent_km,
                                                                      const double* __restrict__ points, int G, SpreadQuantiles Q, int nq,
                                                                      double* __restrict__ expected_km, double* __restrict__ expected_score,
                                                                      double* __restrict__ radius_km, double* __restrict__ scratch) {
    extern __shared__ __attribute__((aligned(16))) double spread_cells[];
    // block_sum alternates between the two slots, so its one barrier per call is enough: a wave reaches the second next call only
    // after every wave has read this one
    __shared__ double red[2][4][SPREAD_MAX_Q];
    __shared__ float redmax[4];
    __shared__ int redbad[2][4];
    const int tid = threadIdx.x;
    const int64_t pair = blockIdx.x;                   // b * G + g
    const int64_t b = pair / G;
    double* keys = GLOBAL ? scratch + pair * 2 * (int64_t)C : spread_cells;
    double* wts = keys + C;

    // 1. the row, once
    const float* row = logits + b * (int64_t)C;
    int head = (int)((4 - (((uintptr_t)row >> 2) & 3)) & 3);
    head = head < C ? head : C;
    const int nvec = (C - head) >> 2;
    const int tail0 = head + 4 * nvec;
    float mx = -INFINITY;
    int bad = 0;
    if (tid < head) {
        const float v = row[tid];
        wts[tid] = (double)v; bad |= (v != v || v == INFINITY); mx = v > mx ? v : mx;
    }
    for (int i = tid; i < nvec; i += SPREAD_THREADS) {
        const f32x4 q = *(const f32x4*)(row + head + 4 * i);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float v = q[e];
            wts[head + 4 * i + e] = (double)v; bad |= (v != v || v == INFINITY); mx = v > mx ? v : mx;
        }
    }
    if (tail0 + tid < C) {
        const float v = row[tail0 + tid];
        wts[tail0 + tid] = (double)v; bad |= (v != v || v == INFINITY); mx = v > mx ? v : mx;
    }
    const double plng = points[2 * pair], plat = points[2 * pair + 1];
    bad |= !(fabs(plng) < INFINITY && fabs(plat) < INFINITY);
    if (GLOBAL) __threadfence_block();                 // the staged row is global memory: visible to the block's next pass
    block_max_flag(mx, bad, redmax, redbad[0]);
    bad |= !(mx > -INFINITY);                          // a row of -inf only
    const double m = (double)mx;

    // 2. weight, distance, key; Z and the two numerators
    double acc[SPREAD_MAX_Q] = {0.0, 0.0, 0.0, 0.0};
    if (!bad) {                                        // uniform: exp(l - m) needs a finite m
        for (int c = tid; c < C; c += SPREAD_THREADS) {
            const double w = exp(wts[c] - m);
            const double d = pg_haversine_km<double>(plng, plat, centroids[2 * (int64_t)c], centroids[2 * (int64_t)c + 1]);
            const double key = extent_km ? d + extent_km[c] : d;
            bad |= !(key >= 0.0 && key < INFINITY && d >= 0.0);
            keys[c] = key;
            wts[c] = w;
            acc[0] += w;
            acc[1] += w * d;
            acc[2] += w * PG_SCORE_MAX * exp(-d / PG_SCORE_DECAY_KM);
        }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) bad |= __shfl_xor(bad, o, 64);
    if ((tid & 63) == 0) redbad[1][tid >> 6] = bad;
    block_sum(acc, red[0]);
    bad = redbad[1][0] | redbad[1][1] | redbad[1][2] | redbad[1][3];
    if (bad) {                                         // uniform
        if (tid == 0) { expected_km[pair] = NAN; expected_score[pair] = NAN; }
        if (tid < nq) radius_km[pair * nq + tid] = NAN;
        return;
    }
    const double Z = acc[0];
    if (tid == 0) { expected_km[pair] = acc[1] / Z; expected_score[pair] = acc[2] / Z; }

    // 3. the quantiles: the smallest bit pattern u with M(u) >= q Z, all nq at once
    uint64_t lo[SPREAD_MAX_Q], hi[SPREAD_MAX_Q];
    double target[SPREAD_MAX_Q];
#pragma unroll
    for (int j = 0; j < SPREAD_MAX_Q; ++j) {
        lo[j] = 0;
        hi[j] = j < nq ? SPREAD_INF_BITS : 0;          // an unused slot is converged from the start
        target[j] = Q.q[j] * Z;
    }
    for (int step = 1; step <= 64; ++step) {           // hi - lo < 2^63 halves every step: 63 steps at the most
        uint64_t mid[SPREAD_MAX_Q];
        bool open = false;
#pragma unroll
        for (int j = 0; j < SPREAD_MAX_Q; ++j) { mid[j] = lo[j] + ((hi[j] - lo[j]) >> 1); open |= lo[j] < hi[j]; }
        if (!open) break;                              // uniform: lo and hi are the same in every thread
        double ms[SPREAD_MAX_Q] = {0.0, 0.0, 0.0, 0.0};
        for (int c = tid; c < C; c += SPREAD_THREADS) {
            const uint64_t k = (uint64_t)__double_as_longlong(keys[c]);
            const double w = wts[c];
#pragma unroll
            for (int j = 0; j < SPREAD_MAX_Q; ++j) ms[j] += k <= mid[j] ? w : 0.0;
        }
        block_sum(ms, red[step & 1]);
#pragma unroll
        for (int j = 0; j < SPREAD_MAX_Q; ++j) {
            if (lo[j] < hi[j]) {
                if (ms[j] >= target[j]) hi[j] = mid[j]; else lo[j] = mid[j] + 1;
            }
        }
    }
    if (tid == 0) {
#pragma unroll
        for (int j = 0; j < SPREAD_MAX_Q; ++j)
            if (j < nq) radius_km[pair * nq + j] = __longlong_as_double((long long)hi[j]);
    }
}

extern "C" int pg_guess_spread_plan(int C, int32_t out[4]) {
    return row_cells_plan("guess_spread_plan", C, SPREAD_LDS_CELLS, SPREAD_CELL_BYTES, SPREAD_THREADS, out);
}

extern "C" int pg_guess_spread(const float* logits, int B, int C, const double* centroids, const double* extent_km, const double* points,
                               int G, const double* quantiles, int nq, double* expected_km, double* expected_score, double* radius_km,
                               void* stream) {
    if (B < 0) { pg_set_error("guess_spread: B = %d", B); return PG_EINVAL; }
    if (G < 0) { pg_set_error("guess_spread: G = %d", G); return PG_EINVAL; }
    if (C < 1) { pg_set_error("guess_spread: C must be at least 1 (got %d)", C); return PG_EINVAL; }
    if (nq < 1 || nq > SPREAD_MAX_Q) { pg_set_error("guess_spread: nq must be 1 .. %d (got %d)", SPREAD_MAX_Q, nq); return PG_EINVAL; }
    PG_NEED("guess_spread", quantiles);
    SpreadQuantiles Q = {{1.0, 1.0, 1.0, 1.0}};
    for (int j = 0; j < nq; ++j) {
        if (!(quantiles[j] > 0.0 && quantiles[j] <= 1.0)) {
            pg_set_error("guess_spread: quantiles[%d] = %g is outside (0, 1]", j, quantiles[j]); return PG_EINVAL;
        }
        Q.q[j] = quantiles[j];
    }
    if (B == 0 || G == 0) return PG_OK;                    // nothing to do: the (empty) buffers may be NULL
    PG_NEED("guess_spread", logits);
    PG_NEED("guess_spread", centroids);
    PG_NEED("guess_spread", points);
    PG_NEED("guess_spread", expected_km);
    PG_NEED("guess_spread", expected_score);
    PG_NEED("guess_spread", radius_km);
    const int64_t pairs = (int64_t)B * G;
    if (pairs > 0x7fffffffLL) { pg_set_error("guess_spread: B * G = %lld exceeds 2^31 - 1", (long long)pairs); return PG_EINVAL; }
    hipStream_t s = (hipStream_t)stream;
    return row_cells_launch<guess_spread_kernel<false>, guess_spread_kernel<true>>(
        "guess_spread", "guess_spread (large C)", pairs, C, SPREAD_LDS_CELLS, SPREAD_CELL_BYTES, s,
        [&](auto kernel, size_t lds, void* scratch) {
            hipLaunchKernelGGL(kernel, dim3((unsigned)pairs), dim3(SPREAD_THREADS), lds, s, logits, C, centroids, extent_km, points, G, Q, nq,
                               expected_km, expected_score, radius_km, (double*)scratch);
        });
}
