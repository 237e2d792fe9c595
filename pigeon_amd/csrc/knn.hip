// knn.hip -- the k nearest rows of the embedding bank, exactly: pg_knn_prepare, pg_knn_workspace_bytes, pg_knn_search, pg_knn_plan,
// pg_tune_knn_spans (contract: include/pigeon_hip.h, restated in tests/_knnref.py).
//
// THE RESULT.  d2(q, x) is ONE fp32 chain, acc = fmaf(q[j] - x[j], q[j] - x[j], acc) for j = 0 .. 1023 ascending (knn_d2_step; the
// subtraction is rounded on its own).  A query's answer is the k rows of smallest d2, ascending, ties to the lower row, NaN after
// +inf.  Every comparison in this file is one unsigned 64-bit comparison of an ENTRY = (ordered key << 32) | row, where the ordered
// key (knn_ukey) is the float's bits mapped so that unsigned order is numeric order and every NaN is 0xffffffff; the entry of all
// ones is "nothing" (rows are below 2^32 - 1) and comes out as -1 / +inf.
//
// HOW IT IS REACHED.  Four launches on one stream in mode 0, no host synchronisation:
//   1. knn_filter_kernel (MFMA), grid (spans, ceil(B / 32)): a workgroup holds 32 queries as fp16 in LDS and walks its contiguous
//      span of bank rows in tiles of 128, wave w owning rows 32 w .. 32 w + 31 of the tile.  Lane l loads 16 bytes of x16 row l % 32
//      per K step straight into the B fragment; the A fragment is the queries' 16 bytes from LDS.  a(q, x) = hn[x] - q16 . x16 comes
//      out with the bank row on the lane and 16 queries in the accumulator registers.  The tile's ordered keys go through LDS to the
//      wave that owns the query (query i belongs to wave i % 4), which keeps the query's 128 smallest entries of the span in LDS:
//      an entry below the list's largest replaces it, and the largest is found again (knn_wave_insert).  The list is a set under a
//      total order, so it does not depend on the order of arrival.  The span's list goes to part_f (B, spans, 128).
//   2. knn_merge_kernel, by levels: a workgroup takes seven lists of a query through one 1024-entry bitonic sort in LDS and keeps the
//      128 smallest, level after level (256 -> 37 -> 6 -> 1) until one list is left: the 128 smallest entries of the bank (ascending)
//      go to cand, the key of the 128th to cutoff.
//   3. knn_rerank_kernel, one workgroup of 128 threads a query: thread i computes d2 of candidate i, the 128 entries are sorted, the
//      first k are the answer, and the certificate below is evaluated.
//   4. knn_exact_kernel + knn_merge_kernel: d2 of EVERY row for the queries that are not certified (all of them in mode 1), eight
//      queries a workgroup, 256 rows a tile (one row a thread, the bank staged through LDS in slabs of 32 columns), a running top-k
//      per query as in 1, the partial lists merged into idx / d2.  A workgroup none of whose queries needs it returns before it
//      reads the bank.
//
// THE CERTIFICATE.  Write Q = |q|, X = xmax >= |x| for every bank row, u = 2^-24.  For finite inputs that fp16 holds (|v| <= 65504):
//   conversion   |q16_j - q_j| <= 2^-11 |q_j| + 2^-25 (the second term is half the fp16 subnormal spacing), the same for x, so with
//                Cauchy-Schwarz and |v|_1 <= 32 |v|_2:  |q16 . x16 - q . x| <= 2^-10 Q X (1 + 2^-11) + 2^-20 (Q + X)(1 + 2^-11) + 2^-40
//   MFMA         products of two fp16 are exact in fp32; 1024 of them are added in an order and with a rounding the hardware does not
//                state: at most 2 u relative (truncation) per addition, 1024 additions: <= 2 * 1024 u Q X to first order
//   hn           0.5 |x|^2 summed in fp64 and rounded once: |hn - 0.5 |x|^2| <= 2^-25 X^2
//   subtraction  a = fl(hn - S): <= u (0.5 X^2 + Q X) to first order
//   eps(q) = 1.01 * [ (2^-10 + 2^-13 + 2^-24) Q X + 2^-24 X^2 + 2^-20 (Q + X) + 2^-40 ]      (1.01 pays every second-order term)
//   so |a(q, x) - (0.5 d2_true(q, x) - 0.5 Q^2)| <= eps(q) for every row.  A row that is no candidate has a >= cutoff, hence
//   d2_true >= 2 (cutoff - eps) + Q^2, and the exact stage computes for it at least that times (1 - 1030 u) (1026 u: the rounded
//   subtraction, squared, and 1024 fused additions; the rest second order).  Query b is certified when the k-th reranked d2 is
//   STRICTLY below that number: then no row outside the candidates can enter the top k, not even by the tie rule.  Q^2 is summed in
//   fp64 and taken 1e-12 low, X^2 = 2 max hn is taken 2^-22 high.  N <= 128: every row is a candidate, the query is certified.  A
//   non-finite or fp16-overflowing query value, or bank (stats[1] != 0: the filter and the merge return at once), certifies nothing.
//
// No float atomics, no input value forms an address or bounds a loop: a candidate row read back from the workspace is compared with n.
#include "common.h"
#include "pigeon_internal.h"

#include <cmath>

#define KNN_D 1024
#define KNN_KP 128                                   // K': candidates the filter keeps per query
#define KNN_TR 128                                   // filter: bank rows per tile (4 waves x 32)
#define KNN_QT 32                                    // filter: queries per workgroup
#define KNN_QLD (KNN_D + 8)                          // halves per query row in LDS: 2064 B, 16 lanes of a ds_read_b128 group on 64 banks
#define KNN_THREADS 256
#define KNN_SPANS 256                                // default number of spans: one workgroup per CU and query tile
#define KNN_ER 256                                   // exact tier: rows per tile (one a thread)
#define KNN_EQ 8                                     // exact tier: queries per workgroup
#define KNN_EKC 32                                   // exact tier: columns per staged slab
#define KNN_ELD (KNN_ER + 1)
#define KNN_ESPANS 512
#define KNN_MERGE 1024                               // entries the merge sorts at once
#define KNN_KMAX 64
#define KNN_NONE 0xffffffffffffffffULL
#define KNN_FILTER_LDS (KNN_QT * KNN_QLD * 2 + KNN_QT * KNN_KP * 8 + KNN_QT * KNN_TR * 4 + KNN_QT * 16)
#define KNN_EXACT_LDS (KNN_D * KNN_EQ * 4 + KNN_EKC * KNN_ELD * 4 + KNN_EQ * KNN_ER * 4 + KNN_EQ * KNN_KMAX * 8 + KNN_EQ * 16 + 64)

static int g_knn_spans = 0;                          // pg_tune_knn_spans: 0 = the defaults

// ------------------------------------------------------------------------------------------------ the order
__device__ __forceinline__ uint32_t knn_ukey(float v) {
    if (v != v) return 0xffffffffu;
    const uint32_t u = __builtin_bit_cast(uint32_t, v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float knn_unkey(uint32_t k) {
    if (k > 0xff800000u) return NAN;                                          // above +inf: a NaN
    return __builtin_bit_cast(float, (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}
__device__ __forceinline__ uint64_t knn_entry(uint32_t ukey, uint32_t row) { return ((uint64_t)ukey << 32) | row; }

// one step of THE chain
__device__ __forceinline__ float knn_d2_step(float acc, float q, float x) {
    const float t = __fsub_rn(q, x);
    return __fmaf_rn(t, t, acc);
}

// A wave keeps `cap` entries (lane + 64 i < cap) and their largest.  `e` replaces the largest; the largest is found again.
template <int EPL>
__device__ __forceinline__ void knn_wave_insert(uint64_t (&l)[EPL], int cap, int lane, uint64_t& worst, int& wpos, uint64_t e) {
#pragma unroll
    for (int i = 0; i < EPL; ++i)
        if (wpos == lane + 64 * i) l[i] = e;
    uint64_t m = 0;
#pragma unroll
    for (int i = 0; i < EPL; ++i)
        if (lane + 64 * i < cap && l[i] > m) m = l[i];
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const uint64_t other = __shfl_xor((unsigned long long)m, o, 64);
        m = other > m ? other : m;
    }
    worst = m;
    wpos = 0;
#pragma unroll
    for (int i = EPL - 1; i >= 0; --i) {
        const unsigned long long hit = __ballot(lane + 64 * i < cap && l[i] == m);
        if (hit) wpos = 64 * i + (int)__builtin_ctzll(hit);
    }
}
// every lane offers one entry; those below the largest are inserted in lane order.  Returns whether the list changed (the largest
// need not: while the list still holds "nothing" entries, one of them is replaced and the largest is the next).
template <int EPL>
__device__ __forceinline__ bool knn_wave_offer(uint64_t (&l)[EPL], int cap, int lane, uint64_t& worst, int& wpos, uint64_t e) {
    unsigned long long m = __ballot(e < worst);
    bool changed = false;
    while (m) {
        const int src = (int)__builtin_ctzll(m);
        const uint64_t ev = __shfl((unsigned long long)e, src, 64);
        if (ev < worst) { knn_wave_insert<EPL>(l, cap, lane, worst, wpos, ev); changed = true; }
        m &= m - 1;
    }
    return changed;
}

// ------------------------------------------------------------------------------------------------ prepare
// one workgroup a row: the fp16 copy, hn = fp32(0.5 sum x^2) summed in fp64 (thread t: elements 4 t .. 4 t + 3, then row_block's
// order), and the bank's statistics by integer atomics (a maximum of non-negative float bits and a count: order-free)
__global__ __launch_bounds__(KNN_THREADS) void knn_prepare_kernel(const float* __restrict__ x, int64_t n, _Float16* __restrict__ x16,
                                                                  float* __restrict__ hn, unsigned long long* __restrict__ stats) {
    __shared__ double red[4];
    __shared__ int redbad[4];
    __shared__ float redmax[4];
    const int tid = threadIdx.x;
    const int64_t row = blockIdx.x;
    const f32x4 v = *(const f32x4*)(x + row * KNN_D + 4 * tid);
    double s = 0.0;
    int bad = 0;
    float mx = 0.f;
    uint16_t h[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float a = fabsf(v[i]);
        bad += !(a <= 65504.f);                                               // NaN, +-inf and what fp16 cannot hold
        mx = (a <= 65504.f && a > mx) ? a : mx;
        s = fma((double)v[i], (double)v[i], s);
        h[i] = __builtin_bit_cast(uint16_t, (_Float16)v[i]);                 // v_cvt_f16_f32: round to nearest even
    }
    u32x2 packed = {(uint32_t)h[0] | ((uint32_t)h[1] << 16), (uint32_t)h[2] | ((uint32_t)h[3] << 16)};
    *(u32x2*)(x16 + row * KNN_D + 4 * tid) = packed;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        s += __shfl_xor(s, o, 64);
        bad += __shfl_xor(bad, o, 64);
        mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    }
    if ((tid & 63) == 0) { red[tid >> 6] = s; redbad[tid >> 6] = bad; redmax[tid >> 6] = mx; }
    __syncthreads();
    if (tid == 0) {
        const float half_norm = (float)(0.5 * ((red[0] + red[1]) + (red[2] + red[3])));
        hn[row] = half_norm;
        const int nbad = redbad[0] + redbad[1] + redbad[2] + redbad[3];
        const float m = fmaxf(fmaxf(redmax[0], redmax[1]), fmaxf(redmax[2], redmax[3]));
        if (nbad) atomicAdd(&stats[1], (unsigned long long)nbad);
        else atomicMax(&stats[0], (unsigned long long)__builtin_bit_cast(uint32_t, half_norm));     // finite and >= +0
        atomicMax(&stats[2], (unsigned long long)__builtin_bit_cast(uint32_t, m));
    }
}

// ------------------------------------------------------------------------------------------------ 1. the filter
__global__ __launch_bounds__(KNN_THREADS) void knn_filter_kernel(const _Float16* __restrict__ x16, const float* __restrict__ hn,
                                                                 const float* __restrict__ q, int B, int64_t n, int tiles, int tps,
                                                                 int spans, const unsigned long long* __restrict__ stats,
                                                                 uint64_t* __restrict__ part) {
    extern __shared__ __attribute__((aligned(16))) unsigned char knn_lds[];
    if (stats[1] != 0) return;                                               // a bank fp16 cannot hold: the exact tier answers
    _Float16* qs = (_Float16*)knn_lds;
    uint64_t* list = (uint64_t*)(knn_lds + KNN_QT * KNN_QLD * 2);
    uint32_t* tk = (uint32_t*)(knn_lds + KNN_QT * KNN_QLD * 2 + KNN_QT * KNN_KP * 8);
    uint64_t* worst = (uint64_t*)(knn_lds + KNN_QT * KNN_QLD * 2 + KNN_QT * KNN_KP * 8 + KNN_QT * KNN_TR * 4);
    int* wpos = (int*)(worst + KNN_QT);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int span = blockIdx.x, q0 = blockIdx.y * KNN_QT;
    for (int i = tid; i < KNN_QT * (KNN_D / 4); i += KNN_THREADS) {
        const int qi = i >> 8, j = (i & 255) * 4;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (q0 + qi < B) v = *(const f32x4*)(q + (int64_t)(q0 + qi) * KNN_D + j);
        _Float16* d = qs + qi * KNN_QLD + j;
#pragma unroll
        for (int e = 0; e < 4; ++e) d[e] = (_Float16)v[e];
    }
    for (int i = tid; i < KNN_QT * KNN_KP; i += KNN_THREADS) list[i] = KNN_NONE;
    if (tid < KNN_QT) { worst[tid] = KNN_NONE; wpos[tid] = 0; }
    __syncthreads();
    const int r = lane & 31, h = lane >> 5;
    const int nq = B - q0 < KNN_QT ? B - q0 : KNN_QT;                        // the slots past B hold zeros and no list
    const int t0 = span * tps, t1 = (t0 + tps < tiles) ? t0 + tps : tiles;
    for (int t = t0; t < t1; ++t) {
        const int64_t base = (int64_t)t * KNN_TR;
        int64_t row = base + wave * 32 + r;
        if (row >= n) row = n - 1;                                           // loaded, never offered
        const f16x8* bp = (const f16x8*)(x16 + row * KNN_D + 8 * h);
        const _Float16* ap = qs + r * KNN_QLD + 8 * h;
        f32x16 acc;
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[i] = 0.f;
#pragma unroll 8
        for (int ks = 0; ks < KNN_D / 16; ++ks) {
            const f16x8 b = bp[2 * ks];                                      // 16 halves a step: this lane's 8 at + 8 h
            const f16x8 a = *(const f16x8*)(ap + 16 * ks);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, acc, 0, 0, 0);
        }
        const float hnr = hn[row];
#pragma unroll
        for (int i = 0; i < 16; ++i) {                                       // C/D map: column (bank row) = lane % 32, row (query) below
            const int qi = (i & 3) + 8 * (i >> 2) + 4 * h;
            tk[qi * KNN_TR + wave * 32 + r] = knn_ukey(hnr - acc[i]);
        }
        __syncthreads();
        for (int qi = wave; qi < nq; qi += 4) {
            uint64_t l[2] = {list[qi * KNN_KP + lane], list[qi * KNN_KP + 64 + lane]};
            uint64_t w = worst[qi];
            int wp = wpos[qi];
            bool changed = false;
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int64_t rr = base + lane + 64 * i;
                const uint64_t e = rr < n ? knn_entry(tk[qi * KNN_TR + lane + 64 * i], (uint32_t)rr) : KNN_NONE;
                changed |= knn_wave_offer<2>(l, KNN_KP, lane, w, wp, e);
            }
            if (changed) {
                list[qi * KNN_KP + lane] = l[0];
                list[qi * KNN_KP + 64 + lane] = l[1];
                if (lane == 0) { worst[qi] = w; wpos[qi] = wp; }
            }
        }
        __syncthreads();
    }
    for (int i = tid; i < KNN_QT * KNN_KP; i += KNN_THREADS) {
        const int qi = i >> 7;
        if (q0 + qi < B) part[((int64_t)(q0 + qi) * spans + span) * KNN_KP + (i & 127)] = list[i];
    }
}

// ------------------------------------------------------------------------------------------------ 2. the merge
// Workgroup (b, g) of a level: the `keep` smallest of query b's lists [g per, (g + 1) per) of `len` entries each, ascending.  A level
// of several groups writes them to out_part (B, groups, keep), the next level's lists; the last level (one group) writes, final == 0,
// cand (B, keep) and the keep-th key to cutoff, or, final == 1, idx / d2 (B, keep) decoded.  A query whose skip flag is set is left alone.
__global__ __launch_bounds__(KNN_THREADS) void knn_merge_kernel(const uint64_t* __restrict__ part, int lists, int len, int keep, int per,
                                                                const uint8_t* __restrict__ skip, const unsigned long long* __restrict__ stats,
                                                                uint64_t* __restrict__ out_part, int final, uint64_t* __restrict__ cand,
                                                                float* __restrict__ cutoff, int64_t* __restrict__ idx, float* __restrict__ d2) {
    __shared__ uint64_t buf[KNN_MERGE];
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x;
    if (skip && skip[b]) return;
    if (stats && stats[1] != 0) return;
    const int l0 = blockIdx.y * per, l1 = l0 + per < lists ? l0 + per : lists;
    const int64_t total = (int64_t)(l1 - l0) * len;
    const uint64_t* src = part + (b * lists + l0) * len;
    int S = 256;
    while (S < KNN_MERGE && S < keep + total) S <<= 1;
    for (int i = tid; i < keep; i += KNN_THREADS) buf[i] = KNN_NONE;
    int64_t done = 0;
    do {
        for (int i = keep + tid; i < S; i += KNN_THREADS) {
            const int64_t j = done + (i - keep);
            buf[i] = j < total ? src[j] : KNN_NONE;
        }
        done += S - keep;
        __syncthreads();
        for (int k = 2; k <= S; k <<= 1)
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int i = tid; i < S; i += KNN_THREADS) {
                    const int p = i ^ j;
                    if (p > i) {
                        const uint64_t a = buf[i], c = buf[p];
                        if ((a > c) == ((i & k) == 0)) { buf[i] = c; buf[p] = a; }
                    }
                }
                __syncthreads();
            }
    } while (done < total);
    for (int i = tid; i < keep; i += KNN_THREADS) {
        const uint64_t e = buf[i];
        if (out_part) {
            out_part[(b * gridDim.y + blockIdx.y) * keep + i] = e;
        } else if (final) {
            idx[b * keep + i] = e == KNN_NONE ? -1 : (int64_t)(uint32_t)e;
            d2[b * keep + i] = e == KNN_NONE ? INFINITY : knn_unkey((uint32_t)(e >> 32));
        } else {
            cand[b * keep + i] = e;
            if (i == keep - 1) cutoff[b] = e == KNN_NONE ? INFINITY : knn_unkey((uint32_t)(e >> 32));
        }
    }
}

// ------------------------------------------------------------------------------------------------ 3. the rerank and the certificate
__global__ __launch_bounds__(KNN_KP) void knn_rerank_kernel(const float* __restrict__ x, int64_t n, const float* __restrict__ q,
                                                            const int64_t* __restrict__ exclude, int k, const uint64_t* __restrict__ cand,
                                                            const float* __restrict__ cutoff, const unsigned long long* __restrict__ stats,
                                                            int64_t* __restrict__ idx, float* __restrict__ d2, uint8_t* __restrict__ cert,
                                                            uint8_t* __restrict__ certified) {
    __shared__ __attribute__((aligned(16))) float qs[KNN_D];
    __shared__ uint64_t buf[KNN_KP];
    __shared__ double red[2];
    __shared__ int redbad[2];
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x;
    const bool bank_bad = stats[1] != 0;
    if (bank_bad) {                                                          // nothing was filtered: nothing to read
        if (tid < k) { idx[b * k + tid] = -1; d2[b * k + tid] = INFINITY; }
        if (tid == 0) { cert[b] = 0; if (certified) certified[b] = 0; }
        return;
    }
    const float* qrow = q + b * KNN_D;
    double s = 0.0;
    int bad = 0;
    for (int j = tid * 8; j < tid * 8 + 8; ++j) {
        const float v = qrow[j];
        qs[j] = v;
        bad |= !(fabsf(v) <= 65504.f);
        s = fma((double)v, (double)v, s);
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) { s += __shfl_xor(s, o, 64); bad |= __shfl_xor(bad, o, 64); }
    if ((tid & 63) == 0) { red[tid >> 6] = s; redbad[tid >> 6] = bad; }
    __syncthreads();
    const uint64_t e = cand[b * KNN_KP + tid];
    const int64_t ex = exclude ? exclude[b] : -1;
    const uint32_t row = (uint32_t)e;
    uint64_t mine = KNN_NONE;
    if (e != KNN_NONE && (int64_t)row < n && (int64_t)row != ex) {
        const f32x4* xr = (const f32x4*)(x + (int64_t)row * KNN_D);
        float acc = 0.f;
        for (int j = 0; j < KNN_D / 4; ++j) {
            const f32x4 xv = xr[j];
            const f32x4 qv = *(const f32x4*)(qs + 4 * j);
#pragma unroll
            for (int c = 0; c < 4; ++c) acc = knn_d2_step(acc, qv[c], xv[c]);
        }
        mine = knn_entry(knn_ukey(acc), row);
    }
    buf[tid] = mine;
    __syncthreads();
    for (int kk = 2; kk <= KNN_KP; kk <<= 1)
        for (int j = kk >> 1; j > 0; j >>= 1) {
            const int p = tid ^ j;
            if (p > tid) {
                const uint64_t a = buf[tid], c = buf[p];
                if ((a > c) == ((tid & kk) == 0)) { buf[tid] = c; buf[p] = a; }
            }
            __syncthreads();
        }
    if (tid < k) {
        const uint64_t o = buf[tid];
        idx[b * k + tid] = o == KNN_NONE ? -1 : (int64_t)(uint32_t)o;
        d2[b * k + tid] = o == KNN_NONE ? INFINITY : knn_unkey((uint32_t)(o >> 32));
    }
    if (tid == 0) {
        int ok;
        if (n <= KNN_KP) ok = 1;                                             // every row is a candidate
        else {
            const double u = 5.9604644775390625e-08;                         // 2^-24
            const double qq = red[0] + red[1];
            const double Q = sqrt(qq) * (1.0 + 1e-12);
            const double X = sqrt(2.0 * (double)__builtin_bit_cast(float, (uint32_t)stats[0]) * (1.0 + 4.0 * u));
            const double eps = 1.01 * ((0.0009765625 + 0.0001220703125 + u) * Q * X + u * X * X + 9.5367431640625e-07 * (Q + X) + 9.094947017729282e-13);
            const double lb = 2.0 * ((double)cutoff[b] - eps) + qq * (1.0 - 1e-12);
            const double lbc = lb * (1.0 - 1030.0 * u);
            const uint64_t kth = buf[k - 1];
            const double dk = kth == KNN_NONE ? (double)INFINITY : (double)knn_unkey((uint32_t)(kth >> 32));
            ok = !(redbad[0] | redbad[1]) && lb > 0.0 && dk < lbc;           // false for any NaN
        }
        cert[b] = (uint8_t)ok;
        if (certified) certified[b] = (uint8_t)ok;
    }
}

// ------------------------------------------------------------------------------------------------ 4. the exact tier
__global__ __launch_bounds__(KNN_THREADS) void knn_exact_kernel(const float* __restrict__ x, int64_t n, const float* __restrict__ q, int B,
                                                                const int64_t* __restrict__ exclude, int k, const uint8_t* __restrict__ skip,
                                                                int tiles, int tps, int spans, uint64_t* __restrict__ part) {
    extern __shared__ __attribute__((aligned(16))) unsigned char knn_lds[];
    float* qs = (float*)knn_lds;                                             // [column][slot]
    float* xs = qs + KNN_D * KNN_EQ;                                         // [column of the slab][row], row stride 257
    uint32_t* tk = (uint32_t*)(xs + KNN_EKC * KNN_ELD);                      // [slot][row]
    static_assert((KNN_D * KNN_EQ * 4 + KNN_EKC * KNN_ELD * 4 + KNN_EQ * KNN_ER * 4) % 8 == 0, "the lists are 8-byte entries");
    uint64_t* list = (uint64_t*)(knn_lds + KNN_D * KNN_EQ * 4 + KNN_EKC * KNN_ELD * 4 + KNN_EQ * KNN_ER * 4);
    uint64_t* worst = list + KNN_EQ * KNN_KMAX;
    int* wpos = (int*)(worst + KNN_EQ);
    __shared__ int slot_q[KNN_EQ];
    __shared__ int nslots;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int span = blockIdx.x, q0 = blockIdx.y * KNN_EQ;
    if (tid == 0) {
        int ns = 0;
        for (int i = 0; i < KNN_EQ; ++i)
            if (q0 + i < B && !(skip && skip[q0 + i])) slot_q[ns++] = q0 + i;
        nslots = ns;
    }
    __syncthreads();
    const int ns = nslots;
    if (ns == 0) return;                                                     // every query of the tile is certified
    for (int i = tid; i < KNN_D * KNN_EQ; i += KNN_THREADS) {
        const int s = i >> 10, j = i & 1023;
        qs[j * KNN_EQ + s] = s < ns ? q[(int64_t)slot_q[s] * KNN_D + j] : 0.f;
    }
    for (int i = tid; i < KNN_EQ * KNN_KMAX; i += KNN_THREADS) list[i] = KNN_NONE;
    if (tid < KNN_EQ) { worst[tid] = KNN_NONE; wpos[tid] = 0; }
    int64_t ex[KNN_EQ];
#pragma unroll
    for (int s = 0; s < KNN_EQ; ++s) ex[s] = -1;
    __syncthreads();
    if (exclude) {
#pragma unroll
        for (int s = 0; s < KNN_EQ; ++s)
            if (s < ns) ex[s] = exclude[slot_q[s]];
    }
    const int t0 = span * tps, t1 = (t0 + tps < tiles) ? t0 + tps : tiles;
    for (int t = t0; t < t1; ++t) {
        const int64_t base = (int64_t)t * KNN_ER;
        float acc[KNN_EQ];
#pragma unroll
        for (int s = 0; s < KNN_EQ; ++s) acc[s] = 0.f;
        for (int c0 = 0; c0 < KNN_D; c0 += KNN_EKC) {
#pragma unroll
            for (int i = 0; i < KNN_ER * KNN_EKC / 4 / KNN_THREADS; ++i) {   // 8 lanes read 128 contiguous bytes of one row
                const int f = tid + KNN_THREADS * i, rr = f >> 3, c4 = (f & 7) * 4;
                int64_t row = base + rr;
                if (row >= n) row = n - 1;
                const f32x4 v = *(const f32x4*)(x + row * KNN_D + c0 + c4);
#pragma unroll
                for (int e = 0; e < 4; ++e) xs[(c4 + e) * KNN_ELD + rr] = v[e];
            }
            __syncthreads();
#pragma unroll 4
            for (int c = 0; c < KNN_EKC; ++c) {
                const float xv = xs[c * KNN_ELD + tid];
                const f32x4 qa = *(const f32x4*)(qs + (c0 + c) * KNN_EQ);
                const f32x4 qb = *(const f32x4*)(qs + (c0 + c) * KNN_EQ + 4);
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    acc[s] = knn_d2_step(acc[s], qa[s], xv);
                    acc[4 + s] = knn_d2_step(acc[4 + s], qb[s], xv);
                }
            }
            __syncthreads();
        }
        const int64_t myrow = base + tid;
#pragma unroll
        for (int s = 0; s < KNN_EQ; ++s) tk[s * KNN_ER + tid] = (myrow < n && myrow != ex[s]) ? knn_ukey(acc[s]) : 0u;
        // 0 is no key of a d2 (the chain never leaves [+0, +inf] or NaN, whose keys have the top bit set): it marks "do not offer"
        __syncthreads();
        for (int s = wave; s < ns; s += 4) {
            uint64_t l[1] = {list[s * KNN_KMAX + lane]};
            uint64_t w = worst[s];
            int wp = wpos[s];
            bool changed = false;
#pragma unroll
            for (int i = 0; i < KNN_ER / 64; ++i) {
                const uint32_t key = tk[s * KNN_ER + lane + 64 * i];
                const uint64_t e = key ? knn_entry(key, (uint32_t)(base + lane + 64 * i)) : KNN_NONE;
                changed |= knn_wave_offer<1>(l, k, lane, w, wp, e);
            }
            if (changed) {
                list[s * KNN_KMAX + lane] = l[0];
                if (lane == 0) { worst[s] = w; wpos[s] = wp; }
            }
        }
        __syncthreads();
    }
    for (int i = tid; i < KNN_EQ * KNN_KMAX; i += KNN_THREADS) {
        const int s = i >> 6, j = i & 63;
        if (s < ns && j < k) part[((int64_t)slot_q[s] * spans + span) * k + j] = list[i];
    }
}

// nothing to search: every position is -1 / +inf, every query certified
__global__ __launch_bounds__(KNN_THREADS) void knn_empty_kernel(int64_t total, int B, int64_t* __restrict__ idx, float* __restrict__ d2,
                                                                uint8_t* __restrict__ certified) {
    const int64_t i = (int64_t)blockIdx.x * KNN_THREADS + threadIdx.x;
    if (i < total) { idx[i] = -1; d2[i] = INFINITY; }
    if (certified && i < B) certified[i] = 1;
}

// ------------------------------------------------------------------------------------------------ host
struct KnnPlan {
    int tiles_f, spans_f, tps_f, tiles_e, spans_e, tps_e;
    size_t part_f, cand, cutoff, cert, part_e, level, total;
};

// lists of `keep` entries that one workgroup of the merge takes in one sort, and the groups a level of `lists` lists has
static int knn_per(int keep) { return (KNN_MERGE - keep) / keep; }
static int knn_groups(int lists, int keep) { return (lists + knn_per(keep) - 1) / knn_per(keep); }

// the levels of one merge: lists -> groups -> ... -> 1, the outputs of a level alternating between the two level buffers
static int knn_merge(const char* what, const uint64_t* part, int lists, int keep, int B, const uint8_t* skip, const unsigned long long* stats,
                     uint64_t* level_a, uint64_t* level_b, int final, uint64_t* cand, float* cutoff, int64_t* idx, float* d2, hipStream_t s) {
    const int per = knn_per(keep);
    for (int flip = 0;; flip ^= 1) {
        const int groups = (lists + per - 1) / per;
        uint64_t* out = groups > 1 ? (flip ? level_b : level_a) : nullptr;
        hipLaunchKernelGGL(knn_merge_kernel, dim3((unsigned)B, (unsigned)groups), dim3(KNN_THREADS), 0, s, part, lists, keep, keep, per, skip, stats,
                           out, final, cand, cutoff, idx, d2);
        const int rc = pg_check_launch(what);
        if (rc != PG_OK || groups == 1) return rc;
        part = out;
        lists = groups;
    }
}

static KnnPlan knn_plan(int64_t n, int B, int k) {
    KnnPlan p;
    auto split = [](int64_t tiles, int want, int& spans, int& tps) {
        spans = (int)(g_knn_spans > 0 ? g_knn_spans : (tiles < want ? (tiles > 0 ? tiles : 1) : want));
        tps = (int)((tiles + spans - 1) / spans);
    };
    p.tiles_f = (int)((n + KNN_TR - 1) / KNN_TR);
    p.tiles_e = (int)((n + KNN_ER - 1) / KNN_ER);
    split(p.tiles_f, KNN_SPANS, p.spans_f, p.tps_f);
    split(p.tiles_e, KNN_ESPANS, p.spans_e, p.tps_e);
    auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    p.part_f = up((size_t)B * p.spans_f * KNN_KP * 8);
    p.cand = up((size_t)B * KNN_KP * 8);
    p.cutoff = up((size_t)B * 4);
    p.cert = up((size_t)B);
    p.part_e = up((size_t)B * p.spans_e * (size_t)k * 8);
    const size_t lf = (size_t)knn_groups(p.spans_f, KNN_KP) * KNN_KP, le = (size_t)knn_groups(p.spans_e, k) * (size_t)k;
    p.level = up((size_t)B * (lf > le ? lf : le) * 8);                       // one level's output; two of them, used in turn
    p.total = p.part_f + p.cand + p.cutoff + p.cert + p.part_e + 2 * p.level;
    return p;
}

static int knn_check_shape(const char* who, int64_t n, int B, int k) {
    if (n < 0 || n > 0x7ffffff0LL) { pg_set_error("%s: n = %lld (0 .. 2^31 - 16 rows)", who, (long long)n); return PG_EINVAL; }
    if (B < 0 || B > 262144) { pg_set_error("%s: B = %d (0 .. 262144 queries)", who, B); return PG_EINVAL; }
    if (k < 1 || k > KNN_KMAX) { pg_set_error("%s: k = %d (1 .. %d)", who, k, KNN_KMAX); return PG_EINVAL; }
    return PG_OK;
}

extern "C" int pg_tune_knn_spans(int spans) {
    if (spans < 0 || spans > 4096) { pg_set_error("tune_knn_spans: spans = %d (0 = default, 1 .. 4096)", spans); return PG_EINVAL; }
    g_knn_spans = spans;
    return PG_OK;
}

extern "C" int pg_knn_plan(int64_t n, int B, int k, int32_t out[8]) {
    PG_NEED("knn_plan", out);
    const int rc = knn_check_shape("knn_plan", n, B, k);
    if (rc != PG_OK) return rc;
    const KnnPlan p = knn_plan(n, B, k);
    out[0] = KNN_KP;
    out[1] = KNN_TR;
    out[2] = KNN_QT;
    out[3] = p.spans_f;
    out[4] = KNN_FILTER_LDS;
    out[5] = p.tps_f;
    out[6] = KNN_ER;
    out[7] = p.spans_e;
    return PG_OK;
}

extern "C" int pg_knn_workspace_bytes(int64_t n, int B, int k, size_t* bytes) {
    PG_NEED("knn_workspace_bytes", bytes);
    const int rc = knn_check_shape("knn_workspace_bytes", n, B, k);
    if (rc != PG_OK) return rc;
    *bytes = knn_plan(n, B, k).total;
    return PG_OK;
}

extern "C" int pg_knn_prepare(const float* x, int64_t n, void* x16, float* hn, uint64_t* stats, void* stream) {
    if (n < 0 || n > 0x7ffffff0LL) { pg_set_error("knn_prepare: n = %lld (0 .. 2^31 - 16 rows)", (long long)n); return PG_EINVAL; }
    PG_NEED("knn_prepare", stats);
    if (n > 0) {
        PG_NEED("knn_prepare", x);
        PG_NEED("knn_prepare", x16);
        PG_NEED("knn_prepare", hn);
        if (((uintptr_t)x & 15) || ((uintptr_t)x16 & 15)) { pg_set_error("knn_prepare: x and x16 must be 16-byte aligned"); return PG_EINVAL; }
    }
    hipStream_t s = (hipStream_t)stream;
    PG_HIP(hipMemsetAsync(stats, 0, 4 * sizeof(uint64_t), s));
    if (n == 0) return PG_OK;
    hipLaunchKernelGGL(knn_prepare_kernel, dim3((unsigned)n), dim3(KNN_THREADS), 0, s, x, n, (_Float16*)x16, hn, (unsigned long long*)stats);
    return pg_check_launch("knn_prepare");
}

extern "C" int pg_knn_search(const pg_knn_bank* bank, const float* q, int B, int k, const int64_t* exclude, int mode, int64_t* idx, float* d2,
                             uint8_t* certified, void* workspace, size_t workspace_bytes, void* stream) {
    PG_NEED("knn_search", bank);
    const int64_t n = bank->n;
    const int rc0 = knn_check_shape("knn_search", n, B, k);
    if (rc0 != PG_OK) return rc0;
    if (mode < 0 || mode > 2) { pg_set_error("knn_search: mode = %d (0 auto, 1 exact tier only, 2 filter and rerank only)", mode); return PG_EINVAL; }
    if (B == 0) return PG_OK;
    PG_NEED("knn_search", q);
    PG_NEED("knn_search", idx);
    PG_NEED("knn_search", d2);
    if ((uintptr_t)q & 15) { pg_set_error("knn_search: q must be 16-byte aligned"); return PG_EINVAL; }
    const KnnPlan p = knn_plan(n, B, k);
    if (n > 0) {
        PG_NEED("knn_search", bank->x);
        if ((uintptr_t)bank->x & 15) { pg_set_error("knn_search: bank->x must be 16-byte aligned"); return PG_EINVAL; }
        if (mode != 1) {
            PG_NEED("knn_search", bank->x16);
            PG_NEED("knn_search", bank->hn);
            PG_NEED("knn_search", bank->stats);
            if ((uintptr_t)bank->x16 & 15) { pg_set_error("knn_search: bank->x16 must be 16-byte aligned"); return PG_EINVAL; }
        }
        PG_NEED("knn_search", workspace);
        if ((uintptr_t)workspace & 255) { pg_set_error("knn_search: workspace must be 256-byte aligned"); return PG_EINVAL; }
        if (workspace_bytes < p.total) {
            pg_set_error("knn_search: workspace_bytes = %zu, pg_knn_workspace_bytes asks for %zu", workspace_bytes, p.total);
            return PG_EINVAL;
        }
    }
    hipStream_t s = (hipStream_t)stream;
    if (n == 0) {
        const int64_t total = (int64_t)B * k;
        hipLaunchKernelGGL(knn_empty_kernel, dim3((unsigned)((total + KNN_THREADS - 1) / KNN_THREADS)), dim3(KNN_THREADS), 0, s, total, B, idx, d2,
                           certified);
        return pg_check_launch("knn_search (empty bank)");
    }
    static bool attr_set = false;
    if (!attr_set) {
        PG_HIP(hipFuncSetAttribute((const void*)knn_filter_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, KNN_FILTER_LDS));
        PG_HIP(hipFuncSetAttribute((const void*)knn_exact_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, KNN_EXACT_LDS));
        attr_set = true;
    }
    char* ws = (char*)workspace;
    uint64_t* part_f = (uint64_t*)ws;
    uint64_t* cand = (uint64_t*)(ws + p.part_f);
    float* cutoff = (float*)(ws + p.part_f + p.cand);
    uint8_t* cert = (uint8_t*)(ws + p.part_f + p.cand + p.cutoff);
    uint64_t* part_e = (uint64_t*)(ws + p.part_f + p.cand + p.cutoff + p.cert);
    uint64_t* level_a = (uint64_t*)(ws + p.part_f + p.cand + p.cutoff + p.cert + p.part_e);
    uint64_t* level_b = (uint64_t*)(ws + p.part_f + p.cand + p.cutoff + p.cert + p.part_e + p.level);
    const unsigned long long* stats = (const unsigned long long*)bank->stats;
    int rc = PG_OK;
    if (mode != 1) {
        hipLaunchKernelGGL(knn_filter_kernel, dim3((unsigned)p.spans_f, (unsigned)((B + KNN_QT - 1) / KNN_QT)), dim3(KNN_THREADS), KNN_FILTER_LDS, s,
                           (const _Float16*)bank->x16, bank->hn, q, B, n, p.tiles_f, p.tps_f, p.spans_f, stats, part_f);
        rc = pg_check_launch("knn_search (filter)");
        if (rc != PG_OK) return rc;
        rc = knn_merge("knn_search (merge)", part_f, p.spans_f, KNN_KP, B, nullptr, stats, level_a, level_b, 0, cand, cutoff, nullptr, nullptr, s);
        if (rc != PG_OK) return rc;
        hipLaunchKernelGGL(knn_rerank_kernel, dim3((unsigned)B), dim3(KNN_KP), 0, s, bank->x, n, q, exclude, k, cand, cutoff, stats, idx, d2, cert,
                           certified);
        rc = pg_check_launch("knn_search (rerank)");
        if (rc != PG_OK) return rc;
    }
    if (mode != 2) {
        const uint8_t* skip = mode == 0 ? cert : nullptr;
        hipLaunchKernelGGL(knn_exact_kernel, dim3((unsigned)p.spans_e, (unsigned)((B + KNN_EQ - 1) / KNN_EQ)), dim3(KNN_THREADS), KNN_EXACT_LDS, s,
                           bank->x, n, q, B, exclude, k, skip, p.tiles_e, p.tps_e, p.spans_e, part_e);
        rc = pg_check_launch("knn_search (exact tier)");
        if (rc != PG_OK) return rc;
        rc = knn_merge("knn_search (exact merge)", part_e, p.spans_e, k, B, skip, nullptr, level_a, level_b, 1, nullptr, nullptr, idx, d2, s);
        if (rc != PG_OK) return rc;
        if (mode == 1 && certified) PG_HIP(hipMemsetAsync(certified, 1, (size_t)B, s));
    }
    return rc;
}
