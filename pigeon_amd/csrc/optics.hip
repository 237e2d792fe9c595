// optics.hip -- the prototype cluster table's device half: per-geocell OPTICS graphs over haversine distances.
//
// Replaces the distance matrix and `OPTICS(metric='precomputed').fit` of reference dataset_creation/prototype/prototype.py:121-149,
// which the reference runs one geocell at a time in 64 CPU processes.  The xi extraction that turns a graph into labels is O(n) and
// stays on the host (pigeon_amd/prototypes.py).  Everything here is fp64 with plain IEEE operations: this file is compiled with
// -ffp-contract=off (pigeon_amd/build.py), uses no fast-math, no inline assembly and no atomics, and no result depends on the launch
// geometry -- counts and lexicographic minima are exact whatever the order they are reduced in.
//
//   pg_haversine_blocks   the n x n distance matrix of every cell's own points, one launch for all cells: pg_haversine_matrix's fp64
//                         arithmetic (geo_proto.hip) on the upper triangle, mirrored, zeros and identical points as `zero_as`
//                         (prototype.py:130-133).
//   pg_optics_graph       sklearn.cluster._optics.compute_optics_graph(metric='precomputed', max_eps=inf), bit for bit:
//                           core[i]  = R(k-th smallest of row i, self included), k = min_samples
//                           reach[:] = inf; pred[:] = -1; repeat n times: p = the unprocessed point of smallest reach, ties (inf
//                           included) to the smallest index; mark it, append it to the ordering; for every unprocessed j:
//                           r = R(max(D[p,j], core[p])); if r < reach[j]: reach[j] = r, pred[j] = p
//                           R(x) = rint(x * 1e15) / 1e15   (np.around(x, 15), _optics.py:627-631, 712)
//                         core_kernel: one wave per row, the order statistic found bit by bit on the ordered bit pattern (64 counting
//                         passes over the row, wave-uniform counts from ballots).  order_kernel: one workgroup per cell, largest cells
//                         first; every thread owns the points j = tid, tid + T, ... -- their reach / pred / processed state is touched
//                         by no other thread -- so an iteration is one coalesced pass over row D[p,:] that updates the state and
//                         carries the thread's running minimum of (reach, index), one reduction and ONE barrier (the cross-wave scratch
//                         alternates between two buffers).  The state lives in LDS up to pg_optics_plan's out[2] points and in the
//                         output arrays plus a byte per point of stream-ordered scratch above that: the same code, the same bits.
#include "pigeon_internal.h"

#include <algorithm>
#include <cmath>
#include <vector>

#define OPTICS_MAX_POINTS 32768
#define OPTICS_LDS_POINTS 8192            // 13 bytes of LDS per point: 104 KiB of the CU's 160 KiB at the limit

static int g_lds_points = 0;              // pg_tune_optics_lds_points; 0 = OPTICS_LDS_POINTS

static int lds_points() { return g_lds_points > 0 ? g_lds_points : OPTICS_LDS_POINTS; }
static int plan_threads(int64_t n) { return n <= 128 ? 64 : (n <= 1024 ? 256 : 1024); }

extern "C" int pg_tune_optics_lds_points(int max_points) {
    if (max_points < 0 || max_points > OPTICS_LDS_POINTS) {
        pg_set_error("pg_tune_optics_lds_points: 0 (default %d) or 1 .. %d", OPTICS_LDS_POINTS, OPTICS_LDS_POINTS);
        return PG_EINVAL;
    }
    g_lds_points = max_points;
    return PG_OK;
}

static int check_cell_size(const char* who, int64_t c, int64_t n, int min_samples) {
    if (n < min_samples) {
        pg_set_error("%s: cell %lld has %lld points, fewer than min_samples = %d", who, (long long)c, (long long)n, min_samples);
        return PG_EINVAL;
    }
    if (n > OPTICS_MAX_POINTS) {
        pg_set_error("%s: cell %lld has %lld points, more than the %d a cell may hold", who, (long long)c, (long long)n, OPTICS_MAX_POINTS);
        return PG_EINVAL;
    }
    return PG_OK;
}

extern "C" int pg_optics_plan(int64_t n, int min_samples, int32_t out[4]) {
    if (!out) { pg_set_error("optics_plan: null argument"); return PG_EINVAL; }
    if (min_samples < 2) { pg_set_error("optics_plan: min_samples must be at least 2 (got %d)", min_samples); return PG_EINVAL; }
    if (int rc = check_cell_size("optics_plan", 0, n, min_samples)) return rc;
    out[0] = n > lds_points() ? 1 : 0;
    out[1] = plan_threads(n);
    out[2] = lds_points();
    out[3] = OPTICS_MAX_POINTS;
    return PG_OK;
}

// the cell of packed row r: the c with cell_off[c] <= r < cell_off[c + 1] (empty cells are stepped over)
__device__ __forceinline__ int cell_of_row(const int64_t* __restrict__ cell_off, int C, int64_t r) {
    int lo = 0, hi = C;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (cell_off[mid] <= r) lo = mid; else hi = mid;
    }
    return lo;
}

// --------------------------------------------------------------------------------------------- haversine blocks
// haversine_matrix_kernel<double> (geo_proto.hip) is compiled with the compiler's default contraction, this file without any.  Its
// code object fuses exactly two of the formula's operations -- the longitude difference and the sum under the root -- and those are
// written as fma() here; everything else (the library's sin / cos / asin / sqrt included) is the same instruction sequence in both.
// Element (i, j) with i <= j is that kernel's value for x = point i, y = point j, bit for bit (tests/test_gpu_optics.py pins it).  Two
// things differ, and both are what the reference's numpy matrix has and OPTICS at small min_samples depends on:
//   * a pair of IDENTICAL coordinates (the diagonal, exact duplicates) is `zero_as` without looking at the arithmetic.  numpy computes an
//     exact 0 there; the fused longitude difference x*D - round(x*D) is the rounding error of x*D, and the matrix kernel returns ~1e-13 km.
//   * the lower triangle mirrors the upper one.  numpy's matrix is exactly symmetric; the fused difference is not antisymmetric, so the
//     matrix kernel's (i, j) and (j, i) differ in the last bits.  D[a,b] == D[b,a] is a tie the graph's strict `r < reach` sees at
//     min_samples = 3 (core[a] = D[a,b], core[b] = D[b,a]): broken, predecessors and then xi labels change.  Only the longitude
//     difference depends on which point plays x (the latitude difference changes sign exactly, the cosines commute).
#define OPTICS_DEG2RAD 0.017453292519943295769236907684886127134428718885417
__global__ __launch_bounds__(256) void haversine_blocks_kernel(const double* __restrict__ pts, const int64_t* __restrict__ cell_off,
                                                               const int64_t* __restrict__ mat_off, int C, double zero_as,
                                                               double* __restrict__ out) {
    const int64_t r = (int64_t)blockIdx.x + cell_off[0];
    const int c = cell_of_row(cell_off, C, r);
    const int64_t first = cell_off[c], n = cell_off[c + 1] - first;
    const double xlng_deg = pts[2 * r], xlat_deg = pts[2 * r + 1];
    const double xlng = xlng_deg * OPTICS_DEG2RAD, xlat = xlat_deg * OPTICS_DEG2RAD;
    const int64_t i = r - first;
    double* __restrict__ row = out + mat_off[c] + i * n;
    for (int64_t j = threadIdx.x; j < n; j += 256) {
        const double ylng_deg = pts[2 * (first + j)], ylat_deg = pts[2 * (first + j) + 1];
        const double ylng = ylng_deg * OPTICS_DEG2RAD, ylat = ylat_deg * OPTICS_DEG2RAD;
        const double dlng = j >= i ? fma(xlng_deg, OPTICS_DEG2RAD, -ylng) : fma(ylng_deg, OPTICS_DEG2RAD, -xlng);
        const double dlat = xlat - ylat;
        const double p = cos(xlat) * cos(ylat);
        const double s1 = sin(dlat / 2), s0 = sin(dlng / 2);
        const double a = fma(s1, s1, p * (s0 * s0));
        const double cc = 2 * asin(sqrt(a));
        const double km = (6378137.0 * cc) / 1000;
        row[j] = (km == 0.0 || (xlng_deg == ylng_deg && xlat_deg == ylat_deg)) ? zero_as : km;
    }
}

// cell_off | mat_off (| order) -> one stream-ordered device buffer
static int upload_i64(const std::vector<int64_t>& host, int64_t** dev, hipStream_t s) {
    PG_HIP(hipMallocAsync((void**)dev, host.size() * sizeof(int64_t), s));
    hipError_t e = hipMemcpyAsync(*dev, host.data(), host.size() * sizeof(int64_t), hipMemcpyHostToDevice, s);
    if (e != hipSuccess) {
        (void)hipFreeAsync(*dev, s);
        pg_set_error("hipMemcpyAsync of the cell table failed: %s", hipGetErrorString(e));
        return PG_EHIP;
    }
    return PG_OK;
}

extern "C" int pg_haversine_blocks(const double* pts, const int64_t* cell_off, const int64_t* mat_off, int C, double zero_as,
                                   double* out, void* stream) {
    if (C < 0) { pg_set_error("haversine_blocks: negative cell count"); return PG_EINVAL; }
    if (C == 0) return PG_OK;
    if (!pts || !cell_off || !mat_off || !out) { pg_set_error("haversine_blocks: null argument"); return PG_EINVAL; }
    for (int c = 0; c < C; ++c) {
        const int64_t n = cell_off[c + 1] - cell_off[c];
        if (n < 0 || mat_off[c] < 0) { pg_set_error("haversine_blocks: cell %d has a negative size or offset", c); return PG_EINVAL; }
        if (mat_off[c + 1] - mat_off[c] < n * n) {
            pg_set_error("haversine_blocks: cell %d: mat_off leaves %lld elements for a %lld x %lld matrix", c,
                         (long long)(mat_off[c + 1] - mat_off[c]), (long long)n, (long long)n);
            return PG_EINVAL;
        }
    }
    const int64_t N = cell_off[C] - cell_off[0];
    if (N == 0) return PG_OK;
    if (N > 0x7fffffffLL) { pg_set_error("haversine_blocks: too many points"); return PG_EINVAL; }
    hipStream_t s = (hipStream_t)stream;
    std::vector<int64_t> tab(cell_off, cell_off + C + 1);
    tab.insert(tab.end(), mat_off, mat_off + C + 1);
    int64_t* dtab = nullptr;
    if (int rc = upload_i64(tab, &dtab, s)) return rc;
    // pts is indexed by the packed row itself (row r of pts is point r), so the kernel reads pts + 2 r with r from cell_off[0]
    hipLaunchKernelGGL(haversine_blocks_kernel, dim3((unsigned)N), dim3(256), 0, s, pts, dtab, dtab + C + 1, C, zero_as, out);
    int rc = pg_check_launch("haversine_blocks");
    (void)hipFreeAsync(dtab, s);
    if (rc == PG_OK) PG_HIP(hipStreamSynchronize(s));             // `tab` is the source of an asynchronous copy
    return rc;
}

// --------------------------------------------------------------------------------------------- OPTICS graph
__device__ __forceinline__ double round15(double x) { return rint(x * 1e15) / 1e15; }

// bit pattern -> an unsigned key with the order of the doubles (negative values included), and back
__device__ __forceinline__ unsigned long long order_key(double x) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(x);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double key_value(unsigned long long k) {
    return __longlong_as_double((long long)((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k));
}

// One wave per packed row.  res grows from the top bit down: after the step of bit b, the k-th smallest key lies in
// [res, res + 2^b) -- fewer than k keys are below res, at least k below res + 2^b.
__global__ __launch_bounds__(256) void optics_core_kernel(const double* __restrict__ dist, const int64_t* __restrict__ cell_off,
                                                          const int64_t* __restrict__ mat_off, int C, int k, int64_t N,
                                                          double* __restrict__ core) {
    const int lane = threadIdx.x & 63;
    const int64_t ri = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (ri >= N) return;                                           // whole waves leave; the kernel has no barrier
    const int64_t r = ri + cell_off[0];
    const int c = cell_of_row(cell_off, C, r);
    const int64_t first = cell_off[c];
    const int n = (int)(cell_off[c + 1] - first);
    const double* __restrict__ row = dist + mat_off[c] + (r - first) * (int64_t)n;
    unsigned long long res = 0;
    for (int bit = 63; bit >= 0; --bit) {
        const unsigned long long cand = res | (1ull << bit);
        int below = 0;
        for (int base = 0; base < n; base += 64) {
            const int j = base + lane;
            const bool lt = j < n && order_key(row[j]) < cand;
            below += __popcll(__ballot(lt));
        }
        if (below < k) res = cand;
    }
    if (lane == 0) core[ri] = round15(key_value(res));
}

template <int THREADS, bool GLOBAL>
__device__ __forceinline__ void optics_order_cell(const double* __restrict__ D, const int n, const double* __restrict__ core,
                                                  int64_t* __restrict__ ordering, double* __restrict__ reach_out,
                                                  int64_t* __restrict__ pred_out, unsigned char* __restrict__ done_g,
                                                  double* sm_reach, int* sm_pred, unsigned char* sm_done,
                                                  double (*red_r)[16], int (*red_i)[16]) {
    const int tid = threadIdx.x;
    const double inf = __longlong_as_double(0x7ff0000000000000ll);
    for (int j = tid; j < n; j += THREADS) {
        if (GLOBAL) { reach_out[j] = inf; pred_out[j] = -1; done_g[j] = 0; }
        else { sm_reach[j] = inf; sm_pred[j] = -1; sm_done[j] = 0; }
    }
    int p = 0;                                                     // every reach is inf: the smallest index
    for (int t = 0; t < n; ++t) {
        if (tid == 0) ordering[t] = p;
        if (p % THREADS == tid) { if (GLOBAL) done_g[p] = 1; else sm_done[p] = 1; }
        if (t == n - 1) break;
        const double cp = core[p];
        const double* __restrict__ row = D + (int64_t)p * n;
        double br = inf;
        int bi = 0x7fffffff;
        for (int j = tid; j < n; j += THREADS) {
            if (GLOBAL ? done_g[j] : sm_done[j]) continue;
            const double d = row[j];
            const double r = round15(d > cp ? d : cp);
            double rj = GLOBAL ? reach_out[j] : sm_reach[j];
            if (r < rj) {
                rj = r;
                if (GLOBAL) { reach_out[j] = r; pred_out[j] = p; } else { sm_reach[j] = r; sm_pred[j] = p; }
            }
            if (rj < br || (rj == br && j < bi)) { br = rj; bi = j; }
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const double r2 = __shfl_xor(br, off, 64);
            const int i2 = __shfl_xor(bi, off, 64);
            if (r2 < br || (r2 == br && i2 < bi)) { br = r2; bi = i2; }
        }
        if (THREADS > 64) {
            // two scratch buffers: a wave that runs ahead writes the OTHER one; it cannot come back to this one before every wave has
            // passed the next iteration's barrier, i.e. has finished reading it
            const int buf = t & 1;
            if ((tid & 63) == 0) { red_r[buf][tid >> 6] = br; red_i[buf][tid >> 6] = bi; }
            __syncthreads();
            br = red_r[buf][0]; bi = red_i[buf][0];
#pragma unroll
            for (int w = 1; w < THREADS / 64; ++w) {
                const double r2 = red_r[buf][w];
                const int i2 = red_i[buf][w];
                if (r2 < br || (r2 == br && i2 < bi)) { br = r2; bi = i2; }
            }
        }
        p = bi < n ? bi : n - 1;                                   // always bi < n (reach is never NaN); never index past the cell
    }
    if (!GLOBAL)
        for (int j = tid; j < n; j += THREADS) { reach_out[j] = sm_reach[j]; pred_out[j] = sm_pred[j]; }
}

// block b of the launch takes cell order[b]; the LDS image of a form-0 cell: reach double[n8] | pred int[n8] | done byte[n], n8 = n
// rounded up to 8
template <int THREADS>
__global__ __launch_bounds__(THREADS) void optics_order_kernel(const double* __restrict__ dist, const int64_t* __restrict__ cell_off,
                                                               const int64_t* __restrict__ mat_off, const int64_t* __restrict__ order,
                                                               const int lds_max_points, const double* __restrict__ core,
                                                               int64_t* __restrict__ ordering, double* __restrict__ reach,
                                                               int64_t* __restrict__ pred, unsigned char* __restrict__ done_ws) {
    extern __shared__ double optics_smem[];
    __shared__ double red_r[2][16];
    __shared__ int red_i[2][16];
    const int64_t c = order[blockIdx.x];
    const int64_t base = cell_off[0], first = cell_off[c];
    const int n = (int)(cell_off[c + 1] - first);
    const double* D = dist + mat_off[c];
    const int64_t o = first - base;                                // the outputs are packed from the first cell on
    if (n > lds_max_points) {
        optics_order_cell<THREADS, true>(D, n, core + o, ordering + o, reach + o, pred + o, done_ws + o, nullptr, nullptr, nullptr,
                                         red_r, red_i);
    } else {
        const int n8 = (n + 7) & ~7;
        double* sm_reach = optics_smem;
        int* sm_pred = (int*)(sm_reach + n8);
        unsigned char* sm_done = (unsigned char*)(sm_pred + n8);
        optics_order_cell<THREADS, false>(D, n, core + o, ordering + o, reach + o, pred + o, nullptr, sm_reach, sm_pred, sm_done,
                                          red_r, red_i);
    }
}

static size_t order_lds_bytes(int64_t n) { return (size_t)((n + 7) & ~(int64_t)7) * 12 + (size_t)((n + 15) & ~(int64_t)15); }

template <int THREADS>
static int launch_order(const double* dist, const int64_t* dtab, int C, const int64_t* dorder, int cells, int64_t lds_n,
                        const double* core, int64_t* ordering, double* reach, int64_t* pred, unsigned char* done_ws, hipStream_t s) {
    const size_t lds = lds_n > 0 ? order_lds_bytes(lds_n) : 0;
    static size_t attr_lds = 0;
    if (lds > attr_lds) {
        const size_t want = order_lds_bytes(OPTICS_LDS_POINTS);    // once: the most any launch of this kernel asks for
        PG_HIP(hipFuncSetAttribute((const void*)optics_order_kernel<THREADS>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)want));
        attr_lds = want;
    }
    hipLaunchKernelGGL(optics_order_kernel<THREADS>, dim3((unsigned)cells), dim3(THREADS), lds, s, dist, dtab, dtab + C + 1, dorder,
                       lds_points(), core, ordering, reach, pred, done_ws);
    return pg_check_launch("optics_order");
}

extern "C" int pg_optics_graph(const double* dist, const int64_t* cell_off, const int64_t* mat_off, int C, int min_samples,
                               int64_t* ordering, double* core, double* reach, int64_t* pred, void* stream) {
    if (C < 0) { pg_set_error("optics_graph: negative cell count"); return PG_EINVAL; }
    if (min_samples < 2) { pg_set_error("optics_graph: min_samples must be at least 2 (got %d)", min_samples); return PG_EINVAL; }
    if (C == 0) return PG_OK;
    if (!cell_off || !mat_off) { pg_set_error("optics_graph: null argument"); return PG_EINVAL; }
    for (int c = 0; c < C; ++c) {
        const int64_t n = cell_off[c + 1] - cell_off[c];
        if (int rc = check_cell_size("optics_graph", c, n, min_samples)) return rc;
        if (mat_off[c] < 0 || mat_off[c + 1] - mat_off[c] < n * n) {
            pg_set_error("optics_graph: cell %d: mat_off leaves %lld elements for a %lld x %lld matrix", c,
                         (long long)(mat_off[c + 1] - mat_off[c]), (long long)n, (long long)n);
            return PG_EINVAL;
        }
    }
    if (!dist || !ordering || !core || !reach || !pred) { pg_set_error("optics_graph: null argument"); return PG_EINVAL; }
    const int64_t N = cell_off[C] - cell_off[0];
    if (N > 0x7fffffffLL) { pg_set_error("optics_graph: too many points"); return PG_EINVAL; }
    hipStream_t s = (hipStream_t)stream;

    // largest cells first; the three thread counts are three contiguous runs of that order
    std::vector<int64_t> tab(cell_off, cell_off + C + 1);
    tab.insert(tab.end(), mat_off, mat_off + C + 1);
    std::vector<int64_t> ord(C);
    for (int c = 0; c < C; ++c) ord[c] = c;
    std::stable_sort(ord.begin(), ord.end(), [&](int64_t a, int64_t b) { return cell_off[a + 1] - cell_off[a] > cell_off[b + 1] - cell_off[b]; });
    tab.insert(tab.end(), ord.begin(), ord.end());
    const int lds_pts = lds_points();
    bool any_global = false;
    for (int c = 0; c < C; ++c) any_global = any_global || cell_off[c + 1] - cell_off[c] > lds_pts;

    int64_t* dtab = nullptr;
    if (int rc = upload_i64(tab, &dtab, s)) return rc;
    unsigned char* done_ws = nullptr;
    if (any_global) {
        hipError_t e = hipMallocAsync((void**)&done_ws, (size_t)N, s);
        if (e != hipSuccess) {
            (void)hipFreeAsync(dtab, s);
            pg_set_error("optics_graph: %lld bytes of scratch: %s", (long long)N, hipGetErrorString(e));
            return PG_ENOMEM;
        }
    }
    hipLaunchKernelGGL(optics_core_kernel, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, s, dist, dtab, dtab + C + 1, C, min_samples, N, core);
    int rc = pg_check_launch("optics_core");
    const int64_t* dorder = dtab + 2 * (C + 1);
    int start = 0;
    while (rc == PG_OK && start < C) {
        const int64_t n0 = cell_off[ord[start] + 1] - cell_off[ord[start]];
        const int threads = plan_threads(n0);
        int end = start;
        int64_t lds_n = 0;                                         // the largest LDS-resident cell of the run
        while (end < C && plan_threads(cell_off[ord[end] + 1] - cell_off[ord[end]]) == threads) {
            const int64_t n = cell_off[ord[end] + 1] - cell_off[ord[end]];
            if (n <= lds_pts && n > lds_n) lds_n = n;
            ++end;
        }
        if (threads == 64) rc = launch_order<64>(dist, dtab, C, dorder + start, end - start, lds_n, core, ordering, reach, pred, done_ws, s);
        else if (threads == 256) rc = launch_order<256>(dist, dtab, C, dorder + start, end - start, lds_n, core, ordering, reach, pred, done_ws, s);
        else rc = launch_order<1024>(dist, dtab, C, dorder + start, end - start, lds_n, core, ordering, reach, pred, done_ws, s);
        start = end;
    }
    if (done_ws) (void)hipFreeAsync(done_ws, s);
    (void)hipFreeAsync(dtab, s);
    if (rc == PG_OK) PG_HIP(hipStreamSynchronize(s));             // `tab` is the source of an asynchronous copy
    return rc;
}
