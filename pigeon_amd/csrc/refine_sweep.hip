// refine_sweep.hip -- the refiner's selection at every point of a (topk, temperature, max_km) grid, from the records ONE
// pg_refine_forward / pg_refine_forward_ex call left: pg_refine_sweep, pg_refine_sweep_totals, pg_refine_sweep_plan (contract:
// include/pigeon_hip.h, restated in tests/_refitref.py).
//
// Finding the nearest prototype and the farthest member of every candidate streams the bank and depends on none of the three settings;
// only refine_select_kernel (refine.hip) does.  A grid point here is that kernel's arithmetic, operation for operation -- the same
// expf, the same sequential sum, the same two divisions and one product per candidate, argmax_torch's order, haversine_km from the one
// shared header, this file compiled with refine.hip's flags -- so a point's choice is pg_refine_forward's, bit for bit.  What the grid
// points of a row share is computed once:
//   sweep_veto_kernel     one thread per (row, candidate): the veto distance, which depends on neither topk nor T.
//   sweep_select_kernel   one workgroup per (64 rows, temperature), lane = row.  ex_j = expf(score_j / T) and cp_j go to LDS as [j][row]
//       (a lane's dynamic index j never conflicts with its neighbours': bank = row), then one wave takes the running sum S_t = the
//       sequential sum over j < t -- the sum refine_select_kernel forms for topk = t, in its order -- and another the running
//       argmax_torch(cp, t), the veto's fallback.  After that the four waves split the topks; a wave's topk is uniform, its lanes' rows
//       differ: t divide-multiply-compare steps find the refined candidate, one gather reads its veto distance, and the nR thresholds
//       cost a comparison and a 64-byte coalesced store of choice bytes each.  No private array is indexed dynamically (64-entry ones,
//       as refine_select_kernel keeps for its single point, would live in scratch memory for the whole grid loop).
//   sweep_totals_kernel   one workgroup per grid point: thread t adds rows t, t + 256, ... ascending, then row_block.h's block_sum.  The
//       order depends on B only, no atomics: a point's totals are the same bits alone and inside any grid.
#include "common.h"
#include "pigeon_internal.h"
#include "refine_common.h"
#include "row_block.h"

#include <cmath>

#define SWEEP_ROWS 64                                 // rows per workgroup of sweep_select_kernel: one per lane
#define SWEEP_THREADS 256
#define SWEEP_MAX_TOPK 64
#define SWEEP_MAX_G (1 << 20)
#define SWEEP_MAX_V 16
#define SWEEP_ACC (SWEEP_MAX_V + 3)                   // V value columns, changed, vetoed, bad bytes

static size_t sweep_lds_bytes(int n_eval) { return (size_t)n_eval * SWEEP_ROWS * (3 * sizeof(float) + 1); }

__global__ __launch_bounds__(256) void sweep_veto_kernel(const float* __restrict__ scratch, int SC, int64_t total, int n_eval,
                                                         const double* __restrict__ init_llh, double* __restrict__ veto_km) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;          // b * n_eval + j
    if (i >= total) return;
    const int64_t b = i / n_eval;
    const float rlng = scratch[i * SC + 1], rlat = scratch[i * SC + 2];
    const double dist = haversine_km(init_llh[2 * b], init_llh[2 * b + 1], rlng, rlat);
    veto_km[i] = dist;
}

// topks, temps, max_kms: DEVICE copies of the caller's three host arrays (pg_refine_sweep makes them)
__global__ __launch_bounds__(SWEEP_THREADS) void sweep_select_kernel(const float* __restrict__ scratch, int SC, int B, int n_eval,
                                                                     const float* __restrict__ cand_prob, int k,
                                                                     const double* __restrict__ veto_km,
                                                                     const int32_t* __restrict__ topks, int nK,
                                                                     const float* __restrict__ temps, int nT,
                                                                     const double* __restrict__ max_kms, int nR,
                                                                     uint8_t* __restrict__ choice) {
    extern __shared__ float sweep_lds[];
    float* ex = sweep_lds;                             // [n_eval][64]
    float* cp = ex + n_eval * SWEEP_ROWS;              // [n_eval][64]
    float* pre = cp + n_eval * SWEEP_ROWS;             // [n_eval][64]: pre[t - 1] = the sum over j < t
    uint8_t* fb = (uint8_t*)(pre + n_eval * SWEEP_ROWS);   // [n_eval][64]: fb[t - 1] = argmax_torch(cp, t)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int iT = blockIdx.x % nT;
    const int b = (blockIdx.x / nT) * SWEEP_ROWS + lane;
    const bool valid = b < B;
    const float temperature = temps[iT];

    if (valid) {
        const float* sc = scratch + (int64_t)b * n_eval * SC;
        for (int j = wave; j < n_eval; j += 4) {
            ex[j * SWEEP_ROWS + lane] = expf(sc[SC * j] / temperature);    // torch.exp(input / T), fp32
            cp[j * SWEEP_ROWS + lane] = cand_prob ? cand_prob[(int64_t)b * k + j] : (j == 0 ? 1.0f : 0.0f);
        }
    }
    __syncthreads();
    if (valid && wave == 0) {
        float sum = 0.f;
        for (int j = 0; j < n_eval; ++j) {
            sum += ex[j * SWEEP_ROWS + lane];          // torch.sum, sequential: after j the sum refine_select_kernel has for topk = j + 1
            pre[j * SWEEP_ROWS + lane] = sum;
        }
    }
    if (valid && wave == 1) {                          // argmax_torch(cp, t) for every t: its loop, stopped after t elements
        int bi = 0; float bv = cp[lane];
        fb[lane] = 0;
        for (int j = 1; j < n_eval; ++j) {
            const float x = cp[j * SWEEP_ROWS + lane];
            if (!(bv != bv) && (x != x || x > bv)) { bv = x; bi = j; }
            fb[j * SWEEP_ROWS + lane] = (uint8_t)bi;
        }
    }
    __syncthreads();
    if (!valid) return;

    for (int iK = wave; iK < nK; iK += 4) {
        const int topk = topks[iK];                    // uniform in the wave; 1 <= topk <= n_eval (checked on the host)
        const float sum = pre[(topk - 1) * SWEEP_ROWS + lane];
        int refined = 0;
        float bv = cp[lane] * (ex[lane] / sum);
        for (int j = 1; j < topk; ++j) {
            const float x = cp[j * SWEEP_ROWS + lane] * (ex[j * SWEEP_ROWS + lane] / sum);
            if (!(bv != bv) && (x != x || x > bv)) { bv = x; refined = j; }     // argmax_torch: first maximum, the first NaN wins
        }
        const double dist = veto_km[(int64_t)b * n_eval + refined];
        const uint8_t fallback = fb[(topk - 1) * SWEEP_ROWS + lane] | 0x80;
        uint8_t* out = choice + ((int64_t)iK * nT + iT) * nR * (int64_t)B + b;
        for (int iR = 0; iR < nR; ++iR) out[(int64_t)iR * B] = dist > max_kms[iR] ? fallback : (uint8_t)refined;
    }
}

__global__ __launch_bounds__(SWEEP_THREADS) void sweep_totals_kernel(const uint8_t* __restrict__ choice, int B, int n_eval,
                                                                     const double* __restrict__ values, int V,
                                                                     double* __restrict__ totals) {
    __shared__ double red[4][SWEEP_ACC];
    const int tid = threadIdx.x;
    const int64_t g = blockIdx.x;
    const uint8_t* row = choice + g * (int64_t)B;
    double acc[SWEEP_ACC];
#pragma unroll
    for (int v = 0; v < SWEEP_ACC; ++v) acc[v] = 0.0;
    for (int b = tid; b < B; b += SWEEP_THREADS) {
        const int byte = row[b];
        int c = byte & 63;
        const bool bad = c >= n_eval;                  // not a byte pg_refine_sweep wrote: it forms no address
        c = bad ? 0 : c;
        const double* val = values + ((int64_t)b * n_eval + c) * V;
#pragma unroll
        for (int v = 0; v < SWEEP_MAX_V; ++v)
            if (v < V) acc[v] += val[v];
        acc[SWEEP_MAX_V] += c != 0 ? 1.0 : 0.0;
        acc[SWEEP_MAX_V + 1] += (byte & 0x80) ? 1.0 : 0.0;
        acc[SWEEP_MAX_V + 2] += bad ? 1.0 : 0.0;
    }
    block_sum(acc, red);
    const bool nan = acc[SWEEP_MAX_V + 2] != 0.0;
    double* out = totals + g * (V + 2);
#pragma unroll
    for (int v = 0; v < SWEEP_MAX_V; ++v)
        if (v < V && tid == v) out[v] = nan ? (double)NAN : acc[v];
    if (tid == SWEEP_MAX_V) out[V] = nan ? (double)NAN : acc[SWEEP_MAX_V];
    if (tid == SWEEP_MAX_V + 1) out[V + 1] = nan ? (double)NAN : acc[SWEEP_MAX_V + 1];
}

// ---------------------------------------------------------------------------------------------------------------------------- host
static int sweep_sizes(const char* who, int B, int n_eval) {
    if (B < 0) { pg_set_error("%s: B = %d", who, B); return PG_EINVAL; }
    if (n_eval < 1 || n_eval > SWEEP_MAX_TOPK) { pg_set_error("%s: n_eval must be 1 .. %d (got %d)", who, SWEEP_MAX_TOPK, n_eval); return PG_EINVAL; }
    return PG_OK;
}

extern "C" int pg_refine_sweep_plan(int B, int n_eval, int64_t G, int V, int64_t out[4]) {
    if (!out) { pg_set_error("refine_sweep_plan: null argument out"); return PG_EINVAL; }
    const int rc = sweep_sizes("refine_sweep_plan", B, n_eval);
    if (rc != PG_OK) return rc;
    if (G < 1 || G > SWEEP_MAX_G) { pg_set_error("refine_sweep_plan: G must be 1 .. %d (got %lld)", SWEEP_MAX_G, (long long)G); return PG_EINVAL; }
    if (V < 1 || V > SWEEP_MAX_V) { pg_set_error("refine_sweep_plan: V must be 1 .. %d (got %d)", SWEEP_MAX_V, V); return PG_EINVAL; }
    out[0] = SWEEP_ROWS;
    out[1] = (int64_t)sweep_lds_bytes(n_eval);
    out[2] = ((int64_t)B + SWEEP_ROWS - 1) / SWEEP_ROWS;
    out[3] = G * (int64_t)B;
    return PG_OK;
}

extern "C" int pg_refine_sweep(const float* scratch, int SC, int B, int n_eval, const float* cand_prob, int k, const double* init_llh,
                               const int32_t* topks, int nK, const float* temps, int nT, const double* max_kms, int nR,
                               uint8_t* choice, double* veto_km, void* stream) {
    int rc = sweep_sizes("refine_sweep", B, n_eval);
    if (rc != PG_OK) return rc;
    if (SC != 4 && SC != 12) { pg_set_error("refine_sweep: SC must be 4 or 12 (got %d)", SC); return PG_EINVAL; }
    if (nK < 1) { pg_set_error("refine_sweep: nK must be at least 1 (got %d)", nK); return PG_EINVAL; }
    if (nT < 1) { pg_set_error("refine_sweep: nT must be at least 1 (got %d)", nT); return PG_EINVAL; }
    if (nR < 1) { pg_set_error("refine_sweep: nR must be at least 1 (got %d)", nR); return PG_EINVAL; }
    const int64_t G = (int64_t)nK * nT * nR;
    if ((int64_t)nK * nT > SWEEP_MAX_G || G > SWEEP_MAX_G) {
        pg_set_error("refine_sweep: G = nK * nT * nR = %lld exceeds %d", (long long)G, SWEEP_MAX_G); return PG_EINVAL;
    }
    if (cand_prob && n_eval > k) { pg_set_error("refine_sweep: n_eval = %d exceeds k = %d columns of cand_prob", n_eval, k); return PG_EINVAL; }
    PG_NEED("refine_sweep", topks);
    PG_NEED("refine_sweep", temps);
    PG_NEED("refine_sweep", max_kms);
    for (int i = 0; i < nK; ++i)
        if (topks[i] < 1 || topks[i] > n_eval) {
            pg_set_error("refine_sweep: topks[%d] = %d is outside 1 .. min(n_eval, 64) = %d", i, topks[i], n_eval); return PG_EINVAL;
        }
    for (int i = 0; i < nT; ++i)
        if (!(temps[i] > 0.f && temps[i] < INFINITY)) {
            pg_set_error("refine_sweep: temps[%d] = %g is not a finite positive number", i, (double)temps[i]); return PG_EINVAL;
        }
    for (int i = 0; i < nR; ++i)
        if (max_kms[i] != max_kms[i]) { pg_set_error("refine_sweep: max_kms[%d] is NaN", i); return PG_EINVAL; }
    const int64_t groups = ((int64_t)B + SWEEP_ROWS - 1) / SWEEP_ROWS;
    if (groups * nT > 0x7fffffffLL) { pg_set_error("refine_sweep: B = %d rows x nT = %d temperatures exceed the grid", B, nT); return PG_EINVAL; }
    if (B == 0) return PG_OK;                              // an empty batch is a no-op: its (empty) buffers may be NULL
    PG_NEED("refine_sweep", scratch);
    PG_NEED("refine_sweep", init_llh);
    PG_NEED("refine_sweep", choice);

    hipStream_t s = (hipStream_t)stream;
    // stream-ordered scratch: the veto distances when the caller wants none, then the three host arrays
    const size_t veto_bytes = veto_km ? 0 : (size_t)B * n_eval * sizeof(double);
    const size_t r_bytes = (size_t)nR * sizeof(double), t_bytes = ((size_t)nT * sizeof(float) + 7) & ~(size_t)7;
    const size_t k_bytes = (size_t)nK * sizeof(int32_t);
    char* dev = nullptr;
    PG_HIP(hipMallocAsync((void**)&dev, veto_bytes + r_bytes + t_bytes + k_bytes, s));
    double* d_veto = veto_km ? veto_km : (double*)dev;
    double* d_r = (double*)(dev + veto_bytes);
    float* d_t = (float*)(dev + veto_bytes + r_bytes);
    int32_t* d_k = (int32_t*)(dev + veto_bytes + r_bytes + t_bytes);
    hipError_t e = hipMemcpyAsync(d_r, max_kms, r_bytes, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(d_t, temps, (size_t)nT * sizeof(float), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(d_k, topks, k_bytes, hipMemcpyHostToDevice, s);
    if (e != hipSuccess) {
        pg_set_error("refine_sweep: copying the grid to the device failed: %s", hipGetErrorString(e));
        (void)hipFreeAsync(dev, s);
        return PG_EHIP;
    }
    const int64_t total = (int64_t)B * n_eval;
    hipLaunchKernelGGL(sweep_veto_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, scratch, SC, total, n_eval, init_llh, d_veto);
    rc = pg_check_launch("refine_sweep (veto distances)");
    if (rc == PG_OK) {
        hipLaunchKernelGGL(sweep_select_kernel, dim3((unsigned)(groups * nT)), dim3(SWEEP_THREADS), sweep_lds_bytes(n_eval), s, scratch, SC, B,
                           n_eval, cand_prob, k, (const double*)d_veto, (const int32_t*)d_k, nK, (const float*)d_t, nT, (const double*)d_r, nR,
                           choice);
        rc = pg_check_launch("refine_sweep");
    }
    (void)hipFreeAsync(dev, s);
    return rc;
}

extern "C" int pg_refine_sweep_totals(const uint8_t* choice, int64_t G, int B, int n_eval, const double* values, int V, double* totals,
                                      void* stream) {
    const int rc = sweep_sizes("refine_sweep_totals", B, n_eval);
    if (rc != PG_OK) return rc;
    if (G < 1 || G > SWEEP_MAX_G) { pg_set_error("refine_sweep_totals: G must be 1 .. %d (got %lld)", SWEEP_MAX_G, (long long)G); return PG_EINVAL; }
    if (V < 1 || V > SWEEP_MAX_V) { pg_set_error("refine_sweep_totals: V must be 1 .. %d (got %d)", SWEEP_MAX_V, V); return PG_EINVAL; }
    PG_NEED("refine_sweep_totals", totals);
    if (B > 0) {
        PG_NEED("refine_sweep_totals", choice);
        PG_NEED("refine_sweep_totals", values);
    }
    // B == 0: every sum is empty, the kernel writes +0.0 and reads nothing
    hipLaunchKernelGGL(sweep_totals_kernel, dim3((unsigned)G), dim3(SWEEP_THREADS), 0, (hipStream_t)stream, choice, B, n_eval, values, V, totals);
    return pg_check_launch("refine_sweep_totals");
}
