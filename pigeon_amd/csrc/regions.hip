// regions.hip -- exact point-in-region lookup over a bank of (multi)polygons with holes: the device half of the country metric and of
// the geocell labels.
//
// Replaces the geopandas / shapely lookups of the reference:
//   find_country          evaluation/metrics.py:56-72        the first region that covers the point (interior or boundary,
//   generate_cell_labels  preprocessing/dataset_preprocessing.py:60-94   `covered_by`), else the nearest one: planar distance in
//                                                            degrees to the region's boundary, as GEOS computes it on EPSG:4326
//   country_accuracy      evaluation/metrics.py:74-88        correct iff the label's country `contains` the prediction: strictly
//                                                            interior, a prediction on the boundary is wrong
// A region is the set of its rings under the even-odd rule: a point in a hole is outside, a point on any ring is on the boundary.
//
// Everything here is fp64 with plain IEEE operations: this file is compiled with -ffp-contract=off (pigeon_amd/build.py), uses no
// fast-math, no inline assembly and no atomics, and no result depends on the launch geometry -- parities, flags and lexicographic
// minima are exact whatever the order they are reduced in.
//
// CLASSIFYING a point p against a region: OUTSIDE (0), INSIDE (1, strictly interior) or AMBIGUOUS (2).  The device never guesses:
//   * bounding boxes are closed and compared exactly; a region whose box misses p is OUTSIDE, a ring whose box misses p is skipped
//     (a closed ring has an even number of straddling edges, and p is not on it);
//   * crossing number with the half-open rule: edge a -> b straddles iff (a.y <= p.y) != (b.y <= p.y) -- exact comparisons;
//   * a straddling edge is decided by the sign of  det = l - r,  l = (a.x - p.x) * (b.y - p.y),  r = (a.y - p.y) * (b.x - p.x):
//     an upward edge crosses the ray towards +x iff det > 0, a downward one iff det < 0.  The sign is accepted only if
//     |det| > (3 + 16 eps) eps (|l| + |r|), eps = 2^-53: Shewchuk's stage-A bound of orient2d, which also covers the rounding of the
//     four differences -- and only if |l| + |r| >= 2^-960, below which a product may have underflowed and the bound does not hold;
//   * the pair is AMBIGUOUS when a straddling edge is not certified that way (det == 0 included), when a horizontal edge at p.y holds
//     p.x in its closed x-range, or when a vertex equals p.  Every point ON a ring meets one of these, so INSIDE and OUTSIDE are
//     certain; the host settles the ambiguous pairs in rational arithmetic (pigeon_amd/regions.py exact_state).
//
// NEAREST region of a point: the minimum over every edge a -> b of every region of the point-to-segment distance, ties to the lower
// region index.  The fp64 operations per edge, in this order, no contraction (tests/test_gpu_regions.py derives its bound from them):
//     dx = b.x - a.x;  dy = b.y - a.y;  wx = p.x - a.x;  wy = p.y - a.y;
//     len2 = dx * dx + dy * dy;   dot = wx * dx + wy * dy;
//     len2 == 0 or dot <= 0:  d2 = wx * wx + wy * wy
//     dot >= len2:            ux = p.x - b.x;  uy = p.y - b.y;  d2 = ux * ux + uy * uy
//     otherwise:              cr = wx * dy - wy * dx;  d2 = (cr * cr) / len2
//   dist = sqrt(min d2), the minimum taken on (d2, region index) lexicographically.
//
// MAPPING: lanes stride over a ring's edges (two 16-byte loads per edge); parity and the ambiguous flag are reduced by ballot /
// popcount inside a wave, then across waves through LDS.  A point is served by one wave (banks of small rings: geocells) or by one
// workgroup of four waves (large rings: countries); pg_region_plan says which, as a pure function of the bank.
#include "pigeon_internal.h"

#include <climits>
#include <vector>

#define REGION_WAVE_EDGES 128             // a bank whose largest ring has more edges than this gets a workgroup per point
#define REGION_MAX_COUNT (1 << 30)        // regions, rings: 32-bit indices with room for the 64-wide scan

static int g_wave_edges = -1;             // pg_tune_region_wave_edges; < 0 = REGION_WAVE_EDGES

static int wave_edges() { return g_wave_edges >= 0 ? g_wave_edges : REGION_WAVE_EDGES; }

extern "C" int pg_tune_region_wave_edges(int max_edges) {
    g_wave_edges = max_edges < 0 ? -1 : max_edges;
    return PG_OK;
}

// the bank as the kernels see it: the device arrays plus the extents every index is clamped to
struct RegionArgs {
    const int64_t* region_off;
    const int64_t* ring_off;
    const double2* xy;
    const double* ring_bbox;
    const double* region_bbox;
    int R;
    int64_t n_rings, n_vertices;
};

// the CSR as the host holds it: counts, ascending offsets that end at the arrays' sizes, rings of at least one edge
static int check_bank(const char* who, const pg_region_bank* b, bool need_device, int64_t* max_edges) {
    if (!b) { pg_set_error("%s: null bank", who); return PG_EINVAL; }
    const int64_t R = b->num_regions, nr = b->num_rings, nv = b->num_vertices;
    if (R < 0 || nr < 0 || nv < 0) { pg_set_error("%s: negative count in the bank (%lld regions, %lld rings, %lld vertices)", who, (long long)R, (long long)nr, (long long)nv); return PG_EINVAL; }
    if (R > REGION_MAX_COUNT || nr > REGION_MAX_COUNT) { pg_set_error("%s: more than %d regions or rings", who, REGION_MAX_COUNT); return PG_EINVAL; }
    if (nv > INT_MAX) { pg_set_error("%s: %lld vertices, more than the %d a bank may hold", who, (long long)nv, INT_MAX); return PG_EINVAL; }
    if (max_edges) *max_edges = 0;
    if (R == 0) return PG_OK;
    if (!b->region_off_host || !b->ring_off_host) { pg_set_error("%s: the bank's host offset arrays are null", who); return PG_EINVAL; }
    if (need_device && (!b->region_off || !b->ring_off || !b->region_bbox || (nr > 0 && !b->ring_bbox) || (nv > 0 && !b->xy))) {
        pg_set_error("%s: a device array of the bank is null", who);
        return PG_EINVAL;
    }
    if (need_device && ((uintptr_t)b->xy & 15)) { pg_set_error("%s: xy is not 16-byte aligned", who); return PG_EINVAL; }
    const int64_t* go = b->region_off_host;
    const int64_t* ro = b->ring_off_host;
    if (go[0] != 0) { pg_set_error("%s: region_off[0] is %lld, not 0", who, (long long)go[0]); return PG_EINVAL; }
    for (int64_t g = 0; g < R; ++g)
        if (go[g + 1] < go[g] || go[g + 1] > nr) {
            pg_set_error("%s: region %lld: region_off goes from %lld to %lld (the bank has %lld rings)", who, (long long)g, (long long)go[g], (long long)go[g + 1], (long long)nr);
            return PG_EINVAL;
        }
    if (go[R] != nr) { pg_set_error("%s: region_off ends at %lld, the bank has %lld rings", who, (long long)go[R], (long long)nr); return PG_EINVAL; }
    if (ro[0] != 0) { pg_set_error("%s: ring_off[0] is %lld, not 0", who, (long long)ro[0]); return PG_EINVAL; }
    int64_t most = 0;
    for (int64_t r = 0; r < nr; ++r) {
        if (ro[r + 1] > nv || ro[r + 1] - ro[r] < 2) {
            pg_set_error("%s: ring %lld: ring_off goes from %lld to %lld (a ring needs at least 2 vertices; the bank has %lld)", who, (long long)r, (long long)ro[r], (long long)ro[r + 1], (long long)nv);
            return PG_EINVAL;
        }
        if (ro[r + 1] - ro[r] - 1 > most) most = ro[r + 1] - ro[r] - 1;
    }
    if (ro[nr] != nv) { pg_set_error("%s: ring_off ends at %lld, the bank has %lld vertices", who, (long long)ro[nr], (long long)nv); return PG_EINVAL; }
    if (max_edges) *max_edges = most;
    return PG_OK;
}

static RegionArgs args_of(const pg_region_bank* b) {
    RegionArgs a;
    a.region_off = b->region_off; a.ring_off = b->ring_off; a.xy = (const double2*)b->xy;
    a.ring_bbox = b->ring_bbox; a.region_bbox = b->region_bbox;
    a.R = (int)b->num_regions; a.n_rings = b->num_rings; a.n_vertices = b->num_vertices;
    return a;
}

extern "C" int pg_region_plan(const pg_region_bank* bank, int32_t out[4]) {
    if (!out) { pg_set_error("region_plan: null argument"); return PG_EINVAL; }
    int64_t most = 0;
    if (int rc = check_bank("region_plan", bank, false, &most)) return rc;
    out[0] = most > wave_edges() ? 1 : 0;
    out[1] = out[0] ? 256 : 64;
    out[2] = (int32_t)most;
    out[3] = wave_edges();
    return PG_OK;
}

// --------------------------------------------------------------------------------------------- classification
#define REGION_EPS 1.1102230246251565404e-16                       // 2^-53
#define REGION_ERRBOUND ((3.0 + 16.0 * REGION_EPS) * REGION_EPS)
#define REGION_MIN_SUM 1.0261342003245940e-289                     // 2^-960

__device__ __forceinline__ bool in_box(const double* __restrict__ bb, double px, double py) {
    return px >= bb[0] && px <= bb[2] && py >= bb[1] && py <= bb[3];           // closed, exact; a NaN is in no box
}

// bit 0: the edge crosses the ray from p towards +x; bit 1: the edge cannot be decided here
__device__ __forceinline__ unsigned edge_bits(double px, double py, double2 a, double2 b) {
    if ((a.x == px && a.y == py) || (b.x == px && b.y == py)) return 2u;
    const bool au = a.y <= py, bu = b.y <= py;
    if (au == bu) {
        if (a.y == py && b.y == py) {                                          // horizontal at p.y
            const double lo = a.x < b.x ? a.x : b.x, hi = a.x < b.x ? b.x : a.x;
            if (px >= lo && px <= hi) return 2u;
        }
        return 0u;
    }
    const double l = (a.x - px) * (b.y - py), r = (a.y - py) * (b.x - px);
    const double det = l - r;
    const double sum = fabs(l) + fabs(r);
    if (!(sum >= REGION_MIN_SUM) || !(fabs(det) > REGION_ERRBOUND * sum)) return 2u;   // NaN (overflowed differences) lands here too
    return (au ? det > 0.0 : det < 0.0) ? 1u : 0u;
}

// The state of p against region g, the same value in every thread of the group (64 * WAVES threads, t = the thread's index in it).
// WAVES > 1: one barrier per call that reaches the edges; the cross-wave scratch alternates between two buffers (`flip`), so a wave
// that runs ahead writes the other one.
template <int WAVES>
__device__ __forceinline__ int classify_region(const RegionArgs& B, double px, double py, int g, int t, unsigned (*red)[4], int& flip) {
    if (!in_box(B.region_bbox + 4 * (int64_t)g, px, py)) return 0;
    int64_t r0 = B.region_off[g], r1 = B.region_off[g + 1];
    if (r0 < 0) r0 = 0;
    if (r1 > B.n_rings) r1 = B.n_rings;
    unsigned bits = 0;                                                         // bit 0: parity of this thread's crossings, bit 1: ambiguous
    for (int64_t r = r0; r < r1; ++r) {
        if (!in_box(B.ring_bbox + 4 * r, px, py)) continue;
        int64_t v0 = B.ring_off[r], v1 = B.ring_off[r + 1];
        if (v0 < 0) v0 = 0;
        if (v1 > B.n_vertices) v1 = B.n_vertices;
        for (int64_t j = v0 + t; j + 1 < v1; j += 64 * WAVES) {
            const unsigned e = edge_bits(px, py, B.xy[j], B.xy[j + 1]);
            bits = (bits ^ (e & 1u)) | (e & 2u);
        }
    }
    unsigned res = (unsigned)(__popcll(__ballot(bits & 1u)) & 1) | (__ballot(bits & 2u) ? 2u : 0u);
    if (WAVES > 1) {
        if ((t & 63) == 0) red[flip][t >> 6] = res;
        __syncthreads();
        res = 0;
#pragma unroll
        for (int w = 0; w < WAVES; ++w) { const unsigned o = red[flip][w]; res = (res ^ (o & 1u)) | (o & 2u); }
        flip ^= 1;
    }
    return (res & 2u) ? 2 : (int)(res & 1u);
}

// WAVES == 1: four points per block, one per wave, no barrier (whole waves leave).  WAVES == 4: one point per block.
template <int WAVES>
__global__ __launch_bounds__(256) void region_locate_kernel(const RegionArgs B, const double* __restrict__ pts, const int32_t* __restrict__ start,
                                                            int64_t N, int32_t* __restrict__ cover, unsigned char* __restrict__ state) {
    __shared__ unsigned red[2][4];
    const int lane = threadIdx.x & 63;
    const int64_t i = WAVES == 1 ? (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6) : (int64_t)blockIdx.x;
    if (i >= N) return;
    const int t = WAVES == 1 ? lane : (int)threadIdx.x;
    const double px = pts[2 * i], py = pts[2 * i + 1];
    int s = start ? start[i] : 0;
    if (s < 0) s = 0;
    int found = -1, st = 0, flip = 0;
    // 64 region boxes per step, one per lane; the candidates of a step are classified in ascending order.  Every wave of a
    // workgroup computes the same masks from the same data, so the loop is uniform over the block.
    for (int base = s; base < B.R && found < 0; base += 64) {
        const int g = base + lane;
        const bool hit = g < B.R && in_box(B.region_bbox + 4 * (int64_t)g, px, py);
        unsigned long long m = __ballot(hit);
        while (m) {
            const int k = __ffsll((long long)m) - 1;
            m &= m - 1;
            const int c = classify_region<WAVES>(B, px, py, base + k, t, red, flip);
            if (c) { found = base + k; st = c; break; }
        }
    }
    if (t == 0) { cover[i] = found; state[i] = (unsigned char)st; }
}

template <int WAVES>
__global__ __launch_bounds__(256) void region_classify_kernel(const RegionArgs B, const double* __restrict__ pts, const int32_t* __restrict__ region,
                                                              int64_t N, unsigned char* __restrict__ state) {
    __shared__ unsigned red[2][4];
    const int64_t i = WAVES == 1 ? (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6) : (int64_t)blockIdx.x;
    if (i >= N) return;
    const int t = WAVES == 1 ? (int)(threadIdx.x & 63) : (int)threadIdx.x;
    const int g = region[i];
    int flip = 0;
    const int c = (g < 0 || g >= B.R) ? 0 : classify_region<WAVES>(B, pts[2 * i], pts[2 * i + 1], g, t, red, flip);
    if (t == 0) state[i] = (unsigned char)c;
}

// --------------------------------------------------------------------------------------------- nearest
__device__ __forceinline__ double segment_d2(double px, double py, double2 a, double2 b) {
    const double dx = b.x - a.x, dy = b.y - a.y, wx = px - a.x, wy = py - a.y;
    const double len2 = dx * dx + dy * dy;
    const double dot = wx * dx + wy * dy;
    if (len2 == 0.0 || dot <= 0.0) return wx * wx + wy * wy;
    if (dot >= len2) {
        const double ux = px - b.x, uy = py - b.y;
        return ux * ux + uy * uy;
    }
    const double cr = wx * dy - wy * dx;
    return (cr * cr) / len2;
}

template <int WAVES>
__global__ __launch_bounds__(256) void region_nearest_kernel(const RegionArgs B, const double* __restrict__ pts, int64_t N,
                                                             int32_t* __restrict__ idx, double* __restrict__ dist) {
    __shared__ double red_d[4];
    __shared__ int red_g[4];
    const int64_t i = WAVES == 1 ? (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6) : (int64_t)blockIdx.x;
    if (i >= N) return;
    const int t = WAVES == 1 ? (int)(threadIdx.x & 63) : (int)threadIdx.x;
    const double px = pts[2 * i], py = pts[2 * i + 1];
    double bd = __longlong_as_double(0x7ff0000000000000ll);
    int bg = INT_MAX;
    for (int g = 0; g < B.R; ++g) {
        int64_t r0 = B.region_off[g], r1 = B.region_off[g + 1];
        if (r0 < 0) r0 = 0;
        if (r1 > B.n_rings) r1 = B.n_rings;
        for (int64_t r = r0; r < r1; ++r) {
            int64_t v0 = B.ring_off[r], v1 = B.ring_off[r + 1];
            if (v0 < 0) v0 = 0;
            if (v1 > B.n_vertices) v1 = B.n_vertices;
            for (int64_t j = v0 + t; j + 1 < v1; j += 64 * WAVES) {
                const double d2 = segment_d2(px, py, B.xy[j], B.xy[j + 1]);
                if (d2 < bd) { bd = d2; bg = g; }                              // regions ascend: a tie keeps the lower index
            }
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const double d2 = __shfl_xor(bd, off, 64);
        const int g2 = __shfl_xor(bg, off, 64);
        if (d2 < bd || (d2 == bd && g2 < bg)) { bd = d2; bg = g2; }
    }
    if (WAVES > 1) {
        if ((t & 63) == 0) { red_d[t >> 6] = bd; red_g[t >> 6] = bg; }
        __syncthreads();
        bd = red_d[0]; bg = red_g[0];
#pragma unroll
        for (int w = 1; w < WAVES; ++w) {
            const double d2 = red_d[w];
            const int g2 = red_g[w];
            if (d2 < bd || (d2 == bd && g2 < bg)) { bd = d2; bg = g2; }
        }
    }
    if (t == 0) { idx[i] = bg == INT_MAX ? -1 : bg; dist[i] = sqrt(bd); }
}

// --------------------------------------------------------------------------------------------- entry points
static unsigned grid_of(int64_t N, bool group) { return (unsigned)(group ? N : (N + 3) / 4); }

// a HOST int32 array -> stream-ordered device scratch
static int upload_i32(const char* who, const int32_t* host, int64_t n, int32_t** dev, hipStream_t s) {
    PG_HIP(hipMallocAsync((void**)dev, (size_t)n * sizeof(int32_t), s));
    hipError_t e = hipMemcpyAsync(*dev, host, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, s);
    if (e != hipSuccess) {
        (void)hipFreeAsync(*dev, s);
        pg_set_error("%s: hipMemcpyAsync of the index array failed: %s", who, hipGetErrorString(e));
        return PG_EHIP;
    }
    return PG_OK;
}

extern "C" int pg_region_locate(const pg_region_bank* bank, const double* pts, const int32_t* start, int64_t N, int32_t* cover,
                                uint8_t* state, void* stream) {
    if (N < 0 || N > INT_MAX) { pg_set_error("region_locate: N = %lld is outside 0 .. %d", (long long)N, INT_MAX); return PG_EINVAL; }
    int64_t most = 0;
    if (int rc = check_bank("region_locate", bank, true, &most)) return rc;
    if (N == 0) return PG_OK;
    if (!pts || !cover || !state) { pg_set_error("region_locate: null argument"); return PG_EINVAL; }
    const int64_t R = bank->num_regions;
    if (start)
        for (int64_t i = 0; i < N; ++i)
            if (start[i] < 0 || start[i] > R) {
                pg_set_error("region_locate: start[%lld] = %d is outside 0 .. %lld", (long long)i, start[i], (long long)R);
                return PG_EINVAL;
            }
    hipStream_t s = (hipStream_t)stream;
    if (R == 0) {                                                   // no region covers anything
        PG_HIP(hipMemsetAsync(cover, 0xff, (size_t)N * sizeof(int32_t), s));
        PG_HIP(hipMemsetAsync(state, 0, (size_t)N, s));
        return PG_OK;
    }
    int32_t* dstart = nullptr;
    if (start) if (int rc = upload_i32("region_locate", start, N, &dstart, s)) return rc;
    const RegionArgs B = args_of(bank);
    const bool group = most > wave_edges();
    if (group) hipLaunchKernelGGL(region_locate_kernel<4>, dim3(grid_of(N, true)), dim3(256), 0, s, B, pts, dstart, N, cover, state);
    else hipLaunchKernelGGL(region_locate_kernel<1>, dim3(grid_of(N, false)), dim3(256), 0, s, B, pts, dstart, N, cover, state);
    int rc = pg_check_launch("region_locate");
    if (dstart) {
        (void)hipFreeAsync(dstart, s);
        if (rc == PG_OK) PG_HIP(hipStreamSynchronize(s));           // `start` is the source of an asynchronous copy
    }
    return rc;
}

extern "C" int pg_region_classify(const pg_region_bank* bank, const double* pts, const int32_t* region, int64_t N, uint8_t* state,
                                  void* stream) {
    if (N < 0 || N > INT_MAX) { pg_set_error("region_classify: N = %lld is outside 0 .. %d", (long long)N, INT_MAX); return PG_EINVAL; }
    int64_t most = 0;
    if (int rc = check_bank("region_classify", bank, true, &most)) return rc;
    if (N == 0) return PG_OK;
    if (!pts || !region || !state) { pg_set_error("region_classify: null argument"); return PG_EINVAL; }
    const int64_t R = bank->num_regions;
    for (int64_t i = 0; i < N; ++i)
        if (region[i] < -1 || region[i] >= R) {
            pg_set_error("region_classify: region[%lld] = %d is outside -1 .. %lld", (long long)i, region[i], (long long)R - 1);
            return PG_EINVAL;
        }
    hipStream_t s = (hipStream_t)stream;
    if (R == 0) { PG_HIP(hipMemsetAsync(state, 0, (size_t)N, s)); return PG_OK; }
    int32_t* dregion = nullptr;
    if (int rc = upload_i32("region_classify", region, N, &dregion, s)) return rc;
    const RegionArgs B = args_of(bank);
    if (most > wave_edges()) hipLaunchKernelGGL(region_classify_kernel<4>, dim3(grid_of(N, true)), dim3(256), 0, s, B, pts, dregion, N, state);
    else hipLaunchKernelGGL(region_classify_kernel<1>, dim3(grid_of(N, false)), dim3(256), 0, s, B, pts, dregion, N, state);
    int rc = pg_check_launch("region_classify");
    (void)hipFreeAsync(dregion, s);
    if (rc == PG_OK) PG_HIP(hipStreamSynchronize(s));               // `region` is the source of an asynchronous copy
    return rc;
}

extern "C" int pg_region_nearest(const pg_region_bank* bank, const double* pts, int64_t N, int32_t* idx, double* dist, void* stream) {
    if (N < 0 || N > INT_MAX) { pg_set_error("region_nearest: N = %lld is outside 0 .. %d", (long long)N, INT_MAX); return PG_EINVAL; }
    int64_t most = 0;
    if (int rc = check_bank("region_nearest", bank, true, &most)) return rc;
    if (N == 0) return PG_OK;
    if (!pts || !idx || !dist) { pg_set_error("region_nearest: null argument"); return PG_EINVAL; }
    hipStream_t s = (hipStream_t)stream;
    const RegionArgs B = args_of(bank);                             // R = 0: the kernel's loop is empty, idx = -1, dist = inf
    if (most > wave_edges()) hipLaunchKernelGGL(region_nearest_kernel<4>, dim3(grid_of(N, true)), dim3(256), 0, s, B, pts, N, idx, dist);
    else hipLaunchKernelGGL(region_nearest_kernel<1>, dim3(grid_of(N, false)), dim3(256), 0, s, B, pts, N, idx, dist);
    return pg_check_launch("region_nearest");
}
