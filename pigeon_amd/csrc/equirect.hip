// equirect.hip -- perspective (gnomonic) views of equirectangular panoramas, the step in FRONT of the ragged resize: one H x W
// panorama in, S x S views out, written straight into the packed buffer pg_prep_ragged_forward reads (pigeon_hip.h, pg_equirect_*).
//
// The reference has no code for this (its four views came from an API that renders them), so the contract is this project's own and
// is stated per pixel in DESIGN.md ("Equirectangular panoramas in") and restated in numpy by tests/_equirectref.py: IEEE float64,
// every operation in the order written there, NO contraction (this file is compiled with -ffp-contract=off), a bilinear blend in
// 8.8 fixed point whose four weights sum to 65536.  Only atan2 and sqrt can differ from numpy's in the last bits.
//
// Kernel: equirect_kernel, grid (ceil(max quads / 256), n views).  The view is blockIdx.y, so its descriptor is read through
// wave-uniform addresses (scalar loads).  A lane makes 4 consecutive pixels of the view's flat (S * S) sequence: 12 bytes = three dword
// stores at a dword-aligned offset (a view starts at a multiple of 16); the last S * S mod 4 pixels go out as bytes, as
// jpeg_rgb_kernel does.  The source bytes are gathered directly: neighbouring lanes read neighbouring source pixels, nothing is staged
// in LDS.  Addresses are formed from clamped or wrapped integers only: no coordinate value, NaN included, can move one.
#include <cmath>
#include <cstring>
#include <vector>

#include "pigeon_internal.h"

static_assert(sizeof(pg_eq_item) == PG_EQ_ITEM_BYTES, "pg_eq_item layout");
static_assert(sizeof(pg_eq_view) == 96, "pg_eq_view layout");

#define EQ_MAX_SRC 16384
#define EQ_MAX_VIEW PG_EQ_MAX_VIEW

__device__ __forceinline__ uint32_t equirect_pixel(const pg_eq_item* __restrict__ it, const uint8_t* __restrict__ src, int p) {
    const int S = it->size, H = it->src_h, W = it->src_w;
    const int i = p / S, j = p - i * S;
    const double half = (double)S / 2.0, inv_f = it->inv_f;
    const double x = ((double)j + 0.5 - half) * inv_f, y = ((double)i + 0.5 - half) * inv_f;
    const double wx = (it->rot[0] * x + it->rot[1] * y) + it->rot[2];
    const double wy = (it->rot[3] * x + it->rot[4] * y) + it->rot[5];
    const double wz = (it->rot[6] * x + it->rot[7] * y) + it->rot[8];
    const double lam = atan2(wx, wz), phi = atan2(-wy, sqrt(wx * wx + wz * wz));
    const double u = (lam * (1.0 / (2.0 * M_PI)) + 0.5) * (double)W - 0.5;
    double v = (0.5 - phi * (1.0 / M_PI)) * (double)H - 0.5;
    v = fmin(fmax(v, 0.0), (double)(H - 1));                       // (fmax drops a NaN: v is a number in [0, H - 1] from here on)
    double u0f = floor(u);
    if (!(u0f >= -2.0 && u0f <= (double)W + 1.0)) u0f = 0.0;       // never for finite descriptors; a NaN must not reach the cast
    const double v0f = floor(v);
    const double fa = floor((u - u0f) * 256.0 + 0.5), fb = floor((v - v0f) * 256.0 + 0.5);
    const int a = (fa >= 0.0 && fa <= 256.0) ? (int)fa : 0, b = (fb >= 0.0 && fb <= 256.0) ? (int)fb : 0;
    const int u0 = (int)u0f, v0 = (int)v0f;
    const int c0 = ((u0 % W) + W) % W, c1 = (((u0 + 1) % W) + W) % W;              // true modulo: the seam wraps
    const int r0 = v0, r1 = v0 + 1 < H ? v0 + 1 : H - 1;
    const uint8_t* p00 = src + ((size_t)r0 * W + c0) * 3;
    const uint8_t* p01 = src + ((size_t)r0 * W + c1) * 3;
    const uint8_t* p10 = src + ((size_t)r1 * W + c0) * 3;
    const uint8_t* p11 = src + ((size_t)r1 * W + c1) * 3;
    const uint32_t w00 = (uint32_t)((256 - a) * (256 - b)), w01 = (uint32_t)(a * (256 - b));
    const uint32_t w10 = (uint32_t)((256 - a) * b), w11 = (uint32_t)(a * b);
    uint32_t out = 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const uint32_t s = p00[c] * w00 + p01[c] * w01 + p10[c] * w10 + p11[c] * w11 + 32768u;      // at most 255 * 65536 + 32768
        out |= (s >> 16) << (8 * c);
    }
    return out;
}

__global__ __launch_bounds__(256) void equirect_kernel(const pg_eq_item* __restrict__ items, const uint8_t* __restrict__ src_base,
                                                       uint8_t* __restrict__ packed) {
    const pg_eq_item* __restrict__ it = items + blockIdx.y;
    const int npix = it->size * it->size;
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q * 4 >= npix) return;
    const uint8_t* src = src_base + it->src_off;
    uint8_t* dst = packed + it->dst_off + (size_t)q * 12;
    if (q * 4 + 4 <= npix) {
        const uint32_t p0 = equirect_pixel(it, src, q * 4), p1 = equirect_pixel(it, src, q * 4 + 1);
        const uint32_t p2 = equirect_pixel(it, src, q * 4 + 2), p3 = equirect_pixel(it, src, q * 4 + 3);
        uint32_t* d4 = (uint32_t*)dst;
        d4[0] = p0 | p1 << 24;
        d4[1] = p1 >> 8 | p2 << 16;
        d4[2] = p2 >> 16 | p3 << 8;
    } else {
        for (int i = q * 4; i < npix; ++i, dst += 3) {
            const uint32_t p = equirect_pixel(it, src, i);
            dst[0] = (uint8_t)p; dst[1] = (uint8_t)(p >> 8); dst[2] = (uint8_t)(p >> 16);
        }
    }
}

// ---- host ----------------------------------------------------------------------------------------------------------------
// the checks a view's own numbers must pass, shared by the plan and the forward; `i` names the view
static int equirect_check_view(const char* who, int i, int src_h, int src_w, int size, const double* rot, double inv_f) {
    if (src_h < 1 || src_w < 1 || src_h > EQ_MAX_SRC || src_w > EQ_MAX_SRC) {
        pg_set_error("%s: view %d: source size %dx%d out of range (1..%d)", who, i, src_h, src_w, EQ_MAX_SRC);
        return PG_EINVAL;
    }
    if (size < 1 || size > EQ_MAX_VIEW) { pg_set_error("%s: view %d: view size %d out of range (1..%d)", who, i, size, EQ_MAX_VIEW); return PG_EINVAL; }
    for (int k = 0; k < 9; ++k)
        if (!std::isfinite(rot[k])) { pg_set_error("%s: view %d: rot[%d] is not finite", who, i, k); return PG_EINVAL; }
    if (!std::isfinite(inv_f) || !(inv_f > 0.0)) { pg_set_error("%s: view %d: inv_f = %g is not finite and positive", who, i, inv_f); return PG_EINVAL; }
    return PG_OK;
}

extern "C" int pg_equirect_plan(int n, const pg_eq_view* views, int n_src, const uint64_t* src_offs, pg_eq_item* items_out,
                                pg_prep_item* prep_items_out, size_t* packed_bytes, size_t* prep_workspace_bytes) {
    const char* who = "equirect_plan";
    if (n < 0) { pg_set_error("%s: n = %d is negative", who, n); return PG_EINVAL; }
    if (!packed_bytes || !prep_workspace_bytes) { pg_set_error("%s: null size pointer", who); return PG_EINVAL; }
    *packed_bytes = *prep_workspace_bytes = 0;
    if (n == 0) return PG_OK;
    if (!views || !src_offs || !items_out || !prep_items_out) { pg_set_error("%s: null argument", who); return PG_EINVAL; }
    if (n > PG_PREP_RAGGED_MAX_IMAGES) { pg_set_error("%s: n = %d, at most %d views per call", who, n, PG_PREP_RAGGED_MAX_IMAGES); return PG_EINVAL; }
    std::vector<int32_t> hw(2 * (size_t)n);
    for (int i = 0; i < n; ++i) {
        const pg_eq_view& v = views[i];
        int rc = equirect_check_view(who, i, v.src_h, v.src_w, v.size, v.rot, v.inv_f);
        if (rc) return rc;
        if (v.src_index < 0 || v.src_index >= n_src) { pg_set_error("%s: view %d: source index %d outside the %d sources", who, i, v.src_index, n_src); return PG_EINVAL; }
        if (src_offs[v.src_index] % 16) {
            pg_set_error("%s: view %d: source offset %llu is not a multiple of 16", who, i, (unsigned long long)src_offs[v.src_index]);
            return PG_EINVAL;
        }
        hw[2 * i] = hw[2 * i + 1] = v.size;
    }
    int rc = pg_prep_ragged_plan(n, hw.data(), prep_items_out, packed_bytes, prep_workspace_bytes);
    if (rc) return rc;
    for (int i = 0; i < n; ++i) {
        const pg_eq_view& v = views[i];
        pg_eq_item it;
        memset(&it, 0, sizeof(it));
        it.src_off = src_offs[v.src_index];
        it.dst_off = prep_items_out[i].src_off;
        it.src_h = v.src_h; it.src_w = v.src_w; it.size = v.size;
        for (int k = 0; k < 9; ++k) it.rot[k] = v.rot[k];
        it.inv_f = v.inv_f;
        items_out[i] = it;
    }
    return PG_OK;
}

extern "C" int pg_equirect_forward(const void* src_dev, size_t src_bytes, const pg_eq_item* items_host, const pg_prep_item* prep_items_host,
                                   int n, void* packed_dev, size_t packed_bytes, void* stream) {
    const char* who = "equirect_forward";
    if (n < 0) { pg_set_error("%s: n = %d is negative", who, n); return PG_EINVAL; }
    if (n == 0) return PG_OK;
    if (!src_dev || !items_host || !prep_items_host || !packed_dev) { pg_set_error("%s: null argument", who); return PG_EINVAL; }
    if (n > PG_PREP_RAGGED_MAX_IMAGES) { pg_set_error("%s: n = %d, at most %d views per call", who, n, PG_PREP_RAGGED_MAX_IMAGES); return PG_EINVAL; }
    if (((uintptr_t)src_dev & 15) || ((uintptr_t)packed_dev & 15)) {
        pg_set_error("%s: the source buffer and the packed buffer must be 16-byte aligned", who);
        return PG_EINVAL;
    }
    const uintptr_t s0 = (uintptr_t)src_dev, p0 = (uintptr_t)packed_dev;
    if (s0 < p0 + packed_bytes && p0 < s0 + src_bytes) { pg_set_error("%s: the source buffer and the packed buffer overlap", who); return PG_EINVAL; }
    size_t dst_end = (size_t)n * PG_PREP_ITEM_BYTES;
    int max_quads = 0;
    for (int i = 0; i < n; ++i) {
        const pg_eq_item& it = items_host[i];
        int rc = equirect_check_view(who, i, it.src_h, it.src_w, it.size, it.rot, it.inv_f);
        if (rc) return rc;
        if (it.reserved0 || it.reserved[0] || it.reserved[1] || it.reserved[2] || it.reserved[3]) {
            pg_set_error("%s: view %d: a reserved field is not zero", who, i);
            return PG_EINVAL;
        }
        if (it.size != prep_items_host[i].in_h || it.size != prep_items_host[i].in_w || it.dst_off != prep_items_host[i].src_off) {
            pg_set_error("%s: view %d: size or offset differs from the resize's descriptor", who, i);
            return PG_EINVAL;
        }
        const size_t src_b = (size_t)it.src_h * it.src_w * 3, dst_b = (size_t)it.size * it.size * 3;
        if (it.src_off % 16) { pg_set_error("%s: view %d: source offset %llu is not a multiple of 16", who, i, (unsigned long long)it.src_off); return PG_EINVAL; }
        if (it.src_off > src_bytes || src_b > src_bytes - it.src_off) {
            pg_set_error("%s: view %d: source range [%llu, +%zu) ends past the source buffer's %zu bytes", who, i, (unsigned long long)it.src_off, src_b, src_bytes);
            return PG_EINVAL;
        }
        if (it.dst_off % 16) { pg_set_error("%s: view %d: destination offset %llu is not a multiple of 16", who, i, (unsigned long long)it.dst_off); return PG_EINVAL; }
        if (it.dst_off < dst_end) {
            pg_set_error("%s: view %d: destination offset %llu overlaps what lies before it (ends at %zu)", who, i, (unsigned long long)it.dst_off, dst_end);
            return PG_EINVAL;
        }
        if (it.dst_off > packed_bytes || dst_b > packed_bytes - it.dst_off) {
            pg_set_error("%s: view %d: destination range [%llu, +%zu) ends past the packed buffer's %zu bytes", who, i, (unsigned long long)it.dst_off, dst_b, packed_bytes);
            return PG_EINVAL;
        }
        dst_end = it.dst_off + dst_b;
        const int quads = (it.size * it.size + 3) / 4;
        if (quads > max_quads) max_quads = quads;
    }
    hipStream_t s = (hipStream_t)stream;
    // the views' descriptors: stream-ordered device scratch, freed behind the launch (neither buffer of the caller has room for them)
    pg_eq_item* items_dev = nullptr;
    PG_HIP(hipMallocAsync((void**)&items_dev, (size_t)n * PG_EQ_ITEM_BYTES, s));
    hipError_t e = hipMemcpyAsync(items_dev, items_host, (size_t)n * PG_EQ_ITEM_BYTES, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(packed_dev, prep_items_host, (size_t)n * PG_PREP_ITEM_BYTES, hipMemcpyHostToDevice, s);
    if (e != hipSuccess) {
        (void)hipFreeAsync(items_dev, s);
        pg_set_error("%s: hipMemcpyAsync of the descriptors failed: %s", who, hipGetErrorString(e));
        return PG_EHIP;
    }
    hipLaunchKernelGGL(equirect_kernel, dim3((max_quads + 255) / 256, n), dim3(256), 0, s, (const pg_eq_item*)items_dev,
                       (const uint8_t*)src_dev, (uint8_t*)packed_dev);
    int rc = pg_check_launch("equirect");
    (void)hipFreeAsync(items_dev, s);
    return rc;
}
