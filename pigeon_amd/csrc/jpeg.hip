// jpeg.hip -- baseline JPEG decoding in front of the ragged resize (include/pigeon_hip.h, "Baseline JPEG decoding").
// Host: pg_jpeg_probe / pg_jpeg_plan / pg_jpeg_entropy_decode over csrc/jpeg_entropy.h (no HIP call in any of them).
// Device: two integer kernels, dequantise + inverse DCT into 8-bit planes, then chroma upsampling + colour conversion into the
// packed RGB buffer.  Compiled with -ffp-contract=off like preprocess.hip (everything here is integer).
#include <atomic>
#include <thread>
#include <vector>

#include "jpeg_entropy.h"
#include "pigeon_internal.h"

static_assert(sizeof(pg_jpeg_item) == PG_JPEG_ITEM_BYTES, "pg_jpeg_item layout");
static_assert(sizeof(pg_jpeg_info) == 32, "pg_jpeg_info layout");

static inline size_t jalign(size_t v, size_t a) { return (v + a - 1) / a * a; }

// ---- device --------------------------------------------------------------------------------------------------------------
// libjpeg's accurate integer inverse DCT ("islow") of one line of 8, in 32-bit wrap-around arithmetic: y = (.. + round) >> s.
template <int S>
__device__ __forceinline__ void idct8(const uint32_t x[8], int32_t y[8]) {
    uint32_t z1 = (x[2] + x[6]) * 4433u;
    const uint32_t t2 = z1 - x[6] * 15137u, t3 = z1 + x[2] * 6270u;
    const uint32_t t0 = (x[0] + x[4]) << 13, t1 = (x[0] - x[4]) << 13;
    const uint32_t t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    uint32_t a = x[7], b = x[5], c = x[3], d = x[1];
    z1 = a + d;
    uint32_t z2 = b + c, z3 = a + c, z4 = b + d;
    const uint32_t z5 = (z3 + z4) * 9633u;
    a *= 2446u; b *= 16819u; c *= 25172u; d *= 12299u;
    z1 *= (uint32_t)-7373; z2 *= (uint32_t)-20995; z3 = z3 * (uint32_t)-16069 + z5; z4 = z4 * (uint32_t)-3196 + z5;
    a += z1 + z3; b += z2 + z4; c += z2 + z3; d += z1 + z4;
    const uint32_t r = 1u << (S - 1);
    y[0] = (int32_t)(t10 + d + r) >> S; y[7] = (int32_t)(t10 - d + r) >> S;
    y[1] = (int32_t)(t11 + c + r) >> S; y[6] = (int32_t)(t11 - c + r) >> S;
    y[2] = (int32_t)(t12 + b + r) >> S; y[5] = (int32_t)(t12 - b + r) >> S;
    y[3] = (int32_t)(t13 + a + r) >> S; y[4] = (int32_t)(t13 - a + r) >> S;
}

// range_limit[v & 1023]: the low 10 bits as a signed value, plus 128, clamped to a byte
__device__ __forceinline__ uint32_t range_limit(int32_t v) {
    const int32_t s = ((v & 1023) ^ 512) - 512;
    return (uint32_t)min(max(s + 128, 0), 255);
}

// 8 lanes per block: lane j of the 8 loads row j of the coefficients (16 bytes; a wave reads 8 blocks = 1024 contiguous bytes) and row
// j of the quantisation table, dequantises, and the 8 x 8 goes through LDS twice: transposed for the column pass (lane j = column j),
// back for the row pass (lane j = row j), whose 8 samples are one 8-byte store into the plane.  grid (ceil(max blocks / 32), n).
#define JPEG_BLOCKS_PER_WG 32
#define JPEG_LDS_STRIDE 73        /* 8 rows of 9 words + 1: column reads of the 8 lanes and of neighbouring blocks spread over the banks */
__global__ __launch_bounds__(256) void jpeg_idct_kernel(const uint8_t* __restrict__ coef, uint8_t* __restrict__ ws) {
    __shared__ int32_t tile[JPEG_BLOCKS_PER_WG * JPEG_LDS_STRIDE];
    const pg_jpeg_item* __restrict__ it = (const pg_jpeg_item*)coef + blockIdx.y;
    const int ncomp = it->ncomp;
    const int nb0 = it->bw[0] * it->bh[0], nb1 = ncomp == 3 ? it->bw[1] * it->bh[1] : 0;
    const int total = ncomp == 0 ? 0 : nb0 + 2 * nb1;
    if ((int)blockIdx.x * JPEG_BLOCKS_PER_WG >= total) return;         // (uniform over the workgroup)
    const int slot = threadIdx.x >> 3, j = threadIdx.x & 7;
    const int l = blockIdx.x * JPEG_BLOCKS_PER_WG + slot;
    const bool live = l < total;
    const int c = l < nb0 ? 0 : (l < nb0 + nb1 ? 1 : 2);
    const int lc = l - (c == 0 ? 0 : (c == 1 ? nb0 : nb0 + nb1));
    int32_t* t = tile + slot * JPEG_LDS_STRIDE;
    uint32_t x[8];
    int32_t y[8];
    if (live) {
        const uint4 cv = *(const uint4*)(coef + it->coef_off[c] + (size_t)lc * 128 + j * 16);
        const uint4 qv = *(const uint4*)(&it->qt[it->qsel[c] & 3][j * 8]);
        const uint32_t cw[4] = {cv.x, cv.y, cv.z, cv.w}, qw[4] = {qv.x, qv.y, qv.z, qv.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            t[j * 9 + 2 * k] = (int32_t)((uint32_t)(int32_t)(int16_t)(cw[k] & 0xffff) * (qw[k] & 0xffff));
            t[j * 9 + 2 * k + 1] = (int32_t)((uint32_t)(int32_t)(int16_t)(cw[k] >> 16) * (qw[k] >> 16));
        }
    }
    __syncthreads();
    if (live) {
#pragma unroll
        for (int k = 0; k < 8; ++k) x[k] = (uint32_t)t[k * 9 + j];      // column j
        idct8<11>(x, y);
    }
    __syncthreads();
    if (live) {
#pragma unroll
        for (int k = 0; k < 8; ++k) t[k * 9 + j] = y[k];
    }
    __syncthreads();
    if (live) {
#pragma unroll
        for (int k = 0; k < 8; ++k) x[k] = (uint32_t)t[j * 9 + k];      // row j
        idct8<18>(x, y);
        const int bw = it->bw[c];
        const int by = lc / bw, bx = lc - by * bw;
        uint2 o;
        o.x = range_limit(y[0]) | range_limit(y[1]) << 8 | range_limit(y[2]) << 16 | range_limit(y[3]) << 24;
        o.y = range_limit(y[4]) | range_limit(y[5]) << 8 | range_limit(y[6]) << 16 | range_limit(y[7]) << 24;
        *(uint2*)(ws + it->plane_off[c] + ((size_t)(by * 8 + j) * bw + bx) * 8) = o;
    }
}

// One chroma sample at full resolution, as libjpeg-turbo's fancy upsampling gives it over the REAL chroma plane (cw x ch samples of a
// plane `stride` bytes wide); chroma widths of 1 and 2 are replicated, not filtered (libjpeg's own rule).
__device__ __forceinline__ int chroma_at(const uint8_t* __restrict__ p, int stride, int cw, int ch, int hs, int vs, int y, int x) {
    if (hs == 1) return p[(size_t)y * stride + x];
    const int cx = x >> 1;
    if (cw <= 2) return p[(size_t)(vs == 2 ? y >> 1 : y) * stride + cx];
    if (vs == 1) {
        const uint8_t* r = p + (size_t)y * stride;
        if (x & 1) return cx == cw - 1 ? r[cx] : (3 * r[cx] + r[cx + 1] + 2) >> 2;
        return cx == 0 ? r[0] : (3 * r[cx] + r[cx - 1] + 1) >> 2;
    }
    const int cy = y >> 1;
    const int ny = (y & 1) ? min(cy + 1, ch - 1) : max(cy - 1, 0);     // rows outside the plane replicate the edge row
    const uint8_t* r0 = p + (size_t)cy * stride;
    const uint8_t* r1 = p + (size_t)ny * stride;
    const int t = 3 * r0[cx] + r1[cx];
    if (x & 1) {
        if (cx == cw - 1) return (4 * t + 7) >> 4;
        return (3 * t + 3 * r0[cx + 1] + r1[cx + 1] + 7) >> 4;
    }
    if (cx == 0) return (4 * t + 8) >> 4;
    return (3 * t + 3 * r0[cx - 1] + r1[cx - 1] + 8) >> 4;
}

__device__ __forceinline__ uint32_t clamp_u8(int v) { return (uint32_t)min(max(v, 0), 255); }

__device__ __forceinline__ uint32_t jpeg_pixel(const pg_jpeg_item* __restrict__ it, const uint8_t* __restrict__ ws, int cw, int ch, int pix) {
    const int w = it->width;
    const int y = pix / w, x = pix - y * w;
    const int Y = ws[it->plane_off[0] + (size_t)y * (it->bw[0] * 8) + x];
    if (it->ncomp == 1) return (uint32_t)Y * 0x010101u;
    const int stride = it->bw[1] * 8;
    const int cb = chroma_at(ws + it->plane_off[1], stride, cw, ch, it->hs, it->vs, y, x) - 128;
    const int cr = chroma_at(ws + it->plane_off[2], stride, cw, ch, it->hs, it->vs, y, x) - 128;
    const uint32_t R = clamp_u8(Y + ((91881 * cr + 32768) >> 16));
    const uint32_t G = clamp_u8(Y + ((-22554 * cb + 32768 - 46802 * cr) >> 16));
    const uint32_t B = clamp_u8(Y + ((116130 * cb + 32768) >> 16));
    return R | G << 8 | B << 16;
}

// A lane makes 4 consecutive pixels of the image's flat (H * W) pixel sequence: 12 bytes = three dword stores at a dword-aligned
// offset (the image starts at a multiple of 16).  The last H * W mod 4 pixels go out as bytes.  grid (ceil(max quads / 256), n).
__global__ __launch_bounds__(256) void jpeg_rgb_kernel(const uint8_t* __restrict__ coef, const uint8_t* __restrict__ ws, uint8_t* __restrict__ packed) {
    const pg_jpeg_item* __restrict__ it = (const pg_jpeg_item*)coef + blockIdx.y;
    if (it->ncomp == 0) return;
    const int npix = it->height * it->width;
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q * 4 >= npix) return;
    const int cw = (it->width + it->hs - 1) / it->hs, ch = (it->height + it->vs - 1) / it->vs;
    uint8_t* dst = packed + it->rgb_off + (size_t)q * 12;
    if (q * 4 + 4 <= npix) {
        const uint32_t p0 = jpeg_pixel(it, ws, cw, ch, q * 4), p1 = jpeg_pixel(it, ws, cw, ch, q * 4 + 1);
        const uint32_t p2 = jpeg_pixel(it, ws, cw, ch, q * 4 + 2), p3 = jpeg_pixel(it, ws, cw, ch, q * 4 + 3);
        uint32_t* d4 = (uint32_t*)dst;
        d4[0] = p0 | p1 << 24;
        d4[1] = p1 >> 8 | p2 << 16;
        d4[2] = p2 >> 16 | p3 << 8;
    } else {
        for (int i = q * 4; i < npix; ++i, dst += 3) {
            const uint32_t p = jpeg_pixel(it, ws, cw, ch, i);
            dst[0] = (uint8_t)p; dst[1] = (uint8_t)(p >> 8); dst[2] = (uint8_t)(p >> 16);
        }
    }
}

// ---- host ----------------------------------------------------------------------------------------------------------------
extern "C" const char* pg_jpeg_reason(int reason) { return pgjpeg::reason_text(reason); }

extern "C" int pg_jpeg_probe(const void* data, size_t nbytes, pg_jpeg_info* info) {
    if (!data || !info) { pg_set_error("jpeg_probe: null argument"); return PG_EINVAL; }
    pgjpeg::Header h;
    pgjpeg::parse_header((const uint8_t*)data, nbytes, &h);
    memset(info, 0, sizeof(*info));
    info->reason = h.reason; info->height = h.height; info->width = h.width; info->ncomp = h.ncomp; info->hs = h.hs; info->vs = h.vs;
    return PG_OK;
}

static bool jpeg_sampling_ok(int ncomp, int hs, int vs) {
    if (ncomp == 1) return hs == 1 && vs == 1;
    return ncomp == 3 && ((hs == 1 && vs == 1) || (hs == 2 && vs == 1) || (hs == 2 && vs == 2));
}

extern "C" int pg_jpeg_plan(int n, const pg_jpeg_info* infos, pg_jpeg_item* items_out, pg_prep_item* prep_items_out, size_t* coef_bytes,
                            size_t* workspace_bytes, size_t* packed_bytes, size_t* prep_workspace_bytes) {
    const char* who = "jpeg_plan";
    if (n < 0) { pg_set_error("%s: n = %d is negative", who, n); return PG_EINVAL; }
    if (!coef_bytes || !workspace_bytes || !packed_bytes || !prep_workspace_bytes) { pg_set_error("%s: null size pointer", who); return PG_EINVAL; }
    *coef_bytes = *workspace_bytes = *packed_bytes = *prep_workspace_bytes = 0;
    if (n == 0) return PG_OK;
    if (!infos || !items_out || !prep_items_out) { pg_set_error("%s: null argument", who); return PG_EINVAL; }
    if (n > PG_PREP_RAGGED_MAX_IMAGES) { pg_set_error("%s: n = %d, at most %d images per call", who, n, PG_PREP_RAGGED_MAX_IMAGES); return PG_EINVAL; }
    std::vector<int32_t> hw(2 * (size_t)n);
    for (int i = 0; i < n; ++i) { hw[2 * i] = infos[i].height; hw[2 * i + 1] = infos[i].width; }
    int rc = pg_prep_ragged_plan(n, hw.data(), prep_items_out, packed_bytes, prep_workspace_bytes);   // (names the image of a bad size itself)
    if (rc) return rc;
    size_t coef = jalign((size_t)n * PG_JPEG_ITEM_BYTES, 128), ws = 0;
    for (int i = 0; i < n; ++i) {
        pg_jpeg_item it;
        memset(&it, 0, sizeof(it));
        it.rgb_off = prep_items_out[i].src_off;
        it.height = infos[i].height; it.width = infos[i].width;
        if (infos[i].reason == PG_JPEG_R_OK) {
            if (!jpeg_sampling_ok(infos[i].ncomp, infos[i].hs, infos[i].vs)) {
                pg_set_error("%s: image %d: %d components with luma sampling %dx%d is not decoded here", who, i, infos[i].ncomp, infos[i].hs, infos[i].vs);
                return PG_EINVAL;
            }
            it.ncomp = infos[i].ncomp; it.hs = infos[i].hs; it.vs = infos[i].vs;
            pgjpeg::block_grid(it.height, it.width, it.ncomp, it.hs, it.vs, it.bw, it.bh);
            for (int c = 0; c < it.ncomp; ++c) {
                const size_t blocks = (size_t)it.bw[c] * it.bh[c];
                it.coef_off[c] = coef; coef += blocks * 128;
                ws = jalign(ws, 256);
                it.plane_off[c] = ws; ws += blocks * 64;
            }
        }
        items_out[i] = it;
    }
    *coef_bytes = coef;
    *workspace_bytes = jalign(ws, 256);
    return PG_OK;
}

extern "C" int pg_jpeg_entropy_decode(int n, const void* const* data, const size_t* nbytes, pg_jpeg_item* items, void* coef, size_t coef_bytes,
                                      int threads, int* bad_index) {
    const char* who = "jpeg_entropy_decode";
    if (bad_index) *bad_index = -1;
    if (n < 0) { pg_set_error("%s: n = %d is negative", who, n); return PG_EINVAL; }
    if (n == 0) return PG_OK;
    if (!data || !nbytes || !items || !coef) { pg_set_error("%s: null argument", who); return PG_EINVAL; }
    if ((uintptr_t)coef & 15) { pg_set_error("%s: the coefficient buffer must be 16-byte aligned", who); return PG_EINVAL; }
    const size_t head = jalign((size_t)n * PG_JPEG_ITEM_BYTES, 128);
    if (coef_bytes < head) { pg_set_error("%s: coefficient buffer of %zu bytes is smaller than its %d descriptors", who, coef_bytes, n); return PG_EINVAL; }
    for (int i = 0; i < n; ++i) {
        if (items[i].ncomp == 0) continue;
        if (!data[i]) { pg_set_error("%s: image %d: null data", who, i); return PG_EINVAL; }
        for (int c = 0; c < 3 && c < items[i].ncomp; ++c)
            if (items[i].coef_off[c] < head) { pg_set_error("%s: image %d: its coefficients overlap the descriptors", who, i); return PG_EINVAL; }
    }
    std::vector<int> err((size_t)n, 0);
    std::atomic<int> next(0);
    auto work = [&]() {
        for (int i = next.fetch_add(1); i < n; i = next.fetch_add(1))
            if (items[i].ncomp != 0)
                err[i] = pgjpeg::decode_image((const uint8_t*)data[i], nbytes[i], &items[i], (uint8_t*)coef, coef_bytes);
    };
    const int nt = threads < 1 ? 1 : (threads > 16 ? 16 : threads);
    const int spawn = (nt < n ? nt : n) - 1;
    std::vector<std::thread> pool;
    for (int t = 0; t < spawn; ++t) pool.emplace_back(work);
    work();
    for (auto& t : pool) t.join();
    for (int i = 0; i < n; ++i)
        if (err[i]) {
            if (bad_index) *bad_index = i;
            pg_set_error("%s: image %d: %s", who, i, pgjpeg::error_text(err[i]));
            return PG_EINVAL;
        }
    memcpy(coef, items, (size_t)n * PG_JPEG_ITEM_BYTES);
    return PG_OK;
}

extern "C" int pg_jpeg_forward(const void* coef_dev, size_t coef_bytes, const pg_jpeg_item* items_host, const pg_prep_item* prep_items_host,
                               int n, void* packed_dev, size_t packed_bytes, void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "jpeg_forward";
    if (n < 0) { pg_set_error("%s: n = %d is negative", who, n); return PG_EINVAL; }
    if (n == 0) return PG_OK;
    if (!coef_dev || !items_host || !prep_items_host || !packed_dev) { pg_set_error("%s: null argument", who); return PG_EINVAL; }
    if (n > PG_PREP_RAGGED_MAX_IMAGES) { pg_set_error("%s: n = %d, at most %d images per call", who, n, PG_PREP_RAGGED_MAX_IMAGES); return PG_EINVAL; }
    if (((uintptr_t)coef_dev & 15) || ((uintptr_t)packed_dev & 15) || ((uintptr_t)workspace & 15)) {
        pg_set_error("%s: the coefficient buffer, the packed buffer and the workspace must be 16-byte aligned", who);
        return PG_EINVAL;
    }
    size_t coef_end = jalign((size_t)n * PG_JPEG_ITEM_BYTES, 128), ws_end = 0, rgb_end = (size_t)n * PG_PREP_ITEM_BYTES;
    if (coef_bytes < coef_end) { pg_set_error("%s: coefficient buffer of %zu bytes is smaller than its %d descriptors", who, coef_bytes, n); return PG_EINVAL; }
    int max_blocks = 0, max_quads = 0, decoded = 0;
    for (int i = 0; i < n; ++i) {
        const pg_jpeg_item& it = items_host[i];
        if (it.height < 1 || it.width < 1 || it.height > 16384 || it.width > 16384) {
            pg_set_error("%s: image %d: size %dx%d out of range (1..16384)", who, i, it.height, it.width);
            return PG_EINVAL;
        }
        if (it.height != prep_items_host[i].in_h || it.width != prep_items_host[i].in_w || it.rgb_off != prep_items_host[i].src_off) {
            pg_set_error("%s: image %d: size or offset differs from the resize's descriptor", who, i);
            return PG_EINVAL;
        }
        const size_t rgb_bytes = (size_t)it.height * it.width * 3;
        if (it.rgb_off % 16) { pg_set_error("%s: image %d: RGB offset %llu is not a multiple of 16", who, i, (unsigned long long)it.rgb_off); return PG_EINVAL; }
        if (it.rgb_off < rgb_end) { pg_set_error("%s: image %d: RGB offset %llu overlaps what lies before it (ends at %zu)", who, i, (unsigned long long)it.rgb_off, rgb_end); return PG_EINVAL; }
        if (it.rgb_off > packed_bytes || rgb_bytes > packed_bytes - it.rgb_off) {
            pg_set_error("%s: image %d: RGB range [%llu, +%zu) ends past the packed buffer's %zu bytes", who, i, (unsigned long long)it.rgb_off, rgb_bytes, packed_bytes);
            return PG_EINVAL;
        }
        rgb_end = it.rgb_off + rgb_bytes;
        if (it.ncomp == 0) continue;
        if (!jpeg_sampling_ok(it.ncomp, it.hs, it.vs)) { pg_set_error("%s: image %d: %d components with luma sampling %dx%d", who, i, it.ncomp, it.hs, it.vs); return PG_EINVAL; }
        int32_t bw[3], bh[3];
        pgjpeg::block_grid(it.height, it.width, it.ncomp, it.hs, it.vs, bw, bh);
        int blocks_i = 0;
        for (int c = 0; c < it.ncomp; ++c) {
            if (it.bw[c] != bw[c] || it.bh[c] != bh[c]) { pg_set_error("%s: image %d: block grid of component %d is not the one of its size and sampling", who, i, c); return PG_EINVAL; }
            if (it.qsel[c] < 0 || it.qsel[c] > 3) { pg_set_error("%s: image %d: quantisation table %d of component %d", who, i, it.qsel[c], c); return PG_EINVAL; }
            const size_t blocks = (size_t)bw[c] * bh[c];
            if (it.coef_off[c] % 16 || it.plane_off[c] % 16) { pg_set_error("%s: image %d: an offset of component %d is not a multiple of 16", who, i, c); return PG_EINVAL; }
            if (it.coef_off[c] < coef_end || it.plane_off[c] < ws_end) { pg_set_error("%s: image %d: component %d overlaps what lies before it", who, i, c); return PG_EINVAL; }
            if (it.coef_off[c] > coef_bytes || blocks * 128 > coef_bytes - it.coef_off[c]) {
                pg_set_error("%s: image %d: coefficients of component %d end past the buffer's %zu bytes", who, i, c, coef_bytes);
                return PG_EINVAL;
            }
            if (!workspace || it.plane_off[c] > workspace_bytes || blocks * 64 > workspace_bytes - it.plane_off[c]) {
                pg_set_error("%s: image %d: plane of component %d ends past the workspace's %zu bytes", who, i, c, workspace_bytes);
                return PG_ENOMEM;
            }
            coef_end = it.coef_off[c] + blocks * 128;
            ws_end = it.plane_off[c] + blocks * 64;
            blocks_i += (int)blocks;
        }
        if (blocks_i > max_blocks) max_blocks = blocks_i;
        const int quads = (it.height * it.width + 3) / 4;
        if (quads > max_quads) max_quads = quads;
        ++decoded;
    }
    hipStream_t s = (hipStream_t)stream;
    PG_HIP(hipMemcpyAsync(packed_dev, prep_items_host, (size_t)n * PG_PREP_ITEM_BYTES, hipMemcpyHostToDevice, s));
    if (!decoded) return PG_OK;
    hipLaunchKernelGGL(jpeg_idct_kernel, dim3((max_blocks + JPEG_BLOCKS_PER_WG - 1) / JPEG_BLOCKS_PER_WG, n), dim3(256), 0, s,
                       (const uint8_t*)coef_dev, (uint8_t*)workspace);
    int rc = pg_check_launch("jpeg_idct");
    if (rc) return rc;
    hipLaunchKernelGGL(jpeg_rgb_kernel, dim3((max_quads + 255) / 256, n), dim3(256), 0, s, (const uint8_t*)coef_dev,
                       (const uint8_t*)workspace, (uint8_t*)packed_dev);
    return pg_check_launch("jpeg_rgb");
}
