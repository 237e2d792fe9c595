// preprocess.hip -- CLIP image preprocessing on the GPU: uint8 RGB (N,H,W,3) -> pixel_values (N,3,336,336), the step in
// FRONT of the hot path.
//
// Replaces `CLIPProcessor(images=pil_image, return_tensors='pt')` at reference models/clip_embedder.py:52,
// dataset_creation/finetune/embed_dataset.py:20, preprocessing/dataset_preprocessing.py:193,
// dataset_creation/benchmark/benchmark_dataset.py:99, i.e. (transformers 4.23.1 CLIPFeatureExtractor, reference env.yml:60)
//   resize shorter edge -> 336 with PIL BICUBIC ; centre crop 336x336 ; float32 / 255.0 ; (x - mean) / std ; HWC -> CHW
// bit for bit: Pillow resamples 8-bit images in FIXED POINT (libImaging/Resample.c: 22-bit coefficients, horizontal pass
// then vertical pass, the intermediate image rounded and clipped to uint8), so the same integer arithmetic on the GPU
// reproduces the uint8 result exactly; the float part takes only 3 x 256 distinct values and is a lookup table built with
// IEEE float32 divisions.  The 1.35 MB/image fp32 host->device stream of the reference becomes <= 1.2 MB of uint8 (640x640)
// and the ViT's im2col reads 16-bit pixels.
//
// Kernels (both HBM-bound byte streams, one block per image row):
//   prep_h_kernel   source row (W x 3 bytes) staged in LDS; thread xo of 336 accumulates its taps for R,G,B -> uint8 temp
//   prep_v_kernel   output row yo: thread xo accumulates the vertical taps over temp rows (coalesced 3-byte pixels),
//                   clips, looks up the normalised value and writes the three channel planes (coalesced along x); with out dtype
//                   PG_DTYPE_U8 it writes the clipped byte itself and the encoder's im2col does the lookup (pg_norm_lut_fill below
//                   is the table's one definition, exported as pg_prep_norm_lut)
// Only the rows / columns the 336x336 crop needs are ever computed (Pillow computes the full resized image, then crops:
// rows and columns are independent, so the cropped values are identical).
//
// Ragged batches (pg_prep_ragged_*: n images of n sizes in one packed buffer, layout in pigeon_hip.h) run three kernels per call:
//   prep_ragged_tables_kernel  one block per (image, axis): thread o computes the bounds and weights of output o of the crop, in
//                              double, with the function the host tables of pg_prep_create are made with (prep_coeffs_one)
//   prep_ragged_h_kernel       one block per temp row of the WHOLE batch; the block finds its image by binary search in the
//                              descriptors' row prefix, then works as prep_h_kernel (prep_h_taps)
//   prep_ragged_v_kernel       grid (336, n), as prep_v_kernel (prep_v_taps / prep_store)
#include "common.h"
#include "pigeon_internal.h"

#include <cmath>
#include <map>
#include <mutex>
#include <vector>

#define PREP_BITS 22              // Pillow PRECISION_BITS = 32 - 8 - 2
#define PREP_SIZE 336
#define PREP_TROW (PREP_SIZE * 3) // bytes per temp row

struct pg_prep {
    int device = 0;
    int in_h = 0, in_w = 0, new_h = 0, new_w = 0, top = 0, left = 0;
    int ksize_h = 0, ksize_v = 0;
    int row0 = 0, nrows = 0;                     // source rows the vertical pass needs
    int32_t *bounds_h = nullptr, *kk_h = nullptr, *bounds_v = nullptr, *kk_v = nullptr;
    float* lut = nullptr;                        // [3][256]
};

// ---- Pillow's coefficient tables, in double, same expression order as Resample.c (host AND device: one body) -------------
__host__ __device__ static inline double bicubic_filter(double x) {
    const double a = -0.5;
    if (x < 0.0) x = -x;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
}

// Full-box precompute_coeffs + normalize_coeffs_8bpc for ONE output `xx` of an in_size -> out_size resize: bounds2 = {first source
// pixel, tap count}, kk[0 .. ksize) = the 22-bit weights (zero behind the tap count); kk == nullptr: bounds only.
// in_size == out_size is Pillow's "pass not needed" case: an identity tap (2^22 at the pixel itself reproduces it exactly).
// The filter is evaluated twice per tap (once for the sum, once for the weight) instead of being kept in an array of ksize doubles:
// the same expression on the same argument gives the same double, and a device thread needs no scratch memory for it.
__host__ __device__ static inline void prep_coeffs_one(int in_size, int out_size, int xx, int ksize, int32_t* bounds2, int32_t* kk) {
    if (in_size == out_size) {
        bounds2[0] = xx; bounds2[1] = 1;
        if (kk) { kk[0] = 1 << PREP_BITS; for (int x = 1; x < ksize; ++x) kk[x] = 0; }
        return;
    }
    double scale, filterscale;
    filterscale = scale = (double)in_size / out_size;
    if (filterscale < 1.0) filterscale = 1.0;
    const double support = 2.0 * filterscale;
    const double ss = 1.0 / filterscale;
    const double center = 0.0 + (xx + 0.5) * scale;
    double ww = 0.0;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > in_size) xmax = in_size;
    xmax -= xmin;
    bounds2[0] = xmin; bounds2[1] = xmax;
    if (!kk) return;
    for (int x = 0; x < xmax; ++x) ww += bicubic_filter((x + xmin - center + 0.5) * ss);
    for (int x = 0; x < xmax; ++x) {
        double v = bicubic_filter((x + xmin - center + 0.5) * ss);
        if (ww != 0.0) v /= ww;
        kk[x] = v < 0 ? (int)(-0.5 + v * (1 << PREP_BITS)) : (int)(0.5 + v * (1 << PREP_BITS));
    }
    for (int x = xmax > 0 ? xmax : 0; x < ksize; ++x) kk[x] = 0;
}

// taps per output of an in_size -> out_size pass (Pillow's ksize; 1 for the identity)
static int prep_ksize(int in_size, int out_size) {
    if (in_size == out_size) return 1;
    double filterscale = (double)in_size / out_size;
    if (filterscale < 1.0) filterscale = 1.0;
    return (int)std::ceil(2.0 * filterscale) * 2 + 1;
}

// The tables of outputs [o0, o0 + PREP_SIZE) (host, for pg_prep_create).
static int make_coeffs(int in_size, int out_size, int o0, std::vector<int32_t>& bounds, std::vector<int32_t>& kk) {
    const int ksize = prep_ksize(in_size, out_size);
    bounds.assign(PREP_SIZE * 2, 0);
    kk.assign((size_t)PREP_SIZE * ksize, 0);
    for (int i = 0; i < PREP_SIZE; ++i) prep_coeffs_one(in_size, out_size, o0 + i, ksize, &bounds[2 * i], &kk[(size_t)i * ksize]);
    return ksize;
}

// transformers 4.23.1 ImageFeatureExtractionMixin.resize(size=336, default_to_square=False) + the centre crop's corner
struct PrepGeom { int new_h, new_w, top, left; };
static PrepGeom prep_geom(int in_h, int in_w) {
    const int shortside = in_w <= in_h ? in_w : in_h, longside = in_w <= in_h ? in_h : in_w;
    int new_short = shortside, new_long = longside;
    if (shortside != PREP_SIZE) { new_short = PREP_SIZE; new_long = (int)((double)PREP_SIZE * longside / shortside); }
    PrepGeom g;
    g.new_w = in_w <= in_h ? new_short : new_long;
    g.new_h = in_w <= in_h ? new_long : new_short;
    g.top = (g.new_h - PREP_SIZE) / 2;
    g.left = (g.new_w - PREP_SIZE) / 2;
    return g;
}

// ((v / 255.0f) - mean) / std in IEEE float32 (what numpy does for float32 arrays).  THE definition of the normalisation table: the
// resize handles, the encoder handle (pg_vit_finalize) and the op-level im2col entry points all get theirs from here.
void pg_norm_lut_fill(float* lut) {
    const float mean[3] = {0.48145466f, 0.4578275f, 0.40821073f}, stdv[3] = {0.26862954f, 0.26130258f, 0.27577711f};
    for (int c = 0; c < 3; ++c)
        for (int v = 0; v < 256; ++v) {
            volatile float x = (float)v / 255.0f;
            volatile float y = x - mean[c];
            lut[c * 256 + v] = y / stdv[c];
        }
}
static std::vector<float> make_lut() {
    std::vector<float> lut(PG_NORM_LUT_SIZE);
    pg_norm_lut_fill(lut.data());
    return lut;
}
extern "C" int pg_prep_norm_lut(float* out) {
    if (!out) { pg_set_error("prep_norm_lut: null argument"); return PG_EINVAL; }
    pg_norm_lut_fill(out);
    return PG_OK;
}

template <typename T>
static int upload(const std::vector<T>& v, T** dst) {
    PG_HIP(hipMalloc((void**)dst, v.size() * sizeof(T)));
    PG_HIP(hipMemcpy(*dst, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    return PG_OK;
}

// A device copy of the table for the entry points that have no handle (pg_op_im2col, pg_op_x3_im2col with PG_DTYPE_U8 pixels): made at
// the first use on a device, kept for the life of the process (3 KB per device).
int pg_norm_lut_device(const float** lut) {
    static std::mutex mu;
    static std::map<int, float*> per_device;
    int dev = 0;
    PG_HIP(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lock(mu);
    auto it = per_device.find(dev);
    if (it == per_device.end()) {
        float* d = nullptr;
        const int rc = upload(make_lut(), &d);
        if (rc) return rc;
        it = per_device.emplace(dev, d).first;
    }
    *lut = it->second;
    return PG_OK;
}

extern "C" int pg_prep_create(pg_prep** out, int device, int in_h, int in_w) {
    if (!out) { pg_set_error("prep_create: null argument"); return PG_EINVAL; }
    if (in_h < 1 || in_w < 1 || in_h > 16384 || in_w > 16384) {
        pg_set_error("prep_create: image size %dx%d out of range (1..16384)", in_h, in_w);
        return PG_EINVAL;
    }
    int n = 0;
    PG_HIP(hipGetDeviceCount(&n));
    if (device < 0 || device >= n) { pg_set_error("prep_create: device %d of %d", device, n); return PG_EINVAL; }
    PG_HIP(hipSetDevice(device));
    pg_prep* h = new pg_prep();
    h->device = device; h->in_h = in_h; h->in_w = in_w;
    const PrepGeom g = prep_geom(in_h, in_w);
    h->new_w = g.new_w; h->new_h = g.new_h;
    if (h->new_w < PREP_SIZE || h->new_h < PREP_SIZE) {
        pg_set_error("prep_create: resized image %dx%d is smaller than the 336x336 crop", h->new_h, h->new_w);
        delete h;
        return PG_EINVAL;
    }
    h->top = g.top;
    h->left = g.left;
    std::vector<int32_t> bh, kh, bv, kv;
    h->ksize_h = make_coeffs(in_w, h->new_w, h->left, bh, kh);
    h->ksize_v = make_coeffs(in_h, h->new_h, h->top, bv, kv);
    h->row0 = bv[0];
    h->nrows = bv[2 * (PREP_SIZE - 1)] + bv[2 * (PREP_SIZE - 1) + 1] - h->row0;
    for (int i = 0; i < PREP_SIZE; ++i) bv[2 * i] -= h->row0;           // vertical taps index the temp image
    const std::vector<float> lut = make_lut();
    int rc = upload(bh, &h->bounds_h);
    if (!rc) rc = upload(kh, &h->kk_h);
    if (!rc) rc = upload(bv, &h->bounds_v);
    if (!rc) rc = upload(kv, &h->kk_v);
    if (!rc) rc = upload(lut, &h->lut);
    if (rc) { pg_prep_destroy(h); return rc; }
    *out = h;
    return PG_OK;
}

extern "C" int pg_prep_destroy(pg_prep* h) {
    if (!h) return PG_OK;
    (void)hipFree(h->bounds_h); (void)hipFree(h->kk_h); (void)hipFree(h->bounds_v); (void)hipFree(h->kk_v); (void)hipFree(h->lut);
    delete h;
    return PG_OK;
}

extern "C" int pg_prep_geometry(const pg_prep* h, int32_t* out6) {
    if (!h || !out6) { pg_set_error("prep_geometry: null argument"); return PG_EINVAL; }
    out6[0] = h->new_h; out6[1] = h->new_w; out6[2] = h->top; out6[3] = h->left; out6[4] = h->row0; out6[5] = h->nrows;
    return PG_OK;
}

extern "C" int pg_prep_workspace_bytes(const pg_prep* h, int n_images, size_t* bytes) {
    if (!h || !bytes || n_images < 0) { pg_set_error("prep_workspace_bytes: bad argument"); return PG_EINVAL; }
    *bytes = (size_t)(n_images > 0 ? n_images : 1) * h->nrows * PREP_TROW + 256;
    return PG_OK;
}

// ---- device -----------------------------------------------------------------------------------------------------------
// The horizontal taps of output column xo over one source row (bytes, `p` at the first tap's pixel) -> the temp row's pixel.
__device__ __forceinline__ void prep_h_taps(const uint8_t* p, const int32_t* __restrict__ k, int cnt, uint8_t* __restrict__ o) {
    int s0 = 1 << (PREP_BITS - 1), s1 = s0, s2 = s0;
    for (int x = 0; x < cnt; ++x) {
        const int w = k[x];
        s0 += (int)p[3 * x] * w; s1 += (int)p[3 * x + 1] * w; s2 += (int)p[3 * x + 2] * w;
    }
    o[0] = (uint8_t)min(max(s0 >> PREP_BITS, 0), 255);
    o[1] = (uint8_t)min(max(s1 >> PREP_BITS, 0), 255);
    o[2] = (uint8_t)min(max(s2 >> PREP_BITS, 0), 255);
}

// The vertical taps of one output pixel over temp rows (`p` at the first tap's row, this column), the lookup of the normalised
// values and the store into the three channel planes.
template <typename OUT>
__device__ __forceinline__ void prep_v_taps(const uint8_t* __restrict__ p, const int32_t* __restrict__ k, int cnt, const float* slut,
                                            OUT* __restrict__ o) {
    int s0 = 1 << (PREP_BITS - 1), s1 = s0, s2 = s0;
    for (int y = 0; y < cnt; ++y) {
        const int w = k[y];
        const uint8_t* q = p + (size_t)y * PREP_TROW;
        s0 += (int)q[0] * w; s1 += (int)q[1] * w; s2 += (int)q[2] * w;
    }
    const int v0 = min(max(s0 >> PREP_BITS, 0), 255), v1 = min(max(s1 >> PREP_BITS, 0), 255), v2 = min(max(s2 >> PREP_BITS, 0), 255);
    const size_t plane = (size_t)PREP_SIZE * PREP_SIZE;
    if constexpr (sizeof(OUT) == 1) {                        // PG_DTYPE_U8: the byte itself, the lookup is the reader's (im2col)
        o[0] = (uint8_t)v0; o[plane] = (uint8_t)v1; o[2 * plane] = (uint8_t)v2;
    } else if constexpr (sizeof(OUT) == 4) {
        o[0] = slut[v0]; o[plane] = slut[256 + v1]; o[2 * plane] = slut[512 + v2];
    } else {
        o[0] = f32_to_f16_bits(slut[v0]); o[plane] = f32_to_f16_bits(slut[256 + v1]); o[2 * plane] = f32_to_f16_bits(slut[512 + v2]);
    }
}

__global__ __launch_bounds__(384) void prep_h_kernel(const uint8_t* __restrict__ img, uint8_t* __restrict__ tmp,
                                                     const int32_t* __restrict__ bounds, const int32_t* __restrict__ kk,
                                                     int ksize, int in_h, int in_w, int row0, int nrows) {
    extern __shared__ uint8_t srow[];
    const int n = blockIdx.y, r = blockIdx.x;
    const uint8_t* src = img + ((size_t)n * in_h + (row0 + r)) * (size_t)in_w * 3;
    const int nbytes = in_w * 3;
    for (int i = threadIdx.x; i < nbytes; i += blockDim.x) srow[i] = src[i];
    __syncthreads();
    const int xo = threadIdx.x;
    if (xo >= PREP_SIZE) return;
    const int xmin = bounds[2 * xo], cnt = bounds[2 * xo + 1];
    prep_h_taps(srow + xmin * 3, kk + (size_t)xo * ksize, cnt, tmp + ((size_t)n * nrows + r) * PREP_TROW + xo * 3);
}

template <typename OUT>
__global__ __launch_bounds__(384) void prep_v_kernel(const uint8_t* __restrict__ tmp, OUT* __restrict__ out,
                                                     const int32_t* __restrict__ bounds, const int32_t* __restrict__ kk,
                                                     const float* __restrict__ lut, int ksize, int nrows) {
    __shared__ float slut[3 * 256];
    for (int i = threadIdx.x; i < 3 * 256; i += blockDim.x) slut[i] = lut[i];
    __syncthreads();
    const int n = blockIdx.y, yo = blockIdx.x, xo = threadIdx.x;
    if (xo >= PREP_SIZE) return;
    const int ymin = bounds[2 * yo], cnt = bounds[2 * yo + 1];
    const size_t plane = (size_t)PREP_SIZE * PREP_SIZE;
    prep_v_taps<OUT>(tmp + ((size_t)n * nrows + ymin) * PREP_TROW + xo * 3, kk + (size_t)yo * ksize, cnt, slut,
                     out + (size_t)n * 3 * plane + (size_t)yo * PREP_SIZE + xo);
}

// ---- device, ragged batches: the descriptors are read from the head of the packed buffer -------------------------------
// One block per (axis, image): thread o < 336 writes the bounds and weights of output o0 + o (o0 = the crop's corner on that axis).
__global__ __launch_bounds__(384) void prep_ragged_tables_kernel(const pg_prep_item* __restrict__ items, uint8_t* __restrict__ ws) {
    const pg_prep_item it = items[blockIdx.y];
    const int o = threadIdx.x;
    if (o >= PREP_SIZE) return;
    const bool vert = blockIdx.x == 1;
    const int in_size = vert ? it.in_h : it.in_w, out_size = vert ? it.new_h : it.new_w, o0 = vert ? it.top : it.left;
    const int ksize = vert ? it.ksize_v : it.ksize_h;
    int32_t* bounds = (int32_t*)(ws + (vert ? it.bounds_v_off : it.bounds_h_off));
    int32_t* kk = (int32_t*)(ws + (vert ? it.kk_v_off : it.kk_h_off));
    prep_coeffs_one(in_size, out_size, o0 + o, ksize, bounds + 2 * o, kk + (size_t)o * ksize);
}

// One block per temp row of the batch.  The source row is staged in LDS with 16-byte loads from the 16-byte block its first byte
// lies in (`lead` bytes early) to the one its last byte lies in: images start at multiples of 16 and the packed buffer's length is
// one, so both stay inside the buffer.
__global__ __launch_bounds__(384) void prep_ragged_h_kernel(const uint8_t* __restrict__ packed, uint8_t* __restrict__ ws, int n,
                                                            size_t tmp_off) {
    extern __shared__ __attribute__((aligned(16))) uint8_t srow_r[];
    const pg_prep_item* __restrict__ items = (const pg_prep_item*)packed;
    const int row = blockIdx.x;
    int lo = 0, hi = n - 1;                          // the last image whose first temp row is <= row (every image has >= 1 row)
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (items[mid].tmp_row <= row) lo = mid; else hi = mid - 1;
    }
    const pg_prep_item it = items[lo];
    const int r = row - it.tmp_row;
    if (r >= it.nrows) return;                       // (cannot happen with a checked prefix: the grid is its total)
    const uint8_t* src = packed + it.src_off + (size_t)(it.row0 + r) * (size_t)it.in_w * 3;
    const int lead = (int)((uintptr_t)src & 15);
    const int n16 = (lead + it.in_w * 3 + 15) >> 4;
    const uint4* s4 = (const uint4*)(src - lead);
    uint4* l4 = (uint4*)srow_r;
    for (int i = threadIdx.x; i < n16; i += blockDim.x) l4[i] = s4[i];
    __syncthreads();
    const int xo = threadIdx.x;
    if (xo >= PREP_SIZE) return;
    const int32_t* bounds = (const int32_t*)(ws + it.bounds_h_off);
    const int32_t* kk = (const int32_t*)(ws + it.kk_h_off);
    const int xmin = bounds[2 * xo], cnt = bounds[2 * xo + 1];
    prep_h_taps(srow_r + lead + xmin * 3, kk + (size_t)xo * it.ksize_h, cnt, ws + tmp_off + (size_t)row * PREP_TROW + xo * 3);
}

template <typename OUT>
__global__ __launch_bounds__(384) void prep_ragged_v_kernel(const uint8_t* __restrict__ packed, const uint8_t* __restrict__ ws,
                                                            size_t tmp_off, OUT* __restrict__ out, const float* __restrict__ lut) {
    __shared__ float slut[3 * 256];
    for (int i = threadIdx.x; i < 3 * 256; i += blockDim.x) slut[i] = lut[i];
    __syncthreads();
    const int n = blockIdx.y, yo = blockIdx.x, xo = threadIdx.x;
    if (xo >= PREP_SIZE) return;
    const pg_prep_item it = ((const pg_prep_item*)packed)[n];
    const int32_t* bounds = (const int32_t*)(ws + it.bounds_v_off);
    const int32_t* kk = (const int32_t*)(ws + it.kk_v_off);
    const int ymin = bounds[2 * yo] - it.row0, cnt = bounds[2 * yo + 1];     // the table holds source rows; the temp image starts at row0
    const size_t plane = (size_t)PREP_SIZE * PREP_SIZE;
    prep_v_taps<OUT>(ws + tmp_off + ((size_t)it.tmp_row + ymin) * PREP_TROW + xo * 3, kk + (size_t)yo * it.ksize_v, cnt, slut,
                     out + (size_t)n * 3 * plane + (size_t)yo * PREP_SIZE + xo);
}

extern "C" int pg_prep_forward(pg_prep* h, const void* images_u8, int n_images, void* out, int out_dtype, void* workspace,
                               size_t workspace_bytes, void* stream) {
    if (!h) { pg_set_error("prep_forward: null handle"); return PG_EINVAL; }
    if (n_images < 0) { pg_set_error("prep_forward: n_images = %d", n_images); return PG_EINVAL; }
    if (n_images == 0) return PG_OK;                       // an empty batch is a no-op: its (empty) buffers may be NULL
    if (!images_u8 || !out || !workspace) { pg_set_error("prep_forward: null argument"); return PG_EINVAL; }
    if (out_dtype != PG_DTYPE_F32 && out_dtype != PG_DTYPE_F16 && out_dtype != PG_DTYPE_U8) { pg_set_error("prep_forward: out dtype must be F32, F16 or U8"); return PG_EINVAL; }
    size_t need = 0;
    pg_prep_workspace_bytes(h, n_images, &need);
    if (workspace_bytes < need) { pg_set_error("prep_forward: workspace %zu < required %zu bytes", workspace_bytes, need); return PG_ENOMEM; }
    if (n_images > 65535) { pg_set_error("prep_forward: at most 65535 images per call"); return PG_EINVAL; }
    hipStream_t s = (hipStream_t)stream;
    const size_t lds = (size_t)h->in_w * 3;
    hipLaunchKernelGGL(prep_h_kernel, dim3(h->nrows, n_images), dim3(384), lds, s, (const uint8_t*)images_u8, (uint8_t*)workspace,
                       h->bounds_h, h->kk_h, h->ksize_h, h->in_h, h->in_w, h->row0, h->nrows);
    int rc = pg_check_launch("prep_h");
    if (rc) return rc;
    if (out_dtype == PG_DTYPE_F32)
        hipLaunchKernelGGL(prep_v_kernel<float>, dim3(PREP_SIZE, n_images), dim3(384), 0, s, (const uint8_t*)workspace, (float*)out,
                           h->bounds_v, h->kk_v, h->lut, h->ksize_v, h->nrows);
    else if (out_dtype == PG_DTYPE_U8)
        hipLaunchKernelGGL(prep_v_kernel<uint8_t>, dim3(PREP_SIZE, n_images), dim3(384), 0, s, (const uint8_t*)workspace, (uint8_t*)out,
                           h->bounds_v, h->kk_v, h->lut, h->ksize_v, h->nrows);
    else
        hipLaunchKernelGGL(prep_v_kernel<uint16_t>, dim3(PREP_SIZE, n_images), dim3(384), 0, s, (const uint8_t*)workspace, (uint16_t*)out,
                           h->bounds_v, h->kk_v, h->lut, h->ksize_v, h->nrows);
    return pg_check_launch("prep_v");
}

// ---- ragged batches: host ----------------------------------------------------------------------------------------------
static_assert(sizeof(pg_prep_item) == PG_PREP_ITEM_BYTES, "pg_prep_item layout");
struct pg_prep_ragged {
    int device = 0;
    float* lut = nullptr;                        // [3][256]
};

static inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// The part of a descriptor that follows from (in_h, in_w) alone.  false: a size out of range or a resized image below the crop
// (pg_set_error called with `who` and the image index).
static bool ragged_geometry(const char* who, int i, int in_h, int in_w, pg_prep_item* it) {
    if (in_h < 1 || in_w < 1 || in_h > 16384 || in_w > 16384) {
        pg_set_error("%s: image %d: size %dx%d out of range (1..16384)", who, i, in_h, in_w);
        return false;
    }
    const PrepGeom g = prep_geom(in_h, in_w);
    if (g.new_w < PREP_SIZE || g.new_h < PREP_SIZE) {
        pg_set_error("%s: image %d: resized image %dx%d is smaller than the 336x336 crop", who, i, g.new_h, g.new_w);
        return false;
    }
    it->in_h = in_h; it->in_w = in_w; it->new_h = g.new_h; it->new_w = g.new_w; it->top = g.top; it->left = g.left;
    it->ksize_h = prep_ksize(in_w, g.new_w);
    it->ksize_v = prep_ksize(in_h, g.new_h);
    int32_t first[2], last[2];
    prep_coeffs_one(in_h, g.new_h, g.top, 0, first, nullptr);
    prep_coeffs_one(in_h, g.new_h, g.top + PREP_SIZE - 1, 0, last, nullptr);
    it->row0 = first[0];
    it->nrows = last[0] + last[1] - first[0];
    return true;
}

static const size_t kBoundsBytes = (size_t)PREP_SIZE * 2 * sizeof(int32_t);      // 2688, a multiple of 16
static inline size_t kk_bytes(int ksize) { return (size_t)PREP_SIZE * ksize * sizeof(int32_t); }   // 1344 * ksize, a multiple of 16

extern "C" int pg_prep_ragged_plan(int n, const int32_t* hw, pg_prep_item* items_out, size_t* packed_bytes, size_t* workspace_bytes) {
    if (n < 0) { pg_set_error("prep_ragged_plan: n = %d is negative", n); return PG_EINVAL; }
    if (!packed_bytes || !workspace_bytes) { pg_set_error("prep_ragged_plan: null size pointer"); return PG_EINVAL; }
    *packed_bytes = 0; *workspace_bytes = 0;
    if (n == 0) return PG_OK;
    if (!hw || !items_out) { pg_set_error("prep_ragged_plan: null %s pointer", !hw ? "sizes" : "descriptor"); return PG_EINVAL; }
    if (n > PG_PREP_RAGGED_MAX_IMAGES) {
        pg_set_error("prep_ragged_plan: n = %d, at most %d images per call", n, PG_PREP_RAGGED_MAX_IMAGES);
        return PG_EINVAL;
    }
    size_t src = (size_t)n * PG_PREP_ITEM_BYTES, tab = 0, rows = 0;
    for (int i = 0; i < n; ++i) {
        pg_prep_item it = {};
        if (!ragged_geometry("prep_ragged_plan", i, hw[2 * i], hw[2 * i + 1], &it)) return PG_EINVAL;
        src = align_up(src, 16);
        it.src_off = src;
        src += (size_t)it.in_h * it.in_w * 3;
        const size_t tab_end = tab + 2 * kBoundsBytes + kk_bytes(it.ksize_h) + kk_bytes(it.ksize_v);
        if (tab_end > 0xffffffffull || rows + (size_t)it.nrows > 0x7fffffffull) {
            pg_set_error("prep_ragged_plan: image %d: the batch's tables / temp rows overflow the descriptor's 32-bit offsets; "
                         "split the batch", i);
            return PG_EINVAL;
        }
        it.bounds_h_off = (uint32_t)tab;                 tab += kBoundsBytes;
        it.kk_h_off = (uint32_t)tab;                     tab += kk_bytes(it.ksize_h);
        it.bounds_v_off = (uint32_t)tab;                 tab += kBoundsBytes;
        it.kk_v_off = (uint32_t)tab;                     tab += kk_bytes(it.ksize_v);
        it.tmp_row = (int32_t)rows;
        rows += (size_t)it.nrows;
        items_out[i] = it;
    }
    *packed_bytes = align_up(src, 16);
    *workspace_bytes = align_up(tab, 256) + rows * PREP_TROW;
    return PG_OK;
}

extern "C" int pg_prep_ragged_create(pg_prep_ragged** out, int device) {
    if (!out) { pg_set_error("prep_ragged_create: null argument"); return PG_EINVAL; }
    int n = 0;
    PG_HIP(hipGetDeviceCount(&n));
    if (device < 0 || device >= n) { pg_set_error("prep_ragged_create: device %d of %d", device, n); return PG_EINVAL; }
    PG_HIP(hipSetDevice(device));
    pg_prep_ragged* h = new pg_prep_ragged();
    h->device = device;
    const int rc = upload(make_lut(), &h->lut);
    if (rc) { pg_prep_ragged_destroy(h); return rc; }
    *out = h;
    return PG_OK;
}

extern "C" int pg_prep_ragged_destroy(pg_prep_ragged* h) {
    if (!h) return PG_OK;
    (void)hipFree(h->lut);
    delete h;
    return PG_OK;
}

extern "C" int pg_prep_ragged_forward(pg_prep_ragged* h, const void* packed_dev, size_t packed_bytes, const pg_prep_item* items_host,
                                      int n, void* out, int out_dtype, void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "prep_ragged_forward";
    if (!h) { pg_set_error("%s: null handle", who); return PG_EINVAL; }
    if (n < 0) { pg_set_error("%s: n = %d is negative", who, n); return PG_EINVAL; }
    if (n == 0) return PG_OK;                              // an empty batch is a no-op: its (empty) buffers may be NULL
    if (!packed_dev || !items_host || !out || !workspace) { pg_set_error("%s: null argument", who); return PG_EINVAL; }
    if (out_dtype != PG_DTYPE_F32 && out_dtype != PG_DTYPE_F16 && out_dtype != PG_DTYPE_U8) { pg_set_error("%s: out dtype must be F32, F16 or U8", who); return PG_EINVAL; }
    if (n > PG_PREP_RAGGED_MAX_IMAGES) { pg_set_error("%s: n = %d, at most %d images per call", who, n, PG_PREP_RAGGED_MAX_IMAGES); return PG_EINVAL; }
    if (((uintptr_t)packed_dev & 15) || ((uintptr_t)workspace & 15)) {
        pg_set_error("%s: the packed buffer and the workspace must be 16-byte aligned", who);
        return PG_EINVAL;
    }
    if (packed_bytes % 16) { pg_set_error("%s: packed_bytes = %zu is not a multiple of 16", who, packed_bytes); return PG_EINVAL; }
    // Every descriptor against its own size and against the two buffers, before anything is launched: what the kernels index with
    // is either recomputed here (geometry, taps, rows, the row prefix) or confined to its buffer (the offsets).
    size_t src_end = (size_t)n * PG_PREP_ITEM_BYTES, tab_end = 0, rows = 0;
    int max_w = 0;
    for (int i = 0; i < n; ++i) {
        const pg_prep_item& it = items_host[i];
        pg_prep_item want = {};
        if (!ragged_geometry(who, i, it.in_h, it.in_w, &want)) return PG_EINVAL;
        if (it.new_h != want.new_h || it.new_w != want.new_w || it.top != want.top || it.left != want.left || it.ksize_h != want.ksize_h ||
            it.ksize_v != want.ksize_v || it.row0 != want.row0 || it.nrows != want.nrows) {
            pg_set_error("%s: image %d: the descriptor's geometry is not the one of a %dx%d image", who, i, it.in_h, it.in_w);
            return PG_EINVAL;
        }
        if (it.src_off % 16) { pg_set_error("%s: image %d: source offset %llu is not a multiple of 16", who, i, (unsigned long long)it.src_off); return PG_EINVAL; }
        if (it.src_off < src_end) {
            pg_set_error("%s: image %d: source offset %llu overlaps what lies before it (ends at %zu)", who, i, (unsigned long long)it.src_off, src_end);
            return PG_EINVAL;
        }
        const size_t img_bytes = (size_t)it.in_h * it.in_w * 3;
        if (it.src_off > packed_bytes || img_bytes > packed_bytes - it.src_off) {
            pg_set_error("%s: image %d: source range [%llu, +%zu) ends past the packed buffer's %zu bytes", who, i,
                         (unsigned long long)it.src_off, img_bytes, packed_bytes);
            return PG_EINVAL;
        }
        src_end = it.src_off + img_bytes;
        const uint32_t offs[4] = {it.bounds_h_off, it.kk_h_off, it.bounds_v_off, it.kk_v_off};
        const size_t lens[4] = {kBoundsBytes, kk_bytes(it.ksize_h), kBoundsBytes, kk_bytes(it.ksize_v)};
        for (int t = 0; t < 4; ++t) {
            if (offs[t] % 16) { pg_set_error("%s: image %d: table offset %u is not a multiple of 16", who, i, offs[t]); return PG_EINVAL; }
            if (offs[t] < tab_end) { pg_set_error("%s: image %d: table offset %u overlaps what lies before it (ends at %zu)", who, i, offs[t], tab_end); return PG_EINVAL; }
            if (offs[t] > workspace_bytes || lens[t] > workspace_bytes - offs[t]) {
                pg_set_error("%s: image %d: table range [%u, +%zu) ends past the workspace's %zu bytes", who, i, offs[t], lens[t], workspace_bytes);
                return PG_EINVAL;
            }
            tab_end = offs[t] + lens[t];
        }
        if (it.tmp_row < 0 || (size_t)it.tmp_row != rows) {
            pg_set_error("%s: image %d: first temp row %d is not the sum of the rows before it (%zu)", who, i, it.tmp_row, rows);
            return PG_EINVAL;
        }
        rows += (size_t)it.nrows;
        if (rows > 0x7fffffffull) { pg_set_error("%s: image %d: more than 2^31 temp rows; split the batch", who, i); return PG_EINVAL; }
        if (it.in_w > max_w) max_w = it.in_w;
    }
    const size_t tmp_off = align_up(tab_end, 256);
    for (int i = 0; i < n; ++i) {
        const size_t end = tmp_off + ((size_t)items_host[i].tmp_row + items_host[i].nrows) * PREP_TROW;
        if (end > workspace_bytes) {
            pg_set_error("%s: image %d: its temp rows end at byte %zu of a workspace of %zu bytes (the batch needs %zu)", who, i, end,
                         workspace_bytes, tmp_off + rows * PREP_TROW);
            return PG_ENOMEM;
        }
    }
    hipStream_t s = (hipStream_t)stream;
    const uint8_t* packed = (const uint8_t*)packed_dev;
    uint8_t* ws = (uint8_t*)workspace;
    hipLaunchKernelGGL(prep_ragged_tables_kernel, dim3(2, n), dim3(384), 0, s, (const pg_prep_item*)packed, ws);
    int rc = pg_check_launch("prep_ragged_tables");
    if (rc) return rc;
    const size_t lds = (size_t)max_w * 3 + 32;             // the row, up to 15 bytes in front of it, rounded up to 16: at most 48 KiB + 32
    hipLaunchKernelGGL(prep_ragged_h_kernel, dim3((unsigned)rows), dim3(384), lds, s, packed, ws, n, tmp_off);
    rc = pg_check_launch("prep_ragged_h");
    if (rc) return rc;
    if (out_dtype == PG_DTYPE_F32)
        hipLaunchKernelGGL(prep_ragged_v_kernel<float>, dim3(PREP_SIZE, n), dim3(384), 0, s, packed, (const uint8_t*)ws, tmp_off, (float*)out, h->lut);
    else if (out_dtype == PG_DTYPE_U8)
        hipLaunchKernelGGL(prep_ragged_v_kernel<uint8_t>, dim3(PREP_SIZE, n), dim3(384), 0, s, packed, (const uint8_t*)ws, tmp_off, (uint8_t*)out, h->lut);
    else
        hipLaunchKernelGGL(prep_ragged_v_kernel<uint16_t>, dim3(PREP_SIZE, n), dim3(384), 0, s, packed, (const uint8_t*)ws, tmp_off, (uint16_t*)out, h->lut);
    return pg_check_launch("prep_ragged_v");
}
