// vit_handle.h -- the pg_vit handle and what the encoder's host files share: vit_weights.hip (create / load / finalize / destroy,
// fingerprint), vit.hip (the fast forward pass) and vit_precise.hip (the exact mode).  Included by those three only.
// Each workspace has ONE definition here (FastWs / PreciseWs): the size queries return its total, the passes carve by its offsets.
#pragma once
#include "common.h"
#include "pigeon_internal.h"
#include <map>
#include <string>
#include <vector>

struct LayerW {
    uint16_t *wqkv = nullptr, *wo = nullptr, *w1 = nullptr, *w2 = nullptr;     // 16-bit (cfg.mma_dtype: fp16 or bf16) [N][K]
    float *bqkv = nullptr, *bo = nullptr, *b1 = nullptr, *b2 = nullptr;
    float *ln1g = nullptr, *ln1b = nullptr, *ln2g = nullptr, *ln2b = nullptr;
    // LayerNorm folded into the following GEMM (cfg ln_fold): wqkv / w1 then hold gamma-scaled weights, bqkv / b1 hold
    // beta.W^T + b, and sqkv / s1 the row sums of the ROUNDED folded weights
    float *sqkv = nullptr, *s1 = nullptr;
    // exact mode (cfg.precise): split-fp16 triples [N][3K] = [Wh | Wh | (W - Wh) * 2^8] of the UNFOLDED weights (precise.hip) and the
    // raw fp32 biases of the two GEMMs whose fast-path bias carries the LayerNorm fold
    uint16_t *wqkv3 = nullptr, *wo3 = nullptr, *w13 = nullptr, *w23 = nullptr;
    float *bqkv_raw = nullptr, *b1_raw = nullptr;
};

struct pg_vit {
    pg_vit_cfg cfg;
    int device = 0;
    bool finalized = false;
    bool ln_fold = true;                                   // LayerNorm folded into the GEMMs (env PIGEON_LN_FOLD=0: separate kernels)
    std::map<std::string, std::vector<float>> host;      // staged fp32 parameters until finalize
    std::vector<void*> allocs;
    std::map<const void*, size_t> alloc_bytes;             // byte size of every uploaded parameter buffer (pg_vit_fingerprint / pg_vit_param_read)
    uint16_t* wpatch = nullptr;                           // [1024][640] 16-bit, cfg.mma_dtype (K zero padded)
    uint16_t* wpatch3 = nullptr;                          // exact mode: [1024][3 * 640] split-fp16 triple
    float *cls = nullptr, *pos = nullptr, *preg = nullptr, *preb = nullptr;
    float* norm_lut = nullptr;                            // [3][256] the normalisation table PG_DTYPE_U8 pixels are looked up in (im2col)
    std::vector<LayerW> layers;
    // two half-batches on two HIP streams (env PIGEON_VIT_STREAMS=2): the tail of a persistent GEMM of one half -- a partial last
    // round with a handful of CUs busy -- is filled by the other half's next kernel instead of idling the chip
    int streams = 1;                                       // 1..4 parts; part 0 runs on the caller's stream
    hipStream_t sx[3] = {nullptr, nullptr, nullptr};
    hipEvent_t ev_fork = nullptr, ev_join[3] = {nullptr, nullptr, nullptr};
    // fp16 saturation scan (debug): device counter of 16-bit activations sitting on +-65504
    bool sat_check = false;
    unsigned long long* sat_counter = nullptr;
    // always-on fp16 range alarm (rowstat_finalize_kernel): rows of the residual stream whose sum of squares reaches 65504^2
    unsigned long long* range_alarm = nullptr;
    float range_alarm_sumsq = 0.f;
    // hipGraph of the encoder body (round 4): the ~250 launches between im2col and the token mean touch only the workspace and the
    // weights, so one captured graph per (workspace, n_images) replays them with one host call.  Built at the SECOND forward of a
    // key (the first runs eagerly: it also sets the kernels' LDS attributes, which is not a stream operation), on an internal
    // stream (torch's current stream is usually the legacy default stream, which cannot be captured), launched on the caller's.
    // Off while profiling events / the saturation scan / the multi-stream mode are on, and with env PIGEON_VIT_GRAPH=0.
    struct GraphEntry { const void* ws; int n; int seen; hipGraph_t graph; hipGraphExec_t exec; unsigned long long last_use, epoch; hipEvent_t done; };
    std::vector<GraphEntry> graphs;
    bool use_graph = true;
    hipStream_t capture_stream = nullptr;
    unsigned long long graph_clock = 0;
    long long graph_replays = 0, graph_captures = 0;
    // profiling
    bool prof = false;
    unsigned prof_mask = 0xFFFFFFFFu;                      // classes bracketed while prof is on (bit c = class c)
    struct Ev { hipEvent_t a, b; int cls; };
    std::vector<Ev> evs;
    int64_t prof_launches[PG_PROF_CLASSES] = {0};
    double prof_ms[PG_PROF_CLASSES] = {0};
};

void vit_graph_entry_free(pg_vit::GraphEntry& e);          // vit.hip (the graph cache); pg_vit_destroy frees the entries with it
#define RC(x) do { int rc__ = (x); if (rc__) return rc__; } while (0)
static inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// The index of a class in pg_vit_profile_read's arrays (include/pigeon_hip.h) and in _lib.PROF_CLASSES: the numbers are ABI.
enum ProfClass { PROF_GEMM_QKV = 0, PROF_GEMM_OUT = 1, PROF_GEMM_FC1 = 2, PROF_GEMM_FC2 = 3, PROF_GEMM_PATCH = 4, PROF_ATTENTION = 5,
                 PROF_LAYERNORM = 6, PROF_IM2COL = 7, PROF_TOKEN_MEAN = 8 };
static_assert(PROF_TOKEN_MEAN + 1 == PG_PROF_CLASSES, "one name per profile class");
struct ProfScope {
    pg_vit* h; hipStream_t s; int cls; hipEvent_t a = nullptr, b = nullptr;
    ProfScope(pg_vit* h_, hipStream_t s_, ProfClass c) : h(h_), s(s_), cls(c) {
        if (h->prof && ((h->prof_mask >> c) & 1u)) { (void)hipEventCreate(&a); (void)hipEventCreate(&b); (void)hipEventRecord(a, s); }
    }
    ~ProfScope() { if (a) { (void)hipEventRecord(b, s); h->evs.push_back({a, b, cls}); } }
};
// ------------------------------------------------------------------------------------------------ workspace layouts
// Byte offsets of the buffers of a workspace of M token rows, in member order, each rounded up to 256 bytes, and the total (256 bytes
// trail).  A pass over fewer rows than the workspace was sized for lays it out for ITS rows: every offset grows with M.
static inline size_t ws_take(size_t* at, size_t bytes) { const size_t o = *at; *at += align_up(bytes, 256); return o; }

struct FastWs {                          // the fast encoder's: 14 KB per token row, 16 KB with the LayerNorm fold
    size_t X;                            // fp32 [M][1024], the residual stream
    size_t Xn;                           // 16-bit [M][1024], the QKV GEMM's A operand; the attention output O aliases it
    size_t big;                          // 16-bit [M][4096]: QKV; the fc1 output H and the im2col patches P alias it
    size_t Xn2, statpart, rsA, rsB;      // LN fold only: Xn2 16-bit [M][1024] | statpart [M][16][2] fp32 | rowstat A, B [M][2] fp32
    size_t total;
};
static inline FastWs fast_ws(size_t M, bool ln_fold) {
    FastWs w = {}; size_t at = 0;
    w.X = ws_take(&at, M * VIT_HIDDEN * 4); w.Xn = ws_take(&at, M * VIT_HIDDEN * 2); w.big = ws_take(&at, M * VIT_MLP * 2);
    if (ln_fold) {
        w.Xn2 = ws_take(&at, M * VIT_HIDDEN * 2); w.statpart = ws_take(&at, M * (VIT_HIDDEN / 64) * 8);
        w.rsA = ws_take(&at, M * 8); w.rsB = ws_take(&at, M * 8);
    }
    w.total = at + 256;
    return w;
}
struct PreciseWs {                       // the exact mode's (vit_precise.hip's header has the account per token row)
    size_t X;                            // fp32 [M][1024], the residual stream
    size_t T3;                           // fp16 triple [M][3 * 1024] of a 1024-wide row
    size_t F;                            // fp32 [M][4096]: the QKV GEMM's output [M][3072] / fc1's
    size_t G3;                           // fp16 triple [M][3 * 4096]; the im2col triple and the fp32 attention output O alias it
    size_t PP;                           // fp32 [3][M][4096], the K-split partial products of one GEMM
    size_t total;
};
static inline PreciseWs precise_ws(size_t M) {
    PreciseWs w = {}; size_t at = 0;
    w.X = ws_take(&at, M * VIT_HIDDEN * 4); w.T3 = ws_take(&at, M * 3 * VIT_HIDDEN * 2); w.F = ws_take(&at, M * VIT_MLP * 4);
    w.G3 = ws_take(&at, M * 3 * VIT_MLP * 2); w.PP = ws_take(&at, M * 3 * VIT_MLP * 4);
    w.total = at + 256;
    return w;
}

// ------------------------------------------------------------------------------------------------ the forward entry points
// The argument checks of pg_vit_forward_hidden (who = "vit_forward") and pg_vit_forward_precise ("vit_forward_precise", which also
// needs cfg.precise), in this order; needb = the workspace size the call requires.  PG_OK also for n_images == 0: an empty batch is a
// no-op, its (empty) buffers may be NULL -- the caller returns before touching them.
static inline int vit_forward_check(const char* who, const pg_vit* h, bool precise, const void* pixels, int pix_dtype, int n_images,
                                    const float* emb_out, const void* workspace, size_t workspace_bytes, size_t needb) {
    if (!h) { pg_set_error("%s: null handle", who); return PG_EINVAL; }
    if (!h->finalized) { pg_set_error("%s: handle not finalized", who); return PG_ESTATE; }
    if (precise && !h->cfg.precise) { pg_set_error("%s: the handle was created without cfg.precise (no split-weight copy)", who); return PG_ESTATE; }
    if (n_images < 0) { pg_set_error("%s: n_images = %d", who, n_images); return PG_EINVAL; }
    if (n_images == 0) return PG_OK;
    if (!pixels || !emb_out || !workspace) { pg_set_error("%s: null argument", who); return PG_EINVAL; }
    if (pix_dtype != PG_DTYPE_F32 && pix_dtype != PG_DTYPE_BF16 && pix_dtype != PG_DTYPE_F16 && pix_dtype != PG_DTYPE_U8) { pg_set_error("%s: bad pixel dtype", who); return PG_EINVAL; }
    if (pix_dtype == PG_DTYPE_U8 && ((uintptr_t)pixels & 15) != 0) { pg_set_error("%s: PG_DTYPE_U8 pixels must be 16-byte aligned", who); return PG_EINVAL; }
    if (workspace_bytes < needb) { pg_set_error("%s: workspace %zu < required %zu bytes", who, workspace_bytes, needb); return PG_ENOMEM; }
    if (((uintptr_t)workspace & 255) != 0) { pg_set_error("%s: workspace must be 256-byte aligned", who); return PG_EINVAL; }
    return PG_OK;
}

// Where the images from `first` on start in the caller's pixel, embedding and (may be NULL) hidden-state buffers.
struct ChunkIO { const void* pixels; float *emb, *hidden; };
static inline ChunkIO chunk_io(const void* pixels, int pix_dtype, float* emb_out, float* hidden_out, int first) {
    const size_t img_bytes = (size_t)3 * VIT_IMG * VIT_IMG * (pix_dtype == PG_DTYPE_F32 ? 4 : pix_dtype == PG_DTYPE_U8 ? 1 : 2);
    return {(const char*)pixels + (size_t)first * img_bytes, emb_out + (size_t)first * VIT_HIDDEN,
            hidden_out ? hidden_out + (size_t)first * VIT_TOKENS * VIT_HIDDEN : nullptr};
}
