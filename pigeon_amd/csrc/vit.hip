// vit.hip -- the forward-pass orchestration of the ViT-L/14-336 encoder's FAST path over a pg_vit handle (vit_handle.h; the weights:
// vit_weights.hip; the exact mode: vit_precise.hip; the rest of the exported C ABI of include/pigeon_hip.h: abi.hip).
//
// Forward pass for a chunk of n images (M = 577 n rows), all launches asynchronous on the caller's stream:
//   im2col            pixels (n,3,336,336; fp32 / fp16 / bf16, or bytes looked up in the handle's normalisation table) -> P (576 n, 640) bf16
//   gemm<PATCH>       P x Wpatch^T (+ position)            -> X rows 1..576 of every image (fp32 residual stream)
//   pre_layernorm     class token + position[0], LN in place on X
//   24 x { LN1 -> Xn bf16 ; gemm<QKV> -> QKV bf16 ; attention -> O bf16 (aliases Xn) ; gemm<RESID>(O, Wo) -> X
//          LN2 -> Xn bf16 ; gemm<GELU> -> H bf16 (aliases QKV) ; gemm<RESID>(H, W2) -> X }
//   token_mean        X -> emb (n,1024) fp32
// HBM layout per chunk: X 4 KB/row fp32, Xn/O 2 KB/row bf16, QKV/H/P 8 KB/row bf16  => 14 KB per token row,
// 8.1 MB per image; weights 0.61 GB (16-bit) stay resident.  The residual stream and all LayerNorm / softmax
// statistics are fp32; only MFMA operands are 16-bit: fp16 by default, bf16 with cfg.mma_dtype / PIGEON_MMA_DTYPE=bf16.
// Round 4: everything between im2col and token_mean is replayed from a hipGraph per (workspace, n) key (vit_forward_body_graphed).
#include "vit_handle.h"

static const float kQScale = 0.125f * 1.4426950408889634f;    // head_dim^-0.5 * log2(e)
static size_t ws_bytes_for(int chunk, bool ln_fold) { return fast_ws((size_t)chunk * VIT_TOKENS, ln_fold).total; }
// two-stream mode: the batch is cut in two halves, each with a workspace of its own.  -> the parts of a batch and the bytes from one part's
// workspace to the next (the largest chunk a part sees; an empty batch is sized as one image): the size query and the split both ask here.
static size_t part_ws_bytes(const pg_vit* h, int n_images, int* parts) {
    *parts = (h->streams > 1 && n_images >= 32 * h->streams) ? h->streams : 1;
    const int per = (n_images + *parts - 1) / *parts;
    const int chunk = per < h->cfg.max_chunk ? per : h->cfg.max_chunk;
    return align_up(ws_bytes_for(chunk > 0 ? chunk : 1, h->ln_fold), 256);
}
extern "C" int pg_vit_workspace_bytes(const pg_vit* h, int n_images, size_t* bytes) {
    if (!h || !bytes || n_images < 0) { pg_set_error("vit_workspace_bytes: bad argument"); return PG_EINVAL; }
    int parts = 1;
    const size_t per_part = part_ws_bytes(h, n_images, &parts);
    *bytes = (size_t)parts * per_part;
    return PG_OK;
}
#define SAT(buf, rows, cols, ld) do { if (h->sat_check) RC(pg_count_sat16_launch((buf), (rows), (cols), (ld), dt, h->sat_counter, s)); } while (0)

// everything between the im2col and the token mean: reads / writes the workspace and the handle's weights only
static int vit_forward_body(pg_vit* h, int n, char* ws, hipStream_t s) {
    const int64_t M = (int64_t)n * VIT_TOKENS;
    const FastWs w = fast_ws((size_t)M, h->ln_fold);
    float* X = (float*)(ws + w.X);
    uint16_t *Xn = (uint16_t*)(ws + w.Xn), *big = (uint16_t*)(ws + w.big);
    const float eps = h->cfg.ln_eps;
    const int dt = h->cfg.mma_dtype, D = VIT_HIDDEN, F = VIT_MLP;
    // One GEMM of a layer: out [M][N] = epi(A [M][K] . W [N][K]^T + bias) on dense operands (lda = ldw = K, ldc = N), the default
    // variant, this stream; only the QKV epilogues take a scale (kQScale on the first 1024 columns: Q).
    auto gemm = [&](const void* A, const uint16_t* W, const float* bias, void* out, int N, int K, int epi, const PgGemmExtra* ex = nullptr) -> int {
        const bool qkv = epi == EPI_QKV || epi == EPI_QKV_LN;
        return pg_gemm_launch(dt, A, K, W, K, bias, out, N, (int)M, N, K, epi, qkv ? kQScale : 1.f, qkv ? D : 0, nullptr, 0, s, ex);
    };
    SAT(big, (int64_t)n * VIT_PATCHES, VIT_PATCH_KPAD, VIT_PATCH_KPAD);
    { ProfScope p(h, s, PROF_GEMM_PATCH);
      RC(pg_gemm_launch(dt, big, VIT_PATCH_KPAD, h->wpatch, VIT_PATCH_KPAD, nullptr, X, VIT_HIDDEN, n * VIT_PATCHES, VIT_HIDDEN, VIT_PATCH_KPAD,
                        EPI_PATCH, 1.f, 0, h->pos, 0, s)); }
    if (!h->ln_fold) { ProfScope p(h, s, PROF_LAYERNORM); RC(pg_preln_launch(X, h->cls, h->pos, h->preg, h->preb, M, eps, s)); }
    if (h->ln_fold) {
        // LayerNorm folded into the GEMM that consumes it: the residual GEMMs (out_proj, fc2) emit, next to the fp32
        // residual row, its 16-bit copy and per-slice partial (sum, sum of squares); a per-row finalize turns those into
        // (rstd, mean*rstd); the QKV / fc1 GEMMs multiply the RAW 16-bit row with gamma-scaled weights and apply
        // rstd * acc - mean*rstd * colsum + (beta.W^T + b) in their epilogue.  No stand-alone LayerNorm launch in the
        // layer loop (two 6 KB/row streaming passes per layer gone); tools/precision_sim-style emulation and the golden
        // tests show the same embedding error as the unfused order (the rounding point moves from LN(x) to x).
        uint16_t* Xn2 = (uint16_t*)(ws + w.Xn2);
        float *statpart = (float*)(ws + w.statpart), *rsA = (float*)(ws + w.rsA), *rsB = (float*)(ws + w.rsB);
        const int slots = VIT_HIDDEN / 64;
        // class token + position + pre_layrnorm, and in the same pass the 16-bit copy + row statistics layer 0's folded LN1 needs
        { ProfScope p(h, s, PROF_LAYERNORM); RC(pg_preln_launch(X, h->cls, h->pos, h->preg, h->preb, M, eps, s, Xn, dt, rsA)); }
        SAT(Xn, M, VIT_HIDDEN, VIT_HIDDEN);
        for (int l = 0; l < h->cfg.layers; ++l) {
            const LayerW& L = h->layers[l];
            const bool last = l + 1 == h->cfg.layers;
            PgGemmExtra ex;
            { ProfScope p(h, s, PROF_GEMM_QKV); ex = PgGemmExtra(); ex.colsum = L.sqkv; ex.rowstat = rsA;
              RC(gemm(Xn, L.wqkv, L.bqkv, big, 3 * D, D, EPI_QKV_LN, &ex)); }
            SAT(big, M, 3 * VIT_HIDDEN, 3 * VIT_HIDDEN);
            { ProfScope p(h, s, PROF_ATTENTION); RC(pg_attention_launch(dt, big, Xn, n, s)); }
            SAT(Xn, M, VIT_HIDDEN, VIT_HIDDEN);
            { ProfScope p(h, s, PROF_GEMM_OUT); ex = PgGemmExtra(); ex.x16 = Xn2; ex.ldx = VIT_HIDDEN; ex.statpart = statpart;
              RC(gemm(Xn, L.wo, L.bo, X, D, D, EPI_RESID_STAT, &ex)); }
            SAT(Xn2, M, VIT_HIDDEN, VIT_HIDDEN);
            { ProfScope p(h, s, PROF_LAYERNORM); RC(pg_rowstat_finalize_launch(statpart, slots, rsB, M, eps, s, h->range_alarm, h->range_alarm_sumsq)); }
            { ProfScope p(h, s, PROF_GEMM_FC1); ex = PgGemmExtra(); ex.colsum = L.s1; ex.rowstat = rsB;
              RC(gemm(Xn2, L.w1, L.b1, big, F, D, EPI_GELU_LN, &ex)); }
            SAT(big, M, VIT_MLP, VIT_MLP);
            { ProfScope p(h, s, PROF_GEMM_FC2);
              if (last) RC(gemm(big, L.w2, L.b2, X, D, F, EPI_RESID));
              else { ex = PgGemmExtra(); ex.x16 = Xn; ex.ldx = VIT_HIDDEN; ex.statpart = statpart;
                     RC(gemm(big, L.w2, L.b2, X, D, F, EPI_RESID_STAT, &ex)); } }
            if (!last) SAT(Xn, M, VIT_HIDDEN, VIT_HIDDEN);
            if (!last) { ProfScope p(h, s, PROF_LAYERNORM); RC(pg_rowstat_finalize_launch(statpart, slots, rsA, M, eps, s, h->range_alarm, h->range_alarm_sumsq)); }
        }
    } else
    for (int l = 0; l < h->cfg.layers; ++l) {
        const LayerW& L = h->layers[l];
        { ProfScope p(h, s, PROF_LAYERNORM); RC(pg_layernorm_launch(X, L.ln1g, L.ln1b, Xn, dt, M, eps, s)); }
        SAT(Xn, M, VIT_HIDDEN, VIT_HIDDEN);
        { ProfScope p(h, s, PROF_GEMM_QKV); RC(gemm(Xn, L.wqkv, L.bqkv, big, 3 * D, D, EPI_QKV)); }
        SAT(big, M, 3 * VIT_HIDDEN, 3 * VIT_HIDDEN);
        { ProfScope p(h, s, PROF_ATTENTION); RC(pg_attention_launch(dt, big, Xn, n, s)); }
        SAT(Xn, M, VIT_HIDDEN, VIT_HIDDEN);
        { ProfScope p(h, s, PROF_GEMM_OUT); RC(gemm(Xn, L.wo, L.bo, X, D, D, EPI_RESID)); }
        { ProfScope p(h, s, PROF_LAYERNORM); RC(pg_layernorm_launch(X, L.ln2g, L.ln2b, Xn, dt, M, eps, s)); }
        SAT(Xn, M, VIT_HIDDEN, VIT_HIDDEN);
        { ProfScope p(h, s, PROF_GEMM_FC1); RC(gemm(Xn, L.w1, L.b1, big, F, D, EPI_GELU)); }
        SAT(big, M, VIT_MLP, VIT_MLP);
        { ProfScope p(h, s, PROF_GEMM_FC2); RC(gemm(big, L.w2, L.b2, X, D, F, EPI_RESID)); }
    }
    return PG_OK;
}

// An exec may still be running on the caller's stream when its entry is evicted or found stale: wait for the event recorded behind
// its last launch before destroying it.
void vit_graph_entry_free(pg_vit::GraphEntry& e) {
    if (e.done) { (void)hipEventSynchronize(e.done); (void)hipEventDestroy(e.done); }
    if (e.exec) (void)hipGraphExecDestroy(e.exec);
    if (e.graph) (void)hipGraphDestroy(e.graph);
    e.exec = nullptr; e.graph = nullptr; e.done = nullptr;
}
static int graph_replay(pg_vit* h, pg_vit::GraphEntry* ent, hipStream_t s) {
    PG_HIP(hipGraphLaunch(ent->exec, s));
    if (ent->done) (void)hipEventRecord(ent->done, s);
    ++h->graph_replays;
    return PG_OK;
}
// Run the body through its captured graph if there is one for (ws, n); capture it at the second sight of the key; else eagerly.
static int vit_forward_body_graphed(pg_vit* h, int n, char* ws, hipStream_t s) {
    const bool ok = h->use_graph && !h->prof && !h->sat_check && h->streams == 1;
    if (!ok) return vit_forward_body(h, n, ws, s);
    pg_vit::GraphEntry* ent = nullptr;
    for (auto& e : h->graphs) if (e.ws == ws && e.n == n) { ent = &e; break; }
    if (!ent) {
        if (h->graphs.size() >= 8) {                          // evict the least recently used key
            size_t lru = 0;
            for (size_t i = 1; i < h->graphs.size(); ++i) if (h->graphs[i].last_use < h->graphs[lru].last_use) lru = i;
            vit_graph_entry_free(h->graphs[lru]);
            h->graphs.erase(h->graphs.begin() + lru);
        }
        h->graphs.push_back({ws, n, 0, nullptr, nullptr, 0, pg_tune_epoch(), nullptr});
        ent = &h->graphs.back();
    }
    ent->last_use = ++h->graph_clock;
    if (ent->exec && ent->epoch != pg_tune_epoch()) {         // a pg_tune_* call since the capture: the baked-in knobs are stale
        vit_graph_entry_free(*ent);
        ent->seen = 1;                                         // kernel attributes are set already: capture right away
    }
    if (ent->exec) return graph_replay(h, ent, s);
    if (ent->seen++ == 0) return vit_forward_body(h, n, ws, s);      // first sight: eager (sets kernel attributes, warms caches)
    if (!h->capture_stream) PG_HIP(hipStreamCreateWithFlags(&h->capture_stream, hipStreamNonBlocking));
    hipGraph_t graph = nullptr;
    hipError_t e = hipStreamBeginCapture(h->capture_stream, hipStreamCaptureModeThreadLocal);
    if (e != hipSuccess) { (void)hipGetLastError(); h->use_graph = false; return vit_forward_body(h, n, ws, s); }
    const int rc = vit_forward_body(h, n, ws, h->capture_stream);
    e = hipStreamEndCapture(h->capture_stream, &graph);
    if (rc != PG_OK || e != hipSuccess || !graph) {
        (void)hipGetLastError();
        if (graph) (void)hipGraphDestroy(graph);
        h->use_graph = false;                                  // capture is not available here: stay eager from now on
        return vit_forward_body(h, n, ws, s);
    }
    hipGraphExec_t exec = nullptr;
    e = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
    if (e != hipSuccess || !exec) { (void)hipGetLastError(); (void)hipGraphDestroy(graph); h->use_graph = false; return vit_forward_body(h, n, ws, s); }
    ent->graph = graph; ent->exec = exec; ent->epoch = pg_tune_epoch();
    if (!ent->done) (void)hipEventCreateWithFlags(&ent->done, hipEventDisableTiming);
    ++h->graph_captures;
    return graph_replay(h, ent, s);
}

static int vit_forward_chunk(pg_vit* h, const void* pixels, int pix_dtype, int n, float* emb_out, float* hidden_out, char* ws, hipStream_t s) {
    const int64_t M = (int64_t)n * VIT_TOKENS;
    const FastWs w = fast_ws((size_t)M, h->ln_fold);
    float* X = (float*)(ws + w.X);
    uint16_t* big = (uint16_t*)(ws + w.big);                   // the im2col patches P
    { ProfScope p(h, s, PROF_IM2COL); RC(pg_im2col_launch(pixels, pix_dtype, big, h->cfg.mma_dtype, n, s, h->norm_lut)); }
    RC(vit_forward_body_graphed(h, n, ws, s));
    { ProfScope p(h, s, PROF_TOKEN_MEAN); RC(pg_token_mean_launch(X, emb_out, n, s)); }
    if (hidden_out) PG_HIP(hipMemcpyAsync(hidden_out, X, (size_t)M * VIT_HIDDEN * 4, hipMemcpyDeviceToDevice, s));
    return PG_OK;
}

extern "C" int pg_vit_forward_hidden(pg_vit* h, const void* pixels, int pix_dtype, int n_images, float* emb_out,
                                     float* hidden_out, void* workspace, size_t workspace_bytes, void* stream) {
    int parts = 1;
    const size_t wsp = (h && n_images > 0) ? part_ws_bytes(h, n_images, &parts) : 0;
    RC(vit_forward_check("vit_forward", h, false, pixels, pix_dtype, n_images, emb_out, workspace, workspace_bytes, (size_t)parts * wsp));
    if (n_images == 0) return PG_OK;
    hipStream_t s = (hipStream_t)stream;
    auto run_range = [&](int first, int last, char* ws, hipStream_t st) -> int {
        for (int s0 = first; s0 < last; s0 += h->cfg.max_chunk) {
            const int n = (last - s0) < h->cfg.max_chunk ? (last - s0) : h->cfg.max_chunk;
            const ChunkIO io = chunk_io(pixels, pix_dtype, emb_out, hidden_out, s0);
            RC(vit_forward_chunk(h, io.pixels, pix_dtype, n, io.emb, io.hidden, ws, st));
        }
        return PG_OK;
    };
    if (parts > 1) {
        const int per = (n_images + parts - 1) / parts;
        PG_HIP(hipEventRecord(h->ev_fork, s));               // the side streams start where the caller's stream stands
        for (int i = 0; i + 1 < parts; ++i) PG_HIP(hipStreamWaitEvent(h->sx[i], h->ev_fork, 0));
        int rc = PG_OK;
        for (int i = 0; i < parts && rc == PG_OK; ++i) {
            const int first = i * per, last = (i + 1) * per < n_images ? (i + 1) * per : n_images;
            if (first >= last) continue;
            rc = run_range(first, last, (char*)workspace + (size_t)i * wsp, i == 0 ? s : h->sx[i - 1]);
        }
        // ... and the caller's stream continues when every part is done.  Also after a failed launch in the middle: work already
        // queued on the side streams still writes the caller's buffers, so the caller's stream must not run ahead of it (the
        // first error code is what is returned; the join's own errors only matter if there was none).
        for (int i = 0; i + 1 < parts; ++i) {
            hipError_t e = hipEventRecord(h->ev_join[i], h->sx[i]);
            if (e == hipSuccess) e = hipStreamWaitEvent(s, h->ev_join[i], 0);
            if (e != hipSuccess && rc == PG_OK) { pg_set_error("vit_forward: joining side stream %d failed: %s", i, hipGetErrorString(e)); rc = PG_EHIP; }
        }
        return rc;
    }
    return run_range(0, n_images, (char*)workspace, s);
}

extern "C" int pg_vit_forward(pg_vit* h, const void* pixels, int pix_dtype, int n_images, float* emb_out, void* workspace, size_t workspace_bytes, void* stream) {
    return pg_vit_forward_hidden(h, pixels, pix_dtype, n_images, emb_out, nullptr, workspace, workspace_bytes, stream);
}

// ------------------------------------------------------------------------------------------------ counters, graph switch, profiling
// The value of a device counter of the handle (NULL: no such counter here, 0), optionally cleared.  Synchronises the device.
static int read_counter(pg_vit* h, unsigned long long* ptr, int reset, const char* who, int64_t* out) {
    if (!h || !out) { pg_set_error("%s: null argument", who); return PG_EINVAL; }
    *out = 0;
    if (!ptr) return PG_OK;
    int cur = 0; PG_HIP(hipGetDevice(&cur));
    PG_HIP(hipSetDevice(h->device));                         // the counter lives on the handle's device, whatever is current
    hipError_t e = hipDeviceSynchronize();
    unsigned long long v = 0;
    if (e == hipSuccess) e = hipMemcpy(&v, ptr, sizeof(v), hipMemcpyDeviceToHost);
    if (e == hipSuccess && reset) e = hipMemset(ptr, 0, sizeof(v));
    (void)hipSetDevice(cur);                                 // ... and the caller's current device is put back
    if (e != hipSuccess) { pg_set_error("%s: %s", who, hipGetErrorString(e)); return PG_EHIP; }
    *out = (int64_t)v;
    return PG_OK;
}
extern "C" int pg_vit_range_alarm_read(pg_vit* h, int64_t* rows, int reset) {   // (bf16 operands, or the separate-LayerNorm chain: no alarm)
    return read_counter(h, h ? h->range_alarm : nullptr, reset, "range_alarm_read", rows);
}
extern "C" int pg_vit_saturation_check(pg_vit* h, int on) {
    if (!h) { pg_set_error("saturation_check: null handle"); return PG_EINVAL; }
    if (on && !h->sat_counter) {
        PG_HIP(hipSetDevice(h->device));
        PG_HIP(hipMalloc((void**)&h->sat_counter, sizeof(unsigned long long)));
        h->allocs.push_back(h->sat_counter);
        PG_HIP(hipMemset(h->sat_counter, 0, sizeof(unsigned long long)));
    }
    h->sat_check = on != 0;
    return PG_OK;
}
extern "C" int pg_vit_saturation_read(pg_vit* h, int64_t* count, int reset) {
    return read_counter(h, h ? h->sat_counter : nullptr, reset, "saturation_read", count);
}
extern "C" int pg_vit_graph(pg_vit* h, int on, int64_t* replays, int64_t* captures) {
    if (!h) { pg_set_error("vit_graph: null handle"); return PG_EINVAL; }
    if (on == 0 || on == 1) h->use_graph = on != 0;          // any other value: query only
    if (replays) *replays = h->graph_replays;
    if (captures) *captures = h->graph_captures;
    return PG_OK;
}

extern "C" int pg_vit_profile_enable(pg_vit* h, int on) {
    if (!h) { pg_set_error("profile_enable: null handle"); return PG_EINVAL; }
    h->prof = on != 0;
    h->prof_mask = (on == 1 || on == 0) ? 0xFFFFFFFFu : ((unsigned)on >> 1);     // on >= 2: bit (c + 1) selects class c
    return PG_OK;
}
static int prof_drain(pg_vit* h) {
    for (auto& e : h->evs) {
        PG_HIP(hipEventSynchronize(e.b));
        float ms = 0.f;
        PG_HIP(hipEventElapsedTime(&ms, e.a, e.b));
        h->prof_ms[e.cls] += ms;
        h->prof_launches[e.cls] += 1;
        (void)hipEventDestroy(e.a); (void)hipEventDestroy(e.b);
    }
    h->evs.clear();
    return PG_OK;
}
extern "C" int pg_vit_profile_read(pg_vit* h, int64_t* launches, double* ms) {
    if (!h || !launches || !ms) { pg_set_error("profile_read: null argument"); return PG_EINVAL; }
    RC(prof_drain(h));
    for (int i = 0; i < PG_PROF_CLASSES; ++i) { launches[i] = h->prof_launches[i]; ms[i] = h->prof_ms[i]; }
    return PG_OK;
}
extern "C" int pg_vit_profile_reset(pg_vit* h) {
    if (!h) { pg_set_error("profile_reset: null handle"); return PG_EINVAL; }
    RC(prof_drain(h));
    for (int i = 0; i < PG_PROF_CLASSES; ++i) { h->prof_launches[i] = 0; h->prof_ms[i] = 0; }
    return PG_OK;
}
