// vit_weights.hip -- a pg_vit handle (vit_handle.h) outside the forward passes: pg_vit_create reads the configuration and the environment,
// pg_vit_load_weight stages fp32 parameters on the host, pg_vit_finalize converts them (16-bit operands, LayerNorm folded into the QKV / fc1
// weights, the exact mode's split-fp16 triples) and uploads them, pg_vit_destroy frees all; pg_vit_fingerprint digests what the fast path reads.
#include "vit_handle.h"
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <type_traits>
#ifndef PG_DEFAULT_VIT_STREAMS
#define PG_DEFAULT_VIT_STREAMS 1
#endif

static std::string canon(const char* name) {
    std::string s(name);
    const std::string pre = "vision_model.";
    if (s.compare(0, pre.size(), pre) == 0) s = s.substr(pre.size());
    return s;
}

extern "C" int pg_vit_create(pg_vit** out, int device, const pg_vit_cfg* cfg) {
    if (!out || !cfg) { pg_set_error("vit_create: null argument"); return PG_EINVAL; }
    if (cfg->image_size != 336 || cfg->patch != 14 || cfg->hidden != 1024 || cfg->heads != 16 || cfg->mlp != 4096 ||
        cfg->layers < 1) {
        pg_set_error("vit_create: only the ViT-L/14-336 geometry is supported (336/14/1024/16/4096, layers>=1)");
        return PG_EINVAL;
    }
    int n = 0;
    PG_HIP(hipGetDeviceCount(&n));
    if (device < 0 || device >= n) { pg_set_error("vit_create: device %d of %d", device, n); return PG_EINVAL; }
    pg_vit* h = new pg_vit();
    h->cfg = *cfg;
    if (h->cfg.ln_eps <= 0) h->cfg.ln_eps = 1e-5f;
    if (h->cfg.max_chunk <= 0) h->cfg.max_chunk = 512;
    if (h->cfg.mma_dtype == 0) {
        const char* e = getenv("PIGEON_MMA_DTYPE");
        h->cfg.mma_dtype = (e && (!strcmp(e, "bf16") || !strcmp(e, "BF16"))) ? PG_DTYPE_BF16 : PG_DTYPE_F16;
    }
    if (h->cfg.mma_dtype != PG_DTYPE_F16 && h->cfg.mma_dtype != PG_DTYPE_BF16) {
        delete h;
        pg_set_error("vit_create: mma_dtype must be 0 (default), PG_DTYPE_F16 or PG_DTYPE_BF16");
        return PG_EINVAL;
    }
    h->device = device;
    // LayerNorm folded into the next GEMM (gamma into the weights, per-row (rstd, mean*rstd) applied in the epilogue): removes the
    // two 0.31 ms LayerNorm launches per layer (1.8 GB of HBM traffic each) for heavier epilogues.  First measured SLOWER
    // (231.5 vs 229.6 ms per step); with the packed 16-bit conversions, the early residual fetch and the C = 0 first k-step
    // it is 1.3 % faster in the same run (2354 vs 2324 img/s) at the same embedding error (2.7e-4), so it is the default.
    // PIGEON_LN_FOLD=0 selects the separate-LayerNorm chain (kept as the A/B arm and for the non-persistent GEMM variants).
    { const char* e = getenv("PIGEON_LN_FOLD"); h->ln_fold = !(e && e[0] == '0'); }
    if (pg_default_gemm_variant() < 30) h->ln_fold = false;   // the folded epilogues exist only in the persistent GEMM
    h->layers.resize(cfg->layers);
    if (h->ln_fold && h->cfg.mma_dtype == PG_DTYPE_F16) {   // the always-on range alarm of the fp16 residual copies
        PG_HIP(hipSetDevice(device));
        PG_HIP(hipMalloc((void**)&h->range_alarm, sizeof(unsigned long long)));
        h->allocs.push_back(h->range_alarm);
        PG_HIP(hipMemset(h->range_alarm, 0, sizeof(unsigned long long)));
        h->range_alarm_sumsq = 65504.0f * 65504.0f;
    }
    { const char* e = getenv("PIGEON_VIT_GRAPH"); h->use_graph = !(e && e[0] == '0'); }
    { const char* e = getenv("PIGEON_VIT_STREAMS"); h->streams = e ? atoi(e) : PG_DEFAULT_VIT_STREAMS; }
    if (h->streams < 1 || h->streams > 4) h->streams = 1;
    if (h->streams > 1) {
        PG_HIP(hipSetDevice(device));
        PG_HIP(hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming));
        for (int i = 0; i + 1 < h->streams; ++i) {
            PG_HIP(hipStreamCreateWithFlags(&h->sx[i], hipStreamNonBlocking));
            PG_HIP(hipEventCreateWithFlags(&h->ev_join[i], hipEventDisableTiming));
        }
    }
    *out = h;
    return PG_OK;
}

// The shape transformers' CLIPVisionModel gives the parameter `key` (canonical name) where this path reads it: its extents to want[4],
// their number returned; 0 for a name finalize never asks for (post_layernorm.*, position_ids, a layer past cfg.layers).
static int param_shape(const pg_vit* h, const std::string& key, int64_t want[4]) {
    const int64_t D = VIT_HIDDEN, F = VIT_MLP;
    auto set = [&](std::initializer_list<int64_t> e) { int i = 0; for (int64_t v : e) want[i++] = v; return (int)e.size(); };
    if (key == "embeddings.patch_embedding.weight") return set({D, 3, 14, 14});
    if (key == "embeddings.position_embedding.weight") return set({VIT_TOKENS, D});
    if (key == "embeddings.class_embedding" || key == "pre_layrnorm.weight" || key == "pre_layrnorm.bias") return set({D});
    const std::string pre = "encoder.layers.";
    if (key.compare(0, pre.size(), pre) != 0) return 0;
    size_t dot = key.find('.', pre.size());
    if (dot == std::string::npos || dot == pre.size() || dot - pre.size() > 6) return 0;
    int l = 0;
    for (size_t i = pre.size(); i < dot; ++i) { if (key[i] < '0' || key[i] > '9') return 0; l = l * 10 + (key[i] - '0'); }
    if (l >= h->cfg.layers || key.substr(pre.size(), dot - pre.size()) != std::to_string(l)) return 0;
    const std::string s = key.substr(dot + 1);
    for (const char* p : {"self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.out_proj"}) {
        if (s == std::string(p) + ".weight") return set({D, D});
        if (s == std::string(p) + ".bias") return set({D});
    }
    for (const char* p : {"layer_norm1", "layer_norm2"})
        if (s == std::string(p) + ".weight" || s == std::string(p) + ".bias") return set({D});
    if (s == "mlp.fc1.weight") return set({F, D});
    if (s == "mlp.fc1.bias") return set({F});
    if (s == "mlp.fc2.weight") return set({D, F});
    if (s == "mlp.fc2.bias") return set({D});
    return 0;
}
static std::string shape_str(const int64_t* s, int n) {    // "(4096, 1024) of 4194304 elements"; every extent is >= 1
    std::string o = "(";
    uint64_t count = 1;
    bool over = false;
    for (int i = 0; i < n; ++i) {
        o += std::to_string((long long)s[i]) + (i + 1 < n ? ", " : ")");
        if (count > UINT64_MAX / (uint64_t)s[i]) over = true; else count *= (uint64_t)s[i];
    }
    return o + (over ? " of more than 2^64 elements" : " of " + std::to_string((unsigned long long)count) + " elements");
}

extern "C" int pg_vit_load_weight(pg_vit* h, const char* name, const void* data, int dtype, const int64_t* shape, int ndim) {
    if (!h || !name || !data || !shape) { pg_set_error("vit_load_weight: null argument"); return PG_EINVAL; }
    if (dtype != PG_DTYPE_F32) { pg_set_error("vit_load_weight: only fp32 host data is accepted"); return PG_EINVAL; }
    if (h->finalized) { pg_set_error("vit_load_weight: handle already finalized"); return PG_ESTATE; }
    const std::string key = canon(name);
    if (ndim < 1 || ndim > 8) { pg_set_error("vit_load_weight: parameter %s has ndim = %d (1..8)", key.c_str(), ndim); return PG_EINVAL; }
    for (int i = 0; i < ndim; ++i)
        if (shape[i] < 1) { pg_set_error("vit_load_weight: parameter %s has extent %lld in dimension %d", key.c_str(), (long long)shape[i], i); return PG_EINVAL; }
    int64_t want[4];
    const int wn = param_shape(h, key, want);
    if (wn == 0) return PG_OK;                               // not read on this path (post_layernorm.*, layers past cfg.layers): ignored
    bool same = wn == ndim;
    for (int i = 0; same && i < wn; ++i) same = shape[i] == want[i];
    if (!same) {
        pg_set_error("vit_load_weight: parameter %s has shape %s, expected %s", key.c_str(), shape_str(shape, ndim).c_str(),
                     shape_str(want, wn).c_str());
        return PG_EINVAL;
    }
    int64_t n = 1;
    for (int i = 0; i < wn; ++i) n *= want[i];
    const float* f = (const float*)data;
    h->host[key] = std::vector<float>(f, f + n);
    return PG_OK;
}

static uint16_t host_bf16(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}
static uint16_t host_f16(float f) {                       // round to nearest even, saturating
    if (f > 65504.f) f = 65504.f;
    if (f < -65504.f) f = -65504.f;
    _Float16 h = (_Float16)f;
    uint16_t b;
    memcpy(&b, &h, 2);
    return b;
}
static uint16_t host_cvt(int dtype, float f) { return dtype == PG_DTYPE_F16 ? host_f16(f) : host_bf16(f); }
static float host_uncvt(int dtype, uint16_t b) {
    if (dtype == PG_DTYPE_F16) { _Float16 h; memcpy(&h, &b, 2); return (float)h; }
    uint32_t u = (uint32_t)b << 16; float f; memcpy(&f, &u, 4); return f;
}
// W' = cvt(gamma o W) [N][K]; colsum[n] = sum_k float(W'[n][k]) (of the ROUNDED values, so that the identity
// LN(x).W^T = rstd (x.W'^T - mean colsum) + beta.W^T holds exactly for what the MFMA multiplies); cbias = beta.W^T + b.
static void fold_ln(int dt, const float* W, const float* b, const float* gamma, const float* beta, size_t N, size_t K,
                    std::vector<uint16_t>& w16, std::vector<float>& colsum, std::vector<float>& cbias) {
    w16.resize(N * K); colsum.resize(N); cbias.resize(N);
    for (size_t n = 0; n < N; ++n) {
        double s = 0.0, c = 0.0;
        for (size_t k = 0; k < K; ++k) {
            const uint16_t q = host_cvt(dt, W[n * K + k] * gamma[k]);
            w16[n * K + k] = q;
            s += (double)host_uncvt(dt, q);
            c += (double)beta[k] * (double)W[n * K + k];
        }
        colsum[n] = (float)s;
        cbias[n] = (float)(c + (double)b[n]);
    }
}

// exact mode (precise.hip): row n of W [N][K] -> [Wh | Wh | fp16((W - Wh) * 2^8)], K zero padded to Kpad
static void pack_x3(const float* W, size_t N, size_t K, size_t Kpad, std::vector<uint16_t>& w3) {
    w3.assign(N * 3 * Kpad, 0);
    for (size_t n = 0; n < N; ++n) {
        uint16_t* r = w3.data() + n * 3 * Kpad;
        for (size_t k = 0; k < K; ++k) {
            const float w = W[n * K + k];
            const uint16_t hb = host_f16(w);
            const float hf = host_uncvt(PG_DTYPE_F16, hb);
            r[k] = hb; r[Kpad + k] = hb;
            r[2 * Kpad + k] = host_f16((w - hf) * 256.0f);
        }
    }
}

static int need(pg_vit* h, const std::string& k, size_t n, const std::vector<float>** out) {
    auto it = h->host.find(k);
    if (it == h->host.end()) { pg_set_error("vit_finalize: missing parameter %s", k.c_str()); return PG_ESTATE; }
    if (it->second.size() != n) {
        pg_set_error("vit_finalize: parameter %s has %zu elements, expected %zu", k.c_str(), it->second.size(), n);
        return PG_EINVAL;
    }
    *out = &it->second;
    return PG_OK;
}

// n elements (fp32, or 16-bit: bf16 / fp16 / split-fp16 triples) to a device buffer of their own; the handle owns it and records its size
template <class T> static int upload(pg_vit* h, const T* src, size_t n, T** dst) {
    PG_HIP(hipMalloc((void**)dst, n * sizeof(T)));
    h->allocs.push_back(*dst);
    h->alloc_bytes[*dst] = n * sizeof(T);
    PG_HIP(hipMemcpy(*dst, src, n * sizeof(T), hipMemcpyHostToDevice));
    return PG_OK;
}
static int upload(pg_vit* h, const std::vector<uint16_t>& src, uint16_t** dst) { return upload(h, src.data(), src.size(), dst); }

// One staged parameter `k` of N x K elements to the device.  float** dst: as it is; uint16_t** dst: converted to the handle's 16-bit
// operand format, or with x3 packed as the exact mode's triple [N][3K].
template <class T> static int put(pg_vit* h, const std::string& k, size_t N, size_t K, T** dst, bool x3 = false) {
    const std::vector<float>* q;
    RC(need(h, k, N * K, &q));
    if constexpr (std::is_same<T, float>::value) {
        return upload(h, q->data(), N * K, dst);
    } else {
        std::vector<uint16_t> w(x3 ? 0 : N * K);
        if (x3) pack_x3(q->data(), N, K, K, w);
        else for (size_t i = 0; i < N * K; ++i) w[i] = host_cvt(h->cfg.mma_dtype, (*q)[i]);
        return upload(h, w, dst);
    }
}

extern "C" int pg_vit_finalize(pg_vit* h) {
    if (!h) { pg_set_error("vit_finalize: null handle"); return PG_EINVAL; }
    if (h->finalized) return PG_OK;
    PG_HIP(hipSetDevice(h->device));
    const size_t D = VIT_HIDDEN, F = VIT_MLP;
    const int dt = h->cfg.mma_dtype;
    const std::vector<float>* p;
    // patch embedding [1024,3,14,14] -> 16-bit (cfg.mma_dtype) [1024][640], zero padded along K
    RC(need(h, "embeddings.patch_embedding.weight", D * VIT_PATCH_K, &p));
    {
        std::vector<uint16_t> w(D * VIT_PATCH_KPAD, 0);
        for (size_t n = 0; n < D; ++n)
            for (size_t k = 0; k < VIT_PATCH_K; ++k) w[n * VIT_PATCH_KPAD + k] = host_cvt(dt, (*p)[n * VIT_PATCH_K + k]);
        RC(upload(h, w, &h->wpatch));
        if (h->cfg.precise) { std::vector<uint16_t> w3; pack_x3(p->data(), D, VIT_PATCH_K, VIT_PATCH_KPAD, w3); RC(upload(h, w3, &h->wpatch3)); }
    }
    RC(put(h, "embeddings.class_embedding", 1, D, &h->cls));
    RC(put(h, "embeddings.position_embedding.weight", VIT_TOKENS, D, &h->pos));
    RC(put(h, "pre_layrnorm.weight", 1, D, &h->preg));
    RC(put(h, "pre_layrnorm.bias", 1, D, &h->preb));
    {   // the table 8-bit pixels (PG_DTYPE_U8) are looked up in: not a parameter, not in the fingerprint
        float lut[PG_NORM_LUT_SIZE];
        pg_norm_lut_fill(lut);
        RC(upload(h, lut, (size_t)PG_NORM_LUT_SIZE, &h->norm_lut));
    }
    for (int l = 0; l < h->cfg.layers; ++l) {
        LayerW& L = h->layers[l];
        const std::string pre = "encoder.layers." + std::to_string(l) + ".";
        const std::vector<float>*wq, *wk, *wv, *bq, *bk, *bv;
        RC(need(h, pre + "self_attn.q_proj.weight", D * D, &wq)); RC(need(h, pre + "self_attn.k_proj.weight", D * D, &wk));
        RC(need(h, pre + "self_attn.v_proj.weight", D * D, &wv)); RC(need(h, pre + "self_attn.q_proj.bias", D, &bq));
        RC(need(h, pre + "self_attn.k_proj.bias", D, &bk));       RC(need(h, pre + "self_attn.v_proj.bias", D, &bv));
        const std::vector<float>*g1, *be1, *g2, *be2;
        RC(need(h, pre + "layer_norm1.weight", D, &g1)); RC(need(h, pre + "layer_norm1.bias", D, &be1));
        RC(need(h, pre + "layer_norm2.weight", D, &g2)); RC(need(h, pre + "layer_norm2.bias", D, &be2));
        {
            std::vector<float> wf(3 * D * D), b(3 * D);
            for (size_t i = 0; i < D * D; ++i) { wf[i] = (*wq)[i]; wf[D * D + i] = (*wk)[i]; wf[2 * D * D + i] = (*wv)[i]; }
            for (size_t i = 0; i < D; ++i) { b[i] = (*bq)[i]; b[D + i] = (*bk)[i]; b[2 * D + i] = (*bv)[i]; }
            if (h->cfg.precise) {
                std::vector<uint16_t> w3; pack_x3(wf.data(), 3 * D, D, D, w3);
                RC(upload(h, w3, &L.wqkv3)); RC(upload(h, b.data(), 3 * D, &L.bqkv_raw));
            }
            if (h->ln_fold) {
                std::vector<uint16_t> w; std::vector<float> cs, cb;
                fold_ln(dt, wf.data(), b.data(), g1->data(), be1->data(), 3 * D, D, w, cs, cb);
                RC(upload(h, w, &L.wqkv)); RC(upload(h, cb.data(), 3 * D, &L.bqkv)); RC(upload(h, cs.data(), 3 * D, &L.sqkv));
            } else {
                std::vector<uint16_t> w(3 * D * D);
                for (size_t i = 0; i < 3 * D * D; ++i) w[i] = host_cvt(dt, wf[i]);
                RC(upload(h, w, &L.wqkv)); RC(upload(h, b.data(), 3 * D, &L.bqkv));
            }
        }
        RC(put(h, pre + "self_attn.out_proj.weight", D, D, &L.wo)); RC(put(h, pre + "self_attn.out_proj.bias", 1, D, &L.bo));
        if (h->ln_fold) {
            const std::vector<float>*w1f, *b1f;
            RC(need(h, pre + "mlp.fc1.weight", F * D, &w1f)); RC(need(h, pre + "mlp.fc1.bias", F, &b1f));
            std::vector<uint16_t> w; std::vector<float> cs, cb;
            fold_ln(dt, w1f->data(), b1f->data(), g2->data(), be2->data(), F, D, w, cs, cb);
            RC(upload(h, w, &L.w1)); RC(upload(h, cb.data(), F, &L.b1)); RC(upload(h, cs.data(), F, &L.s1));
        } else {
            RC(put(h, pre + "mlp.fc1.weight", F, D, &L.w1));        RC(put(h, pre + "mlp.fc1.bias", 1, F, &L.b1));
        }
        RC(put(h, pre + "mlp.fc2.weight", D, F, &L.w2));            RC(put(h, pre + "mlp.fc2.bias", 1, D, &L.b2));
        if (h->cfg.precise) {
            RC(put(h, pre + "self_attn.out_proj.weight", D, D, &L.wo3, true)); RC(put(h, pre + "mlp.fc1.weight", F, D, &L.w13, true));
            RC(put(h, pre + "mlp.fc2.weight", D, F, &L.w23, true));            RC(put(h, pre + "mlp.fc1.bias", 1, F, &L.b1_raw));
        }
        RC(put(h, pre + "layer_norm1.weight", 1, D, &L.ln1g));      RC(put(h, pre + "layer_norm1.bias", 1, D, &L.ln1b));
        RC(put(h, pre + "layer_norm2.weight", 1, D, &L.ln2g));      RC(put(h, pre + "layer_norm2.bias", 1, D, &L.ln2b));
    }
    h->host.clear();
    h->finalized = true;
    return PG_OK;
}

extern "C" int pg_vit_destroy(pg_vit* h) {
    if (!h) return PG_OK;
    for (void* p : h->allocs) (void)hipFree(p);
    for (int i = 0; i < 3; ++i) { if (h->sx[i]) (void)hipStreamDestroy(h->sx[i]); if (h->ev_join[i]) (void)hipEventDestroy(h->ev_join[i]); }
    if (h->ev_fork) (void)hipEventDestroy(h->ev_fork);
    for (auto& e : h->evs) { (void)hipEventDestroy(e.a); (void)hipEventDestroy(e.b); }
    for (auto& g : h->graphs) vit_graph_entry_free(g);
    if (h->capture_stream) (void)hipStreamDestroy(h->capture_stream);
    delete h;
    return PG_OK;
}
extern "C" int pg_vit_mma_dtype(const pg_vit* h) { return h ? h->cfg.mma_dtype : PG_EINVAL; }

// ------------------------------------------------------------------------------------------------ weight fingerprint
// pg_vit_fingerprint: 128 bits that identify what the FAST encoder computes with -- the key of a stored calibration
// (pigeon_amd/certainty.py).  The order is fixed and part of the definition:
//   buffers (each: pg_fingerprint of the whole device buffer, seed = (group << 8) | slot, group 0 = the embeddings, group l + 1 =
//   encoder layer l):
//     group 0:      0 patch weight (16-bit, [1024][640])  1 class embedding  2 position embedding  3 pre_layrnorm weight  4 its bias
//     group l + 1:  0 QKV weight (16-bit; gamma-folded with ln_fold)  1 QKV bias (with ln_fold: beta.W^T + b)  2 QKV column sums
//                   (ln_fold only)  3 out_proj weight  4 its bias  5 fc1 weight (as QKV)  6 fc1 bias  7 fc1 column sums (ln_fold
//                   only)  8 fc2 weight  9 its bias  10..13 layer_norm1 weight, bias, layer_norm2 weight, bias
//   table of 64-bit words: ['PGVITFP1', layers, mma_dtype, ln_fold, buffers, then per buffer: seed, bytes, digest[0], digest[1]]
//   result: the digest (same function, seed 0) of that table's bytes.
// The exact tier's split-weight copies and raw biases (cfg.precise) are NOT in it: they are a function of the same fp32 weights, and
// a handle built without `precise` gives the same value.

// The parameter buffer (group, slot) of a finalized handle in the numbering above -- ONE table for the fingerprint and for
// pg_vit_param_read; nullptr where this handle has none.  The buffers the fingerprint leaves out continue the numbering: group 0:
// 5 the patch triple, 6 the normalisation table; group l + 1: 14..19 the QKV, out_proj, fc1, fc2 triples, the raw QKV and fc1 biases.
enum { VIT_FP_EMBED_SLOTS = 5, VIT_EMBED_SLOTS = 7, VIT_FP_LAYER_SLOTS = 14, VIT_LAYER_SLOTS = 20 };
static const void* vit_param(const pg_vit* h, int group, int slot, bool* known) {
    if (known) *known = false;
    if (group < 0 || group > h->cfg.layers || slot < 0 || slot >= (group ? VIT_LAYER_SLOTS : VIT_EMBED_SLOTS)) return nullptr;
    if (known) *known = true;
    if (group == 0) {
        const void* p[VIT_EMBED_SLOTS] = {h->wpatch, h->cls, h->pos, h->preg, h->preb, h->wpatch3, h->norm_lut};
        return p[slot];
    }
    const LayerW& L = h->layers[group - 1];
    const void* p[VIT_LAYER_SLOTS] = {L.wqkv, L.bqkv, L.sqkv, L.wo, L.bo, L.w1, L.b1, L.s1, L.w2, L.b2, L.ln1g, L.ln1b, L.ln2g, L.ln2b,
                                      L.wqkv3, L.wo3, L.w13, L.w23, L.bqkv_raw, L.b1_raw};
    return p[slot];
}

extern "C" int pg_vit_fingerprint(const pg_vit* h, uint64_t out[2]) {
    if (!h || !out) { pg_set_error("vit_fingerprint: null argument"); return PG_EINVAL; }
    if (!h->finalized) { pg_set_error("vit_fingerprint: handle not finalized"); return PG_ESTATE; }
    std::vector<PgFpBuf> bufs;
    int missing = 0;
    auto add = [&](const void* p, int group, int slot) {
        if (!p) return;                                        // (the column sums without ln_fold)
        auto it = h->alloc_bytes.find(p);
        if (it == h->alloc_bytes.end()) { ++missing; return; }
        bufs.push_back({p, it->second, ((uint64_t)group << 8) | (uint64_t)slot});
    };
    for (int g = 0; g <= h->cfg.layers; ++g)
        for (int s = 0; s < (g ? VIT_FP_LAYER_SLOTS : VIT_FP_EMBED_SLOTS); ++s) add(vit_param(h, g, s, nullptr), g, s);
    if (missing) { pg_set_error("vit_fingerprint: %d parameter buffers without a recorded size", missing); return PG_ESTATE; }
    int cur = 0;
    PG_HIP(hipGetDevice(&cur));
    PG_HIP(hipSetDevice(h->device));                         // the weights live on the handle's device, whatever is current
    std::vector<uint64_t> dig(bufs.size() * 2);
    const int rc = pg_fingerprint_many(bufs.data(), (int)bufs.size(), dig.data(), nullptr);
    (void)hipSetDevice(cur);
    if (rc != PG_OK) return rc;
    std::vector<uint64_t> table = {0x3150465449564750ull /* 'PGVITFP1' */, (uint64_t)h->cfg.layers, (uint64_t)h->cfg.mma_dtype,
                                   (uint64_t)(h->ln_fold ? 1 : 0), (uint64_t)bufs.size()};
    for (size_t i = 0; i < bufs.size(); ++i) {
        table.push_back(bufs[i].seed); table.push_back((uint64_t)bufs[i].bytes);
        table.push_back(dig[2 * i]); table.push_back(dig[2 * i + 1]);
    }
    pg_fingerprint_host(table.data(), table.size() * sizeof(uint64_t), 0, out);
    return PG_OK;
}

extern "C" int pg_vit_param_read(const pg_vit* h, int group, int slot, void* host_dst, size_t dst_bytes, size_t* bytes) {
    if (!h || !bytes) { pg_set_error("vit_param_read: null argument"); return PG_EINVAL; }
    *bytes = 0;
    if (!h->finalized) { pg_set_error("vit_param_read: handle not finalized"); return PG_ESTATE; }
    bool known = false;
    const void* p = vit_param(h, group, slot, &known);
    if (!known) { pg_set_error("vit_param_read: no buffer (group %d, slot %d) on a handle of %d layers", group, slot, h->cfg.layers); return PG_EINVAL; }
    if (!p) return PG_OK;                                      // (the column sums without ln_fold, the exact tier's slots without cfg.precise)
    auto it = h->alloc_bytes.find(p);
    if (it == h->alloc_bytes.end()) { pg_set_error("vit_param_read: buffer (group %d, slot %d) without a recorded size", group, slot); return PG_ESTATE; }
    *bytes = it->second;
    if (!host_dst) return PG_OK;                               // size query
    if (dst_bytes < it->second) {
        pg_set_error("vit_param_read: destination of %zu bytes, buffer (group %d, slot %d) has %zu", dst_bytes, group, slot, it->second);
        return PG_EINVAL;
    }
    int cur = 0; PG_HIP(hipGetDevice(&cur));
    PG_HIP(hipSetDevice(h->device));                         // the weights live on the handle's device, whatever is current
    const hipError_t e = hipMemcpy(host_dst, p, it->second, hipMemcpyDeviceToHost);
    (void)hipSetDevice(cur);                                 // ... and the caller's current device is put back
    if (e != hipSuccess) { pg_set_error("vit_param_read: %s", hipGetErrorString(e)); return PG_EHIP; }
    return PG_OK;
}
