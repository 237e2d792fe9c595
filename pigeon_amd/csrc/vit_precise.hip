// vit_precise.hip -- the orchestration of the encoder's EXACT mode over a pg_vit handle (vit_handle.h); its kernels: precise.hip.
// pg_vit_forward_precise: the same encoder in near-fp32 arithmetic (precise.hip: split-fp16 GEMM operands on the persistent MFMA
// kernels, fp32 LayerNorm / attention / QuickGELU / residual), for the panoramas whose top-1 margin the 16-bit path cannot decide.
// Workspace per token row: X fp32 4 KB | T3 triple of a 1024-wide row 6 KB | F fp32 QKV (12 KB) / fc1 (16 KB) | G3 triple of the
// 4096-wide activation 24 KB (the im2col triple and the fp32 attention output live there too) | (round 5) PP, the K-split partial
// products of one GEMM, 48 KB (fc1: 3 x 4096 fp32) = 98 KB; equal chunks of <= 128 images.
//
// Round 5: a GEMM of the layer loop whose tiles would not fill the chip is cut along K' into S parts (the products hi.Wh | lo.Wh |
// hi.Wl, or halves of them) that run as ONE persistent launch over S x tilesM x tilesN tiles (PgGemmExtra::parts) into fp32 partial
// buffers, which sum_parts_kernel then adds in a fixed order.  The exact tier runs on the handful of panoramas a step finds
// uncertain -- 4 to 16 images, 10 to 40 row panels: a K' = 12288 launch then puts 40 tiles of 192 K tiles each on 256 CUs (326 us per
// layer for fc2 alone: latency, not work); 240 tiles of 32 K tiles fill the chip instead.  S is chosen per shape by a small cost
// model (gemm_plan.hip precise_parts).  (First tried as S concurrent launches on side streams: the launches did not overlap -- 4 images 15.9
// against 14.3 ms, 52 images 112 against 76 ms, gpurun_out/r05/exact_small_batches_ksplit.txt -- hence the in-kernel form.)
#include "vit_handle.h"
#include <cstdlib>

#define PG_PRECISE_CHUNK 128   // images per internal pass (98 KB of workspace per token row: 7.2 GB at 128); a longer batch is cut into EQUAL chunks
// pg_tune_exact_products (round 6): how many of the three partial products hi.Wh | lo.Wh | hi.Wl the exact mode's weight GEMMs run.
// 3 = all (the exact tier).  2 = the first two: the activations keep both halves, the weights only their fp16 value -- K' = 2K on the
// SAME triple operands (the third K-third of A' / W' is simply not visited).  What is left is the weights' rounding, identical for
// every token of every image: a systematic embedding error that a calibration can measure (pigeon_amd/certainty.py), at 2/3 of the
// exact tier's GEMM work.  The attention (activation x activation) keeps its three products.
static int g_exact_products = 3;
extern "C" int pg_tune_exact_products(int n) {
    if (n != 2 && n != 3) { pg_set_error("pg_tune_exact_products: 2 or 3"); return PG_EINVAL; }
    g_exact_products = n;
    return PG_OK;
}
static size_t precise_ws_bytes_for(int chunk) { return precise_ws((size_t)chunk * VIT_TOKENS).total; }
extern "C" int pg_vit_precise_workspace_bytes(const pg_vit* h, int n_images, size_t* bytes) {
    if (!h || !bytes || n_images < 0) { pg_set_error("vit_precise_workspace_bytes: bad argument"); return PG_EINVAL; }
    const int chunk = n_images < PG_PRECISE_CHUNK ? n_images : PG_PRECISE_CHUNK;
    *bytes = precise_ws_bytes_for(chunk > 0 ? chunk : 1);
    return PG_OK;
}

// One GEMM of the exact mode.  S = 1: the plain launch (EPI_F32 into dst / EPI_RESID onto dst).  S > 1: cut along K' into S parts
// that run as ONE persistent launch (PgGemmExtra::parts: S x tilesM x tilesN tiles on the 256 CUs): part p multiplies columns
// [p Kp, (p + 1) Kp) of the triple operands into the fp32 partial buffer p (the bias rides in part 0); then
// dst = (resid ? dst : 0) + sum of the parts, in part order (sum_parts_kernel).
// Which of the three forms a shape takes (S): precise_plan below, 0 = gemm_mid.hip, S >= 1 = the persistent kernel in S parts.
static int precise_gemm(const uint16_t* A3, int64_t lda, const uint16_t* W3, int64_t ldw, const float* bias, float* parts,
                        float* dst, bool resid, int M, int N, int Ktot, int S, hipStream_t s) {
    if (S <= 1)
        return pg_gemm_launch(PG_DTYPE_F16, A3, lda, W3, ldw, bias, dst, N, M, N, Ktot, resid ? EPI_RESID : EPI_F32, 1.f, 0, nullptr,
                              S == 0 ? PG_GEMM_V_MID : PG_GEMM_V_PP, s);
    const int Kp = Ktot / S;
    const int64_t part_elems = (int64_t)M * N;
    PgGemmExtra ex; ex.parts = S; ex.a_part = Kp; ex.w_part = Kp; ex.c_part = part_elems;
    RC(pg_gemm_launch(PG_DTYPE_F16, A3, lda, W3, ldw, bias, parts, N, M, N, Kp, EPI_F32, 1.f, 0, nullptr, PG_GEMM_V_PP, s, &ex));
    return pg_sum_parts_launch(parts, S, part_elems, dst, part_elems, resid ? 1 : 0, s);
}

// pg_tune_exact_fusion (round 6): the exact pass's two activation splits ride in their producers -- the attention
// writes the triple the out-projection reads (attention_x3_kernel<true>), fc1's epilogue applies QuickGELU and writes the triple fc2
// reads (EPI_GELU_X3, where fc1 runs as one persistent launch: S = 1) -- instead of an fp32 buffer plus a split_x3 launch each.  The
// arithmetic per element is the same expression in both forms (x3.h): results are bit-identical (tests/test_gpu_precise.py).  0 = the
// unfused form (the A/B arm and the checker).
static int g_exact_fusion = -1;
extern "C" int pg_tune_exact_fusion(int on) {
    g_exact_fusion = on ? 1 : 0;
    return PG_OK;
}
static bool exact_fusion_on() {
    if (g_exact_fusion < 0) { const char* e = getenv("PIGEON_EXACT_FUSION"); g_exact_fusion = (e && e[0] == '0') ? 0 : 1; }
    return g_exact_fusion != 0;
}

// The form of one internal pass of n images under the current knobs: the route of each of the layer's four weight GEMMs
// (pg_gemm_precise_route: 0 = gemm_mid.hip, 1 = one persistent launch, S > 1 = S K-parts + sum_parts_kernel) and which of the two
// activation splits ride in their producers.  Host arithmetic only.  The ONE place that decides it: vit_precise_chunk runs what this
// returns, pg_vit_precise_plan exports it to the tests.
struct PrecisePlan { int qkv, out, fc1, fc2; bool fuse_fc1, attn_x3; };
static PrecisePlan precise_plan(int n) {
    const int M = n * VIT_TOKENS, D = VIT_HIDDEN, F = VIT_MLP;
    static const int S3[2] = {1, 3}, S6[4] = {1, 2, 3, 6};    // K-part counts precise_parts may choose from (K' = 3072 / 12288)
    static const int S2[2] = {1, 2}, S4[3] = {1, 2, 4};       // ... with two products (K' = 2048 / 8192)
    const int np = g_exact_products;                          // partial products per weight GEMM (3; 2: pg_tune_exact_products)
    const int* c1 = np == 3 ? S3 : S2; const int* c2 = np == 3 ? S6 : S4; const int n2 = np == 3 ? 4 : 3;
    const bool fuse = exact_fusion_on();
    PrecisePlan p;
    p.qkv = pg_gemm_precise_route(M, 3 * D, np * D, false, c1, 2);
    p.out = pg_gemm_precise_route(M, D, np * D, true, c1, 2);
    p.fc1 = pg_gemm_precise_route(M, F, np * D, false, c1, 2);
    p.fc2 = pg_gemm_precise_route(M, D, np * F, true, c2, n2);
    p.fuse_fc1 = fuse && p.fc1 == 1;                          // one persistent launch: the epilogue can finish the job
    p.attn_x3 = fuse && pg_attention_x3out_available();
    return p;
}
// A batch above PG_PRECISE_CHUNK runs as `count` internal passes of sizes equal to within one image (130 images: 65 + 65, not
// 128 + 2 -- a two-image pass costs as much as a sixteen-image one): the first n - count (big - 1) passes take `big` images, the others big - 1.
static void precise_chunks(int n_images, int* big, int* count) {
    *count = (n_images + PG_PRECISE_CHUNK - 1) / PG_PRECISE_CHUNK;
    if (*count < 1) *count = 1;
    *big = (n_images + *count - 1) / *count;
}
extern "C" int pg_vit_precise_plan(int n_images, int32_t out[8]) {
    if (n_images < 1 || n_images > (1 << 20) || !out) { pg_set_error("vit_precise_plan: bad argument"); return PG_EINVAL; }
    int big = 0, count = 0;
    precise_chunks(n_images, &big, &count);
    const PrecisePlan p = precise_plan(big);
    out[0] = p.qkv; out[1] = p.out; out[2] = p.fc1; out[3] = p.fc2;
    out[4] = p.fuse_fc1 ? 1 : 0; out[5] = p.attn_x3 ? 1 : 0; out[6] = big; out[7] = count;
    return PG_OK;
}

static int vit_precise_chunk(pg_vit* h, const void* pixels, int pix_dtype, int n, float* emb_out, float* hidden_out, char* ws, hipStream_t s) {
    const int64_t M = (int64_t)n * VIT_TOKENS;
    const int D = VIT_HIDDEN, F = VIT_MLP;
    const PreciseWs w = precise_ws((size_t)M);
    float *X = (float*)(ws + w.X), *Fb = (float*)(ws + w.F);
    uint16_t *T3 = (uint16_t*)(ws + w.T3), *G3 = (uint16_t*)(ws + w.G3);
    float* O = (float*)G3;                                    // fp32 attention output, dead before G3 is written
    float* PP = (float*)(ws + w.PP);                          // K-split partial products of one GEMM
    const float eps = h->cfg.ln_eps;
    const int dt = PG_DTYPE_F16, V = PG_GEMM_V_PP;            // the 256 x 256 persistent kernel takes every epilogue used here
    const int np = g_exact_products;                          // partial products per weight GEMM (3; 2: pg_tune_exact_products)
    const PrecisePlan plan = precise_plan(n);
    // One weight GEMM of a layer in the plan's form S: dst [M][N] (resid: +)= A3 [M][3K] . W3 [N][3K]^T + bias over np K-thirds
    auto gemm = [&](const uint16_t* A3, const uint16_t* W3, const float* bias, float* dst, bool resid, int N, int K, int S) -> int {
        return precise_gemm(A3, 3 * K, W3, 3 * K, bias, PP, dst, resid, (int)M, N, np * K, S, s);
    };
    RC(pg_x3_im2col_launch(pixels, pix_dtype, G3, n, s, h->norm_lut));
    RC(pg_gemm_launch(dt, G3, 3 * VIT_PATCH_KPAD, h->wpatch3, 3 * VIT_PATCH_KPAD, nullptr, X, D, n * VIT_PATCHES, D, np * VIT_PATCH_KPAD,
                      EPI_PATCH, 1.f, 0, h->pos, V, s));
    RC(pg_preln_launch(X, h->cls, h->pos, h->preg, h->preb, M, eps, s));
    for (int l = 0; l < h->cfg.layers; ++l) {
        const LayerW& L = h->layers[l];
        RC(pg_x3_ln_launch(X, L.ln1g, L.ln1b, T3, M, eps, s));
        RC(gemm(T3, L.wqkv3, L.bqkv_raw, Fb, false, 3 * D, D, plan.qkv));
        if (plan.attn_x3) {
            RC(pg_attention_x3out_launch(Fb, T3, n, s));         // (T3's LayerNorm triple is dead: the QKV GEMM has consumed it)
        } else {
            RC(pg_attention_f32_launch(Fb, O, n, s));
            RC(pg_x3_split_launch(O, T3, M, D, 0, s));
        }
        RC(gemm(T3, L.wo3, L.bo, X, true, D, D, plan.out));
        RC(pg_x3_ln_launch(X, L.ln2g, L.ln2b, T3, M, eps, s));
        if (plan.fuse_fc1) {
            RC(pg_gemm_launch(dt, T3, 3 * D, L.w13, 3 * D, L.b1_raw, G3, 3 * F, (int)M, F, np * D, EPI_GELU_X3, 1.f, 0, nullptr, V, s));
        } else {
            RC(gemm(T3, L.w13, L.b1_raw, Fb, false, F, D, plan.fc1));
            RC(pg_x3_split_launch(Fb, G3, M, F, 1, s));
        }
        RC(gemm(G3, L.w23, L.b2, X, true, D, F, plan.fc2));
    }
    RC(pg_token_mean_launch(X, emb_out, n, s));
    if (hidden_out) PG_HIP(hipMemcpyAsync(hidden_out, X, (size_t)M * D * 4, hipMemcpyDeviceToDevice, s));
    return PG_OK;
}

extern "C" int pg_vit_forward_precise(pg_vit* h, const void* pixels, int pix_dtype, int n_images, float* emb_out, float* hidden_out,
                                      void* workspace, size_t workspace_bytes, void* stream) {
    size_t needb = 0;
    if (h && n_images > 0) pg_vit_precise_workspace_bytes(h, n_images, &needb);
    RC(vit_forward_check("vit_forward_precise", h, true, pixels, pix_dtype, n_images, emb_out, workspace, workspace_bytes, needb));
    if (n_images == 0) return PG_OK;
    int big = 0, nchunks = 0;
    precise_chunks(n_images, &big, &nchunks);
    for (int c = 0, s0 = 0; c < nchunks; ++c) {
        const int n = big - (c < n_images - nchunks * (big - 1) ? 0 : 1);
        const ChunkIO io = chunk_io(pixels, pix_dtype, emb_out, hidden_out, s0);
        RC(vit_precise_chunk(h, io.pixels, pix_dtype, n, io.emb, io.hidden, (char*)workspace, (hipStream_t)stream));
        s0 += n;
    }
    return PG_OK;
}
