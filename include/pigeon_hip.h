/* pigeon_hip.h -- C ABI of libpigeon_hip.so: the MI355X (gfx950) kernels behind PIGEON's inference hot path.
 *
 * The reference (LukasHaas/PIGEON) is 100% Python and has NO native boundary of its own:
 * every GPU FLOP is issued by stock PyTorch ops reached through HuggingFace transformers.  The drop-in
 * boundary is therefore the Python class surface (CLIPEmbedding / SuperGuessr / ProtoRefiner, mirrored in
 * pigeon_amd/), and THIS header is the FFI those mirrors bind with ctypes -- exactly what a maintainer of
 * the reference would bind to replace the library kernels it reaches today.  Each entry point cites the
 * reference call site(s) whose arithmetic it replaces.
 *
 * Conventions
 *   - plain C types only; every pointer documented as DEVICE (HBM, on the handle's device) or HOST;
 *   - every function returns 0 on success or a negative PG_E* code; pg_last_error() gives a message;
 *   - `stream` is a hipStream_t passed as void* (0 = default stream); all work is asynchronous on it, the
 *     library never synchronises the device inside a forward call;
 *   - the caller owns all inputs, outputs and workspaces (torch tensors in the Python host); the library
 *     owns only the packed weight copies held inside a pg_vit handle;
 *   - handles are not thread-safe: one per (device, stream).
 */
#ifndef PIGEON_HIP_H
#define PIGEON_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PG_OK            0
#define PG_EINVAL       -1   /* bad argument / unsupported shape */
#define PG_ENOMEM       -2   /* device allocation failed / workspace too small */
#define PG_EHIP         -3   /* a HIP runtime call failed (see pg_last_error) */
#define PG_ESTATE       -4   /* handle not finalized / weight missing */

#define PG_DTYPE_F32     0
#define PG_DTYPE_BF16    1
#define PG_DTYPE_F16     2
#define PG_DTYPE_F64     3
#define PG_DTYPE_U8      4   /* 8-bit pixels: the byte the resize computes, before the normalisation table (pg_prep_norm_lut) */

#define PG_ABI_VERSION   7   /* 2: pg_vit_cfg.precise, pg_vit_forward_precise, pg_head_margin (round 4); 3: pg_head_certainty, pg_refine_forward_ex,
                              * pg_refine_certainty, pg_tune_gemm_raster (round 5); 4: the deferred exact tier -- pg_requeue_append,
                              * pg_rows_to_slots, pg_requeue_take, pg_scatter_rows, pg_head_wstats (round 6); 5: pg_embedding_debias (round 6);
                              * 6: pg_gemm_plan replaces pg_gemm_route;
                              * 7: pg_vit_precise_plan, pg_op_x3_im2col, pg_op_sum_parts, pg_op_preln, pg_op_attention_x3;
                              * 7 (+ pg_aux_heads_forward, additive; + pg_fingerprint, pg_vit_fingerprint, additive;
                              *    + pg_prep_ragged_plan / _create / _destroy / _forward and pg_prep_item, additive;
                              *    + pg_haversine_blocks, pg_optics_graph, pg_optics_plan, pg_tune_optics_lds_points, additive;
                              *    + pg_region_locate, pg_region_classify, pg_region_nearest, pg_region_plan, pg_tune_region_wave_edges, additive;
                              *    + PG_DTYPE_U8 pixels and pg_prep_norm_lut, additive; + pg_vit_param_read, additive;
                              *    + pg_refine_certainty_bank, additive;
                              *    + pg_jpeg_probe, pg_jpeg_reason, pg_jpeg_plan, pg_jpeg_entropy_decode, pg_jpeg_forward, pg_jpeg_info and
                              *      pg_jpeg_item, additive;
                              *    + pg_token_attribution, additive;
                              *    + pg_equirect_plan, pg_equirect_forward, pg_eq_view and pg_eq_item, additive;
                              *    + pg_guess_spread, pg_guess_spread_plan, additive;
                              *    + pg_head_train_loss, pg_head_train_update, pg_head_train_plan, additive;
                              *    + pg_score_table, pg_guess_best, pg_guess_best_plan, additive;
                              *    + pg_knn_prepare, pg_knn_workspace_bytes, pg_knn_search, pg_knn_plan, pg_tune_knn_spans and pg_knn_bank,
                              *      additive;
                              *    + pg_temper_stats, pg_temper_logits, pg_temper_plan, additive;
                              *    + pg_bootstrap_indices, pg_bootstrap_means, pg_bootstrap_quantiles, pg_bootstrap_plan, additive;
                              *    + pg_refine_sweep, pg_refine_sweep_totals, pg_refine_sweep_plan, additive) */

const char* pg_last_error(void);
int pg_abi_version(void);
/* Number of HIP devices visible; <0 on error.  Lets the host fail loudly when there is no GPU. */
int pg_device_count(void);

/* ------------------------------------------------------------------------------------------------
 * ViT-L/14-336 image encoder.
 * Replaces: transformers CLIPVisionModel.forward as called at reference models/clip_embedder.py:63 and
 * models/super_guessr.py:395, plus the token mean at models/clip_embedder.py:64-65 /
 * models/super_guessr.py:397-398 (embedding = mean over ALL 577 tokens of last_hidden_state, taken
 * before post_layernorm).
 * ------------------------------------------------------------------------------------------------ */
typedef struct pg_vit pg_vit;

typedef struct pg_vit_cfg {
    int32_t layers;       /* 24 for ViT-L; any >=1 accepted (tests use 2) */
    int32_t image_size;   /* must be 336 */
    int32_t patch;        /* must be 14  */
    int32_t hidden;       /* must be 1024 */
    int32_t heads;        /* must be 16  */
    int32_t mlp;          /* must be 4096 */
    float   ln_eps;       /* 1e-5 */
    int32_t max_chunk;    /* images processed per internal pass (0 = default 512) */
    int32_t mma_dtype;    /* 16-bit MFMA operand format for weights and activations: PG_DTYPE_F16, PG_DTYPE_BF16, or
                             0 = default (fp16, unless env PIGEON_MMA_DTYPE=bf16).  Same MFMA rate on gfx950; fp16
                             keeps embeddings within 1e-3 of the fp32 reference, bf16 measures 2e-3. */
    int32_t precise;      /* != 0: pg_vit_finalize also packs the split-fp16 weight copy pg_vit_forward_precise needs (3x the
                             16-bit weight memory: 1.8 GB for ViT-L); 0: the exact mode is not available on this handle */
} pg_vit_cfg;

int pg_vit_create(pg_vit** out, int device, const pg_vit_cfg* cfg);
/* Copy one parameter into the handle.  `name` is the state-dict key of transformers' CLIPVisionModel, either
 * layout: 4.23.1 "vision_model.embeddings.patch_embedding.weight" or 5.x "embeddings.patch_embedding.weight"
 * (reference loads by name: models/utils.py:24-45, models/super_guessr.py:222-238).  `data` is a HOST pointer
 * to contiguous fp32 (PG_DTYPE_F32), anything else is PG_EINVAL; pg_vit_finalize converts GEMM weights to the handle's 16-bit operand
 * format (cfg.mma_dtype: fp16, saturating, or bf16; round to nearest even) and keeps its own device copy.  `shape` / `ndim` must be the
 * parameter's transformers shape -- (1024,3,14,14) patch weight, (577,1024) position embedding, (4096,1024) fc1, (1024,4096) fc2,
 * (1024,1024) projections, (N) vectors: a known name with any other shape (a transposed fc1, say, which has the right element count)
 * is PG_EINVAL with a message naming both shapes.  ndim outside 1..8 or an extent < 1 is PG_EINVAL before `data` is read.  A name
 * loaded twice keeps the last value.  Names this path does not read (post_layernorm.*, position_ids, layers past cfg.layers) are
 * accepted and ignored.  PG_ESTATE after pg_vit_finalize. */
int pg_vit_load_weight(pg_vit* h, const char* name, const void* data, int dtype,
                       const int64_t* shape, int ndim);
/* Checks that every required parameter was loaded and uploads fused/packed forms, and the handle's 3 KB device copy of the
 * normalisation table (pg_prep_norm_lut) that PG_DTYPE_U8 pixels are looked up in. */
int pg_vit_finalize(pg_vit* h);
/* Bytes of DEVICE workspace pg_vit_forward needs for n_images (caller allocates, e.g. a torch uint8 tensor). */
int pg_vit_workspace_bytes(const pg_vit* h, int n_images, size_t* bytes);
/* pixels: DEVICE (n_images,3,336,336) contiguous NCHW, fp32 (PG_DTYPE_F32), fp16 (what pg_prep_forward writes), bf16, or the
 * bytes pg_prep_forward writes with PG_DTYPE_U8: the im2col looks each byte up in the handle's copy of pg_prep_norm_lut, so the pass
 * computes from bytes b exactly what it computes from the fp32 pixels table[c][b], bit for bit (an image is 338 688 bytes: every
 * image of a 16-byte aligned batch is 16-byte aligned).  Any other code is PG_EINVAL "bad pixel dtype".
 * emb_out: DEVICE (n_images,1024) fp32 -- mean over the 577 tokens of last_hidden_state.
 * n_images = 0 is a no-op (PG_OK; the buffers of an empty batch may be NULL), n_images < 0 is PG_EINVAL -- the same holds for
 * pg_prep_forward, pg_head_forward (B) and pg_refine_forward (B). */
int pg_vit_forward(pg_vit* h, const void* pixels, int pix_dtype, int n_images, float* emb_out,
                   void* workspace, size_t workspace_bytes, void* stream);
/* Same, additionally copying the final residual stream (n_images,577,1024) fp32 to `hidden_out` (DEVICE,
 * may be NULL).  Used by parity tests to compare last_hidden_state itself. */
int pg_vit_forward_hidden(pg_vit* h, const void* pixels, int pix_dtype, int n_images, float* emb_out,
                          float* hidden_out, void* workspace, size_t workspace_bytes, void* stream);
/* EXACT MODE (round 4).  The same encoder in near-fp32 arithmetic, for the few inputs whose downstream decision the 16-bit
 * operands cannot settle -- the reference's geocell `torch.argmax` (models/super_guessr.py:454) is fp32 end to end, and a panorama
 * whose top-1 / top-2 logit margin lies inside the fast path's error band (pg_head_margin below) may flip.  Every GEMM operand is
 * split into two fp16 halves (x = hi + lo, W = Wh + Wl) and the products hi.Wh + lo.Wh + hi.Wl are accumulated in fp32 by the same
 * persistent MFMA kernels over a 3x longer K; LayerNorm, attention (fp32 MFMA), QuickGELU (expf, IEEE division) and the residual
 * stream are fp32.  Measured against the fp32 reference: embeddings to ~1e-6 relative (fast path: 2.7e-4), at ~5x the time per
 * image.  Needs cfg.precise at creation.  Workspace from pg_vit_precise_workspace_bytes (98 KB per token row, equal chunks of at most 128 images).
 * hidden_out (DEVICE (n_images,577,1024) fp32, may be NULL) receives last_hidden_state.  pixels / pix_dtype as pg_vit_forward: from
 * PG_DTYPE_U8 bytes both tiers start from the identical fp32 value. */
int pg_vit_precise_workspace_bytes(const pg_vit* h, int n_images, size_t* bytes);
/* What pg_vit_forward_precise does with a batch of n_images (>= 1) under the current knobs.  Host arithmetic only: no launch, no device
 * work; pg_vit_forward_precise runs what this reports (one function decides both).
 *   out[0..3]  the form of the layer's QKV / out-projection / fc1 / fc2 GEMM in the first (largest) internal pass: 0 = csrc/gemm_mid.hip,
 *              1 = one launch of the 256 x 256 persistent kernel, S > 1 = S K-parts in one launch + the fixed-order sum of the parts
 *   out[4]     1 = fc1's epilogue writes the QuickGELU triple (only where out[2] == 1 and pg_tune_exact_fusion is on)
 *   out[5]     1 = the attention writes the triple the out-projection reads
 *   out[6]     images in the largest internal pass: n_images up to 128; above, ceil(n_images / out[7])
 *   out[7]     internal passes: ceil(n_images / 128); the first n_images - out[7] * (out[6] - 1) take out[6] images, the others one fewer */
int pg_vit_precise_plan(int n_images, int32_t out[8]);
int pg_vit_forward_precise(pg_vit* h, const void* pixels, int pix_dtype, int n_images, float* emb_out, float* hidden_out,
                           void* workspace, size_t workspace_bytes, void* stream);
/* hipGraph of the encoder (round 4).  pg_vit_forward replays the ~250 launches between im2col and the token mean -- they touch only
 * the workspace and the handle's weights -- from a graph captured at the second forward with the same (workspace, n_images); default
 * on (env PIGEON_VIT_GRAPH=0: off).  Results are bit-identical either way (same kernels, same order).  Forwards run un-graphed while
 * pg_vit_profile_enable / pg_vit_saturation_check are on.  on = 1 / 0 switches it, any other value only queries; replays / captures
 * (may be NULL) return the counts since creation. */
int pg_vit_graph(pg_vit* h, int on, int64_t* replays, int64_t* captures);
int pg_vit_destroy(pg_vit* h);
/* The operand format the handle resolved to (PG_DTYPE_F16 or PG_DTYPE_BF16). */
int pg_vit_mma_dtype(const pg_vit* h);

/* WEIGHT FINGERPRINT: the key of a stored calibration.  The reference maps (weights, image) to an embedding deterministically
 * (models/clip_embedder.py:63-65); this path's fast embeddings additionally depend on a measurement taken once per set of weights
 * (the bias pg_embedding_debias subtracts, the certainty tolerance).  A stored measurement is only safe with the weights it was
 * taken on, and those exist only on the device (16-bit, LayerNorm-folded, packed by pg_vit_finalize) -- so the key is computed there.
 *
 * pg_fingerprint: a 128-bit digest of `bytes` bytes at DEVICE pointer `data` (16-byte aligned, else PG_EINVAL with a message and `out`
 * untouched; on the current device), written to HOST out[2].  Position-sensitive, seed- and length-dependent, independent of grid and
 * reduction order (wrap-around integer sums); defined completely in csrc/fingerprint.hip's header, restated in tests/_fpref.py.
 * bytes = 0 is legal (the digest of the empty buffer, no launch).  Runs on `stream` and SYNCHRONISES it before returning (the result
 * is a host value); allocates and frees a small scratch buffer.  Not for the hot path.
 * pg_vit_fingerprint: the digests of every parameter buffer pg_vit_forward reads (packed 16-bit weights, folded column sums and
 * biases, LayerNorm parameters, class and position embeddings), each with its byte size and a per-buffer seed, folded in a fixed
 * order (csrc/vit_weights.hip) with the layer count, the MFMA operand dtype and whether LayerNorm is folded.  The exact tier's split-weight
 * copy (cfg.precise) is not included: handles with and without it give the same value.  Two launches on the null stream, one
 * synchronous copy back (~0.6 GB read for ViT-L).  Any change of a weight that changes a stored bit changes the result. */
int pg_fingerprint(const void* data, size_t bytes, uint64_t seed, uint64_t out[2], void* stream);
int pg_vit_fingerprint(const pg_vit* h, uint64_t out[2]);
/* TEST / DEBUG entry, not for the hot path: copies one parameter buffer of a finalized handle (PG_ESTATE before) to HOST `host_dst`,
 * synchronously, on the handle's device (the caller's current device is restored).  (group, slot) is pg_vit_fingerprint's numbering
 * (csrc/vit_weights.hip: group 0 slots 0..4 the embeddings, group l + 1 slots 0..13 encoder layer l), continued by the buffers the
 * fingerprint leaves out: group 0 slot 5 the patch weight's split-fp16 triple, 6 the normalisation table; group l + 1 slots 14..19 the
 * QKV, out_proj, fc1 and fc2 triples and the raw QKV and fc1 biases.  *bytes receives the buffer's size; host_dst == NULL only
 * queries it.  A buffer this handle does not have (the column sums without the LayerNorm fold, the exact tier's slots without
 * cfg.precise) is PG_OK with *bytes = 0; any other (group, slot) is PG_EINVAL; dst_bytes < *bytes is PG_EINVAL and copies nothing. */
int pg_vit_param_read(const pg_vit* h, int group, int slot, void* host_dst, size_t dst_bytes, size_t* bytes);

/* Per-kernel-class timing (HIP events on `stream`), for bench.py's roofline object.
 * pg_vit_profile_enable(h,1) makes subsequent forwards bracket every launch with events; a value >= 2 is a class mask
 * shifted left by one (bit c+1 = class c, e.g. 1 << 3 = the fc1 GEMMs only): bench.py --profile dominant keeps just the
 * dominant class's events inside its timed region; 0 switches the events off;
 * pg_vit_profile_read synchronises those events and returns, per class, launches and total milliseconds.
 * Classes: 0 gemm_qkv 1 gemm_out 2 gemm_fc1 3 gemm_fc2 4 gemm_patch 5 attention 6 layernorm 7 im2col
 *          8 token_mean  (PG_PROF_CLASSES entries). */
#define PG_PROF_CLASSES 9
int pg_vit_profile_enable(pg_vit* h, int on);
int pg_vit_profile_read(pg_vit* h, int64_t* launches /*[PG_PROF_CLASSES]*/, double* ms /*[PG_PROF_CLASSES]*/);
int pg_vit_profile_reset(pg_vit* h);

/* fp16 saturation check (debug aid, off by default; costs one scan per 16-bit activation buffer per layer).  The
 * encoder's fp32 -> fp16 conversions clamp at +-65504 instead of overflowing to inf; with the check enabled the forward
 * pass counts, buffer by buffer, the 16-bit activations sitting exactly on that limit (bf16 operands: the +-inf).
 * pg_vit_saturation_read returns the total since the last reset (synchronises the device); 0 = nothing was clamped. */
/* Tuning knob (process-wide, default from the build / env PIGEON_GEMM_STAGGER): the persistent GEMMs start XCD x of the 8
 * XCDs x/8 * fraction of a tile period late, so that the epilogue (HBM) phase of one XCD overlaps the mainloop (MFMA)
 * phases of the others; 0 = all blocks start together.  Changes timing only, never results. */
int pg_tune_gemm_stagger(float fraction);
/* Tuning knob (also env PIGEON_GEMM_TAIL_ROWS; default 768): when a GEMM's tiles do not fill the last round of the persistent
 * kernels and at most `rows` rows lie beyond the last whole round, those rows go to a small-tile kernel (csrc/gemm_tail.hip)
 * that spreads them over all CUs; 0 = never.  Both kernels produce the same bits for a row: timing only, never results. */
int pg_tune_gemm_tail_rows(int rows);
/* ... and only for GEMMs with K >= min_k or N >= min_n (env PIGEON_GEMM_TAIL_MIN_K / PIGEON_GEMM_TAIL_MIN_N; defaults 2048 / 4096:
 * of the model's four GEMMs the split pays for fc2 and fc1 only).  (0, 0) = every shape.  Timing only, never results. */
int pg_tune_gemm_tail_shape(int min_k, int min_n);
/* Raster of the 384 x 256 persistent GEMM (QKV, fc1, fc2; also env PIGEON_GEMM_RASTER_GN): N tiles per group an XCD's round walks
 * before it moves to the next row panels.  0 = default (4: 8 x 4 super-tiles, 2 MB of weights resident per XCD), -1 = all N tiles
 * (each activation panel crosses the fabric once, the weight panels are re-streamed per XCD), 1..64 = explicit (honoured for a GEMM only when it divides that
 * GEMM's count of 256-column tiles, or is at least that count; otherwise the default stays).  Timing only, never results. */
int pg_tune_gemm_raster(int gn);
/* Small and middle batches (round 6; also env PIGEON_GEMM_MID=0 / 1 / 2): a GEMM launch of up to ~64 images (40 000 token rows) is
 * routed between the variant's own persistent kernel (384 x 256 tiles where they exist), the 256 x 256 persistent kernel and a 128 x 128
 * one-tile-per-block kernel (csrc/gemm_mid.hip) by a cost model of how their row panels fill rounds of the CUs (csrc/gemm_plan.hip
 * gemm_model_us).  1 = on (default), 0 = a variant always means its own kernel, 2 = gemm_mid.hip is the only alternative (A/B arm).
 * All GEMM kernels produce the same bits for a row: timing only, never results. */
int pg_tune_gemm_mid(int on);
/* What pg_op_gemm16* / the encoder would launch for this shape under the current knobs (variant 0 = the default): *kernel takes rows
 * [0, *rows_main) -- 0 the 384 x 256 persistent kernel, 1 the 256 x 256 one, 2 csrc/gemm_mid.hip, 3 csrc/gemm_tail.hip, 4 the
 * one-tile-per-block kernel of csrc/gemm_bf16.hip -- and *rest the remaining rows: -1 none, 2 gemm_mid, 3 gemm_tail.  PG_EINVAL where
 * the GEMM launch refuses the variant / shape / epilogue.
 * Host arithmetic only: no launch, no device work (tests/test_host_cpu.py checks the picks against profiles/r06/gemm_three_sweep.txt). */
int pg_gemm_plan(int variant, int epi, int M, int N, int K, int* kernel, int* rows_main, int* rest);
/* Exact mode's attention (also env PIGEON_EXACT_ATTN=f32): 0 = split-fp16 operands on v_mfma_f32_32x32x16_f16 (default, round 5),
 * 1 = plain fp32 on v_mfma_f32_32x32x2_f32 (round 4's kernel; the A/B arm).  Both are fp32-grade (6e-7 / 8e-7 against fp64). */
int pg_tune_exact_attention(int use_f32_mfma);
/* Exact mode's weight GEMMs (round 6, experimental): 3 = all three partial products hi.Wh + lo.Wh + hi.Wl (default: the exact tier), 2 = the
 * first two (both halves of the activations, the weights at their fp16 value: K' = 2K on the same operands) -- what remains is the
 * weights' rounding, a systematic embedding error the same for every image up to its dependence on the activations; 2/3 of the GEMM
 * work.  Process-wide; anything else is PG_EINVAL. */
int pg_tune_exact_products(int n);
/* Exact mode's activation splits (round 6; also env PIGEON_EXACT_FUSION=0): 1 = fused into their producers (default: the attention writes
 * the split-fp16 triple the out-projection reads, fc1's epilogue applies QuickGELU and writes the triple fc2 reads -- csrc/x3.h holds
 * the one definition of both forms' arithmetic), 0 = an fp32 buffer plus a split kernel each (the checker).  Bit-identical results. */
int pg_tune_exact_fusion(int on);
int pg_vit_saturation_check(pg_vit* h, int on);
int pg_vit_saturation_read(pg_vit* h, int64_t* count, int reset);
/* Always-on range alarm of the fp16 operand path (no scan, no cost worth naming): the kernel that turns the residual GEMMs' row
 * statistics into (rstd, mean rstd) also counts the rows whose sum of squares reaches 65504^2 -- a NECESSARY condition for an
 * element of that row's 16-bit copy (the next GEMM's operand) to have been clamped at the fp16 limit.  0 = no residual row ever
 * came near the limit since the last reset; > 0 = run pg_vit_saturation_check for the exact element count, or switch the
 * handle to bf16 operands.  Always 0 with bf16 operands or the separate-LayerNorm chain.  Synchronises the device. */
int pg_vit_range_alarm_read(pg_vit* h, int64_t* rows, int reset);

/* ------------------------------------------------------------------------------------------------
 * SuperGuessr geocell head.
 * Replaces: models/super_guessr.py:437 (panel mean), :447 (cell_layer Linear), :448 (softmax), :454 (argmax),
 * :455 (index_select of lla_geocells), :459 (topk).  fp32 throughout; centroids float64.
 *   emb      DEVICE (B,P,1024) fp32, P = 4 (panorama) or 1
 *   W, bias  DEVICE (C,1024) / (C) fp32 -- cell_layer.weight / .bias
 *   centroids DEVICE (C,2) float64 [lng,lat] -- lla_geocells
 *   logits   DEVICE (B,C) fp32 out (required; also scratch)
 *   topk_val DEVICE (B,k) fp32 out: softmax probabilities, descending; ties -> lower index first
 *   topk_idx DEVICE (B,k) int64 out
 *   argmax   DEVICE (B) int64 out (== topk_idx[:,0])
 *   pred_llh DEVICE (B,2) float64 out = centroids[argmax]
 * Limits: 1 <= k <= C, P >= 1; anything else is PG_EINVAL.  Up to C = 38 400 a row's probabilities live in LDS while its top k are
 * picked (the reference's geocell sets have 2 000 - 11 000 cells); larger heads take the same kernel over a stream-ordered device
 * scratch of B x C floats (hipMallocAsync / hipFreeAsync on `stream`), same results.
 * ------------------------------------------------------------------------------------------------ */
int pg_head_forward(const float* emb, int B, int P, const float* W, const float* bias,
                    const double* centroids, int C, int k, float* logits,
                    float* topk_val, int64_t* topk_idx, int64_t* argmax, double* pred_llh, void* stream);

/* Certainty of the top-1 (round 4; reference models/super_guessr.py:454 `torch.argmax`): per row of `logits` (B,C) as written by
 * pg_head_forward,
 *   margin DEVICE (B) fp32 out = logit(top-1) - logit(top-2)   (value desc, index asc -- the order of the selection above)
 *   sens   DEVICE (B) fp32 out = |mean_p emb|_2 * |W[top1] - W[top2]|_2 / sqrt(1024): the change of the margin per unit RELATIVE
 *          embedding error in a random direction; the host calls a row certain when margin > kappa * eps * sens, eps = its bound
 *          on the encoder's relative embedding error (pigeon_amd/super_guessr.py)
 *   top2   DEVICE (B) int64 out, may be NULL: the runner-up cell.   C == 1: margin = +inf, sens = 0, top2 = top1. */
int pg_head_margin(const float* logits, int B, int C, const float* emb, int P, const float* W, float* margin, float* sens,
                   int64_t* top2, void* stream);

/* Certainty of the top-1 against EVERY cell (round 5; supersedes pg_head_margin's top-1 / top-2 pair).  The embedding this path
 * feeds the head differs from the reference's fp32 one by  |e| (beta + r):  beta a calibrated systematic part (relative to |e|,
 * may be NULL), r of relative RMS norm eps in an unknown direction.  Per row,
 *   tol  DEVICE (B) fp32 out = min over cells c != top1 of (logit(top1) - logit(c) - |e| g.beta) / (|e| |g| / 32),  g = W[top1] - W[c]:
 *        the largest eps, in standard deviations of the margin change, that the reference's argmax (models/super_guessr.py:454) survives;
 *        the cells are the kx listed in topk_idx (as pg_head_forward wrote them, descending) and -- bounded with the list's last logit,
 *        |g| <= |W[top1]| + wstats[0] and g.beta <= W[top1].beta + wstats[1] -- every cell not listed.  The host calls a row certain
 *        when tol > kappa * eps.
 *   code DEVICE (B) int32 out: the list position j >= 1 that sets tol, -1 = the cells beyond the list, -2 = bad index in the list
 *   margin, sens DEVICE (B) fp32 out, may be NULL: pg_head_margin's pair (top-1 against top-2), for reports
 *   wstats DEVICE (2) fp32: [0] the largest row norm of W, [1] max over cells of |W[c].beta| (0 without beta).
 *   Limits: 1 <= kx <= C; kx == C: nothing beyond the list. */
int pg_head_certainty(const float* logits, int B, int C, const float* emb, int P, const float* W, const int64_t* topk_idx, int kx,
                      const float* beta, const float* wstats, float* tol, int32_t* code, float* margin, float* sens, void* stream);

/* Auxiliary heads of SuperGuessr(multi_task=True) (reference models/super_guessr.py:333-338: multi_task_head 1024 -> 6, climate_layer
 * 1024 -> 28, month_layer 1024 -> 12) in ONE launch, fp32 end to end, one block per row.
 *   emb      DEVICE (B,P,1024) fp32, as pg_head_forward takes it (the heads read the mean over the P panels)
 *   W, bias  DEVICE (A,1024), (A) fp32: rows [regression | climate | month], A = n_reg + n_climate + n_month <= 64;
 *            any of the three counts may be 0 (n_month = 0: yfcc), not all of them
 *   beta     DEVICE (1024) fp32 or NULL: the systematic part of the embedding error, as pg_head_certainty takes it
 *   preds    DEVICE (B,A) fp32 out = mean_p(emb[b]) . W[a] + bias[a]; one fixed summation order per element: a row's bits do not
 *            depend on B or on the other rows of the batch
 *   cls      DEVICE (B,2) int64 out: argmax of the climate outputs, argmax of the month outputs (first maximum in torch.argmax's
 *            order: a NaN ranks above every number, ties go to the lowest index); -1 where the classifier has no outputs
 *   tol      DEVICE (B) fp32 out: pg_head_certainty's tolerance of the two argmaxes -- the minimum over every alternative class c of
 *            both classifiers of (m - |e| g.beta) / (|e| |g| / 32), m = preds[c0] - preds[c], g = W[c0] - W[c]; +inf when there is
 *            no alternative, 0 when a margin is NaN.  The regression outputs are continuous and have none.
 *   code     DEVICE (B) int32 out: 1 + c when climate class c sets tol, 101 + c for month class c, 0 when nothing does
 *   row_tol  DEVICE (B) fp32 in/out, may be NULL: if (tol[b] < row_tol[b]) row_tol[b] = tol[b]   (the row's tolerance over all of its
 *            discrete outputs, e.g. pg_head_certainty's `tol`)
 * B = 0 is a no-op (buffers may be NULL), B < 0, P < 1, a negative count, A = 0 and A > 64 are PG_EINVAL.  Asynchronous on `stream`. */
int pg_aux_heads_forward(const float* emb, int B, int P, const float* W, const float* bias, int n_reg, int n_climate, int n_month,
                         const float* beta, float* preds, int64_t* cls, float* tol, int32_t* code, float* row_tol, void* stream);

/* ------------------------------------------------------------------------------------------------
 * ProtoRefiner prototype-distance refinement over a CSR prototype bank.
 * Replaces: models/proto_refiner.py:154-222 (the per-sample / per-candidate Python loop), :233-255
 * (within-cluster refinement: FARTHEST member), :332-344 (torch.cdist L2), :346-357 (temperature softmax
 * without max shift) and preprocessing/geo_utils.py:40-55 (haversine veto: float64, the refined fp32 point promoted after deg2rad / cos as torch does).
 * The bank arrays are BORROWED device pointers (caller keeps the tensors alive):
 *   proto_emb (P,1024) f32; cell_off (C+1) i64; proto_lnglat (P,2) f32; proto_count (P) i32;
 *   member_off (P+1) i64; member_idx (Nm) i64; train_emb (Ntr,1024) f32; train_lnglat (Ntr,2) f32.
 * ------------------------------------------------------------------------------------------------ */
typedef struct pg_bank {
    const float*   proto_emb;
    const int64_t* cell_off;
    const float*   proto_lnglat;
    const int32_t* proto_count;
    const int64_t* member_off;
    const int64_t* member_idx;
    const float*   train_emb;
    const float*   train_lnglat;
    int64_t num_cells;
    int64_t num_protos;
    int64_t num_train;
} pg_bank;

/*   q          DEVICE (B,P,1024) fp32 query embeddings (P panels are averaged first: proto_refiner.py:139-140)
 *   init_llh   DEVICE (B,2) float64 initial [lng,lat] predictions
 *   cand       DEVICE (B,k) int64 candidate geocells;  cand_prob DEVICE (B,k) fp32 (NULL -> [1,0,0,...], :143-145)
 *   topk <= k, topk <= 64
 *   scratch    DEVICE >= B*topk*4 floats; on return (score, lng, lat, bank rows streamed) per (query, candidate)
 *   out_llh    DEVICE (B,2) fp32; out_cell DEVICE (B) int64; out_choice DEVICE (B) int32 (index of the chosen
 *              candidate, the reference's guess_index, proto_refiner.py:220)                              */
int pg_refine_forward(const pg_bank* bank, const float* q, int B, int P, const double* init_llh,
                      const int64_t* cand, const float* cand_prob, int k, int topk,
                      float temperature, double max_refine_km, float* scratch,
                      float* out_llh, int64_t* out_cell, int32_t* out_choice, void* stream);

/* pg_refine_forward with n_eval >= topk candidates evaluated per query (topk <= n_eval <= k): the selection is pg_refine_forward's,
 * over the first topk only; the candidates beyond take no part in it and exist for pg_refine_certainty (could one of them enter the
 * set and win?).  scratch12: DEVICE >= B*n_eval*12 floats; per (query, candidate) on return
 *   [0] score = -distance to the nearest prototype (-100000: empty cell)  [1] lng  [2] lat  [3] bank rows streamed
 *   [4] distance of the runner-up prototype (+inf: none)   [5] / [6] bank rows of the nearest / runner-up prototype
 *   [7] / [8] distance of the farthest / second farthest member of the chosen cluster (-1: none)
 *   [9] / [10] their training-bank rows   [11] member count of the chosen prototype      ([5] [6] [9] [10] [11]: int32 bit patterns, -1 = none)
 * out_refined DEVICE (B) int32, may be NULL: the candidate picked BEFORE the haversine veto (out_choice: after it). */
int pg_refine_forward_ex(const pg_bank* bank, const float* q, int B, int P, const double* init_llh,
                         const int64_t* cand, const float* cand_prob, int k, int topk, int n_eval,
                         float temperature, double max_refine_km, float* scratch12,
                         float* out_llh, int64_t* out_cell, int32_t* out_choice, int32_t* out_refined, void* stream);

/* Certainty of the refined cell and point (round 5; reference models/proto_refiner.py:176-222).  Same error model and units as
 * pg_head_certainty; the decisions of a row are: the winning candidate r against every other candidate of the set
 * (s_j = log p_j - d_j / T; gradient W[c_r] - W[c_j] - (u_r - u_j) / T with u_j the unit vector from candidate j's nearest prototype to
 * the query), every evaluated candidate outside the set (it must get into the set AND -- unless it pushes r out -- win), the cells
 * beyond the evaluated ones (getting in counts; only when n_eval > topk, i.e. when the caller supplied candidates past the set), and
 * for the refined and the finally chosen candidate the nearest-prototype and farthest-member picks.  The haversine veto compares
 * two discrete points and has no margin.   W (C,1024) = the head's weights (the candidates' log-probabilities move with the
 * embedding through them), wstats as above, refined / choice as pg_refine_forward_ex wrote them.
 *   tol DEVICE (B) fp32 out;  code DEVICE (B) int32 out: 1000 + j / 2000 + j / 2999 / 3000 + w / 4000 + w (see csrc/certainty.hip; round 6: the nearest
 *   prototype / farthest member are checked against EVERY other prototype of the cell / member of the cluster, whose rows are streamed again), -9 = the winning product underflows in fp32, or
 *   an empty cell wins a set that is not all empty (uncertain), -8 = refined / choice outside [0, topk) (tol 0), 0 = nothing can change
 *   the row.   Limits: topk <= 64, n_eval <= min(k, 96). */
int pg_refine_certainty(const pg_bank* bank, const float* q, int B, int P, const int64_t* cand, const float* cand_prob, int k,
                        int topk, int n_eval, const float* scratch12, const float* W, int C, const float* beta,
                        const float* wstats, float temperature, const int32_t* refined, const int32_t* choice,
                        float* tol, int32_t* code, void* stream);

/* pg_refine_certainty for a bank whose rows carry an error of their own (a bank built from embeddings of the 16-bit encoder;
 * derivation: csrc/certainty.hip "Bank error").  Every bank row p is taken to be off by |p| r_p, r_p of relative RMS
 * norm eps_b in an unknown direction, independent from row to row, the systematic part removed (a bank that was not debiased declares
 * its whole error).  bank_sigma = kappa * eps_b, ONE scalar for all rows (finite, >= 0; else PG_EINVAL): the z-score the host compares
 * tolerances with, times the bank's relative error.  Per decision, with num = m - |e| g.beta, A = |e| |g| / 32 and
 * Bk = bank_sigma sqrt(bsum) / 32, bsum = sum of w^2 |row|^2 over the bank rows that enter it (candidate-score pairs: the nearest
 * prototype of both candidates, w = 1 / T, empty cells nothing; nearest prototype / farthest member: the pick and the alternative,
 * w = 1; set-boundary margins: none), the tolerance is sqrt((num - Bk)(num + Bk)) / A, 0 where num <= Bk (no query accuracy settles
 * it), and pg_refine_certainty's own expression where bank_sigma or bsum is 0 -- bank_sigma = 0 gives pg_refine_certainty's tol and
 * code bit for bit.  tol keeps its meaning (the largest relative query error, in standard deviations, every decision survives), so one
 * value serves the fast and the exact tier's threshold; code as above.  The row norms come from the rows the pass streams anyway. */
int pg_refine_certainty_bank(const pg_bank* bank, const float* q, int B, int P, const int64_t* cand, const float* cand_prob, int k,
                             int topk, int n_eval, const float* scratch12, const float* W, int C, const float* beta,
                             const float* wstats, float temperature, const int32_t* refined, const int32_t* choice,
                             float* tol, int32_t* code, float bank_sigma, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The deferred exact tier (round 6; csrc/requeue.hip).  The reference's discrete outputs are fp32 end to end
 * (models/super_guessr.py:447-459, models/proto_refiner.py:176-222); a sample that pg_head_certainty / pg_refine_certainty cannot call
 * certain is re-encoded by pg_vit_forward_precise.  These entry points keep that decision ON THE DEVICE: no `nonzero`, no host
 * synchronisation per step.  The caller owns a circular queue of `cap` slots -- the pixels of the queued rows (cap x row_bytes) and, per
 * slot, the row of its result ring the sample belongs to -- and a result ring that the exact tier's outputs are scattered into before
 * the host collects anything (the reference concatenates at the end of its loop: training/train_eval_loop.py:98-112).
 *
 * pg_requeue_append: per row r < B
 *     certain[r] = head_tol[r] > thr && (refine_tol == NULL || refine_tol[r] > thr) && !force_all     (a NaN tolerance is not certain)
 *     cause[r]   = 0 certain | 1 the head's top-1 | else refine_code[r] (pg_refine_certainty's decision code; 2 when that is 0 / NULL)
 *   and, for the rows that are not certain and while the queue has room (appended - flushed < cap), in row order:
 *     slot = appended % cap;  slot_dst[slot] = dst_base + r;  row_slot[r] = slot;  ++appended
 *   row_slot[r] = -1 for certain rows, -2 for rows that did not fit (counted in counters[1]; the host sizes the queue so that this
 *   cannot happen and checks the counter).  counters DEVICE int64[2] = { rows ever appended, rows that did not fit }; `flushed` = rows
 *   the host has already taken out (it knows: it enqueued those flushes).  cap = 0: flags and causes only (counters, slot_dst,
 *   row_slot may be NULL) -- how the exact tier's own results are judged.   certain DEVICE uint8[B], cause DEVICE int32[B], may be NULL.
 * pg_rows_to_slots:  dst + row_slot[r] * row_bytes <- src + r * row_bytes for every r < B with row_slot[r] >= 0 (the queued pixels).
 * pg_requeue_take:   dst_out[i] = i < n_valid ? slot_dst[(head + i) % cap] : -1,  i < n_pad   (ring rows of the slots being flushed;
 *                    the padding rows exist so that every rank of a data-parallel job runs the exact tier on the same batch size).
 * pg_scatter_rows:   dst + d * row_bytes <- src + i * row_bytes, d = dst_row[i] >= 0, i < n.  remap_wb > 0: dst_row addresses the
 *                    GATHERED ring (slabs of remap_wb rows, this rank's rows at [remap_off, remap_off + remap_b) of a slab) while dst is
 *                    a local-only array with slabs of remap_b rows: d = (dst_row / remap_wb) * remap_b + dst_row % remap_wb - remap_off,
 *                    rows of other ranks are skipped.  Rows with d >= dst_rows are skipped.
 * pg_head_wstats:    out2 DEVICE float[2] = { max_c |W[c]|_2, max_c |W[c] . beta| } (beta DEVICE (1024), may be NULL -> 0): the bounds
 *                    pg_head_certainty / pg_refine_certainty take for the cells they do not visit one by one.
 * All asynchronous on `stream`. */
int pg_requeue_append(const float* head_tol, const float* refine_tol, const int32_t* refine_code, int B, float thr, int force_all,
                      int64_t dst_base, int64_t flushed, int64_t cap, int64_t* counters, int64_t* slot_dst, int32_t* row_slot,
                      uint8_t* certain, int32_t* cause, void* stream);
int pg_rows_to_slots(const void* src, int64_t row_bytes, const int32_t* row_slot, int B, void* dst, void* stream);
int pg_requeue_take(const int64_t* slot_dst, int64_t cap, int64_t head, int n_valid, int n_pad, int64_t* dst_out, void* stream);
int pg_scatter_rows(const void* src, int64_t row_bytes, const int64_t* dst_row, int n, void* dst, int64_t dst_rows,
                    int64_t remap_wb, int64_t remap_b, int64_t remap_off, void* stream);
int pg_head_wstats(const float* W, int C, const float* beta, float* out2, void* stream);

/* The systematic part of the 16-bit encoder's error taken out of its embeddings, in place:  emb[r] <- emb[r] - |emb[r]|_2 * bias
 * for every row r < n of the DEVICE (n, dim) fp32 matrix (dim must be 1024); bias DEVICE (1024) fp32 = the mean over a few calibration
 * images of (fast - exact) / |exact| (pigeon_amd/certainty.py: measured once per set of weights by sending the same images through
 * pg_vit_forward and pg_vit_forward_precise).  The reference's encoder is fp32 (models/clip_embedder.py:63-65,
 * models/super_guessr.py:395-398) and has no such term; what is left of this path's error after the subtraction is the part that
 * differs from image to image, which pg_head_certainty / pg_refine_certainty account for.  The norm is summed in a fixed order (a row's
 * bits do not depend on the batch).  Asynchronous on `stream`. */
int pg_embedding_debias(float* emb, int64_t n, int dim, const float* bias, void* stream);

/* Patch attribution: a geocell logit, or the difference of two, as an exact sum over tokens (csrc/attribution.hip).  The embedding is
 * the plain mean of the 577 rows of last_hidden_state and the head one Linear over the mean of the P views (reference
 * models/clip_embedder.py:65, models/super_guessr.py:398, :437, :447), so
 *     logit[c] - logit[r] = (b[c] - b[r]) + sum over views p, tokens t of  h[p,t,:] . (W[c] - W[r]) / (577 P)
 * and this entry point computes the summands.
 *   hidden   DEVICE (n_images, 577, 1024) fp32: what pg_vit_forward_hidden / pg_vit_forward_precise write as `hidden_out`;
 *            n_images = B * P, P >= 1 views per sample as in pg_head_forward (anything else: PG_EINVAL)
 *   W        DEVICE (C, 1024) fp32, the head's weight;  hidden and W 16-byte aligned
 *   cells    DEVICE (B, K) int64, 1 <= K <= 16: the cells to explain, per sample
 *   against  DEVICE (B) int64 or NULL: the cell each of the sample's K cells is compared with; an entry of -1 (or NULL) means none
 *   out      DEVICE (B, P, 577, K) fp32:
 *              g[j] = W[cells[b,k]][j] - W[against[b]][j]   in fp32, one rounding (W[cells[b,k]][j] itself without `against`)
 *              d    = sum_j h[b,p,t,j] * g[j]               in fp32, in this fixed order: lane l = 0..63 of a wave runs
 *                     s_l = fma(h[j], g[j], s_l) over j = 256 i + 4 l + e, i = 0..3 outer, e = 0..3 inner, from s_l = 0; then the
 *                     64 partial sums are added by the butterfly v <- v + v(lane xor o), o = 32, 16, 8, 4, 2, 1
 *              out  = d / (float)(577 P)                     one IEEE division
 * The bits of out[b,p,t,k] are a function of that hidden row, the two rows of W and P alone: not of the batch size, of K, or of the
 * position k.  Token 0 is the class token, token 1 + 24 y + x the patch in row y, column x of the 336 x 336 crop.
 * The indices are device data and the kernel checks them: cells[b,k] outside [0, C) makes column (b, k) NaN on all of its P * 577
 * rows; against[b] outside [0, C) other than -1 makes every column of sample b NaN; no such index ever forms an address, and nothing
 * else in `out` is affected.  Nothing outside `out` is written.
 * n_images = 0 is a no-op (PG_OK; the buffers may be NULL); n_images < 0 or not a multiple of P, P < 1, K outside 1..16, C < 1, a
 * NULL hidden / W / cells / out and a misaligned hidden / W are PG_EINVAL with a message naming the argument.  One launch,
 * asynchronous on `stream`. */
int pg_token_attribution(const float* hidden, int n_images, int P, const float* W, int C, const int64_t* cells,
                         const int64_t* against, int K, float* out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * CLIP image preprocessing (the step in front of the encoder): uint8 RGB -> pixel_values.
 * Replaces `CLIPProcessor(images=..., return_tensors='pt')` (reference models/clip_embedder.py:52,
 * dataset_creation/finetune/embed_dataset.py:20, preprocessing/dataset_preprocessing.py:193,
 * dataset_creation/benchmark/benchmark_dataset.py:99): resize shorter edge to 336 with Pillow's fixed-point BICUBIC,
 * centre crop 336x336, float32 /255.0, (x-mean)/std, HWC->CHW -- bit-exact with Pillow + numpy float32.
 * A handle is bound to one input geometry (in_h, in_w); coefficient tables live on the device.
 * ------------------------------------------------------------------------------------------------ */
typedef struct pg_prep pg_prep;
int pg_prep_create(pg_prep** out, int device, int in_h, int in_w);
int pg_prep_destroy(pg_prep* h);
/* out6 = { resized_h, resized_w, crop_top, crop_left, first_source_row, source_rows_used } */
int pg_prep_geometry(const pg_prep* h, int32_t* out6);
int pg_prep_workspace_bytes(const pg_prep* h, int n_images, size_t* bytes);
/* The normalisation table: out[c * 256 + v] = ((v / 255) - mean[c]) / std[c] evaluated in IEEE float32, operation by operation, as
 * numpy does for float32 arrays -- every value a pixel can take.  HOST ONLY (no HIP call).  PG_EINVAL for a null pointer. */
int pg_prep_norm_lut(float out[768]);
/* images_u8: DEVICE (n_images, in_h, in_w, 3) uint8 RGB; out: DEVICE (n_images,3,336,336) fp32 (PG_DTYPE_F32), fp16
 * (PG_DTYPE_F16, the fp32 value rounded to nearest even -- exactly what the encoder's im2col would do to the fp32 value) or uint8
 * (PG_DTYPE_U8: the resized, clamped byte itself, planar; table[c][byte] is the fp32 output, a quarter of its size).  Same grids and
 * workspace for all three.  Asynchronous on `stream`. */
int pg_prep_forward(pg_prep* h, const void* images_u8, int n_images, void* out, int out_dtype, void* workspace,
                    size_t workspace_bytes, void* stream);

/* Ragged batches: n images of n different sizes in ONE packed buffer, one host-to-device copy and three launches, the same bits
 * as pg_prep_forward on each image alone.  One descriptor per image (plain data, PG_PREP_ITEM_BYTES bytes):
 *
 *   packed buffer  [ n descriptors | image 0 | image 1 | ... ]   every image (in_h, in_w, 3) uint8 RGB, starting at a multiple of
 *                  16 bytes, back to back in index order behind the n * PG_PREP_ITEM_BYTES bytes of the descriptors; the total is
 *                  rounded up to 16.  The descriptors travel in the buffer's head, so one copy carries both.
 *   workspace      [ tables of image 0 | tables of image 1 | ... | temp image ]   per image and axis the bounds (336 x 2 int32:
 *                  first source pixel, tap count -- Pillow's, i.e. in source coordinates) and the weights (336 x ksize int32, 22-bit
 *                  fixed point, zero behind the tap count), written by the first kernel; the temp image (the horizontally resized
 *                  rows the crop's vertical taps read: sum of nrows rows of 336 x 3 bytes, image after image) begins at the
 *                  first multiple of 256 behind the last table. */
#define PG_PREP_ITEM_BYTES 80
#define PG_PREP_RAGGED_MAX_IMAGES 65535
typedef struct pg_prep_item {
    uint64_t src_off;                 /* byte offset of the image in the packed buffer (multiple of 16) */
    int32_t in_h, in_w;               /* source size */
    int32_t new_h, new_w, top, left;  /* size after the resize, corner of the 336 x 336 crop in it (as pg_prep_geometry) */
    int32_t ksize_h, ksize_v;         /* taps per output of the horizontal / vertical pass (1 where the axis keeps its size) */
    int32_t row0, nrows;              /* source rows [row0, row0 + nrows) are the ones the crop's vertical taps read */
    int32_t tmp_row;                  /* the image's first row in the shared temp image: exclusive prefix sum of nrows */
    uint32_t bounds_h_off, kk_h_off, bounds_v_off, kk_v_off;   /* byte offsets of the four tables in the workspace (multiples of 16) */
    int32_t reserved[3];              /* zero */
} pg_prep_item;
/* HOST ONLY (no HIP call; works in a process that never opens a GPU): hw = n pairs (height, width); fills items_out[n] and the sizes
 * of the two buffers.  PG_EINVAL with a message for n < 0, n > PG_PREP_RAGGED_MAX_IMAGES, a null pointer, a size outside 1..16384
 * and tables that outgrow the descriptor's 32-bit offsets (the image is named).  n = 0: both sizes 0, pointers may be NULL. */
int pg_prep_ragged_plan(int n, const int32_t* hw, pg_prep_item* items_out, size_t* packed_bytes, size_t* workspace_bytes);
/* The handle owns the 3 x 256 normalisation table only; it serves every geometry. */
typedef struct pg_prep_ragged pg_prep_ragged;
int pg_prep_ragged_create(pg_prep_ragged** out, int device);
int pg_prep_ragged_destroy(pg_prep_ragged* h);
/* packed_dev: DEVICE, packed_bytes bytes, 16-byte aligned, laid out as above -- its first n * PG_PREP_ITEM_BYTES bytes MUST be a copy
 * of items_host (the kernels read the descriptors there; the host copy is what this call checks).  out: DEVICE (n,3,336,336) fp32,
 * fp16 or uint8 as pg_prep_forward.  workspace: DEVICE, 16-byte aligned.  Before anything is launched every descriptor is checked against
 * its own (in_h, in_w) and against packed_bytes / workspace_bytes -- geometry, range, alignment, ascending overlap-free offsets:
 * PG_EINVAL (PG_ENOMEM for a workspace too small for the temp image) with a message that names the image.  n = 0 is a no-op (buffers
 * may be NULL).  Asynchronous on `stream`: three launches whatever the sizes; the horizontal pass stages one source row in dynamic
 * LDS, widest in_w x 3 + 32 bytes (48 KiB + 32 at in_w = 16384). */
int pg_prep_ragged_forward(pg_prep_ragged* h, const void* packed_dev, size_t packed_bytes, const pg_prep_item* items_host, int n,
                           void* out, int out_dtype, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Baseline JPEG decoding in front of the ragged resize: files go in as bytes, the host parses the headers and undoes the Huffman
 * coding (pg_jpeg_entropy_decode, serial per file, a thread per file), the GPU dequantises, applies libjpeg's accurate integer inverse
 * DCT, expands the chroma as libjpeg-turbo's "fancy" upsampling does and converts to RGB (pg_jpeg_forward, two launches), writing
 * straight into the packed buffer pg_prep_ragged_forward reads.  The pixels are the ones Pillow (libjpeg-turbo) produces for
 * `Image.open(f).convert('RGB')`, bit for bit.
 *
 * Supported: SOF0 / SOF1 with 8-bit samples and Huffman coding, one interleaved scan, 1 component (grey: R = G = B = Y) or 3
 * components libjpeg reads as YCbCr (a JFIF marker, or an Adobe marker with transform 1, or neither and component ids other than
 * 'R','G','B'), luma sampling 1x1, 2x1 or 2x2 with both chroma components 1x1, sizes 1..16384.  Anything else is REFUSED by
 * pg_jpeg_probe with a reason -- not an error: the caller decodes such a file elsewhere and copies its pixels to its place.
 * ------------------------------------------------------------------------------------------------ */
#define PG_JPEG_R_OK            0
#define PG_JPEG_R_NOT_JPEG      1
#define PG_JPEG_R_PROGRESSIVE   2
#define PG_JPEG_R_LOSSLESS      3
#define PG_JPEG_R_HIERARCHICAL  4
#define PG_JPEG_R_ARITHMETIC    5
#define PG_JPEG_R_PRECISION     6    /* 12-bit samples */
#define PG_JPEG_R_COMPONENTS    7    /* 2 or 4 components (CMYK / YCCK) */
#define PG_JPEG_R_COLORSPACE    8    /* Adobe transform 0 or 2, component ids 'R','G','B' */
#define PG_JPEG_R_SAMPLING      9    /* 4:4:0, 4:1:1, chroma not 1x1 */
#define PG_JPEG_R_MULTISCAN     10
#define PG_JPEG_R_DNL           11
#define PG_JPEG_R_SIZE          12   /* height or width 0 or above 16384 */
#define PG_JPEG_R_MALFORMED     13   /* the header is damaged or ends before SOS */
typedef struct pg_jpeg_info {
    int32_t reason;                   /* PG_JPEG_R_* */
    int32_t height, width;            /* as far as the header got, else 0 */
    int32_t ncomp;                    /* 1 or 3 where reason is PG_JPEG_R_OK */
    int32_t hs, vs;                   /* luma sampling: 1x1, 2x1 or 2x2 (1x1 for grey) */
    int32_t reserved[2];              /* zero */
} pg_jpeg_info;
/* One image of a batch (plain data, PG_JPEG_ITEM_BYTES bytes).  ncomp = 0 marks an image whose pixels the caller supplies itself (a
 * refused file): it has a place in the packed buffer and nothing else.
 *
 *   coefficient buffer  [ n descriptors, rounded up to 128 bytes | blocks of image 0 | blocks of image 1 | ... ]   per image and
 *                       component the blocks of the component's padded block grid (whole MCUs: bw x bh blocks) in RASTER order, each
 *                       64 int16 in natural (de-zigzagged) order, a row of 8 = one row of the block; components in order, images in
 *                       order, no gaps.  The descriptors travel in the buffer's head, so one copy carries both.
 *   workspace           per image and component one 8-bit plane of (bh * 8) rows of (bw * 8) bytes, each at a multiple of 256.
 *   packed buffer       the one of pg_prep_ragged_forward: rgb_off is the image's pg_prep_item.src_off. */
#define PG_JPEG_ITEM_BYTES 640
typedef struct pg_jpeg_item {
    uint64_t rgb_off;                 /* byte offset of the image's (height, width, 3) RGB in the packed buffer (multiple of 16) */
    uint64_t coef_off[3];             /* byte offset of each component's blocks in the coefficient buffer (multiples of 128) */
    uint64_t plane_off[3];            /* byte offset of each component's plane in the workspace (multiples of 256) */
    int32_t height, width;
    int32_t ncomp;                    /* 1, 3, or 0: pixels supplied by the caller */
    int32_t hs, vs;                   /* luma sampling */
    int32_t bw[3], bh[3];             /* block grid per component */
    int32_t qsel[3];                  /* which of qt[] each component is dequantised with (filled by pg_jpeg_entropy_decode) */
    int32_t reserved[4];              /* zero */
    uint16_t qt[4][64];               /* quantisation tables, natural order (filled by pg_jpeg_entropy_decode) */
} pg_jpeg_item;
/* HOST ONLY.  Reads the markers of `data` up to SOS and fills *info.  Always PG_OK for non-null arguments: a refusal is a value of
 * info->reason.  pg_jpeg_reason: a static string for a reason code. */
int pg_jpeg_probe(const void* data, size_t nbytes, pg_jpeg_info* info);
const char* pg_jpeg_reason(int reason);
/* HOST ONLY.  The layout of a batch: infos[i] with reason PG_JPEG_R_OK is decoded on the GPU, any other reason makes image i one the
 * caller supplies (ncomp = 0; its height and width must be set by the caller).  Fills items_out[n], prep_items_out[n] and the four
 * sizes; prep_items_out, *packed_bytes and *prep_workspace_bytes are exactly what pg_prep_ragged_plan gives for the same (height,
 * width) list.  PG_EINVAL naming the image for a size outside 1..16384 or a sampling the decoder does not have. */
int pg_jpeg_plan(int n, const pg_jpeg_info* infos, pg_jpeg_item* items_out, pg_prep_item* prep_items_out, size_t* coef_bytes,
                 size_t* workspace_bytes, size_t* packed_bytes, size_t* prep_workspace_bytes);
/* HOST ONLY.  Entropy-decodes the files of the batch whose items have ncomp != 0 into the HOST coefficient buffer `coef` (coef_bytes
 * bytes, 16-byte aligned, laid out by pg_jpeg_plan; the regions are zeroed first) and fills each item's qsel / qt; finally copies the
 * n descriptors into the buffer's head.  data[i] / nbytes[i]: file i (ignored where ncomp = 0).  Files are independent: `threads`
 * (clamped to 1..16) workers take them in turn.  A Huffman code that does not exist, a marker or the end of the data inside an MCU,
 * a coefficient index past 63, a wrong RSTn or a missing EOI is PG_EINVAL with a message naming the image, whose index goes to
 * *bad_index (may be NULL; the lowest such index).  No read leaves [data[i], data[i] + nbytes[i]) and no write leaves the image's
 * coefficient region, whatever the bytes are. */
int pg_jpeg_entropy_decode(int n, const void* const* data, const size_t* nbytes, pg_jpeg_item* items, void* coef, size_t coef_bytes,
                           int threads, int* bad_index);
/* coef_dev: DEVICE copy of the coefficient buffer (16-byte aligned; its head MUST hold items_host).  Writes the RGB of every image with
 * ncomp != 0 to [rgb_off, rgb_off + height * width * 3) of packed_dev and nothing else behind the descriptors; copies prep_items_host
 * (n * PG_PREP_ITEM_BYTES bytes) into the head of packed_dev, which can then go to pg_prep_ragged_forward as it is.  Before anything is
 * launched every descriptor is checked against its own size and sampling and against the three buffer sizes -- grids, ascending
 * overlap-free offsets, alignment, rgb_off == prep_items_host[i].src_off: PG_EINVAL naming the image.  The arithmetic is 32-bit with
 * wrap-around, so any coefficient values give defined pixels and none can move an address.  n = 0 is a no-op.  Asynchronous on
 * `stream`: one copy and two launches. */
int pg_jpeg_forward(const void* coef_dev, size_t coef_bytes, const pg_jpeg_item* items_host, const pg_prep_item* prep_items_host, int n,
                    void* packed_dev, size_t packed_bytes, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Equirectangular panoramas in front of the ragged resize: perspective (gnomonic) S x S views of an H x W equirectangular image,
 * 8-bit RGB, written straight into the packed buffer pg_prep_ragged_forward reads.  One integer result per pixel (DESIGN.md,
 * "Equirectangular panoramas in"; tests/_equirectref.py is the numpy restatement).  The host computes the only two quantities that
 * carry the angles, in float64, and they travel as doubles:
 *   inv_f = tan(fov / 2) / (S / 2)
 *   rot   = Ry(yaw) . Rx(pitch), camera -> panorama, row-major; axes x right, y DOWN, z forward; yaw positive to the right, pitch
 *           positive upwards:  [[C, Sn*s, Sn*c], [0, c, -s], [-Sn, C*s, C*c]]  with c, s of the pitch and C, Sn of the yaw.
 * Pixel (row i, column j), IEEE float64, in this order, no contraction:
 *   x = (j + 0.5 - S/2) * inv_f,  y = (i + 0.5 - S/2) * inv_f,  w_k = (rot[k][0]*x + rot[k][1]*y) + rot[k][2]
 *   lambda = atan2(w_X, w_Z),  phi = atan2(-w_Y, sqrt(w_X*w_X + w_Z*w_Z))
 *   u = (lambda * (1/(2 pi)) + 0.5) * W - 0.5,  v = (0.5 - phi * (1/pi)) * H - 0.5 clamped to [0, H - 1]
 *   u0 = floor(u), v0 = floor(v), a = floor((u - u0) * 256 + 0.5), b = floor((v - v0) * 256 + 0.5)     (0 .. 256)
 *   columns u0 mod W and (u0 + 1) mod W (true modulo: the seam wraps), rows v0 and min(v0 + 1, H - 1)
 *   out_c = (p00*(256-a)*(256-b) + p01*a*(256-b) + p10*(256-a)*b + p11*a*b + 32768) >> 16
 * The weights sum to 65536: a constant image stays constant.  Addresses come from clamped or wrapped integers only.
 * ------------------------------------------------------------------------------------------------ */
#define PG_EQ_ITEM_BYTES 128
#define PG_EQ_MAX_VIEW 4096
typedef struct pg_eq_view {           /* what the caller knows of one view (input of pg_equirect_plan), 96 bytes */
    int32_t src_h, src_w;             /* the panorama's size, 1..16384 */
    int32_t src_index;                /* which of the plan's source offsets holds it */
    int32_t size;                     /* S, 1..PG_EQ_MAX_VIEW */
    double rot[9];                    /* row-major, finite */
    double inv_f;                     /* finite, positive */
} pg_eq_view;
typedef struct pg_eq_item {           /* one view of a batch (plain data, PG_EQ_ITEM_BYTES bytes) */
    uint64_t src_off;                 /* byte offset of the panorama's (src_h, src_w, 3) RGB in the source buffer (multiple of 16) */
    uint64_t dst_off;                 /* byte offset of the view's (size, size, 3) RGB in the packed buffer: its pg_prep_item.src_off */
    int32_t src_h, src_w, size;
    int32_t reserved0;                /* zero */
    double rot[9];
    double inv_f;
    int32_t reserved[4];              /* zero */
} pg_eq_item;
/* HOST ONLY (no HIP call; works in a process that never opens a GPU).  n views; view i reads the panorama at src_offs[views[i].src_index]
 * of the source buffer (n_src offsets, multiples of 16; several views may name one panorama).  Fills items_out[n]; prep_items_out[n],
 * *packed_bytes and *prep_workspace_bytes are exactly what pg_prep_ragged_plan gives for n images of size x size, and
 * items_out[i].dst_off == prep_items_out[i].src_off.  PG_EINVAL naming the view for a size out of range, a rot or inv_f that is not
 * finite (inv_f: and positive), a source index outside [0, n_src) or a misaligned source offset.  n = 0: both sizes 0. */
int pg_equirect_plan(int n, const pg_eq_view* views, int n_src, const uint64_t* src_offs, pg_eq_item* items_out,
                     pg_prep_item* prep_items_out, size_t* packed_bytes, size_t* prep_workspace_bytes);
/* src_dev: DEVICE, src_bytes bytes, 16-byte aligned: the panoramas at their offsets.  It may be a packed buffer written by
 * pg_jpeg_forward or filled from host pixels -- its descriptors in the head are simply not read -- so a panorama file goes file bytes
 * -> JPEG kernels -> this kernel -> resize without visiting the host.  Writes every view to [dst_off, dst_off + size * size * 3) of
 * packed_dev, copies prep_items_host (n * PG_PREP_ITEM_BYTES bytes) into its head, and writes nothing else; packed_dev can then go to
 * pg_prep_ragged_forward as it is.  Before anything is launched every descriptor is checked: sizes 1..16384 (source) and
 * 1..PG_EQ_MAX_VIEW (view), finite rot and finite positive inv_f, zero reserved fields, offsets that are multiples of 16, ascending
 * overlap-free destination ranges inside packed_bytes, source ranges inside src_bytes, dst_off == prep_items_host[i].src_off, and the
 * two buffers must not overlap: PG_EINVAL naming the view.  n = 0 is a no-op.  Asynchronous on `stream`: two copies (the two
 * descriptor arrays; the views' go to stream-ordered scratch) and one launch. */
int pg_equirect_forward(const void* src_dev, size_t src_bytes, const pg_eq_item* items_host, const pg_prep_item* prep_items_host, int n,
                        void* packed_dev, size_t packed_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The one collective of the path: all-gather over RCCL (xGMI inside a node).
 * Replaces: `accelerator.gather(index)` / `accelerator.gather(output)` at preprocessing/embed.py:36-37 (rank-major
 * concatenation on every rank).  One process per GPU; rank 0 creates the PG_COMM_ID_BYTES-byte id and the host program
 * ships it to the other ranks over its own bootstrap channel (a TCP store, MPI, a file ...); all ranks then call
 * pg_comm_init_rank concurrently with the HIP device they own set current.  RCCL is bound at run time
 * (dlopen "librccl.so.1"; env PIGEON_RCCL_LIB overrides), so a process that already carries an RCCL keeps a single copy.
 *   send  DEVICE bytes_per_rank bytes; recv DEVICE nranks * bytes_per_rank bytes (rank r's block at r * bytes_per_rank);
 *   asynchronous on `stream`, no host synchronisation. */
#define PG_COMM_ID_BYTES 128
int pg_comm_unique_id(void* id_out /*[PG_COMM_ID_BYTES]*/);
int pg_comm_init_rank(void** comm, int nranks, const void* unique_id /*[PG_COMM_ID_BYTES]*/, int rank);
int pg_comm_count(void* comm, int* nranks);          /* ranks as RCCL sees them */
int pg_allgather(void* comm, const void* send, void* recv, size_t bytes_per_rank, void* stream);
/* `count` buffers gathered in one RCCL group (one fused launch); buffer i: send[i] bytes_per_rank[i] bytes ->
 * recv[i] nranks * bytes_per_rank[i] bytes, rank-major.  The data-parallel step gathers embeddings, candidate cells /
 * probabilities, initial predictions and sample indices this way. */
int pg_allgather_many(void* comm, int count, const void* const* send, void* const* recv, const size_t* bytes_per_rank,
                      void* stream);
int pg_comm_destroy(void* comm);
int pg_comm_rccl_version(void);                       /* NCCL_VERSION_CODE of the bound library, < 0 on failure */

/* ------------------------------------------------------------------------------------------------
 * Around the hot path.
 * ------------------------------------------------------------------------------------------------ */
/* Prototype construction (reference models/proto_refiner.py:359-384): proto_emb[p] = fp32 mean, in member order, of
 * train_emb[member_idx[member_off[p] .. member_off[p+1])], each member first averaged over its `panels` (1 or 4) panel
 * embeddings; an empty prototype gets zeros.  train_emb: DEVICE (num_train, panels, 1024) fp32; proto_emb: DEVICE
 * (num_protos,1024) fp32.  Bit-identical to torch's `embeddings.mean(dim=1).mean(dim=0)` on the CPU. */
int pg_proto_build(const float* train_emb, int panels, int64_t num_train, const int64_t* member_off,
                   const int64_t* member_idx, int64_t num_protos, float* proto_emb, void* stream);
/* Great-circle distance matrix (reference preprocessing/geo_utils.py:58-74): x DEVICE (N,2) [lng,lat] degrees, fp32
 * (PG_DTYPE_F32: deg2rad / cos(lat) in fp32 then promoted, torch's type promotion) or fp64; y DEVICE (M,2) fp64 (note:
 * row-major (M,2), i.e. lla_geocells itself, where the reference passes its transpose); out DEVICE (N,M) fp64 km. */
int pg_haversine_matrix(const void* x, int x_dtype, const double* y, int N, int M, double* out, void* stream);
/* Row-paired great-circle distance (reference preprocessing/geo_utils.py:40-55 `haversine(x, y)`): x DEVICE (N,2) fp64,
 * y DEVICE (N,2) fp32 or fp64 (fp32: deg2rad / cos(lat) of y in fp32, then promoted -- the dtypes of the refiner's veto
 * call, models/proto_refiner.py:198-202); out DEVICE (N,) fp64 km. */
int pg_haversine_pairs(const double* x, const void* y, int y_dtype, int64_t N, double* out, void* stream);
/* Label smoothing (reference preprocessing/utils.py:7-19): out = exp(-(d - rowmin(d)) / constant), NaN/inf -> 0.
 * distances, out: DEVICE (N,M) fp64 (may alias). */
int pg_smooth_labels(const double* distances, int N, int M, double constant, double* out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Guess spread (csrc/spread.hip): how far off a point may be, from the head's logits.  The reference has no code for it; the contract is
 * this project's own and is restated in tests/_spreadref.py.  Per batch row b and query point g, all arithmetic in float64:
 *   m   = max_c l[b,c]        w_c = exp((double)l[b,c] - (double)m)        Z = sum_c w_c
 *   d_c = the km pg_haversine_matrix computes for x = point[b,g] (fp64), y = centroid[c] -- one device function, csrc/haversine.h
 *   expected_km[b,g]    = (sum_c w_c * d_c) / Z
 *   expected_score[b,g] = (sum_c w_c * 5000 * exp(-d_c / 1492.7)) / Z         the GeoGuessr score before its rounding
 *   key_c = d_c + extent_c      extent_c >= 0: how far cell c reaches from its centroid; extent_km == NULL: key_c = d_c
 *   M(t)  = sum over { c : key_c <= t } of w_c
 *   radius_km[b,g,j]    = min { key_c : M(key_c) >= quantiles[j] * Z }
 * radius[j] is the smallest circle around the point that holds, whole, cells carrying quantiles[j] of the probability.  With extent 0
 * the mass sits at the centroids: a confident head asked about its own centroid gets a radius of (almost) 0, not the cell's size.
 * Every sum over cells is taken in one fixed order that depends on C only (no atomics): a (row, point)'s outputs are the same bits
 * alone, inside any batch, at any position, in LDS or in scratch; M(+inf) is the same sequence of additions as Z.  A -inf logit is a
 * cell of weight 0 (a masked cell).  A NaN or +inf logit, a non-finite point, a row of -inf only, and a key that is not a finite
 * non-negative number (non-finite centroids or extents) give NaN in every output of that (row, point) and touch no other.
 * logits DEVICE (B,C) fp32; centroids DEVICE (C,2) fp64 [lng,lat]; extent_km DEVICE (C,) fp64 or NULL; points DEVICE (B,G,2) fp64;
 * quantiles HOST nq doubles in (0, 1], nq 1 .. 4; expected_km, expected_score DEVICE (B,G) fp64; radius_km DEVICE (B,G,nq) fp64.
 * B == 0 or G == 0 is a no-op.  PG_EINVAL, naming the argument and before any HIP call, for C < 1, nq outside 1 .. 4, a quantile outside
 * (0, 1], a negative B or G, B * G > 2^31 - 1 and a null pointer.  C above pg_guess_spread_plan's out[2] takes 16 * B * G * C bytes
 * of stream-ordered scratch.
 * ------------------------------------------------------------------------------------------------ */
int pg_guess_spread(const float* logits, int B, int C, const double* centroids, const double* extent_km, const double* points, int G,
                    const double* quantiles, int nq, double* expected_km, double* expected_score, double* radius_km, void* stream);
/* What pg_guess_spread does with C cells (host arithmetic, no GPU; PG_EINVAL for C < 1):
 *   out[0]  where the cells' (key, weight) pairs live: 0 = LDS, 1 = stream-ordered device scratch (same bits)
 *   out[1]  bytes of dynamic LDS a workgroup asks for (0 in form 1)
 *   out[2]  the largest C of form 0
 *   out[3]  threads of the workgroup; there is one per (row, point) */
int pg_guess_spread_plan(int C, int32_t out[4]);

/* ------------------------------------------------------------------------------------------------
 * The guess by expected score (csrc/guess_best.hip): of M candidate points shared by the batch, the one whose expectation under the
 * head's softmax is best.  The reference has no code for it (layers/hedge.py opens with a TODO); the contract is this project's own
 * and is restated in tests/_bestref.py.
 *
 * pg_score_table.  candidates DEVICE (M,2) fp64 [lng,lat]; centroids DEVICE (C,2) fp64; table DEVICE (M,C) fp64, candidate-major:
 *   d = the km pg_haversine_matrix computes for x = candidates[j] (fp64), y = centroids[c] -- one device function, csrc/haversine.h
 *   kind 0 (km):     table[j,c] = d
 *   kind 1 (score):  table[j,c] = 5000.0 * exp(-d / 1492.7)                     the GeoGuessr score before its rounding
 * A non-finite candidate or centroid gives NaN entries.  M == 0 is a no-op.  PG_EINVAL, naming the argument and before any HIP call,
 * for C < 1, a negative M, a kind other than 0 and 1, M * C beyond one launch (2^39 elements) and a null pointer.
 *
 * pg_guess_best.  logits DEVICE (B,C) fp32; table DEVICE (M,C) fp64 (any values: pg_score_table's, or the caller's own);
 * best_idx DEVICE (B,) int32; best_value DEVICE (B,) fp64; expected DEVICE (B,M) fp64 or NULL.  Per row b, all in float64:
 *   m = max_c l[b,c]      w_c = exp((double)l[b,c] - (double)m)      Z = sum_c w_c         pg_guess_spread's weights and Z, the same bits
 *   E[b,j]        = (sum_c w_c * table[j,c]) / Z
 *   best_idx[b]   = the smallest j whose E[b,j] equals max_j E[b,j] (maximize != 0; min_j for maximize == 0); a NaN E[b,j] never wins
 *   best_value[b] = E[b, best_idx[b]]
 * Every sum over cells is taken in one fixed order that depends on C only (no atomics, no split over C): E[b,j] is the same bits for a
 * row alone, inside any batch, at any row position, with any M, at any candidate position and in either form of the plan.  The pick
 * across candidate tiles is a second pass over per-tile partials.  A -inf logit is a cell of weight 0, and 0 * NaN is NaN: a NaN
 * table entry makes its candidate NaN for every row.  A NaN or +inf logit, or a row of -inf only, gives best_idx = -1, best_value =
 * NaN and a NaN `expected` row, and touches no other row; a row whose every E is NaN gives -1 / NaN as well.  No input value forms an
 * address or bounds a loop.  B == 0 or M == 0 is a no-op.  PG_EINVAL, naming the argument and before any HIP call, for C < 1, a
 * negative B or M, B * M > 2^31 - 1 and a null logits, table, best_idx or best_value.  Takes pg_guess_best_plan's out[5] bytes of
 * stream-ordered scratch: the weights (B,C) fp64, Z, and one (value, index) partial per row and candidate tile.
 * ------------------------------------------------------------------------------------------------ */
int pg_score_table(const double* candidates, int M, const double* centroids, int C, int kind, double* table, void* stream);
int pg_guess_best(const float* logits, int B, int C, const double* table, int M, int maximize, int32_t* best_idx, double* best_value,
                  double* expected, void* stream);
/* What pg_guess_best does with these shapes (host arithmetic, no GPU; PG_EINVAL as pg_guess_best's for the three sizes):
 *   out[0]  the form: 0 = 32 x 32 tiles, 1 = 64 x 64 tiles, taken when ceil(B / 64) * ceil(M / 64) >= 256 workgroups (same bits)
 *   out[1]  rows per tile
 *   out[2]  candidates per tile
 *   out[3]  cells per K step (a C that is no multiple of it is padded with zeros on both sides of the product)
 *   out[4]  workgroups of the product kernel: ceil(B / out[1]) * ceil(M / out[2])
 *   out[5]  bytes of stream-ordered scratch (saturates at 2^31 - 1; 0 when B or M is 0)
 *   out[6]  threads of a workgroup
 *   out[7]  candidate tiles = partials per row that the second pass reads */
int pg_guess_best_plan(int B, int C, int M, int32_t out[8]);

/* ------------------------------------------------------------------------------------------------
 * Calibrated head probabilities (csrc/temper.hip): the statistics a temperature is fitted with, and the calibrated logits.  The
 * reference has no code for it; the contract is this project's own and is restated in tests/_tempref.py.  With beta = 1 / T the
 * calibrated probabilities are softmax(beta * l); the total negative log-likelihood of the labels is convex in beta.
 *
 * pg_temper_stats.  logits DEVICE (N,C) fp32; labels DEVICE (N,) int64; betas HOST K doubles, K 1 .. 16, each finite and positive;
 * row_stats DEVICE (N,K,3) fp64 or NULL; conf DEVICE (N,K) fp64 or NULL; state DEVICE (N,) uint8 or NULL; totals DEVICE (K,3) fp64;
 * counts DEVICE (2,) int64.  Per row n with label y = labels[n], all arithmetic in float64:
 *   m = max_c l[n,c]      a = the first index that attains it (torch.argmax's order)      x_c = (double)l[n,c] - (double)m
 *   per beta_k:  w_c = exp(beta_k * x_c)      Z = sum_c w_c      A = sum_c w_c * x_c      Q = sum_c (w_c * x_c) * x_c
 *   row_stats[n,k,0] = log(Z) - beta_k * x_y                           the negative log-likelihood of the label
 *   row_stats[n,k,1] = A / Z - x_y                                     its first derivative in beta
 *   row_stats[n,k,2] = max(0, Q / Z - (A / Z) * (A / Z))               its second derivative in beta
 *   conf[n,k]        = 1.0 / Z                                         the probability of the argmax
 *   state[n]         = 0: valid, a != y;  1: valid, a == y;  2: invalid
 * A -inf logit is a cell of weight +0.0 (a masked cell): it adds +0.0 to every sum, never 0 * inf.  A row is invalid when its label
 * is outside [0, C), when a logit is NaN or +inf, when every logit is -inf, or when the label's logit is -inf; an invalid row gets NaN
 * row_stats and conf and touches no other row.  x_y is picked by the comparison c == y: no input value forms an address or bounds a
 * loop.
 *   totals[k,j] = sum over the valid rows of row_stats[n,k,j]          an invalid row adds +0.0
 *   counts      = { valid rows, valid rows of state 1 }
 * totals and counts are written whether or not row_stats and state are given (the per-row values then live in stream-ordered
 * scratch, pg_temper_plan's out[3] bytes at the most).
 * Every sum over cells is taken in one fixed order that depends on C only, and the sum over rows in one that depends on N only (no
 * atomics): a row's outputs are the same bits alone, inside any batch, at any position, at any position of its beta inside betas,
 * with any K and with or without the optional outputs.  The order over rows: thread t of 256 adds rows t, t + 256, ... ascending,
 * the 64 lanes of a wave combine as v += v(lane xor o), o = 32 .. 1, and the four waves as (w0 + w1) + (w2 + w3).
 * N == 0 writes zero totals and counts.  PG_EINVAL, naming the argument and before any HIP call, for a negative N (or one above
 * 2^31 - 1), C < 1, K outside 1 .. 16, a beta that is not finite and positive, and a null logits, labels, betas, totals or counts.
 *
 * pg_temper_logits.  out[n,c] = l[n,c] * (float)beta: one correctly rounded fp32 multiplication; -inf, NaN and +inf pass through.
 * logits, out DEVICE (N,C) fp32, out may alias logits.  N == 0 is a no-op.  PG_EINVAL for a negative N, C < 1, a beta that is not
 * finite and positive and a null pointer.
 * ------------------------------------------------------------------------------------------------ */
int pg_temper_stats(const float* logits, int64_t N, int C, const int64_t* labels, const double* betas, int K, double* row_stats,
                    double* conf, uint8_t* state, double* totals, int64_t* counts, void* stream);
int pg_temper_logits(const float* logits, int64_t N, int C, double beta, float* out, void* stream);
/* What pg_temper_stats does with these shapes (host arithmetic, no GPU; PG_EINVAL as pg_temper_stats's for the three sizes):
 *   out[0]  threads of a workgroup; there is one workgroup per row
 *   out[1]  betas per pass over a row: the row is read 1 + ceil(K / out[1]) times (the bits do not depend on the grouping)
 *   out[2]  workgroups of the totals pass: one per (k, j) and one for the counts
 *   out[3]  bytes of stream-ordered scratch of a call without row_stats and state (saturates at 2^31 - 1) */
int pg_temper_plan(int64_t N, int C, int K, int32_t out[4]);

/* ------------------------------------------------------------------------------------------------
 * Bootstrap intervals of evaluation statistics (csrc/bootstrap.hip): resampled means and resampled quantiles of per-item columns.
 * The reference has no code for it; the contract is this project's own and is restated in tests/_bootref.py.
 *
 * The resampling contract.  Draws come from Philox4x32-10 with the multipliers 0xD2511F53 and 0xCD9E8D57 and the key increments
 * 0x9E3779B9 and 0xBB67AE85.  The key is (seed & 0xffffffff, seed >> 32).  For draw j of replicate r the counter is
 * ((j >> 1) & 0xffffffff, (j >> 1) >> 32, r, 0) and the output words are o0 .. o3; an even j uses u = o0 | o1 << 32, an odd j uses
 * u = o2 | o3 << 32.  The item index is idx(r, j) = floor(u * N / 2^64), the high 64 bits of the 128-bit product; its bias is at most
 * N / 2^64.  Known answers (counter / key / output): 0,0,0,0 / 0,0 / 6627e8d5 e169c58d bc57ac4c 9b00dbd8; all ffffffff / all ffffffff /
 * 408f276d 41c83b0e a20bc7c6 6d5451fd; 243f6a88 85a308d3 13198a2e 03707344 / a4093822 299f31d0 / d16cfe09 94fdcceb 5001e420 24126ea1.
 * Pairing: one replicate uses the same N indices for every column, which is what makes differences of statistics paired.  Replicate
 * r's outputs depend on (seed, r, N, the column) only: not on R, not on which other columns are in the call, not on how columns are
 * grouped into workgroups.  The draws are regenerated wherever they are needed; nothing of size R x N is stored.
 *
 * pg_bootstrap_indices.  out DEVICE (count,) int64: out[i] = idx(r, j0 + i).  For tests and the host restatement.  count == 0 is a
 * no-op.  PG_EINVAL for N < 1, r outside 0 .. 2^32 - 1, a negative j0 or count and a null out.
 *
 * pg_bootstrap_means.  x DEVICE (M,N) fp64 row-major, one column of per-item values a row; out DEVICE (R,M) fp64:
 *   out[r,m] = (sum_j x[m, idx(r,j)]) / N
 * The sum is taken in one order that depends on N only: thread t of 256 adds j = t, t + 256, ... ascending, the 64 lanes of a wave
 * combine as v += v(lane xor o), o = 32 .. 1, and the four waves as (w0 + w1) + (w2 + w3).  No atomics.  Non-finite values propagate
 * into the replicates that drew them.
 *
 * pg_bootstrap_quantiles.  rank DEVICE (M,N) int32: rank[m,i] is item i's position in column m sorted ascending (a stable sort: ties
 * by item index); sorted DEVICE (M,N) fp64: that sorted column (no NaN); q HOST Q doubles in [0, 1], Q 1 .. 16; out DEVICE (R,M,Q)
 * fp64.  Per replicate and column the multiset is { rank[m, idx(r,j)] } with order statistics rho_(0) <= ... <= rho_(N-1), and
 *   h = q (N - 1)      lo = floor(h)      t = h - lo      a = sorted[m, rho_(lo)]      b = sorted[m, rho_(min(lo + 1, N - 1))]
 *   out[r,m,k] = t >= 0.5 ? b - (b - a) * (1 - t) : a + (b - a) * t
 * which is numpy.quantile(resampled column, q, method='linear') bit for bit.  Integer ranks make the selection exact: counts of
 * rank >> shift in LDS (integer atomics: the counts do not depend on arrival order), a scan, and further passes over the regenerated
 * draws that resolve the wanted orders' bins.  No input value forms an address: a rank is bounds-checked before it is counted and
 * before it indexes `sorted`; a replicate that draws a rank outside [0, N) gets NaN for that column.
 *
 * Both: R, M and N of any legal value work (the grid walks the (replicate, column group) pairs).  PG_EINVAL, naming the argument and
 * before any HIP call, for N < 1 or N above pg_bootstrap_plan's out[6], R < 1 (or above 2^32: r is a 32-bit counter word), M < 1,
 * Q outside 1 .. 16, a q outside [0, 1] or not finite, and a null pointer.  Asynchronous on `stream`.
 * ------------------------------------------------------------------------------------------------ */
int pg_bootstrap_indices(int64_t N, uint64_t seed, int64_t r, int64_t j0, int64_t count, int64_t* out, void* stream);
int pg_bootstrap_means(const double* x, int M, int64_t N, int64_t R, uint64_t seed, double* out, void* stream);
int pg_bootstrap_quantiles(const int32_t* rank, const double* sorted, int M, int64_t N, int64_t R, uint64_t seed, const double* q, int Q,
                           double* out, void* stream);
/* What the two kernels do with these sizes (host arithmetic, no GPU; PG_EINVAL as theirs for the four sizes):
 *   out[0]  coarse bins a column
 *   out[1]  the shift: a coarse bin holds 2^shift ranks; 0 when N <= out[0]
 *   out[2]  passes of pg_bootstrap_quantiles over a replicate's draws: 1, or 1 + ceil(2 Q / (out[0] >> out[1]))
 *   out[3]  columns per workgroup: the columns that share one pass over the draws (the bits do not depend on the grouping)
 *   out[4]  threads of a workgroup
 *   out[5]  bytes of LDS the counters of a workgroup take
 *   out[6]  the largest supported N
 *   out[7]  workgroups: min(R * ceil(M / out[3]), 2^20), each walking the (replicate, column group) pairs with that stride */
int pg_bootstrap_plan(int64_t N, int64_t R, int M, int Q, int32_t out[8]);

/* ------------------------------------------------------------------------------------------------
 * The refiner's selection at every point of a (topk, temperature, max_km) grid (csrc/refine_sweep.hip; restated in
 * tests/_refitref.py).  Finding the nearest prototype and farthest member of every candidate depends on none of the three settings:
 * one pg_refine_forward / pg_refine_forward_ex call at topk = n_eval leaves the records, and the sweep does every selection from them.
 *
 * pg_refine_sweep.  scratch DEVICE (B,n_eval,SC) fp32, SC = 4 (pg_refine_forward's records) or 12 (pg_refine_forward_ex's; only the
 * four leading floats are read); cand_prob DEVICE (B,k) fp32 or NULL (-> [1,0,0,...]); init_llh DEVICE (B,2) fp64; topks HOST nK
 * int32, each in [1, min(n_eval, 64)]; temps HOST nT floats, each finite and positive; max_kms HOST nR doubles, none NaN (+inf: never
 * veto); choice DEVICE (G,B) uint8 out, G = nK * nT * nR, g = (iK * nT + iT) * nR + iR; veto_km DEVICE (B,n_eval) fp64 out or NULL.
 * Per row b and grid point g the arithmetic is refine_select_kernel's (csrc/refine.hip), operation for operation:
 *   ex_j = expf(score_j / T) in fp32;  sum = the sequential fp32 sum of ex_j over j < topk;  fin_j = cp_j * (ex_j / sum), no max
 *   shift (underflow, 0/0 and NaN behave as they do there);  refined = the first maximum of fin over j < topk, a NaN counting as the
 *   maximum (torch.argmax);  the veto fires when haversine_km(init, the refined candidate's point) > max_km, with the fp32 / fp64
 *   promotion csrc/refine_common.h documents, and then the choice is the first maximum of cp over j < topk.
 * choice[g * B + b]: the chosen candidate in bits 0-5, bit 7 set when the veto fired.  For every g, choice & 63 is the out_choice of a
 * pg_refine_forward call with that (topk, T, max_km) on the same inputs, bit for bit.
 * veto_km[b * n_eval + j]: the veto distance the kernel used for candidate j of row b.
 * Limits: n_eval 1 .. 64 (and <= k when cand_prob is given), nK, nT, nR >= 1, G <= 2^20.  Every violation is PG_EINVAL, names the
 * argument and is raised before any HIP call.  B == 0 is a no-op.  Asynchronous on `stream` (the three host arrays are copied before
 * the call returns).
 *
 * pg_refine_sweep_totals.  choice DEVICE (G,B) uint8; values DEVICE (B,n_eval,V) fp64, V 1 .. 16; totals DEVICE (G,V+2) fp64 out:
 *   totals[g,v]     = sum_b values[b, choice[g,b] & 63, v]
 *   totals[g,V]     = rows with (choice & 63) != 0            totals[g,V+1] = rows whose veto bit is set
 * The sum over rows is taken in one order that depends on B only: thread t of 256 adds b = t, t + 256, ... ascending, the 64 lanes of a
 * wave combine as v += v(lane xor o), o = 32 .. 1, and the four waves as (w0 + w1) + (w2 + w3).  No atomics: a grid point's row of
 * totals is the same bits alone and inside any grid, at any g.  A choice byte whose index is >= n_eval forms no address: it is read
 * as candidate 0 and its grid point gets NaN totals.  PG_EINVAL for B < 0, n_eval outside 1 .. 64, G outside 1 .. 2^20, V outside
 * 1 .. 16 and a null pointer.
 * ------------------------------------------------------------------------------------------------ */
int pg_refine_sweep(const float* scratch, int SC, int B, int n_eval, const float* cand_prob, int k, const double* init_llh,
                    const int32_t* topks, int nK, const float* temps, int nT, const double* max_kms, int nR, uint8_t* choice,
                    double* veto_km, void* stream);
int pg_refine_sweep_totals(const uint8_t* choice, int64_t G, int B, int n_eval, const double* values, int V, double* totals,
                           void* stream);
/* What the two kernels do with these sizes (host arithmetic, no GPU; PG_EINVAL as theirs for the four sizes):
 *   out[0]  rows per workgroup of the selection (one per lane; a workgroup owns one temperature of those rows)
 *   out[1]  bytes of LDS such a workgroup takes
 *   out[2]  row groups, ceil(B / out[0]): the selection launches out[2] * nT workgroups, the totals G
 *   out[3]  bytes of choice, G * B */
int pg_refine_sweep_plan(int B, int n_eval, int64_t G, int V, int64_t out[4]);

/* ------------------------------------------------------------------------------------------------
 * The k nearest rows of an embedding bank, exactly (csrc/knn.hip; restated in tests/_knnref.py).
 *
 * Distance.  For a query q and a bank row x, 1024 fp32 each:
 *     acc = 0.f;  for j = 0 .. 1023 ascending:  t = q[j] - x[j] (one fp32 rounding);  acc = fmaf(t, t, acc);     d2(q, x) = acc
 * One fixed order: a pair's bits depend on nothing else (not on B, n, the pair's position, the launch geometry or the path taken);
 * identical rows give exactly 0.f.  It is the square of the refiner's L2.
 * Result.  Per query the k rows of smallest d2, ascending; ties go to the lower row; a NaN distance ranks after every number (after
 * +inf), ties again by row, and is returned as a NaN.  idx (B,k) int64, d2 (B,k) fp32; positions past min(k, n - excluded) hold
 * -1 / +inf.  exclude (B) int64 or NULL: a row that query b must not return (any value that is no row, -1 for instance: none).
 * The result is ALWAYS that, the top k of the exact distance over the whole bank; how it is reached is mode's business:
 *   mode 0  a 16-bit MFMA pass over x16 keeps the 128 rows of smallest a(q,x) = hn[x] - q16 . x16 per query (never a B x n matrix),
 *           d2 is computed for those and sorted, and a query is CERTIFIED when its k-th d2 is strictly below what any other row could
 *           reach given a rigorous bound on the 16-bit pass's error (derivation: knn.hip); the exact tier, d2 over every
 *           row, is enqueued behind it and its workgroups return at once for certified queries.  No host synchronisation.
 *           certified[b] = 1 where the certificate held, 0 where the exact tier answered.  n <= 128 certifies every query.
 *   mode 1  the exact tier only (bank->x16, hn and stats may be NULL); certified = 1.
 *   mode 2  a diagnostic: what the 16-bit pass and the rerank alone return, with their flags; an uncertified answer may be wrong.
 * pg_knn_prepare: x DEVICE (n,1024) fp32 -> x16 DEVICE (n,1024) fp16 (round to nearest even), hn DEVICE (n) fp32 = 0.5 sum x_j^2
 * (summed in fp64, rounded once), stats DEVICE uint64[4]: [0] the fp32 bits of the largest hn among rows fp16 can hold (xmax^2 / 2),
 * [1] the number of values that are not finite or exceed 65504 in magnitude, [2] the fp32 bits of the largest magnitude fp16 can
 * hold, [3] 0.  A bank with stats[1] != 0 is searched by the exact tier only (mode 2 then returns -1 / +inf and no flag).
 * The stated limit: exact for the embeddings it is given; the encoder's own error is not modelled here.
 * Limits: 1 <= k <= 64, 0 <= B <= 262144, 0 <= n <= 2^31 - 16; B == 0 is a no-op; n == 0 fills -1 / +inf.  x, x16, q 16-byte and the
 * workspace 256-byte aligned.  Every refusal is PG_EINVAL naming the argument, before any HIP call: a null bank, q, idx, d2, a null
 * array of the bank that the mode reads, a null or short workspace (pg_knn_workspace_bytes of the same n, B, k).  certified may be
 * NULL.  Asynchronous on `stream`. */
typedef struct pg_knn_bank {
    const float* x;          /* (n,1024) fp32 */
    const void* x16;         /* (n,1024) fp16, pg_knn_prepare's */
    const float* hn;         /* (n) fp32, pg_knn_prepare's */
    const uint64_t* stats;   /* uint64[4], pg_knn_prepare's */
    int64_t n;
} pg_knn_bank;
int pg_knn_prepare(const float* x, int64_t n, void* x16, float* hn, uint64_t* stats, void* stream);
int pg_knn_workspace_bytes(int64_t n, int B, int k, size_t* bytes);
int pg_knn_search(const pg_knn_bank* bank, const float* q, int B, int k, const int64_t* exclude, int mode, int64_t* idx, float* d2,
                  uint8_t* certified, void* workspace, size_t workspace_bytes, void* stream);
/* What pg_knn_search does with these sizes (host arithmetic, no GPU; PG_EINVAL as pg_knn_search's for the three sizes):
 *   out[0]  K' = 128, the candidates kept per query
 *   out[1]  bank rows per tile of the 16-bit pass (a wave owns 32 consecutive rows of it)
 *   out[2]  queries per workgroup of the 16-bit pass; the bank is streamed once per ceil(B / out[2])
 *   out[3]  spans = workgroups per query tile; span s owns tiles [s out[5], (s + 1) out[5]), those past the last tile own nothing
 *   out[4]  bytes of dynamic LDS of the 16-bit pass
 *   out[5]  tiles per span
 *   out[6]  bank rows per tile of the exact tier
 *   out[7]  spans of the exact tier */
int pg_knn_plan(int64_t n, int B, int k, int32_t out[8]);
/* Forces the number of spans of both passes (0 = the defaults: one per tile up to 256 and 512), so that a small bank exercises several
 * tiles per span, more spans than tiles and the span edges.  The result is the same bits.  PG_EINVAL outside 0 .. 4096.  It changes
 * pg_knn_workspace_bytes: size the workspace after it. */
int pg_tune_knn_spans(int spans);

/* ------------------------------------------------------------------------------------------------
 * Training the geocell head on embeddings (csrc/head_train.hip): one step of cell_layer = Linear(1024 -> C) under the reference's
 * loss (models/super_guessr.py:469-474: CrossEntropyLoss against haversine-smoothed or one-hot targets) and torch.optim.AdamW,
 * as two stream-ordered calls.  Restated in tests/_trainref.py.
 *
 * pg_head_train_loss.  emb DEVICE (B,P,1024) fp32, P = 1 or 4; W DEVICE (C,1024) fp32; bias DEVICE (C,) fp32; centroids DEVICE (C,2)
 * fp64 [lng,lat] (may be NULL without labels_llh); labels_llh DEVICE (B,2) fp64 [lng,lat] or NULL; labels_clf DEVICE (B,) int64 or
 * NULL (read only when labels_llh is NULL; one of the two is needed).  Outputs: xbar DEVICE (B,1024) fp32, g DEVICE (B,C) fp32,
 * loss_rows DEVICE (B,) fp64, logits DEVICE (B,C) fp32 or NULL.
 *   xbar[b,j]  = (((0.f + emb[b,0,j]) + emb[b,1,j]) + ...) * (1.0f / P)
 *   logit[b,c] = the fmaf chain over j = 0 .. 1023 ascending from 0.f of xbar[b,j] * W[c,j], then + bias[c]
 * -- pg_head_forward's arithmetic: the logits a head is trained on are the bits inference computes.  Then per row, in fp64 from the
 * fp32 logits l_c, one workgroup per row:
 *   targets  labels_llh given: d_c = the km pg_haversine_matrix computes for x = labels_llh[b] (fp64), y = centroid[c];
 *                              y_c = exp(-(d_c - min_c d_c) / tau), a non-finite y_c is 0 (pg_smooth_labels)
 *            else:             y_c = (c == labels_clf[b]), a comparison
 *   S = sum_c y_c     m = max_c l_c     e_c = exp(l_c - m)     Z = sum_c e_c     T = sum_c y_c * l_c (fused multiply-add)
 *   loss_rows[b] = S * (m + log(Z)) - T
 *   g[b,c]       = (float)(((S * e_c) / Z - y_c) * grad_scale)
 * (the factor S: smoothed targets do not sum to 1 and CrossEntropyLoss with probability targets does not normalise them).  Every sum
 * over cells is taken in one fixed order that depends on C only (thread-strided ascending, wave butterfly, waves pairwise; no
 * atomics): a row's outputs are the same bits alone, inside any batch, at any position, with the targets in LDS or in scratch.
 * A row whose label point is not finite, or whose labels_clf is outside [0, C), gets loss_rows[b] = NaN and a zero g row: it does not
 * train and touches nothing else.  No input value forms an address or bounds a loop; non-finite embeddings or weights propagate as
 * in torch.  C above pg_head_train_plan's out[2] takes 8 * B * C bytes of stream-ordered scratch.
 * B == 0 is a no-op.  PG_EINVAL, naming the argument and before any HIP call: B < 0, C < 1, P not 1 or 4, tau not finite and
 * positive, grad_scale not finite, a null pointer.
 *
 * pg_head_train_update.  g (B,C), xbar (B,1024): what pg_head_train_loss wrote.  W (C,1024), bias (C,), m_W, v_W (C,1024), m_b, v_b
 * (C,): DEVICE fp32, updated in place.  dW_out (C,1024), db_out (C,): DEVICE fp32 or NULL.
 *   dW[c,j] = the fmaf chain over b = 0 .. B-1 ascending from 0.f of g[b,c] * xbar[b,j];  db[c] = (((0.f + g[0,c]) + g[1,c]) + ...)
 * -- no split over b, no atomics, each (cell tile, column tile) produced whole by one workgroup -- and, from the accumulators,
 * torch.optim.AdamW's update of every element (w, m, v) with its gradient d, each line one correctly rounded fp32 operation or fma:
 *   w1 = w * decay;   m' = fma(omb1, d, b1 * m);   v' = fma(omb2, d * d, b2 * v);   q = sqrt(v') / bc2s + eps;
 *   w' = fma(-step_size, m' / q, w1)
 * with the scalars computed on the host in double and rounded to fp32: decay = 1 - lr * weight_decay, b1 = beta1, omb1 = 1 - beta1,
 * b2 = beta2, omb2 = 1 - beta2, step_size = lr / (1 - beta1^step), bc2s = sqrt(1 - beta2^step), eps.  No gradient buffer exists
 * unless dW_out / db_out is given.  W is written here only, in a launch after the one that read it: stream order is the only
 * synchronisation the two calls need.
 * B == 0 is a no-op.  PG_EINVAL, naming the argument and before any HIP call: B < 0, C < 1, step < 1, lr or eps not finite and
 * positive, a beta outside [0, 1), weight_decay negative or not finite, a null pointer.
 * ------------------------------------------------------------------------------------------------ */
int pg_head_train_loss(const float* emb, int B, int P, const float* W, const float* bias, const double* centroids, int C,
                       const double* labels_llh, const int64_t* labels_clf, double tau, double grad_scale, float* xbar, float* g,
                       double* loss_rows, float* logits, void* stream);
int pg_head_train_update(const float* g, const float* xbar, int B, int C, float* W, float* bias, float* m_W, float* v_W, float* m_b,
                         float* v_b, int64_t step, double lr, double beta1, double beta2, double eps, double weight_decay, float* dW_out,
                         float* db_out, void* stream);
/* What pg_head_train_loss does with C cells (host arithmetic, no GPU; PG_EINVAL for C < 1):
 *   out[0]  where a row's targets live: 0 = LDS, 1 = stream-ordered device scratch (same bits)
 *   out[1]  bytes of dynamic LDS a workgroup asks for (0 in form 1)
 *   out[2]  the largest C of form 0
 *   out[3]  threads of the workgroup; there is one per row */
int pg_head_train_plan(int C, int32_t out[4]);

/* ------------------------------------------------------------------------------------------------
 * The prototype cluster table (reference dataset_creation/prototype/prototype.py:121-149): per-geocell OPTICS graphs, csrc/optics.hip.
 * Cells are packed: cell c owns points cell_off[c] .. cell_off[c+1] and the row-major n x n matrix at element mat_off[c] (n its point
 * count; mat_off[c+1] - mat_off[c] >= n * n).  cell_off and mat_off are HOST arrays of C + 1 int64 -- the calls check them before
 * anything is launched, copy them to the device themselves, and SYNCHRONISE `stream` before they return.  C = 0 is a no-op.
 * ------------------------------------------------------------------------------------------------ */
/* pts DEVICE (N,2) fp64 [lng,lat] degrees, row r = packed point r; out DEVICE fp64: the great-circle distances in km among each cell's
 * own points: element (i, j), i <= j, is pg_haversine_matrix's fp64 arithmetic bit for bit, (j, i) mirrors it (the matrix is exactly
 * symmetric, as the reference's numpy matrix is), and every 0.0 and every pair of identical coordinates (the diagonal, exact
 * duplicates) is written as `zero_as` (the reference: 1e-5, prototype.py:130-133).  One launch for all cells. */
int pg_haversine_blocks(const double* pts, const int64_t* cell_off, const int64_t* mat_off, int C, double zero_as, double* out,
                        void* stream);
/* sklearn.cluster._optics.compute_optics_graph(metric='precomputed', max_eps=inf, min_samples) of every cell, bit for bit (the
 * definition: csrc/optics.hip's header, restated in tests/_opticsref.py).  dist DEVICE fp64 (non-negative, inf allowed); the outputs are
 * DEVICE arrays packed by cell_off from the first cell on: ordering int64 and pred int64 are LOCAL to the cell (0 .. n-1, pred -1 where
 * unset), core and reach fp64.  PG_EINVAL, named and before any launch, for min_samples < 2, a cell of fewer than min_samples points and
 * a cell of more than 32768 points. */
int pg_optics_graph(const double* dist, const int64_t* cell_off, const int64_t* mat_off, int C, int min_samples, int64_t* ordering,
                    double* core, double* reach, int64_t* pred, void* stream);
/* What pg_optics_graph does with a cell of n points under the current knobs (host arithmetic, no GPU; the same refusals):
 *   out[0]  the form of the ordering kernel: 0 = reach / pred / processed flags in LDS, 1 = in global memory (same bits)
 *   out[1]  threads of the cell's workgroup
 *   out[2]  the largest n of form 0
 *   out[3]  the largest n accepted */
int pg_optics_plan(int64_t n, int min_samples, int32_t out[4]);
/* Lowers pg_optics_plan's out[2] (1 .. its default; 0 restores the default) so that tests reach form 1 at small n.  Process-wide. */
int pg_tune_optics_lds_points(int max_points);

/* ------------------------------------------------------------------------------------------------
 * Exact point-in-region lookup (csrc/regions.hip): the device half of `Country_accuracy` and of the geocell labels.
 * Replaces: find_country / country_accuracy (reference evaluation/metrics.py:56-88: geopandas sindex `covered_by`, else `nearest`;
 * shapely `contains`) and generate_cell_labels (preprocessing/dataset_preprocessing.py:60-94, the same lookup on the geocell table).
 * A region is a set of rings under the even-odd rule (multipolygons with holes: a point in a hole is outside, a point on any ring is on
 * the boundary).  The bank is plain CSR; ring closure is stored (first vertex == last vertex), boxes are [min lng, min lat, max lng,
 * max lat].  The two offset arrays exist twice: on the device for the kernels, and on the HOST, where every call checks them before
 * anything is launched (ascending, inside the arrays, rings of at least 2 vertices: PG_EINVAL with a message naming the offender);
 * the kernels additionally clamp every offset they read to the counts below.
 * ------------------------------------------------------------------------------------------------ */
typedef struct pg_region_bank {
    const int64_t* region_off;       /* DEVICE (num_regions + 1): region g owns rings region_off[g] .. region_off[g+1] */
    const int64_t* ring_off;         /* DEVICE (num_rings + 1): ring r owns vertices ring_off[r] .. ring_off[r+1] */
    const double*  xy;               /* DEVICE (num_vertices, 2) fp64 [lng, lat], 16-byte aligned */
    const double*  ring_bbox;        /* DEVICE (num_rings, 4) fp64 */
    const double*  region_bbox;      /* DEVICE (num_regions, 4) fp64 */
    const int64_t* region_off_host;  /* HOST copy of region_off */
    const int64_t* ring_off_host;    /* HOST copy of ring_off */
    int64_t num_regions;
    int64_t num_rings;
    int64_t num_vertices;
} pg_region_bank;
/* States of a (point, region) pair.  The device never guesses: INSIDE (strictly interior) and OUTSIDE are certain; AMBIGUOUS is every
 * pair its fp64 filter cannot certify -- all points on a ring among them -- which the host settles in rational arithmetic
 * (pigeon_amd/regions.py exact_state).  The filter is stated in csrc/regions.hip's header. */
#define PG_REGION_OUTSIDE   0
#define PG_REGION_INSIDE    1
#define PG_REGION_AMBIGUOUS 2
/* pts DEVICE (N,2) fp64 [lng, lat]; start HOST (N) int32 or NULL (= all 0), 0 <= start[i] <= num_regions; cover DEVICE (N) int32 out,
 * state DEVICE (N) uint8 out: the lowest region index >= start[i] whose state is not OUTSIDE, and that state; -1 / 0 if there is none.
 * Asynchronous on `stream`; with a `start` array the call copies it to the device itself and SYNCHRONISES the stream before returning.
 * N = 0 and num_regions = 0 are no-ops (the latter fills cover with -1, state with 0). */
int pg_region_locate(const pg_region_bank* bank, const double* pts, const int32_t* start, int64_t N, int32_t* cover, uint8_t* state,
                     void* stream);
/* The state of point i against region[i]: region HOST (N) int32, -1 <= region[i] < num_regions, -1 gives OUTSIDE; state DEVICE (N)
 * uint8 out.  Copies `region` to the device and SYNCHRONISES the stream before returning. */
int pg_region_classify(const pg_region_bank* bank, const double* pts, const int32_t* region, int64_t N, uint8_t* state, void* stream);
/* The minimum point-to-segment distance (planar, in degrees) over all edges of all regions and the region that has it, ties to the
 * lower index: idx DEVICE (N) int32 out (-1 when the bank has no edge), dist DEVICE (N) fp64 out (+inf then).  The fp64 operations are
 * stated in csrc/regions.hip's header.  Asynchronous on `stream`. */
int pg_region_nearest(const pg_region_bank* bank, const double* pts, int64_t N, int32_t* idx, double* dist, void* stream);
/* How the three calls map points onto the device for this bank under the current knob (host arithmetic on the bank's host arrays, no
 * GPU; the device pointers may be NULL; the same refusals):
 *   out[0]  0 = one wave per point (banks of small rings: geocells), 1 = one workgroup of four waves per point (large rings: countries)
 *   out[1]  threads that share a point's edges (64 / 256)
 *   out[2]  edges of the bank's largest ring
 *   out[3]  the largest out[2] that still gets form 0
 * Results do not depend on the form. */
int pg_region_plan(const pg_region_bank* bank, int32_t out[4]);
/* Sets pg_region_plan's out[3] (0: every bank takes form 1; INT32_MAX: every bank form 0; negative restores the default, 128) so that
 * tests reach both forms with any bank.  Process-wide. */
int pg_tune_region_wave_edges(int max_edges);

/* ------------------------------------------------------------------------------------------------
 * Building-block ops (exported so the parity tests can check every kernel in isolation through the ABI).
 * ------------------------------------------------------------------------------------------------ */
/* `dtype` below is the 16-bit operand/activation format: PG_DTYPE_F16 or PG_DTYPE_BF16.
 * C = A (M,K 16-bit, row stride lda) x W^T (N,K 16-bit) with fp32 accumulation and a fused epilogue:
 *   epi 0: out 16-bit (M,ldc) = acc + bias; columns < qcols additionally scaled by qscale     (QKV)
 *   epi 1: out 16-bit = quick_gelu(acc + bias) = x*sigmoid(1.702x)                            (fc1)
 *   epi 2: out fp32 (M,ldc) += acc + bias  (in-place residual add)                            (out_proj, fc2)
 *   epi 3: patch embed: row = img*576+p -> out fp32 row (img*577+1+p) = acc + aux[(1+p)*N + col] (aux = pos emb)
 *   epi 4: out fp32 = acc + bias (bias may be NULL)                                           (tests)
 * N must be a multiple of 256, K a multiple of 64.  variant selects the tile configuration (0 = default). */
int pg_op_gemm16(int dtype, const void* A, int64_t lda, const void* W, const float* bias, void* out, int64_t ldc,
                 int M, int N, int K, int epi, float qscale, int qcols, const float* aux,
                 int variant, void* stream);
/* Same, with an explicit row stride ldw (elements, >= K, multiple of 8) for W: padded strides keep the rows of an
 * operand panel off the same L2 / memory channels (power-of-two strides camp on a few channels). */
int pg_op_gemm16_ld(int dtype, const void* A, int64_t lda, const void* W, int64_t ldw, const float* bias, void* out,
                    int64_t ldc, int M, int N, int K, int epi, float qscale, int qcols, const float* aux,
                    int variant, void* stream);
/* The "LayerNorm folded into the GEMM" building blocks the encoder uses (persistent kernel only: N % 256 == 0,
 * K % 128 == 0; see csrc/vit.hip):
 *   pg_op_rowstat_cast      x fp32 (rows,1024) -> x16 (rows,1024) 16-bit copy, rowstat (rows,2) = (rstd, mean*rstd)
 *   pg_op_gemm16_resid_stat X (M,ldc) fp32 += A.W^T + bias; x16 (M,ldx) = 16-bit copy of the new rows; statpart
 *                           (N/64, M, 2) fp32 = per-64-column (sum, sum of squares) of the new rows; ldx == ldc
 *   pg_op_rowstat_finalize  statpart -> rowstat (rstd, mean*rstd) over `slots` slices of a 1024-wide row
 *   pg_op_gemm16_ln         out 16-bit = epi(rowstat[m].rstd * acc - rowstat[m].mean_rstd * colsum[n] + bias[n]),
 *                           epi 6 = QKV form (columns < qcols scaled by qscale), 7 = QuickGELU form.
 * Memory contract of the fp32 residual epilogues (epi 2 of pg_op_gemm16, pg_op_gemm16_resid_stat): the last, partial row tile of the
 * persistent kernels READS (never writes) up to 383 rows past row M of X / out -- the row term of those loads rides in the SGPR
 * offset, which the buffer bounds check does not cover.  X must be followed by at least 384 * ldc * 4 readable bytes (inside
 * pg_vit_forward it is: the next buffer of the workspace). */
int pg_op_rowstat_cast(const float* x, void* x16, int dtype, float* rowstat, int64_t rows, float eps, void* stream);
int pg_op_gemm16_resid_stat(int dtype, const void* A, int64_t lda, const void* W, int64_t ldw, const float* bias, float* X,
                            int64_t ldc, void* x16, int64_t ldx, float* statpart, int M, int N, int K, int variant, void* stream);
int pg_op_rowstat_finalize(const float* statpart, int slots, float* rowstat, int64_t rows, float eps, void* stream);
int pg_op_gemm16_ln(int dtype, const void* A, int64_t lda, const void* W, int64_t ldw, const float* bias, const float* colsum,
                    const float* rowstat, void* out, int64_t ldc, int M, int N, int K, int epi, float qscale, int qcols,
                    int variant, void* stream);
/* y = LayerNorm(x) over the last dim (1024), eps, gamma/beta fp32.  x fp32 (rows,1024).
 * out_dtype PG_DTYPE_F16/BF16 -> y 16-bit (rows,1024); PG_DTYPE_F32 -> fp32 (may alias x). */
int pg_op_layernorm(const float* x, const float* gamma, const float* beta, void* y, int out_dtype,
                    int64_t rows, float eps, void* stream);
/* Multi-head attention over the fused QKV buffer (n_images*577, 3072) 16-bit -> out (n_images*577,1024) 16-bit.
 * Q must already carry the factor log2(e)/sqrt(64) (the GEMM epilogue applies it); softmax in fp32. */
int pg_op_attention(int dtype, const void* qkv, void* out, int n_images, void* stream);
/* fp32/fp16/bf16/uint8 NCHW pixels -> 16-bit patch matrix (n_images*576, 640), k = c*196+ky*14+kx, cols 588..639 zero.  PG_DTYPE_U8
 * pixels (16-byte aligned) go through the normalisation table first: the same bits as from the fp32 pixels table[c][byte].
 * out_dtype PG_DTYPE_U8 is refused by name (bytes are a pixel format only). */
int pg_op_im2col(const void* pixels, int pix_dtype, void* out, int out_dtype, int n_images, void* stream);
/* mean over the 577 tokens: x fp32 (n_images,577,1024) -> (n_images,1024). */
int pg_op_token_mean(const float* x, float* out, int n_images, void* stream);
/* fp32 -> fp16/bf16 (round to nearest even; fp16 saturates), n elements. */
int pg_op_cast_f32(const float* x, void* y, int out_dtype, int64_t n, void* stream);
/* Exact-mode building blocks (csrc/precise.hip).  A "triple" of an fp32 row of `cols` values is the fp16 row
 * [hi | lo | hi * 2^-8] of 3 * cols values (hi = fp16(x), lo = fp16(x - hi)); multiplied by weight rows [Wh | Wh | (W - Wh) * 2^8]
 * through pg_op_gemm16 (epi 2 / 3 / 4, K = 3 * cols) it yields the fp32-grade product.
 *   pg_op_x3_split      x fp32 (rows,cols) -> triple (rows, 3 cols); gelu != 0: through QuickGELU first (expf, IEEE division)
 *   pg_op_x3_layernorm  LayerNorm(x fp32 (rows,1024)) -> triple (rows, 3072)
 *   pg_op_attention_f32 fused QKV fp32 (n_images*577, 3072), Q NOT pre-scaled -> softmax(q k^T / 8) v, fp32 (n_images*577, 1024)
 *   pg_op_attention_x3  the same attention with the output written as the triple (n_images*577, 3072) the out-projection reads: what
 *                       pg_op_x3_split makes of pg_op_attention_f32's rows, bit for bit.  PG_ESTATE with pg_tune_exact_attention(1).
 *   pg_op_x3_im2col     fp32/fp16/bf16/uint8 (as pg_op_im2col) NCHW pixels -> the triple of the patch matrix (n_images*576, 3*640): segment s holds its 588 values
 *                       at columns [640 s, 640 s + 588), k = c*196+ky*14+kx, the 52 pad columns of every segment zero
 *   pg_op_sum_parts     dst[i] = (resid ? dst[i] : 0) + ((p0[i] + p1[i]) + p2[i] ...), i < n, part k at parts + k*part_elems; n and
 *                       part_elems multiples of 4, n <= part_elems, 1 <= S <= 8 */
/* Class token + position + pre-LayerNorm in place on the fp32 residual stream x (rows,1024): a row with row % 577 == 0 becomes
 * LN(cls + pos0) whatever x held there, every other row LN(x row); pos0 = row 0 of the position embedding.  With x16 / rowstat (both
 * or neither): also the 16-bit copy (x16_dtype) of the NEW row and its (rstd, mean*rstd), as pg_op_rowstat_cast would give. */
int pg_op_preln(float* x, const float* cls, const float* pos0, const float* gamma, const float* beta, int64_t rows, float eps,
                void* x16, int x16_dtype, float* rowstat, void* stream);
/* S independent products in ONE persistent launch (the exact mode's K-split GEMMs, csrc/vit_precise.hip precise_gemm): part p computes
 * parts[p] (M,N) fp32 = A[:, p*Kp:(p+1)*Kp] x W[:, p*Kp:(p+1)*Kp]^T (+ bias for p = 0); A (M, >= S*Kp) and W (N, >= S*Kp) 16-bit with
 * leading dimensions lda / ldw.  N % 256 == 0, Kp % 128 == 0, 1 <= S <= 8.  Each part is bit-identical to pg_op_gemm16_ld on its slice. */
int pg_op_gemm16_parts(int dtype, const void* A, int64_t lda, const void* W, int64_t ldw, const float* bias, float* parts,
                       int M, int N, int Kp, int S, void* stream);
int pg_op_x3_split(const float* x, void* y3, int64_t rows, int cols, int gelu, void* stream);
int pg_op_x3_layernorm(const float* x, const float* gamma, const float* beta, void* y3, int64_t rows, float eps, void* stream);
int pg_op_attention_f32(const float* qkv, float* out, int n_images, void* stream);
int pg_op_attention_x3(const float* qkv, void* out3, int n_images, void* stream);
int pg_op_x3_im2col(const void* pixels, int pix_dtype, void* out3, int n_images, void* stream);
int pg_op_sum_parts(const float* parts, int S, int64_t part_elems, float* dst, int64_t n, int resid, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PIGEON_HIP_H */
