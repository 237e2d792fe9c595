// abi.hip -- the exported C ABI (include/pigeon_hip.h) that belongs to no handle: the thread-local error text every translation unit reports
// through, pg_abi_version, pg_device_count, and the pg_op_* test entry points to single launches of rowops / attention / precise / the GEMMs.
#include "pigeon_internal.h"
#include <cstdarg>
#include <cstdio>

// ------------------------------------------------------------------------------------------------ errors
static thread_local char g_err[512] = "";

void pg_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
int pg_check_launch(const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { pg_set_error("launch of %s failed: %s", what, hipGetErrorString(e)); return PG_EHIP; }
    return PG_OK;
}

extern "C" const char* pg_last_error(void) { return g_err; }
extern "C" int pg_abi_version(void) { return PG_ABI_VERSION; }
extern "C" int pg_device_count(void) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) { pg_set_error("hipGetDeviceCount: %s", hipGetErrorString(e)); return PG_EHIP; }
    return n;
}

// ------------------------------------------------------------------------------------------------ op-level ABI
extern "C" int pg_op_gemm16(int dtype, const void* A, int64_t lda, const void* W, const float* bias, void* out, int64_t ldc,
                            int M, int N, int K, int epi, float qscale, int qcols, const float* aux, int variant,
                            void* stream) {
    if (!A || !W || !out) { pg_set_error("op_gemm16: null argument"); return PG_EINVAL; }
    return pg_gemm_launch(dtype, A, lda, W, K, bias, out, ldc, M, N, K, epi, qscale, qcols, aux, variant, (hipStream_t)stream);
}
extern "C" int pg_op_gemm16_ld(int dtype, const void* A, int64_t lda, const void* W, int64_t ldw, const float* bias, void* out,
                               int64_t ldc, int M, int N, int K, int epi, float qscale, int qcols, const float* aux,
                               int variant, void* stream) {
    if (!A || !W || !out) { pg_set_error("op_gemm16_ld: null argument"); return PG_EINVAL; }
    return pg_gemm_launch(dtype, A, lda, W, ldw, bias, out, ldc, M, N, K, epi, qscale, qcols, aux, variant, (hipStream_t)stream);
}
extern "C" int pg_op_rowstat_cast(const float* x, void* x16, int dtype, float* rowstat, int64_t rows, float eps, void* stream) {
    if (!x || !x16 || !rowstat) { pg_set_error("op_rowstat_cast: null argument"); return PG_EINVAL; }
    return pg_rowstat_cast_launch(x, x16, dtype, rowstat, rows, eps, (hipStream_t)stream);
}
extern "C" int pg_op_rowstat_finalize(const float* statpart, int slots, float* rowstat, int64_t rows, float eps, void* stream) {
    if (!statpart || !rowstat || slots <= 0) { pg_set_error("op_rowstat_finalize: bad argument"); return PG_EINVAL; }
    return pg_rowstat_finalize_launch(statpart, slots, rowstat, rows, eps, (hipStream_t)stream);
}
extern "C" int pg_op_gemm16_resid_stat(int dtype, const void* A, int64_t lda, const void* W, int64_t ldw, const float* bias, float* X,
                                       int64_t ldc, void* x16, int64_t ldx, float* statpart, int M, int N, int K, int variant,
                                       void* stream) {
    if (!A || !W || !X || !x16 || !statpart) { pg_set_error("op_gemm16_resid_stat: null argument"); return PG_EINVAL; }
    PgGemmExtra ex; ex.x16 = x16; ex.ldx = ldx; ex.statpart = statpart;
    return pg_gemm_launch(dtype, A, lda, W, ldw, bias, X, ldc, M, N, K, EPI_RESID_STAT, 1.f, 0, nullptr, variant ? variant : PG_GEMM_V_PP,
                          (hipStream_t)stream, &ex);
}
extern "C" int pg_op_gemm16_ln(int dtype, const void* A, int64_t lda, const void* W, int64_t ldw, const float* bias,
                               const float* colsum, const float* rowstat, void* out, int64_t ldc, int M, int N, int K, int epi,
                               float qscale, int qcols, int variant, void* stream) {
    if (!A || !W || !out || !colsum || !rowstat) { pg_set_error("op_gemm16_ln: null argument"); return PG_EINVAL; }
    if (epi != EPI_QKV_LN && epi != EPI_GELU_LN) { pg_set_error("op_gemm16_ln: epi must be 6 or 7"); return PG_EINVAL; }
    PgGemmExtra ex; ex.colsum = colsum; ex.rowstat = rowstat;
    return pg_gemm_launch(dtype, A, lda, W, ldw, bias, out, ldc, M, N, K, epi, qscale, qcols, nullptr, variant ? variant : PG_GEMM_V_PP,
                          (hipStream_t)stream, &ex);
}
extern "C" int pg_op_layernorm(const float* x, const float* gamma, const float* beta, void* y, int out_dtype,
                               int64_t rows, float eps, void* stream) {
    if (!x || !gamma || !beta || !y) { pg_set_error("op_layernorm: null argument"); return PG_EINVAL; }
    return pg_layernorm_launch(x, gamma, beta, y, out_dtype, rows, eps, (hipStream_t)stream);
}
extern "C" int pg_op_attention(int dtype, const void* qkv, void* out, int n_images, void* stream) {
    if (!qkv || !out) { pg_set_error("op_attention: null argument"); return PG_EINVAL; }
    return pg_attention_launch(dtype, qkv, out, n_images, (hipStream_t)stream);
}
extern "C" int pg_op_im2col(const void* pixels, int pix_dtype, void* out, int out_dtype, int n_images, void* stream) {
    if (!pixels || !out) { pg_set_error("op_im2col: null argument"); return PG_EINVAL; }
    if (out_dtype == PG_DTYPE_U8) { pg_set_error("op_im2col: PG_DTYPE_U8 is a pixel dtype, not an output dtype"); return PG_EINVAL; }
    const float* lut = nullptr;
    if (pix_dtype == PG_DTYPE_U8 && n_images > 0) { const int rc = pg_norm_lut_device(&lut); if (rc) return rc; }
    return pg_im2col_launch(pixels, pix_dtype, out, out_dtype, n_images, (hipStream_t)stream, lut);
}
extern "C" int pg_op_token_mean(const float* x, float* out, int n_images, void* stream) {
    if (!x || !out) { pg_set_error("op_token_mean: null argument"); return PG_EINVAL; }
    return pg_token_mean_launch(x, out, n_images, (hipStream_t)stream);
}
extern "C" int pg_op_cast_f32(const float* x, void* y, int out_dtype, int64_t n, void* stream) {
    if (!x || !y) { pg_set_error("op_cast_f32: null argument"); return PG_EINVAL; }
    return pg_cast_f32_launch(x, y, out_dtype, n, (hipStream_t)stream);
}

extern "C" int pg_op_gemm16_parts(int dtype, const void* A, int64_t lda, const void* W, int64_t ldw, const float* bias, float* parts,
                                  int M, int N, int Kp, int S, void* stream) {
    if (!A || !W || !parts) { pg_set_error("op_gemm16_parts: null argument"); return PG_EINVAL; }
    if (S < 1 || S > 8) { pg_set_error("op_gemm16_parts: 1 <= S <= 8"); return PG_EINVAL; }
    PgGemmExtra ex;
    ex.parts = S; ex.a_part = Kp; ex.w_part = Kp; ex.c_part = (int64_t)M * N;
    return pg_gemm_launch(dtype, A, lda, W, ldw, bias, parts, N, M, N, Kp, EPI_F32, 1.f, 0, nullptr, PG_GEMM_V_PP, (hipStream_t)stream, &ex);
}

// exact-mode building blocks (precise.hip), exported for the parity tests
extern "C" int pg_op_x3_split(const float* x, void* y3, int64_t rows, int cols, int gelu, void* stream) {
    if (!x || !y3) { pg_set_error("op_x3_split: null argument"); return PG_EINVAL; }
    return pg_x3_split_launch(x, y3, rows, cols, gelu, (hipStream_t)stream);
}
extern "C" int pg_op_x3_layernorm(const float* x, const float* gamma, const float* beta, void* y3, int64_t rows, float eps, void* stream) {
    if (!x || !gamma || !beta || !y3) { pg_set_error("op_x3_layernorm: null argument"); return PG_EINVAL; }
    return pg_x3_ln_launch(x, gamma, beta, y3, rows, eps, (hipStream_t)stream);
}
extern "C" int pg_op_attention_f32(const float* qkv, float* out, int n_images, void* stream) {
    if (!qkv || !out) { pg_set_error("op_attention_f32: null argument"); return PG_EINVAL; }
    return pg_attention_f32_launch(qkv, out, n_images, (hipStream_t)stream);
}
extern "C" int pg_op_x3_im2col(const void* pixels, int pix_dtype, void* out3, int n_images, void* stream) {
    if (!pixels || !out3 || n_images < 0) { pg_set_error("op_x3_im2col: bad argument"); return PG_EINVAL; }
    const float* lut = nullptr;
    if (pix_dtype == PG_DTYPE_U8 && n_images > 0) { const int rc = pg_norm_lut_device(&lut); if (rc) return rc; }
    return pg_x3_im2col_launch(pixels, pix_dtype, out3, n_images, (hipStream_t)stream, lut);
}
extern "C" int pg_op_sum_parts(const float* parts, int S, int64_t part_elems, float* dst, int64_t n, int resid, void* stream) {
    if (!parts || !dst) { pg_set_error("op_sum_parts: null argument"); return PG_EINVAL; }
    if (S < 1 || S > 8 || n < 0 || n > part_elems) { pg_set_error("op_sum_parts: 1 <= S <= 8, 0 <= n <= part_elems"); return PG_EINVAL; }
    return pg_sum_parts_launch(parts, S, part_elems, dst, n, resid, (hipStream_t)stream);
}
extern "C" int pg_op_preln(float* x, const float* cls, const float* pos0, const float* gamma, const float* beta, int64_t rows, float eps,
                           void* x16, int x16_dtype, float* rowstat, void* stream) {
    if (!x || !cls || !pos0 || !gamma || !beta) { pg_set_error("op_preln: null argument"); return PG_EINVAL; }
    if ((x16 == nullptr) != (rowstat == nullptr)) { pg_set_error("op_preln: x16 and rowstat go together"); return PG_EINVAL; }
    return pg_preln_launch(x, cls, pos0, gamma, beta, rows, eps, (hipStream_t)stream, x16, x16_dtype, rowstat);
}
extern "C" int pg_op_attention_x3(const float* qkv, void* out3, int n_images, void* stream) {
    if (!qkv || !out3) { pg_set_error("op_attention_x3: null argument"); return PG_EINVAL; }
    return pg_attention_x3out_launch(qkv, out3, n_images, (hipStream_t)stream);
}
