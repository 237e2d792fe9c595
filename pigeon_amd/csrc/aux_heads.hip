// aux_heads.hip -- the auxiliary heads of SuperGuessr(multi_task=True), fp32 end to end, one launch.
//
// Replaces reference models/super_guessr.py:333-338: `multi_task_head` (1024 -> 6 regression outputs), `climate_layer` (1024 -> 28) and
// `month_layer` (1024 -> 12, absent with yfcc) on the pooled embedding (:437 the panel mean), and the two argmaxes the metrics take of
// the climate and month outputs (evaluation/metrics.py:187,198).  Those two are DISCRETE outputs like the geocell top-1, so each gets
// the tolerance of certainty.hip's error model -- the head row of its table, applied to two more classifiers:
//     m = preds[c0] - preds[c],  g = W[c0] - W[c],  t = (m - |e| g.beta) / (|e| |g| / 32)
// minimised over EVERY alternative c of both classifiers (at most 62: there is no "beyond the list" bound here).
//
// One 256-thread block per row.  Wave w computes outputs a = w, w + 4, ...: W[a] 16 columns per lane, an fmaf chain per lane and
// wave_sum's butterfly (dot16) -- one fixed order per element, so a row's bits do not depend on B or on what rides in the batch with
// it.  The A <= 64 outputs meet in LDS; every thread then finds the two argmaxes (first maximum in torch's order: better()), and the
// waves share out the alternatives.  A 128-row step keeps 128 CUs busy with ~12 dot products each for the outputs and ~10 gradient
// rows each for the tolerances; the (A, 1024) weight is 184 KB and stays in L2.
#include "common.h"
#include "pigeon_internal.h"
#include "certainty_common.h"
#include <cfloat>
#include <cmath>

#define AUX_MAX_OUT 64

namespace {

// first maximum of v[0 .. n) in torch's order (NaN above every number, ties to the lowest index); n >= 1
__device__ __forceinline__ int argbest(const float* v, int n) {
    int bi = 0;
    float bv = v[0];
    for (int i = 1; i < n; ++i)
        if (better(v[i], i, bv, bi)) { bv = v[i]; bi = i; }
    return bi;
}

// code: 1 + c  climate class c sets the tolerance;  101 + c  month class c;  0 no alternative (tolerance +inf)
__global__ __launch_bounds__(256) void aux_heads_kernel(const float* __restrict__ emb, int P, const float* __restrict__ W,
                                                        const float* __restrict__ bias, int n_reg, int n_climate, int n_month,
                                                        const float* __restrict__ beta, float* __restrict__ preds,
                                                        int64_t* __restrict__ cls, float* __restrict__ tol, int32_t* __restrict__ code,
                                                        float* __restrict__ row_tol) {
    __shared__ float out[AUX_MAX_OUT];
    __shared__ float red_t[4];
    __shared__ int red_c[4];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int A = n_reg + n_climate + n_month;
    f32x4 ev[4], bv[4];
    panel_mean16(emb + (int64_t)b * P * CT_DIM, P, lane, ev);
    for (int a = wave; a < A; a += 4) {
        f32x4 w[4];
        ld16(W + (int64_t)a * CT_DIM, lane, w);
        const float s = dot16(ev, w) + bias[a];
        if (lane == 0) { out[a] = s; preds[(int64_t)b * A + a] = s; }
    }
    __syncthreads();
    const int o_cl = n_reg, o_mo = n_reg + n_climate;
    const int c0 = n_climate > 0 ? argbest(out + o_cl, n_climate) : -1;
    const int m0 = n_month > 0 ? argbest(out + o_mo, n_month) : -1;
    if (tid == 0) { cls[2 * (int64_t)b] = c0; cls[2 * (int64_t)b + 1] = m0; }

    const float en = sqrtf(dot16(ev, ev));
    if (beta) ld16(beta, lane, bv); else zero16(bv);
    MinTol best; best.t = INFINITY; best.code = 0;
    int task = 0;
    for (int which = 0; which < 2; ++which) {
        const int off = which == 0 ? o_cl : o_mo, n = which == 0 ? n_climate : n_month, win = which == 0 ? c0 : m0;
        for (int c = 0; c < n; ++c) {
            if (c == win) continue;
            if ((task++ & 3) != wave) continue;
            f32x4 g[4];
            zero16(g);
            axpy16(g, W + (int64_t)(off + win) * CT_DIM, 1.f, lane);
            axpy16(g, W + (int64_t)(off + c) * CT_DIM, -1.f, lane);
            best.take(tol_of(out[off + win] - out[off + c], dot16(g, g), dot16(g, bv), en), (which == 0 ? 1 : 101) + c);
        }
    }
    // minimum over the waves; equal tolerances go to the alternative visited first (codes rise in visiting order)
    if (lane == 0) { red_t[wave] = best.t; red_c[wave] = best.code; }
    __syncthreads();
    if (tid == 0) {
        float t = red_t[0];
        int cd = red_c[0];
        for (int w = 1; w < 4; ++w)
            if (red_t[w] < t || (red_t[w] == t && red_c[w] != 0 && (cd == 0 || red_c[w] < cd))) { t = red_t[w]; cd = red_c[w]; }
        tol[b] = t;
        code[b] = cd;
        if (row_tol && t < row_tol[b]) row_tol[b] = t;
    }
}

}  // namespace

extern "C" int pg_aux_heads_forward(const float* emb, int B, int P, const float* W, const float* bias, int n_reg, int n_climate,
                                    int n_month, const float* beta, float* preds, int64_t* cls, float* tol, int32_t* code,
                                    float* row_tol, void* stream) {
    if (B < 0) { pg_set_error("aux_heads: B = %d", B); return PG_EINVAL; }
    if (n_reg < 0 || n_climate < 0 || n_month < 0) {
        pg_set_error("aux_heads: negative output count (n_reg=%d n_climate=%d n_month=%d)", n_reg, n_climate, n_month); return PG_EINVAL;
    }
    if (n_reg > AUX_MAX_OUT || n_climate > AUX_MAX_OUT || n_month > AUX_MAX_OUT || n_reg + n_climate + n_month > AUX_MAX_OUT) {
        pg_set_error("aux_heads: n_reg + n_climate + n_month = %d + %d + %d outputs, at most %d are implemented", n_reg, n_climate,
                     n_month, AUX_MAX_OUT);
        return PG_EINVAL;
    }
    if (n_reg + n_climate + n_month == 0) { pg_set_error("aux_heads: no outputs (n_reg = n_climate = n_month = 0)"); return PG_EINVAL; }
    if (P < 1) { pg_set_error("aux_heads: bad P=%d", P); return PG_EINVAL; }
    if (B == 0) return PG_OK;                              // an empty batch is a no-op: its (empty) buffers may be NULL
    if (!emb || !W || !bias || !preds || !cls || !tol || !code) { pg_set_error("aux_heads: null pointer argument"); return PG_EINVAL; }
    hipLaunchKernelGGL(aux_heads_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, emb, P, W, bias, n_reg, n_climate, n_month, beta,
                       preds, cls, tol, code, row_tol);
    return pg_check_launch("aux_heads");
}
