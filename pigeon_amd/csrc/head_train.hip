// head_train.hip -- one training step of the geocell head cell_layer = Linear(1024 -> C) on precomputed embeddings:
// pg_head_train_loss (panel mean, logits, per-row loss and gradient) and pg_head_train_update (weight gradient with AdamW as its
// epilogue).  Contract: include/pigeon_hip.h; restated in tests/_trainref.py.  Replaces, for this one layer, the reference's
// models/super_guessr.py:437,447,469-474 followed by loss.backward() and torch.optim.AdamW.step() (training/train_eval_loop.py:216-223).
//
// pg_head_train_loss, three kernels on one stream:
//   1. xbar[b,j]  = (((0.f + e[b,0,j]) + e[b,1,j]) + ...) * (1.0f / P)                    head_logits_kernel's panel mean (head.hip)
//   2. logit[b,c] = fmaf chain over j = 0 .. 1023 ascending from 0.f of xbar[b,j] * W[c,j], then + bias[c]: head_logits_kernel's
//      arithmetic, evaluated by v_mfma_f32_32x32x2_f32, whose K loop IS that chain bit for bit (D = fma(a_k1, b_k1, fma(a_k0, b_k0, C)),
//      one rounding per product).  The logits go into the `g` buffer (and into `logits` when the caller asks for them).
//   3. one workgroup of 256 threads per row, fp64 from the fp32 logits l_c:
//        targets   labels_llh given:  d_c = pg_haversine_km<double>(label_b, centroid_c)   (haversine.h: pg_haversine_matrix's function)
//                                     y_c = exp(-(d_c - min_c d_c) / tau), a non-finite y_c is 0   (pg_smooth_labels)
//                  else:              y_c = (c == labels_clf[b]) -- a comparison, the label never forms an address
//        S = sum y_c,  m = max l_c,  e_c = exp(l_c - m),  Z = sum e_c,  T = sum fma(y_c, l_c, .)
//        loss_rows[b] = S * (m + log(Z)) - T
//        g[b,c]       = (float)(((S * e_c) / Z - y_c) * grad_scale)                        (e_c is evaluated a second time, same bits)
//      Every sum over cells is row_block.h's one summation order: it depends on C only, not on B or the row's position.  The y_c are
//      the cells that row_block.h keeps in LDS or in scratch.
//      A row whose label point is not finite, or whose labels_clf is outside [0, C), gets loss_rows[b] = NaN and a zero g row and
//      touches nothing else.  No input value forms an address or bounds a loop.  Non-finite logits propagate as in torch (NaN).
//
// pg_head_train_update, one kernel:
//   dW[c,j] = fmaf chain over b = 0 .. B-1 ascending from 0.f of g[b,c] * xbar[b,j], again as the K loop of v_mfma_f32_32x32x2_f32;
//   db[c]   = (((0.f + g[0,c]) + g[1,c]) + ...), fp32.  No split over b, no atomics: each (cell tile, column tile) of the gradient
//   is produced whole by one workgroup (rows past B are staged as zeros: fma(0, 0, acc) = acc, and acc is never -0), and that
//   workgroup applies AdamW to its tile of W, m_W, v_W straight from the accumulators; the workgroups of column tile 0 do the bias.
//   No gradient buffer exists unless dW_out / db_out is given.
//   The update of one element (w, m, v) with gradient d, every operation one correctly rounded fp32 operation, nothing contracted:
//        w1 = w * decay
//        m' = fmaf(omb1, d, b1 * m)
//        v' = fmaf(omb2, d * d, b2 * v)
//        q  = sqrt(v') / bc2s + eps
//        w' = fmaf(-step_size, m' / q, w1)
//   which is torch.optim.AdamW's default (decoupled decay first, then the moments, then the bias-corrected step).  The host computes
//   the scalars in double and passes them rounded to fp32:  decay = 1 - lr * weight_decay,  b1 = beta1,  omb1 = 1 - beta1,  b2 = beta2,
//   omb2 = 1 - beta2,  step_size = lr / (1 - beta1^t),  bc2s = sqrt(1 - beta2^t),  eps.
//   W is only written here, in a launch after the ones that read it (kernel 2 above): the two calls are stream-ordered, and inside
//   this kernel every element of W, m, v is read and written by one thread only.
#include "common.h"
#include "pigeon_internal.h"
#include "haversine.h"
#include "row_block.h"

#include <cmath>

#define HT_THREADS 256
#define HT_LDS_CELLS row_lds_cells(sizeof(double))   // one target y_c a cell
#define HT_KC 32                                     // reduction rows staged per step

// ------------------------------------------------------------------------------------------------ 1. panel mean
__global__ __launch_bounds__(HT_THREADS) void ht_xbar_kernel(const float* __restrict__ emb, int64_t n, int P, float* __restrict__ xbar) {
    const int64_t i = (int64_t)blockIdx.x * HT_THREADS + threadIdx.x;       // b * 1024 + j
    if (i >= n) return;
    const int64_t b = i >> 10, j = i & (VIT_HIDDEN - 1);
    const float* e = emb + (b * P) * VIT_HIDDEN + j;
    const float invP = 1.0f / (float)P;
    float a = 0.f;
    for (int p = 0; p < P; ++p) a += e[(int64_t)p * VIT_HIDDEN];
    xbar[i] = a * invP;
}

// ------------------------------------------------------------------------------------------------ 2. logits
// out[b,c] = chain_j(xbar[b,j] * W[c,j]) + bias[c].  Workgroup tile 64T x 64T, wave tile 32T x 32T (T x T MFMA accumulators); both
// operands are contiguous along the reduction index and staged [row][k], 33 floats a row.
template <int T>
__global__ __launch_bounds__(HT_THREADS) void ht_logits_kernel(const float* __restrict__ xbar, const float* __restrict__ W,
                                                               const float* __restrict__ bias, int B, int C, float* __restrict__ out) {
    constexpr int TILE = 64 * T;
    __shared__ float Xs[TILE][HT_KC + 1];
    __shared__ float Ws[TILE][HT_KC + 1];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c0 = blockIdx.x * TILE, b0 = blockIdx.y * TILE;
    const int wb = (wave & 1) * 32 * T, wc = (wave >> 1) * 32 * T;
    f32x16 acc[T][T];
#pragma unroll
    for (int i = 0; i < T; ++i)
#pragma unroll
        for (int j = 0; j < T; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    const int sk = tid & 31, sr = tid >> 5;             // staging: 32 consecutive k of one row per half wave
    // the next step's operands travel in registers while this step's MFMAs run
    float px[8 * T], pw[8 * T];
#pragma unroll
    for (int i = 0; i < 8 * T; ++i) {
        const int r = sr + 8 * i;
        px[i] = (b0 + r < B) ? xbar[(int64_t)(b0 + r) * VIT_HIDDEN + sk] : 0.f;
        pw[i] = (c0 + r < C) ? W[(int64_t)(c0 + r) * VIT_HIDDEN + sk] : 0.f;
    }
    for (int k0 = 0; k0 < VIT_HIDDEN; k0 += HT_KC) {
#pragma unroll
        for (int i = 0; i < 8 * T; ++i) {
            Xs[sr + 8 * i][sk] = px[i];
            Ws[sr + 8 * i][sk] = pw[i];
        }
        __syncthreads();
        if (k0 + HT_KC < VIT_HIDDEN) {
#pragma unroll
            for (int i = 0; i < 8 * T; ++i) {
                const int r = sr + 8 * i;
                px[i] = (b0 + r < B) ? xbar[(int64_t)(b0 + r) * VIT_HIDDEN + k0 + HT_KC + sk] : 0.f;
                pw[i] = (c0 + r < C) ? W[(int64_t)(c0 + r) * VIT_HIDDEN + k0 + HT_KC + sk] : 0.f;
            }
        }
#pragma unroll
        for (int kk = 0; kk < HT_KC / 2; ++kk) {
            const int k = 2 * kk + (lane >> 5);
            float a[T], w[T];
#pragma unroll
            for (int i = 0; i < T; ++i) a[i] = Xs[wb + 32 * i + (lane & 31)][k];
#pragma unroll
            for (int j = 0; j < T; ++j) w[j] = Ws[wc + 32 * j + (lane & 31)][k];
#pragma unroll
            for (int i = 0; i < T; ++i)
#pragma unroll
                for (int j = 0; j < T; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], w[j], acc[i][j], 0, 0, 0);
        }
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < T; ++i)
#pragma unroll
        for (int j = 0; j < T; ++j) {
            const int c = c0 + wc + 32 * j + (lane & 31);
            if (c >= C) continue;
            const float bc = bias[c];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int b = b0 + wb + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                if (b < B) out[(int64_t)b * C + c] = acc[i][j][r] + bc;
            }
        }
}

// ------------------------------------------------------------------------------------------------ 3. rows
template <bool GLOBAL>
__global__ __launch_bounds__(HT_THREADS) void ht_row_kernel(float* __restrict__ g, int C, const double* __restrict__ centroids,
                                                            const double* __restrict__ labels_llh, const int64_t* __restrict__ labels_clf,
                                                            double tau, double grad_scale, double* __restrict__ loss_rows,
                                                            float* __restrict__ logits_out, double* __restrict__ scratch) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) double ht_cells[];
    __shared__ double red[4][3];
    __shared__ float redmax[4];
    __shared__ double redmin[4];
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x;
    double* y = GLOBAL ? scratch + b * (int64_t)C : ht_cells;
    float* row = g + b * (int64_t)C;
    float* lout = logits_out ? logits_out + b * (int64_t)C : nullptr;
    const bool smooth = labels_llh != nullptr;
    double plng = 0.0, plat = 0.0;
    int64_t lab = -1;
    bool bad;                                          // uniform: a property of the row
    if (smooth) {
        plng = labels_llh[2 * b]; plat = labels_llh[2 * b + 1];
        bad = !(fabs(plng) < INFINITY && fabs(plat) < INFINITY);
    } else {
        lab = labels_clf[b];
        bad = lab < 0 || lab >= (int64_t)C;
    }
    if (bad) {                                         // such a row does not train
        for (int c = tid; c < C; c += HT_THREADS) {
            if (lout) lout[c] = row[c];
            row[c] = 0.f;
        }
        if (tid == 0) loss_rows[b] = NAN;
        return;
    }
    // a. row maximum of the logits; distances and their minimum
    float mx = -INFINITY;
    double dmin = INFINITY;
    for (int c = tid; c < C; c += HT_THREADS) {
        const float l = row[c];
        if (lout) lout[c] = l;
        mx = l > mx ? l : mx;
        if (smooth) {
            const double d = pg_haversine_km<double>(plng, plat, centroids[2 * (int64_t)c], centroids[2 * (int64_t)c + 1]);
            y[c] = d;
            dmin = d < dmin ? d : dmin;
        }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const float om = __shfl_xor(mx, o, 64);
        const double od = __shfl_xor(dmin, o, 64);
        mx = om > mx ? om : mx;
        dmin = od < dmin ? od : dmin;
    }
    if ((tid & 63) == 0) { redmax[tid >> 6] = mx; redmin[tid >> 6] = dmin; }
    __syncthreads();
    mx = -INFINITY; dmin = INFINITY;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        mx = redmax[w] > mx ? redmax[w] : mx;
        dmin = redmin[w] < dmin ? redmin[w] : dmin;
    }
    const double m = (double)mx;
    // b. targets; S, Z, T
    double acc[3] = {0.0, 0.0, 0.0};
    for (int c = tid; c < C; c += HT_THREADS) {
        const double l = (double)row[c];
        double yc;
        if (smooth) {
            yc = exp(-(y[c] - dmin) / tau);            // own element: written by this thread in pass a
            if (!(fabs(yc) < INFINITY)) yc = 0.0;
        } else {
            yc = ((int64_t)c == lab) ? 1.0 : 0.0;
        }
        y[c] = yc;
        acc[0] += yc;
        acc[1] += exp(l - m);
        acc[2] = fma(yc, l, acc[2]);
    }
    block_sum(acc, red);
    const double S = acc[0], Z = acc[1];
    if (tid == 0) loss_rows[b] = S * (m + log(Z)) - acc[2];
    // c. gradient over the logits, in place
    for (int c = tid; c < C; c += HT_THREADS) {
        const double e = exp((double)row[c] - m);
        row[c] = (float)(((S * e) / Z - y[c]) * grad_scale);
    }
}

// ------------------------------------------------------------------------------------------------ update
struct HtAdam { float decay, b1, omb1, b2, omb2, step_size, bc2s, eps; };

__device__ __forceinline__ void ht_adamw(float& w, float& m, float& v, float d, const HtAdam& A) {
#pragma clang fp contract(off)
    const float w1 = w * A.decay;
    m = fmaf(A.omb1, d, A.b1 * m);
    v = fmaf(A.omb2, d * d, A.b2 * v);
    const float q = __fdiv_rn(__fsqrt_rn(v), A.bc2s) + A.eps;
    w = fmaf(-A.step_size, __fdiv_rn(m, q), w1);
}

// dW tile (cells c0 .. c0 + 64T) x (columns j0 .. j0 + 64T) = sum over b of g[b,c] * xbar[b,j].  Both operands have the reduction
// index as their ROW: staged [b][element], 64T + 32 floats a row (the two half waves of an operand read land in different banks).
template <int T>
__global__ __launch_bounds__(HT_THREADS) void ht_update_kernel(const float* __restrict__ g, const float* __restrict__ xbar, int B, int C,
                                                               float* __restrict__ W, float* __restrict__ bias, float* __restrict__ mW,
                                                               float* __restrict__ vW, float* __restrict__ mb, float* __restrict__ vb,
                                                               HtAdam A, float* __restrict__ dW_out, float* __restrict__ db_out) {
    constexpr int TILE = 64 * T, LD = TILE + 32;
    __shared__ float Gs[HT_KC][LD];
    __shared__ float Xs[HT_KC][LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c0 = blockIdx.x * TILE, j0 = blockIdx.y * TILE;
    const int wc = (wave & 1) * 32 * T, wj = (wave >> 1) * 32 * T;
    f32x16 acc[T][T];
#pragma unroll
    for (int i = 0; i < T; ++i)
#pragma unroll
        for (int j = 0; j < T; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    const int se = tid & (TILE - 1), sr = tid / TILE;   // staging: TILE consecutive elements of one row
    constexpr int RSTEP = HT_THREADS / TILE;
    const bool do_bias = blockIdx.y == 0 && tid < TILE;
    float db = 0.f;
    // the next step's operands travel in registers while this step's MFMAs run
    float pg[HT_KC / RSTEP], px[HT_KC / RSTEP];
    const bool cell_in = c0 + se < C;
#pragma unroll
    for (int i = 0; i < HT_KC / RSTEP; ++i) {
        const int r = sr + RSTEP * i;
        const bool in = r < B;
        pg[i] = (in && cell_in) ? g[(int64_t)r * C + c0 + se] : 0.f;
        px[i] = in ? xbar[(int64_t)r * VIT_HIDDEN + j0 + se] : 0.f;
    }
    for (int kb = 0; kb < B; kb += HT_KC) {
#pragma unroll
        for (int i = 0; i < HT_KC / RSTEP; ++i) {
            Gs[sr + RSTEP * i][se] = pg[i];
            Xs[sr + RSTEP * i][se] = px[i];
        }
        __syncthreads();
        if (kb + HT_KC < B) {
#pragma unroll
            for (int i = 0; i < HT_KC / RSTEP; ++i) {
                const int r = kb + HT_KC + sr + RSTEP * i;
                const bool in = r < B;
                pg[i] = (in && cell_in) ? g[(int64_t)r * C + c0 + se] : 0.f;
                px[i] = in ? xbar[(int64_t)r * VIT_HIDDEN + j0 + se] : 0.f;
            }
        }
#pragma unroll
        for (int kk = 0; kk < HT_KC / 2; ++kk) {
            const int k = 2 * kk + (lane >> 5);
            float a[T], x[T];
#pragma unroll
            for (int i = 0; i < T; ++i) a[i] = Gs[k][wc + 32 * i + (lane & 31)];
#pragma unroll
            for (int j = 0; j < T; ++j) x[j] = Xs[k][wj + 32 * j + (lane & 31)];
#pragma unroll
            for (int i = 0; i < T; ++i)
#pragma unroll
                for (int j = 0; j < T; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], x[j], acc[i][j], 0, 0, 0);
        }
        if (do_bias) {                                 // rows past B hold +0: db + 0 = db, and db is never -0
#pragma unroll
            for (int r = 0; r < HT_KC; ++r) db += Gs[r][tid];
        }
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < T; ++i)
#pragma unroll
        for (int j = 0; j < T; ++j) {
            const int col = j0 + wj + 32 * j + (lane & 31);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int c = c0 + wc + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                if (c >= C) continue;
                const int64_t idx = (int64_t)c * VIT_HIDDEN + col;
                const float d = acc[i][j][r];
                if (dW_out) dW_out[idx] = d;
                float w = W[idx], m = mW[idx], v = vW[idx];
                ht_adamw(w, m, v, d, A);
                W[idx] = w; mW[idx] = m; vW[idx] = v;
            }
        }
    if (do_bias && c0 + tid < C) {
        const int c = c0 + tid;
        if (db_out) db_out[c] = db;
        float w = bias[c], m = mb[c], v = vb[c];
        ht_adamw(w, m, v, db, A);
        bias[c] = w; mb[c] = m; vb[c] = v;
    }
}

// ------------------------------------------------------------------------------------------------ host
// tiles of 128 x 128 once they fill the device twice over, else 64 x 64: the same chain per element either way
static bool ht_big_tiles(int64_t rows, int64_t cols) { return ((rows + 127) / 128) * ((cols + 127) / 128) >= 512; }

static bool ht_pos(double v) { return std::isfinite(v) && v > 0.0; }

extern "C" int pg_head_train_plan(int C, int32_t out[4]) {
    return row_cells_plan("head_train_plan", C, HT_LDS_CELLS, sizeof(double), HT_THREADS, out);
}

extern "C" int pg_head_train_loss(const float* emb, int B, int P, const float* W, const float* bias, const double* centroids, int C,
                                  const double* labels_llh, const int64_t* labels_clf, double tau, double grad_scale, float* xbar,
                                  float* g, double* loss_rows, float* logits, void* stream) {
    if (B < 0) { pg_set_error("head_train_loss: B = %d", B); return PG_EINVAL; }
    if (C < 1) { pg_set_error("head_train_loss: C must be at least 1 (got %d)", C); return PG_EINVAL; }
    if (P != 1 && P != 4) { pg_set_error("head_train_loss: P must be 1 or 4 (got %d)", P); return PG_EINVAL; }
    if (!ht_pos(tau)) { pg_set_error("head_train_loss: tau = %g must be finite and positive", tau); return PG_EINVAL; }
    if (!std::isfinite(grad_scale)) { pg_set_error("head_train_loss: grad_scale = %g must be finite", grad_scale); return PG_EINVAL; }
    if (B == 0) return PG_OK;                              // nothing to do: the (empty) buffers may be NULL
    PG_NEED("head_train_loss", emb);
    PG_NEED("head_train_loss", W);
    PG_NEED("head_train_loss", bias);
    if (!labels_llh && !labels_clf) { pg_set_error("head_train_loss: null arguments labels_llh and labels_clf (one is needed)"); return PG_EINVAL; }
    if (labels_llh) PG_NEED("head_train_loss", centroids);
    PG_NEED("head_train_loss", xbar);
    PG_NEED("head_train_loss", g);
    PG_NEED("head_train_loss", loss_rows);
    hipStream_t s = (hipStream_t)stream;
    const int64_t n = (int64_t)B * VIT_HIDDEN;
    hipLaunchKernelGGL(ht_xbar_kernel, dim3((unsigned)((n + HT_THREADS - 1) / HT_THREADS)), dim3(HT_THREADS), 0, s, emb, n, P, xbar);
    int rc = pg_check_launch("head_train_loss (panel mean)");
    if (rc) return rc;
    if (ht_big_tiles(B, C))
        hipLaunchKernelGGL(ht_logits_kernel<2>, dim3((C + 127) / 128, (B + 127) / 128), dim3(HT_THREADS), 0, s, xbar, W, bias, B, C, g);
    else
        hipLaunchKernelGGL(ht_logits_kernel<1>, dim3((C + 63) / 64, (B + 63) / 64), dim3(HT_THREADS), 0, s, xbar, W, bias, B, C, g);
    rc = pg_check_launch("head_train_loss (logits)");
    if (rc) return rc;
    return row_cells_launch<ht_row_kernel<false>, ht_row_kernel<true>>(
        "head_train_loss (rows)", "head_train_loss (rows, large C)", B, C, HT_LDS_CELLS, sizeof(double), s,
        [&](auto kernel, size_t lds, void* scratch) {
            hipLaunchKernelGGL(kernel, dim3(B), dim3(HT_THREADS), lds, s, g, C, centroids, labels_llh, labels_clf, tau, grad_scale, loss_rows,
                               logits, (double*)scratch);
        });
}

extern "C" int pg_head_train_update(const float* g, const float* xbar, int B, int C, float* W, float* bias, float* m_W, float* v_W,
                                    float* m_b, float* v_b, int64_t step, double lr, double beta1, double beta2, double eps,
                                    double weight_decay, float* dW_out, float* db_out, void* stream) {
    if (B < 0) { pg_set_error("head_train_update: B = %d", B); return PG_EINVAL; }
    if (C < 1) { pg_set_error("head_train_update: C must be at least 1 (got %d)", C); return PG_EINVAL; }
    if (step < 1) { pg_set_error("head_train_update: step = %lld must be at least 1", (long long)step); return PG_EINVAL; }
    if (!ht_pos(lr)) { pg_set_error("head_train_update: lr = %g must be finite and positive", lr); return PG_EINVAL; }
    if (!ht_pos(eps)) { pg_set_error("head_train_update: eps = %g must be finite and positive", eps); return PG_EINVAL; }
    if (!(beta1 >= 0.0 && beta1 < 1.0)) { pg_set_error("head_train_update: beta1 = %g is outside [0, 1)", beta1); return PG_EINVAL; }
    if (!(beta2 >= 0.0 && beta2 < 1.0)) { pg_set_error("head_train_update: beta2 = %g is outside [0, 1)", beta2); return PG_EINVAL; }
    if (!(std::isfinite(weight_decay) && weight_decay >= 0.0)) {
        pg_set_error("head_train_update: weight_decay = %g must be finite and not negative", weight_decay); return PG_EINVAL;
    }
    if (B == 0) return PG_OK;
    PG_NEED("head_train_update", g);
    PG_NEED("head_train_update", xbar);
    PG_NEED("head_train_update", W);
    PG_NEED("head_train_update", bias);
    PG_NEED("head_train_update", m_W);
    PG_NEED("head_train_update", v_W);
    PG_NEED("head_train_update", m_b);
    PG_NEED("head_train_update", v_b);
    HtAdam A;
    A.decay = (float)(1.0 - lr * weight_decay);
    A.b1 = (float)beta1; A.omb1 = (float)(1.0 - beta1);
    A.b2 = (float)beta2; A.omb2 = (float)(1.0 - beta2);
    A.step_size = (float)(lr / (1.0 - std::pow(beta1, (double)step)));
    A.bc2s = (float)std::sqrt(1.0 - std::pow(beta2, (double)step));
    A.eps = (float)eps;
    hipStream_t s = (hipStream_t)stream;
    if (ht_big_tiles(C, VIT_HIDDEN))
        hipLaunchKernelGGL(ht_update_kernel<2>, dim3((C + 127) / 128, VIT_HIDDEN / 128), dim3(HT_THREADS), 0, s, g, xbar, B, C, W, bias, m_W,
                           v_W, m_b, v_b, A, dW_out, db_out);
    else
        hipLaunchKernelGGL(ht_update_kernel<1>, dim3((C + 63) / 64, VIT_HIDDEN / 64), dim3(HT_THREADS), 0, s, g, xbar, B, C, W, bias, m_W,
                           v_W, m_b, v_b, A, dW_out, db_out);
    return pg_check_launch("head_train_update");
}
