// attribution.hip -- patch attribution: each geocell logit (or logit difference) as an exact sum over tokens.
//
// The embedding is the plain mean of the 577 rows of last_hidden_state (reference models/clip_embedder.py:65,
// models/super_guessr.py:398), the panorama head the mean of the P view embeddings through one Linear (:437, :447).  For a
// direction g = W[cell] - W[against] in embedding space therefore
//     logit[cell] - logit[against] = (b[cell] - b[against]) + sum_p sum_t  h[p,t,:] . g / (577 P)
// and this file computes the summands:
//     out[b,p,t,k] = (h[b,p,t,:] . g[b,k,:]) / (float)(577 P),     g[b,k,j] = W[cells[b,k]][j] - W[against[b]][j]   (fp32, one rounding;
//                                                                   W[cells[b,k]][j] itself where there is no `against`)
//
// Mapping.  The kernel is a stream over `hidden` (4 KB per row, read once).  A block of 256 threads owns AT_ROWS = 32 consecutive
// rows of ONE panorama's P * 577 (so that a block has one set of directions; 577 is no multiple of anything, the last block of a
// panorama is short).  It first builds the K directions of its panorama in LDS ([K][1024] fp32, 4 KB each, 64 KB at K = 16), reading
// the 2 K rows of W with 16-byte loads (they are L2-resident: every block of a panorama reads the same ones).  Then a WAVE takes a
// hidden row: lane l loads the four 16-byte pieces at columns 256 i + 4 l (i = 0..3), i.e. a wave-instruction reads 1 KB contiguous;
// two rows per wave are in flight while the previous two are reduced, and a direction read from LDS (ds_read_b128, conflict-free:
// consecutive lanes, consecutive 16 bytes) serves both rows.
//
// Summation order (part of the result; it depends on the column j alone, not on the batch, K, or the position k):
//   lane l:  s_l = 0;  for i = 0..3, for e = 0..3:  s_l = fma(h[256 i + 4 l + e], g[256 i + 4 l + e], s_l)      (16 fused steps)
//   wave:    v = s_l;  for o = 32, 16, 8, 4, 2, 1:   v = v + v(lane xor o)                                        (the butterfly; every
//            lane ends with the same bits, addition being commutative)
//   out = v / (float)(577 P), one IEEE division.
//
// Indices are device data, so the kernel checks them: cells[b,k] outside [0, C) -> that column is NaN on all P * 577 rows of b;
// against[b] outside [0, C) and not -1 -> every column of b is NaN.  A refused index never forms an address (its direction is zeros in
// LDS and W is not read).  Nothing else in `out` changes, and nothing outside `out` is written.
#include "common.h"
#include "pigeon_internal.h"
#include <cmath>

#define AT_ROWS 32                       // hidden rows per block: 8 per wave, two at a time
#define AT_MAXK 16

namespace {

__device__ __forceinline__ void at_ld16(const float* __restrict__ p, int lane, f32x4 (&v)[4]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = *(const f32x4*)(p + i * 256 + lane * 4);
}

// rows_per_b = P * 577 rows of panorama b start at row b * rows_per_b of `hidden`; `chunks` blocks per panorama
__global__ __launch_bounds__(256) void token_attribution_kernel(const float* __restrict__ hidden, int rows_per_b, int chunks,
                                                                const float* __restrict__ W, int C, const int64_t* __restrict__ cells,
                                                                const int64_t* __restrict__ against, int K, float div,
                                                                float* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) float g_lds[];      // [K][1024]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.x / chunks, chunk = blockIdx.x - b * chunks;
    const int r0 = chunk * AT_ROWS + wave * (AT_ROWS / 4);
    const int r_end = min(r0 + AT_ROWS / 4, rows_per_b);               // may be <= r0 in a panorama's last block
    const int64_t base = (int64_t)b * rows_per_b;

    // the first two rows are on their way while the directions are built
    f32x4 x0[4], x1[4];
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < 4; ++i) x0[i] = x1[i] = zero;
    if (r0 < r_end) at_ld16(hidden + (base + r0) * VIT_HIDDEN, lane, x0);
    if (r0 + 1 < r_end) at_ld16(hidden + (base + r0 + 1) * VIT_HIDDEN, lane, x1);

    const int64_t a = against ? against[b] : -1;
    const bool a_none = a == -1;
    const bool a_bad = !a_none && (a < 0 || a >= (int64_t)C);
    unsigned bad = a_bad ? 0xffffu : 0u;                               // bit k: column k of this panorama is NaN
    for (int k = 0; k < K; ++k) {                                      // thread tid writes columns 4 tid .. 4 tid + 3 of direction k
        const int64_t c = cells[(int64_t)b * K + k];
        const bool c_ok = c >= 0 && c < (int64_t)C;
        f32x4 v = zero;
        if (c_ok && !a_bad) {
            v = *(const f32x4*)(W + c * VIT_HIDDEN + tid * 4);
            if (!a_none) v = v - *(const f32x4*)(W + a * VIT_HIDDEN + tid * 4);
        }
        *(f32x4*)(g_lds + k * VIT_HIDDEN + tid * 4) = v;
        if (!c_ok) bad |= 1u << k;
    }
    __syncthreads();

    for (int r = r0; r < r_end; r += 2) {
        f32x4 n0[4], n1[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) n0[i] = n1[i] = zero;
        if (r + 2 < r_end) at_ld16(hidden + (base + r + 2) * VIT_HIDDEN, lane, n0);
        if (r + 3 < r_end) at_ld16(hidden + (base + r + 3) * VIT_HIDDEN, lane, n1);
        float keep0 = 0.f, keep1 = 0.f;
        for (int k = 0; k < K; ++k) {
            f32x4 g[4];
            at_ld16(g_lds + k * VIT_HIDDEN, lane, g);
            float s0 = 0.f, s1 = 0.f;
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    s0 = __fmaf_rn(x0[i][e], g[i][e], s0);
                    s1 = __fmaf_rn(x1[i][e], g[i][e], s1);
                }
            s0 = wave_sum(s0);
            s1 = wave_sum(s1);
            if (lane == k) { keep0 = s0; keep1 = s1; }
        }
        if (lane < K) {                                                // lane k stores column k: K consecutive floats per row
            const bool nan_col = (bad >> lane) & 1u;
            out[(base + r) * K + lane] = nan_col ? NAN : __fdiv_rn(keep0, div);
            if (r + 1 < r_end) out[(base + r + 1) * K + lane] = nan_col ? NAN : __fdiv_rn(keep1, div);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) { x0[i] = n0[i]; x1[i] = n1[i]; }
    }
}

}  // namespace

extern "C" int pg_token_attribution(const float* hidden, int n_images, int P, const float* W, int C, const int64_t* cells,
                                    const int64_t* against, int K, float* out, void* stream) {
    if (n_images < 0) { pg_set_error("token_attribution: n_images = %d", n_images); return PG_EINVAL; }
    if (P < 1 || n_images % P != 0) { pg_set_error("token_attribution: n_images = %d is not a multiple of P = %d (P >= 1)", n_images, P); return PG_EINVAL; }
    if (K < 1 || K > AT_MAXK) { pg_set_error("token_attribution: K = %d directions (1..%d)", K, AT_MAXK); return PG_EINVAL; }
    if (C < 1) { pg_set_error("token_attribution: C = %d", C); return PG_EINVAL; }
    if (n_images == 0) return PG_OK;                       // an empty batch is a no-op: its (empty) buffers may be NULL
    if (!hidden || !W || !cells || !out) { pg_set_error("token_attribution: null pointer argument (hidden, W, cells or out)"); return PG_EINVAL; }
    if (((uintptr_t)hidden | (uintptr_t)W) & 15) { pg_set_error("token_attribution: hidden and W must be 16-byte aligned"); return PG_EINVAL; }
    const int B = n_images / P;
    const int64_t rows_per_b = (int64_t)P * VIT_TOKENS;
    if (rows_per_b > 0x7fffffffLL) { pg_set_error("token_attribution: P = %d views per panorama", P); return PG_EINVAL; }
    const int64_t chunks = (rows_per_b + AT_ROWS - 1) / AT_ROWS;
    if ((int64_t)B * chunks > 0x7fffffffLL) { pg_set_error("token_attribution: n_images = %d exceeds the launch grid", n_images); return PG_EINVAL; }
    const size_t lds = (size_t)K * VIT_HIDDEN * sizeof(float);     // <= 64 KB: inside the default dynamic-LDS limit
    hipLaunchKernelGGL(token_attribution_kernel, dim3((unsigned)(B * chunks)), dim3(256), lds, (hipStream_t)stream, hidden,
                       (int)rows_per_b, (int)chunks, W, C, cells, against, K, (float)(VIT_TOKENS * (int64_t)P), out);
    return pg_check_launch("token_attribution");
}
