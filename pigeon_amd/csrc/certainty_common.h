// certainty_common.h -- device helpers shared by the kernels that judge a DISCRETE output of a 1024-wide embedding row (head.hip,
// certainty.hip, aux_heads.hip): one wave holds a row as 16 columns per lane, dot products are an fmaf chain per lane plus wave_sum's
// butterfly -- one fixed order per element -- and a decision's tolerance is tol_of (error model: certainty.hip's header).
#pragma once
#include "common.h"
#include <cmath>

#define CT_DIM 1024

// (value desc, index asc); a NaN ranks above every number (torch.argmax / torch.topk semantics), lowest index first
__device__ __forceinline__ bool better(float v, int i, float bv, int bi) {
    const bool vn = v != v, bn = bv != bv;
    if (vn || bn) return vn && (!bn || i < bi);
    return (v > bv) || (v == bv && i < bi);
}

namespace {

__device__ __forceinline__ void ld16(const float* __restrict__ p, int lane, f32x4 (&v)[4]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = *(const f32x4*)(p + i * 256 + lane * 4);
}
__device__ __forceinline__ void zero16(f32x4 (&g)[4]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) g[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
}
// g += coef * row   (row == nullptr or coef == 0: nothing; both are wave-uniform)
__device__ __forceinline__ void axpy16(f32x4 (&g)[4], const float* __restrict__ row, float coef, int lane) {
    if (!row || coef == 0.f) return;
    f32x4 v[4];
    ld16(row, lane, v);
#pragma unroll
    for (int i = 0; i < 4; ++i) g[i] += coef * v[i];
}
__device__ __forceinline__ float dot16(const f32x4 (&a)[4], const f32x4 (&b)[4]) {
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) s = fmaf(a[i][e], b[i][e], s);
    return wave_sum(s);
}
// mean over the P panels of row b (the head's and the refiner's query: super_guessr.py:437, proto_refiner.py:139-140)
__device__ __forceinline__ void panel_mean16(const float* __restrict__ emb, int P, int lane, f32x4 (&ev)[4]) {
    ld16(emb, lane, ev);
    for (int p = 1; p < P; ++p) {
        f32x4 t[4];
        ld16(emb + (int64_t)p * CT_DIM, lane, t);
#pragma unroll
        for (int i = 0; i < 4; ++i) ev[i] += t[i];
    }
    if (P > 1) {
        const float inv = 1.0f / (float)P;
#pragma unroll
        for (int i = 0; i < 4; ++i) ev[i] *= inv;
    }
}

// t = (m - en * gb) / (en * sqrt(g2) / 32).  m is >= 0 by construction (the margin in favour of the decision taken); a NaN anywhere
// makes the decision uncertain (0); a zero gradient means no embedding error can move the margin (+inf).
__device__ __forceinline__ float tol_of(float m, float g2, float gb, float en) {
    if (!(m == m)) return 0.f;
    if (!(g2 > 0.f)) return (g2 == g2) ? INFINITY : 0.f;
    const float num = m - en * gb;
    const float t = num / (en * sqrtf(g2) * (1.0f / 32.0f));
    return (t == t) ? t : 0.f;
}

struct MinTol {
    float t; int code;
    __device__ __forceinline__ void take(float x, int c) { if (x < t) { t = x; code = c; } }
};

}  // namespace
