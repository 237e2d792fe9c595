// gemm_epi.h -- the fused epilogues of the GEMM kernels: the element arithmetic that all five kernel files share (gemm_bf16 /
// gemm_pp / gemm_pp6 / gemm_tail / gemm_mid .hip) and the 32-row x 64-column slab epilogue of gemm_tail and gemm_mid.
// The argument block and the device / host helpers around it: gemm_device.h.
#pragma once
#include "gemm_device.h"

// QuickGELU x * sigmoid(1.702 x) (modeling_clip.py QuickGELUActivation) as mul, v_exp_f32 (2^x), add, v_rcp_f32, mul:
// the IEEE division of the obvious form expands to ~10 VALU instructions and made the fc1 epilogue cost ~6 us per tile.
__device__ __forceinline__ float quick_gelu(float v) {
    const float e = __builtin_amdgcn_exp2f(-2.4554669595930157f * v);      // exp(-1.702 v); 1.702 * log2(e)
    return v * __builtin_amdgcn_rcpf(1.0f + e);
}

// Packed-fp32 forms (v_pk_fma_f32 / v_pk_mul_f32 / v_pk_add_f32: two IEEE fp32 operations per instruction, bit-identical to the
// scalar ones).  They run at the plain VALU rate when no MFMA stream is active on the CU (tools/pipe_rate.hip: 5 cycles alone, 37
// next to MFMAs -- they share the matrix pipe), which is exactly the situation of a persistent kernel's epilogue: the 16-bit
// epilogues are VALU-bound there (gemm_pp6.hip, tools/epi_timeline.py), so halving their fma / mul / add count is time saved.
typedef float f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f32x2 pk_fma(f32x2 a, f32x2 b, f32x2 c) { return __builtin_elementwise_fma(a, b, c); }
__device__ __forceinline__ f32x2 quick_gelu2(f32x2 v) {
    const f32x2 t = v * -2.4554669595930157f;
    f32x2 e = {__builtin_amdgcn_exp2f(t[0]), __builtin_amdgcn_exp2f(t[1])};
    e = 1.0f + e;
    const f32x2 r = {__builtin_amdgcn_rcpf(e[0]), __builtin_amdgcn_rcpf(e[1])};
    return v * r;
}
// y = acc * rstd + (-(mean rstd) * colsum + c) on 4 columns, as two packed pairs (same two roundings per element as the fmaf form)
__device__ __forceinline__ f32x4 ln_fold4(f32x4 acc, float rstd, float mrs, const f32x4& colsum, const f32x4& c) {
    const f32x2 r2 = {rstd, rstd}, m2 = {-mrs, -mrs};
    const f32x2 a0 = pk_fma(f32x2{acc[0], acc[1]}, r2, pk_fma(m2, f32x2{colsum[0], colsum[1]}, f32x2{c[0], c[1]}));
    const f32x2 a1 = pk_fma(f32x2{acc[2], acc[3]}, r2, pk_fma(m2, f32x2{colsum[2], colsum[3]}, f32x2{c[2], c[3]}));
    return f32x4{a0[0], a0[1], a1[0], a1[1]};
}
__device__ __forceinline__ f32x4 quick_gelu4(f32x4 v) {
    const f32x2 a0 = quick_gelu2(f32x2{v[0], v[1]}), a1 = quick_gelu2(f32x2{v[2], v[3]});
    return f32x4{a0[0], a0[1], a1[0], a1[1]};
}

// ==== ONE definition of the fused epilogue ARITHMETIC for the slab-transposing kernels (gemm_pp / gemm_pp6 / gemm_tail / gemm_mid).  Round 2 kept a hand copy of these expressions in every file and held them together with
// bit-compare tests only; a row's value must not depend on which kernel (persistent tile, tail tile) computed it, so the
// expressions -- including the association order of the row statistics -- live here and nowhere else.  A lane holds 8 outputs of
// one row as two f32x4 (`lo`, `hi`); which columns those are (8 consecutive, or 4k.. and 32+4k.. for EPI_RESID_STAT) is the
// caller's geometry, the arithmetic does not depend on it.

// 16-bit-output epilogues (EPI_QKV, EPI_GELU and their LayerNorm-fold forms): 8 accumulators -> 8 packed 16-bit outputs.
//   plain: y = acc + b;   LN fold: y = rstd * acc - (mean rstd) * colsum + c   (c = beta.W^T + b, s = colsum)
//   QKV:   the Q strip (q_strip: the tile's columns are below qcols -- qcols is a multiple of 8, so a lane's 8 columns are all in
//          or all out) is scaled by qsc; K / V strips skip the multiply;   GELU: QuickGELU.
// (rstd, mrs) must come through registers of their own (callers move each half of the loaded pair through an asm v_mov:
// hipcc, ROCm 7.2, SLP-packs fmas whose multipliers are the two halves of one dwordx2 and drops the op_sel of the high half).
template <typename T, int EPI>
__device__ __forceinline__ u32x4 epi16_finish(f32x4 lo, f32x4 hi, const f32x4& b_lo, const f32x4& b_hi, const f32x4& s_lo,
                                              const f32x4& s_hi, float rstd, float mrs, bool q_strip, float qsc) {
    if constexpr (epi_is_ln(EPI)) {
        lo = ln_fold4(lo, rstd, mrs, s_lo, b_lo);
        hi = ln_fold4(hi, rstd, mrs, s_hi, b_hi);
    } else {
        lo += b_lo; hi += b_hi;
    }
    if constexpr (epi_is_qkv(EPI)) {
        if (q_strip) { lo *= qsc; hi *= qsc; }
    } else {
        lo = quick_gelu4(lo); hi = quick_gelu4(hi);
    }
    u32x4 pk;
    pk[0] = pack16x2<T>(lo[0], lo[1]); pk[1] = pack16x2<T>(lo[2], lo[3]);
    pk[2] = pack16x2<T>(hi[0], hi[1]); pk[3] = pack16x2<T>(hi[2], hi[3]);
    return pk;
}

// fp32 residual epilogues (EPI_RESID, EPI_RESID_STAT): the new residual values of 4 columns
__device__ __forceinline__ f32x4 epi_resid4(f32x4 x, const f32x4& acc, const f32x4& b) {
    x += acc + b;
    return x;
}
// EPI_RESID_STAT: 16-bit copy of 4 new residual values
template <typename T>
__device__ __forceinline__ u32x2 epi_copy16x4(const f32x4& x) {
    u32x2 h;
    h[0] = pack16x2<T>(x[0], x[1]); h[1] = pack16x2<T>(x[2], x[3]);
    return h;
}
// EPI_RESID_STAT: this lane's share (its 8 new values x, y) of the row's partial (sum, sum of squares) over 64 columns -- the
// association order is part of the result; the 8 lanes of a row are then combined by row8_sum below.
__device__ __forceinline__ void epi_stat8(const f32x4& x, const f32x4& y, float& s1, float& s2) {
    s1 = ((x[0] + x[1]) + (x[2] + x[3])) + ((y[0] + y[1]) + (y[2] + y[3]));
    s2 = ((x[0] * x[0] + x[1] * x[1]) + (x[2] * x[2] + x[3] * x[3])) + ((y[0] * y[0] + y[1] * y[1]) + (y[2] * y[2] + y[3] * y[3]));
}
// sum over the 8 lanes (lane & 7 = 0..7) that hold one row, fixed association: pairs, quads, then the two quads
template <int CTRL>
__device__ __forceinline__ float epi_dpp_mov(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, true));
}
__device__ __forceinline__ float row8_sum(float v) {
    v += epi_dpp_mov<0xB1>(v);       // quad_perm [1,0,3,2]
    v += epi_dpp_mov<0x4E>(v);       // quad_perm [2,3,0,1]
    v += epi_dpp_mov<0x141>(v);      // row_half_mirror: lane i <-> 7 - i inside each group of 8
    return v;
}

// Apply the epilogue to 4 consecutive columns [col, col+4) of one output row (fp32-out epilogues).
template <int EPI>
__device__ __forceinline__ void epi_store_f32x4(const GemmArgs& g, int row, int col, f32x4 v, const f32x4& b4) {
    if (EPI == EPI_RESID) {
        float* p = (float*)g.out + (int64_t)row * g.ldc + col;
        f32x4 x = *(const f32x4*)p;
        x += v + b4;
        *(f32x4*)p = x;
    } else if (EPI == EPI_PATCH) {
        const int img = row / VIT_PATCHES, p = row - img * VIT_PATCHES;
        float* o = (float*)g.out + ((int64_t)img * VIT_TOKENS + 1 + p) * g.ldc + col;
        const f32x4 pos = *(const f32x4*)(g.aux + (int64_t)(1 + p) * g.N + col);
        *(f32x4*)o = v + pos;
    } else {  // EPI_F32
        *(f32x4*)((float*)g.out + (int64_t)row * g.ldc + col) = v + b4;
    }
}

// 16-bit-out epilogues on 8 consecutive columns.
template <typename T, int EPI>
__device__ __forceinline__ void epi_store_bf16x8(const GemmArgs& g, int row, int col, f32x4 lo, f32x4 hi,
                                                 const f32x4& b_lo, const f32x4& b_hi) {
    lo += b_lo; hi += b_hi;
    if (EPI == EPI_QKV) {
        if (col < g.qcols) { lo *= g.qscale; hi *= g.qscale; }   // qcols is a multiple of 8
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) { lo[e] = quick_gelu(lo[e]); hi[e] = quick_gelu(hi[e]); }
    }
    u32x4 pk;
    pk[0] = pack16x2<T>(lo[0], lo[1]); pk[1] = pack16x2<T>(lo[2], lo[3]);
    pk[2] = pack16x2<T>(hi[0], hi[1]); pk[3] = pack16x2<T>(hi[2], hi[3]);
    *(u32x4*)((uint16_t*)g.out + (int64_t)row * g.ldc + col) = pk;
}

// ==== The 32-row x 64-column slab epilogue of the kernels that store through plain pointers (gemm_mid.hip: half of a wave's
// 64 x 64; gemm_tail.hip: its whole tile).  The two 16-row accumulator blocks acc0, acc1 (a lane owns row lane & 15 of a 16 x 16 block
// and the 4 consecutive columns 4 (lane >> 4) ..) go through the wave's private LDS slab into row-major pieces -- lane (rr, cc)
// holds 8 columns of rows rr, rr + 8, rr + 16, rr + 24 of the slab, whose first element is (row0, col0) of the problem -- and the
// fused epilogue runs on those: pp_epilogue's geometry (gemm_pp.hip) and the expressions above, so a row's bits do not depend on
// the kernel that computed it.  Rows past M are skipped.  The caller fences (wave_lds_fence) before it writes the slab again.
// gemm_mid calls this function.  gemm_tail.hip still carries the same statements in its kernel body, token for token: called from
// there (the argument block is the kernel parameter itself) hipcc allocates the kernel's registers differently, and the A/B against
// the previous build (profiles/r07/gemm_shared_epilogue_ab.txt) did not stay inside its margin.  A change here is a change there.
constexpr int EPI_SLAB_ROWPF = 64 + 4;                       // slab row in floats (the persistent kernels' padding)
template <typename T, int EPI>
__device__ __forceinline__ void epi_slab32(const GemmArgs& g, float* slab, int lane, int row0, int col0, const f32x4 (&acc0)[4],
                                           const f32x4 (&acc1)[4]) {
    constexpr bool OUT16 = epi_is_out16(EPI);
    constexpr bool LN = epi_is_ln(EPI);
    constexpr bool STAT = (EPI == EPI_RESID_STAT);
    constexpr bool RESID = epi_is_resid(EPI);
    constexpr int ROWPF = EPI_SLAB_ROWPF;
    const int l15 = lane & 15, lq = lane >> 4;
#pragma unroll
    for (int ib = 0; ib < 2; ++ib)
#pragma unroll
        for (int j = 0; j < 4; ++j) *(f32x4*)(slab + (ib * 16 + l15) * ROWPF + j * 16 + 4 * lq) = (ib ? acc1 : acc0)[j];
    wave_lds_fence();

    // EPI_RESID_STAT uses pp_epilogue's split-halves geometry (columns 4k.. and 32 + 4k.. per lane), everything else 8 consecutive
    constexpr int HOFF = STAT ? 32 : 4;
    const int rr = lane >> 3, cc = STAT ? (lane & 7) * 4 : (lane & 7) * 8;
    const int col = col0 + cc;
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
    f32x4 b_lo = zero4, b_hi = zero4, s_lo = zero4, s_hi = zero4;
    if (g.bias) { b_lo = *(const f32x4*)(g.bias + col); b_hi = *(const f32x4*)(g.bias + col + HOFF); }
    if constexpr (LN) { s_lo = *(const f32x4*)(g.ex.colsum + col); s_hi = *(const f32x4*)(g.ex.colsum + col + 4); }
    const float qsc = (epi_is_qkv(EPI) && col < g.qcols) ? g.qscale : 1.f;

#pragma unroll
    for (int it = 0; it < 4; ++it) {
        const int r = it * 8 + rr;
        const int row = row0 + r;
        if (row >= g.M) continue;
        f32x4 lo = *(const f32x4*)(slab + r * ROWPF + cc);
        f32x4 hi = *(const f32x4*)(slab + r * ROWPF + cc + HOFF);
        if constexpr (OUT16) {
            float rstd = 0.f, mrs = 0.f;
            if constexpr (LN) {
                const u32x2 rs = *(const u32x2*)(g.ex.rowstat + (int64_t)row * 2);
                // (the asm moves: see epi16_finish -- hipcc SLP-packs the fmas and broadcasts the wrong half otherwise)
                asm("v_mov_b32 %0, %1" : "=v"(rstd) : "v"(rs[0]));
                asm("v_mov_b32 %0, %1" : "=v"(mrs) : "v"(rs[1]));
            }
            *(u32x4*)((uint16_t*)g.out + (int64_t)row * g.ldc + col) =
                epi16_finish<T, EPI>(lo, hi, b_lo, b_hi, s_lo, s_hi, rstd, mrs, col0 < g.qcols, qsc);
        } else if constexpr (RESID) {
            float* p = (float*)g.out + (int64_t)row * g.ldc + col;
            const f32x4 x = epi_resid4(*(const f32x4*)p, lo, b_lo);
            const f32x4 y = epi_resid4(*(const f32x4*)(p + HOFF), hi, b_hi);
            *(f32x4*)p = x;
            *(f32x4*)(p + HOFF) = y;
            if constexpr (STAT) {
                uint16_t* p16 = (uint16_t*)g.ex.x16 + (int64_t)row * g.ldc + col;
                *(u32x2*)p16 = epi_copy16x4<T>(x);
                *(u32x2*)(p16 + HOFF) = epi_copy16x4<T>(y);
                float s1, s2;
                epi_stat8(x, y, s1, s2);
                s1 = row8_sum(s1);
                s2 = row8_sum(s2);
                if ((lane & 7) == 0) {
                    float* sp = g.ex.statpart + ((int64_t)(col0 / 64) * g.ex.stat_rows + row) * 2;
                    sp[0] = s1; sp[1] = s2;
                }
            }
        } else {                                             // EPI_F32
            float* p = (float*)g.out + (int64_t)row * g.ldc + col;
            *(f32x4*)p = lo + b_lo;
            *(f32x4*)(p + 4) = hi + b_hi;
        }
    }
}
