// gemm_bf16.hip -- C[M,N] = A[M,K] * W[N,K]^T, 16-bit (fp16 or bf16) operands, fp32 accumulation on MFMA,
// fused epilogues.
//
// Replaces the nn.Linear / Conv2d library GEMMs the reference reaches through transformers
// (modeling_clip.py CLIPAttention.q/k/v/out_proj, CLIPMLP.fc1/fc2, CLIPVisionEmbeddings.patch_embedding),
// SURVEY.md section 2c rows K1,K4,K6,K7,K8 = 91% of the path's FLOPs.
//
// Design (gfx950 / CDNA4, wave64):
//   * v_mfma_f32_32x32x16_{f16,bf16}; both operands are K-contiguous in memory ([M,K] activations, [N,K] weights as
//     nn.Linear stores them) so a lane's fragment is one 16-byte ds_read_b128.
//   * K tile BK = 64 (128-byte rows in LDS).  Tiles are staged global->LDS with the direct-to-LDS DMA
//     (global_load_lds_dwordx4: 64 lanes x 16 B = 8 rows per wave instruction), no VGPR round trip.
//   * LDS image is lane-linear (a DMA constraint), so the bank-conflict swizzle is applied to the SOURCE
//     address: 16-byte chunk c of row r is stored at chunk c ^ ((r>>1)&7).  A ds_read_b128 lane group
//     (16 lanes) then touches 16 distinct 16-byte slots of the 256-byte bank row.
//   * Double-buffered LDS, one barrier per K tile: DMA of tile t+1 is in flight while tile t is multiplied.
//   * The MFMA is issued with the operands swapped (weights as "A", activations as "B") so a lane ends up
//     owning ONE output row m and quads of 4 consecutive columns n: float4-sized pieces that the epilogue
//     transposes through LDS into full-row 16-byte global stores (bf16: 8 columns per lane; fp32: 4).
//   * 1-D grid with a bijective XCD remap; the N tile index runs fastest inside an XCD's chunk so the blocks
//     that share an A row-panel run on the same L2, and the weight matrix stays L2/MALL resident.
//   * M tail: source rows are clamped to M-1 (reads stay in bounds), stores are masked.
#include "common.h"
#include "pigeon_internal.h"

#include "gemm_epi.h"

// Tile rasterisation.  Blocks are first remapped so every XCD owns a contiguous chunk of logical ids (hardware
// places block b on XCD b % 8), then logical ids walk the tile grid in groups of `gn` N-tiles: inside a group
// the N index runs fastest, then M, then the next group.  The gn weight panels of a group (gn x 256 x K) stay
// resident in the XCD's 4 MB L2 while the XCD walks down its rows; an A row-panel is fetched from HBM/MALL once
// per group and shared by the gn blocks that run side by side.
__device__ __forceinline__ void tile_coords(const GemmArgs& g, int& tm, int& tn) {
    const int wg = xcd_remap(blockIdx.x, g.ntiles);
    const int gsz = g.tilesM * g.gn;
    const int grp = wg / gsz, rem = wg - grp * gsz;
    const int gn_here = min(g.gn, g.tilesN - grp * g.gn);
    tm = rem / gn_here;
    tn = grp * g.gn + (rem - tm * gn_here);
}

// ---- LDS-staged epilogue: per wave, one 32 x WTN fp32 slab at a time -------------------------------------------
// The accumulators hold D[n][m] (operands swapped), i.e. lane owns row m = lane&31 and 4-column quads.  Each wave
// parks a 32-row slab in its private LDS region, then re-reads it row-major so that a lane stores 16 contiguous
// bytes (8 x 16-bit or 4 x fp32) and a wave instruction covers whole 128/256-byte row segments.
template <typename T, int EPI, int TM, int TN, int WTM, int WTN>
__device__ __forceinline__ void staged_epilogue(f32x16 (&acc)[TM][TN], const GemmArgs& g, char* smem, int wave, int lane,
                                                int row0 /* first row of this wave's tile */, int col0) {
    constexpr bool OUT16 = epi_is_out16(EPI);                // (this kernel has no LayerNorm-fold epilogues)
    constexpr int ROWPF = WTN + 4;                           // padded slab row, floats (272 B for WTN=64)
    const int lrow = lane & 31, lhalf = lane >> 5;
    float* slab = (float*)(smem + wave * (32 * ROWPF * 4));
    __syncthreads();                                         // every wave is done with the K-loop buffers
    constexpr int CPL = OUT16 ? 8 : 4;                       // columns per lane on the row-major side
    constexpr int LPR = WTN / CPL, RPI = 64 / LPR, ITS = 32 / RPI;
    const int rr = lane / LPR, cc = (lane % LPR) * CPL;
    const int col = col0 + cc;
    f32x4 b_lo = {0.f, 0.f, 0.f, 0.f}, b_hi = {0.f, 0.f, 0.f, 0.f};
    if (g.bias) {
        b_lo = *(const f32x4*)(g.bias + col);
        if (OUT16) b_hi = *(const f32x4*)(g.bias + col + 4);
    }
#pragma unroll
    for (int i = 0; i < TM; ++i) {
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                f32x4 v = {acc[i][j][4 * q], acc[i][j][4 * q + 1], acc[i][j][4 * q + 2], acc[i][j][4 * q + 3]};
                *(f32x4*)(slab + lrow * ROWPF + j * 32 + q * 8 + 4 * lhalf) = v;
            }
        __syncthreads();
#pragma unroll
        for (int it = 0; it < ITS; ++it) {
            const int r = it * RPI + rr;
            const int row = row0 + i * 32 + r;
            const f32x4 lo = *(const f32x4*)(slab + r * ROWPF + cc);
            if (OUT16) {
                const f32x4 hi = *(const f32x4*)(slab + r * ROWPF + cc + 4);
                if (row < g.M) epi_store_bf16x8<T, EPI>(g, row, col, lo, hi, b_lo, b_hi);
            } else {
                if (row < g.M) epi_store_f32x4<EPI>(g, row, col, lo, b_lo);
            }
        }
        __syncthreads();
    }
}

// One K tile (BK = 64 = 4 k-steps of 16) of MFMAs for a wave's TM x TN tiles, fragments software-pipelined (the ds_reads of
// k-step kk+1 are issued before the MFMAs of kk; a_ptr / b_ptr already include the lane's row), and the next tile's
// direct-to-LDS DMAs issued in NDMA/4-sized slices between the k-steps instead of all at once after the barrier: a DMA issue
// can stall its wave for 100+ cycles when the vector-memory queue is backed up, and spreading them lets the other wave of
// the SIMD keep the matrix pipe busy meanwhile.
template <typename T, int TM, int TN, int NDMA>
__device__ __forceinline__ void mma_ktile_dma(f32x16 (&acc)[TM][TN], const char* a_ptr, const char* b_ptr, const int (&xoff)[4],
                                              const uint16_t* const (&src)[NDMA], const int (&ldsoff)[NDMA], char* nxt,
                                              int64_t koff, bool do_dma) {
    static_assert(NDMA % 4 == 0, "DMA count must split over the 4 k-steps");
    constexpr int PER = NDMA / 4;
    typename T::v8 af[2][TM], bfr[2][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i) af[0][i] = *(const typename T::v8*)(a_ptr + i * 32 * ROWB + xoff[0]);
#pragma unroll
    for (int j = 0; j < TN; ++j) bfr[0][j] = *(const typename T::v8*)(b_ptr + j * 32 * ROWB + xoff[0]);
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
        if (kk < 3) {
#pragma unroll
            for (int i = 0; i < TM; ++i)
                af[(kk + 1) & 1][i] = *(const typename T::v8*)(a_ptr + i * 32 * ROWB + xoff[kk < 3 ? kk + 1 : 3]);
#pragma unroll
            for (int j = 0; j < TN; ++j)
                bfr[(kk + 1) & 1][j] = *(const typename T::v8*)(b_ptr + j * 32 * ROWB + xoff[kk < 3 ? kk + 1 : 3]);
        }
        if (do_dma) {
#pragma unroll
            for (int d = 0; d < PER; ++d) glds16(src[kk * PER + d] + koff, nxt + ldsoff[kk * PER + d]);
        }
        __builtin_amdgcn_s_setprio(1);
        // swapped operands: D[n][m] -> lane owns row m = lane&31, columns n = (r&3)+8*(r>>2)+4*(lane>>5)
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
                acc[i][j] = T::mfma(bfr[kk & 1][j], af[kk & 1][i], acc[i][j]);
        __builtin_amdgcn_s_setprio(0);
    }
}

// ================================================================================================================
// Variant 8: 256 x 256 block tile, 2 x 4 waves, 2 LDS stages of (A|W), one __syncthreads per K tile, N-fastest raster.
// (The other tilings -- 128 x 128, 256 x 128, a 3-stage A ring -- and their ablations were removed; see git history.)
// ================================================================================================================
constexpr int OT_BM = 256, OT_BN = 256, OT_WM = 2, OT_WN = 4;

template <typename T, int EPI>
__global__ __launch_bounds__(OT_WM * OT_WN * 64) void gemm_bf16_kernel(GemmArgs g) {
    constexpr int BM = OT_BM, BN = OT_BN, WM = OT_WM, WN = OT_WN;
    constexpr int NW = WM * WN;
    constexpr int WTM = BM / WM, WTN = BN / WN;
    constexpr int TM = WTM / 32, TN = WTN / 32;
    constexpr int STAGE = (BM + BN) * ROWB;
    constexpr int GROUPS = (BM + BN) / 8;        // 8-row DMA groups per stage
    constexpr int LPW = GROUPS / NW;             // DMA instructions per wave per stage
    static_assert(GROUPS % NW == 0, "stage must split evenly over waves");

    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WN, wn = wave % WN;

    int tm, tn;
    tile_coords(g, tm, tn);
    const int m0 = tm * BM, n0 = tn * BN;

    // ---- per-lane DMA source pointers (advance by BK elements per K tile) ----
    const uint16_t* src[LPW];
    int ldsoff[LPW];
#pragma unroll
    for (int i = 0; i < LPW; ++i) {
        const int grp = wave + i * NW;           // 8-row group inside the stage
        const int r = grp * 8 + (lane >> 3);     // row inside the stage image (A rows first, then W rows)
        const int pc = lane & 7;                 // physical 16-byte chunk this lane fills
        const int c = pc ^ ((r >> 1) & 7);       // logical chunk it must fetch (swizzle on the source)
        if (grp * 8 < BM) {
            int row = m0 + r;
            row = row < g.M ? row : g.M - 1;
            src[i] = g.A + (int64_t)row * g.lda + c * 8;
        } else {
            const int row = n0 + (r - BM);
            src[i] = g.W + (int64_t)row * g.ldw + c * 8;
        }
        ldsoff[i] = grp * 8 * ROWB;              // wave-uniform LDS base of this DMA
    }

    // ---- per-lane fragment read offsets ----
    const int lrow = lane & 31;
    const int lhalf = lane >> 5;
    const int sw = (lane >> 1) & 7;              // == ((row>>1)&7) for row = 32*j + lrow
    int xoff[4];
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) xoff[kk] = ((kk * 2 + lhalf) ^ sw) << 4;
    const int a_base = (wm * WTM + lrow) * ROWB;
    const int b_base = (BM + wn * WTN + lrow) * ROWB;

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    const int nt = g.K / BK;

    // prologue: stage tile 0 into buffer 0
#pragma unroll
    for (int i = 0; i < LPW; ++i) glds16(src[i], smem + ldsoff[i]);

    for (int t = 0; t < nt; ++t) {
        // tile t has landed for every wave (the barrier's release carries vmcnt(0) for the in-flight DMA),
        // and every wave is done reading the buffer tile t+1 is about to overwrite.
        __syncthreads();
        const int cur = t & 1;
        mma_ktile_dma<T, TM, TN, LPW>(acc, smem + cur * STAGE + a_base, smem + cur * STAGE + b_base, xoff, src, ldsoff,
                                      smem + (cur ^ 1) * STAGE, (int64_t)(t + 1) * BK, t + 1 < nt);
    }
    staged_epilogue<T, EPI, TM, TN, WTM, WTN>(acc, g, smem, wave, lane, m0 + wm * WTM, n0 + wn * WTN);
}

template <typename T>
static int launch_one_tile(const GemmArgs& g0, int epi, hipStream_t s) {
    GemmArgs g = g0;
    if (g.N % OT_BN != 0 || g.K % BK != 0) { pg_set_error("gemm: N %% %d or K %% 64 != 0 (N=%d K=%d)", OT_BN, g.N, g.K); return PG_EINVAL; }
    g.tilesM = (g.M + OT_BM - 1) / OT_BM;
    g.tilesN = g.N / OT_BN;
    g.ntiles = g.tilesM * g.tilesN;
    g.gn = g.tilesN;                                          // N-fastest raster
    constexpr size_t lds = 2 * (size_t)(OT_BM + OT_BN) * ROWB;
    static_assert(lds == 131072, "the error text below names the size");
    dim3 grid(g.ntiles), block(OT_WM * OT_WN * 64);
#define PG_LAUNCH(E) { static bool a = false; return launch_kernel(gemm_bf16_kernel<T, E>, a, lds, grid, block, g, s, "gemm16", "gemm: set LDS attr (131072 B)"); }
    switch (epi) {
        case EPI_QKV: PG_LAUNCH(EPI_QKV)
        case EPI_GELU: PG_LAUNCH(EPI_GELU)
        case EPI_RESID: PG_LAUNCH(EPI_RESID)
        case EPI_PATCH: PG_LAUNCH(EPI_PATCH)
        case EPI_F32: PG_LAUNCH(EPI_F32)
        default: pg_set_error("gemm: bad epilogue %d", epi); return PG_EINVAL;
    }
#undef PG_LAUNCH
}

// the N tile of the one-tile kernel for `variant`, 0 = not a one-tile variant.  The product library carries ONE one-tile-per-block
// kernel (variant 8): the fallback for shapes the persistent kernels do not take, and the bit-exact reference they are tested against.
int pg_gemm_one_tile_bn(int variant) { return variant == PG_GEMM_V_ONE_TILE ? OT_BN : 0; }

int pg_gemm_one_tile_launch(int dtype, GemmArgs g, int epi, int variant, hipStream_t s) {
    if (variant != PG_GEMM_V_ONE_TILE) { pg_set_error("gemm: variant %d is not a one-tile variant (8)", variant); return PG_EINVAL; }
    if (dtype == PG_DTYPE_F16) return launch_one_tile<T_F16>(g, epi, s);
    if (dtype == PG_DTYPE_BF16) return launch_one_tile<T_BF16>(g, epi, s);
    pg_set_error("gemm: operand dtype must be PG_DTYPE_F16 or PG_DTYPE_BF16 (got %d)", dtype);
    return PG_EINVAL;
}
