// gemm_device.h -- what the GEMM kernel files (gemm_bf16 / gemm_pp / gemm_pp6 / gemm_tail / gemm_mid .hip) share apart from the
// epilogues: the argument block, the launchers' declarations, ONE definition of each device helper around the buffer descriptors,
// the LDS DMA and the waits and barriers, and the host-side launch helpers.  The fused epilogues: gemm_epi.h.
#pragma once
#include "common.h"
#include "pigeon_internal.h"

#define BK 64
#define ROWB 128   // bytes per LDS row (BK bf16)

struct GemmArgs {
    const uint16_t* A; int64_t lda;
    const uint16_t* W; int64_t ldw;   // [N][K], row stride ldw elements
    const float* bias;            // [N] or null
    void* out; int64_t ldc;
    int M, N, K;
    float qscale; int qcols;
    const float* aux;             // epi 3: position embedding [577][N]
    int tilesM, tilesN, ntiles;
    int part_tiles;               // tiles of ONE part (tilesM x tilesN); ntiles = ex.parts x part_tiles (EPI_F32, gemm_pp.hip)
    int gn;                       // N tiles per raster group (see tile_coords)
    int stagger;                  // gemm_pp: per-CU start stagger in shader cycles (0 = off; nothing sets it now); -7 arms PG_TS
    int xcd_stagger_ticks;        // persistent kernels: XCD x starts x * ticks / 8 wall-clock ticks (100 MHz) late (0 = off)
    PgGemmExtra ex;               // LayerNorm-fold epilogues (EPI_RESID_STAT / EPI_QKV_LN / EPI_GELU_LN)
};

// The kernels' launchers (gemm_plan.hip's pg_gemm_launch calls them); tilesM/tilesN/ntiles are filled in by the callee.
// gemm_bf16.hip: the one-tile-per-block kernel (variant 8).  pg_gemm_one_tile_bn: its N tile for `variant`, 0 = not a one-tile
// variant.
int pg_gemm_one_tile_bn(int variant);
int pg_gemm_one_tile_launch(int dtype, GemmArgs g, int epi, int variant, hipStream_t s);
// gemm_pp.hip: persistent ping-pong kernel (variants 33, 36)
int pg_gemm_pp_launch(int dtype, GemmArgs g, int epi, int variant, hipStream_t s);
// gemm_pp6.hip: the same kernel with a 384 x 256 block tile, 16-bit-output epilogues and EPI_RESID_STAT (variant 56)
bool pg_gemm_pp6_supported(int epi, int N, int K);
int pg_gemm_pp6_launch(int dtype, GemmArgs g, int epi, hipStream_t s);
// gemm_tail.hip: rows [m_begin, M) of a problem in 32 x 64 one-wave tiles, bit-identical to the persistent kernels (variant 70
// runs a whole problem through it; pg_gemm_launch uses it for the rows that do not fill the persistent kernels' last round)
bool pg_gemm_tail_supported(int epi, int N, int K);
int pg_gemm_tail_launch(int dtype, GemmArgs g, int epi, int m_begin, hipStream_t s);
// gemm_mid.hip (round 6): a whole problem in 128 x 128 one-tile-per-block tiles through a 3-stage LDS ring, bit-identical to the
// persistent kernels (variant 71 forces it; pg_gemm_launch picks it for batches too small to fill the persistent kernels' first round)
bool pg_gemm_mid_supported(int epi, int N, int K);
int pg_gemm_mid_launch(int dtype, GemmArgs g, int epi, hipStream_t s, int m_begin = 0);

// Which family an epilogue belongs to: compile-time in the kernels (`if constexpr (epi_is_ln(EPI))`), run-time in the launchers.
constexpr bool epi_is_ln(int epi) { return epi == EPI_QKV_LN || epi == EPI_GELU_LN; }
constexpr bool epi_is_qkv(int epi) { return epi == EPI_QKV || epi == EPI_QKV_LN; }
constexpr bool epi_is_out16(int epi) { return epi == EPI_QKV || epi == EPI_GELU || epi_is_ln(epi); }
constexpr bool epi_is_resid(int epi) { return epi == EPI_RESID || epi == EPI_RESID_STAT; }

// XCD-level start stagger of the persistent GEMMs.  Every tile of a launch takes the same time, so blocks that start
// together reach their epilogues together: all 256 CUs then hit HBM at once (the fp32 residual read-modify-write of an
// out-proj / fc2 tile is 640 KB per CU, 164 MB per round) while the matrix pipes idle, and during the mainloops HBM idles.
// Delaying XCD x by x/8 of a tile period keeps the 32 CUs of an XCD in lock step -- they share operand panels through
// their L2 at the same K position, which the per-CU stagger tried in round 1 destroyed -- but lets one XCD's epilogue run
// under the other XCDs' mainloops.  The launch ends with the partial last round anyway (its few tiles go to XCD 0, which is
// not delayed), so a spread below one tile period adds no tail.  Wall clock (100 MHz s_memrealtime), immune to DVFS.
__device__ __forceinline__ void xcd_stagger_wait(int ticks) {
    if (ticks <= 0) return;
    const int xcd = blockIdx.x & 7;
    if (xcd == 0) return;
    const unsigned long long until = __builtin_amdgcn_s_memrealtime() + (unsigned long long)ticks * xcd / 8;
    while (__builtin_amdgcn_s_memrealtime() < until) __builtin_amdgcn_s_sleep(16);
}

// Probe build only (-DPIGEON_PROBES): wall-clock stamps (100 MHz) from inside the persistent kernels, blocks 0 and 100, every wave, first 16 tiles:
// buf[((blk * 16 + tile) * 8 + wave) * 12 + slot].  Armed by pg_dbg_timestamps(buf) (gemm_plan.hip), read by tools/epi_timeline.py.
#ifdef PIGEON_PROBES
#define PG_TS(g, iter, wave, slot)                                                                                             \
    do {                                                                                                                       \
        if ((g).stagger == -7 && (blockIdx.x == 0 || blockIdx.x == 100) && (threadIdx.x & 63) == 0 && (iter) < 16)             \
            ((unsigned long long*)(g).aux)[(((blockIdx.x ? 1 : 0) * 16 + (iter)) * 8 + (wave)) * 12 + (slot)] =                \
                __builtin_amdgcn_s_memrealtime();                                                                              \
    } while (0)
#else
#define PG_TS(g, iter, wave, slot) do {} while (0)
#endif

// ---- global -> LDS DMA and buffer descriptors ---------------------------------------------------------------------------------
typedef __attribute__((address_space(3))) void lds_void;

__device__ __forceinline__ void glds16(const void* gptr, void* lds_base_uniform) {
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)gptr,
                                     (__attribute__((address_space(3))) void*)lds_base_uniform, 16, 0, 0);
}
// raw buffer descriptor over [base, base + bytes): accesses past `bytes` fail its bounds check (loads return 0, stores are
// dropped), which is how every kernel handles its M tail.  0x00020000 = word 3 of the descriptor: DATA_FORMAT 32, nothing else set.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const void* base, uint32_t bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), (short)0, (int)bytes, 0x00020000);
}
// 16 bytes per lane through a descriptor straight into LDS (lane-linear from the wave-uniform LDS address)
__device__ __forceinline__ void dma16(__amdgpu_buffer_rsrc_t rsrc, char* lds_wave_uniform, int voff, int soff) {
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (lds_void*)lds_wave_uniform, 16, voff, soff, 0, 0);
}
// Number of valid rows of this wave's `cap`-row share of a tile, given `left` = M - (the share's first row), for the record count
// of a descriptor.  Wave-uniform, but hipcc clamps with v_med3_i32 (there is no scalar med3): without the readfirstlane the count,
// and with it the whole descriptor, sits in VGPRs and every access through it is wrapped in a waterfall loop (2 % of the
// benchmark in round 2; tests/test_asm_audit.py).
__device__ __forceinline__ int wave_valid_rows(int left, int cap) {
    int rv = left; rv = rv < 0 ? 0 : (rv > cap ? cap : rv);
    rv = __builtin_amdgcn_readfirstlane(rv);
    return rv;
}

// Fragment read from LDS as inline asm, for two reasons.  (1) Written as C++ loads, hipcc may put `s_waitcnt vmcnt(0)` in front of
// an LDS read while a direct-to-LDS DMA is in flight -- it assumes the two can alias -- and the prefetch of the next K tile would be
// serialised.  (2) hipcc precomputes and keeps live an address VGPR per (stage, k-step, operand) -- 16 registers gemm_pp6 does not
// have (it spilled 73): here ONE address register per operand is used, the 16-row blocks are immediates (<= 10 KB).
template <int OFF, typename V>
__device__ __forceinline__ void lds_read_b128(V& dst, uint32_t addr) {
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "n"(OFF));
}

// ---- waits and barriers ----------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void wait_lgkm0() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
}
__device__ __forceinline__ void wait_vm0() {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
}
__device__ __forceinline__ void raw_barrier() {
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
}
// An epilogue slab is private to its wave, so only wave-level ordering is needed between its ds_writes and ds_reads (no block
// barrier): LDS operations of one wave execute in order.
__device__ __forceinline__ void wave_lds_fence() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
}

// ---- host side -------------------------------------------------------------------------------------------------------------------
// Raise the kernel's dynamic-LDS limit once (`attr_set`: one flag per kernel instantiation), launch, check.  `attr_what`: the
// text in front of HIP's error string if the attribute cannot be set.
template <typename KFN>
static int launch_kernel(KFN kfn, bool& attr_set, size_t lds, dim3 grid, dim3 block, const GemmArgs& g, hipStream_t s,
                         const char* name, const char* attr_what) {
    if (!attr_set) {
        hipError_t e = hipFuncSetAttribute((const void*)kfn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) { pg_set_error("%s: %s", attr_what, hipGetErrorString(e)); return PG_EHIP; }
        attr_set = true;
    }
    hipLaunchKernelGGL(kfn, grid, block, lds, s, g);
    return pg_check_launch(name);
}
// An operand panel (bm rows of A, bn rows of W) is addressed through ONE buffer descriptor: 32-bit byte offsets.
static inline int pg_gemm_panel_check(const char* kernel, int64_t lda, int64_t ldw, int bm, int bn) {
    if ((int64_t)lda * 2 * bm >= (1ll << 31) || (int64_t)ldw * 2 * bn >= (1ll << 31)) {
        pg_set_error("%s: operand panel exceeds the 2 GB buffer-descriptor range", kernel);
        return PG_EINVAL;
    }
    return PG_OK;
}
