// fingerprint.hip -- a 128-bit digest of device buffers (pg_fingerprint), the key that ties a stored encoder calibration
// (pigeon_amd/certainty.py: bias vector, rel_tol, force_exact) to the weights it was measured on.  The weights the encoder computes
// with exist only on the device (rounded to 16 bits, LayerNorm-folded and packed by pg_vit_finalize), so the digest is taken there,
// over exactly the buffers pg_vit_forward reads (pg_vit_fingerprint, vit.hip).
//
// THE DEFINITION (stated once; tests/_fpref.py restates it in numpy and must match bit for bit).  All arithmetic is on unsigned
// 64-bit integers, wrapping modulo 2^64; words are little endian.
//   mix(z):            z ^= z >> 30;  z *= 0xBF58476D1CE4E5B9;  z ^= z >> 27;  z *= 0x94D049BB133111EB;  z ^= z >> 31     (splitmix64's finalizer)
//   chunks:            the buffer is read as n = ceil(bytes / 16) chunks of 16 bytes, the last one zero padded; chunk i
//                      (0-based) is two words lo_i (bytes 0..7) and hi_i (bytes 8..15)
//   key:               k_i = mix(seed + i + 1)
//   terms:             a_i = mix(lo_i ^ k_i)        b_i = mix(hi_i ^ rotl(k_i, 32))
//   accumulators:      A = sum_i a_i               B = sum_i b_i                       (empty buffer: A = B = 0)
//   length and seed:   t = mix(seed ^ 0x9E3779B97F4A7C15)
//                      out[0] = mix(A + t + bytes)  out[1] = mix(B + rotl(t, 32) + bytes)
// The sums are wrap-around integer additions: the result does not depend on the grid, on block scheduling or on the order of the
// reduction.  It depends on WHERE a chunk sits (the chunk index is in the key), on every bit, on the seed, and on the byte length
// (15 bytes and the same 15 bytes followed by a zero byte differ).  Not a cryptographic hash: it guards against the wrong file, not
// against an adversary.
//
// Kernels: fingerprint_kernel is grid-stride over the full chunks of a buffer with 16-byte loads (the zero-padded tail chunk is
// assembled byte by byte by one lane), reduces over the wave with shuffles and over the block's four waves through LDS, and writes one
// (A, B) partial per block to a scratch buffer; fingerprint_sum_kernel, one block per buffer, adds the partials.  No atomics.  Both
// take a TABLE of buffers (blockIdx.y / blockIdx.x = buffer): the ~340 parameter buffers of a 24-layer encoder cost two launches.
#include "common.h"
#include "pigeon_internal.h"

#include <vector>

#define FP_THREADS 256
#define FP_MAX_BLOCKS 1024          // blocks per buffer at most (the grid-stride loop covers the rest)
#define FP_CHUNKS_PER_LANE 4        // a buffer gets ceil(full chunks / (FP_THREADS * this)) blocks, at least 1 when it is not empty

namespace {

__host__ __device__ __forceinline__ uint64_t fp_mix(uint64_t z) {
    z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27; z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z;
}
__host__ __device__ __forceinline__ uint64_t fp_rotl32(uint64_t z) { return (z << 32) | (z >> 32); }
__host__ __device__ __forceinline__ void fp_term(uint64_t lo, uint64_t hi, uint64_t seed, uint64_t i, uint64_t& A, uint64_t& B) {
    const uint64_t k = fp_mix(seed + i + 1);
    A += fp_mix(lo ^ k);
    B += fp_mix(hi ^ fp_rotl32(k));
}
// the zero-padded last chunk: `tail` (1..15) bytes at p
__host__ __device__ __forceinline__ void fp_tail_words(const uint8_t* p, int tail, uint64_t& lo, uint64_t& hi) {
    lo = hi = 0;
    for (int j = 0; j < tail; ++j) {
        const uint64_t b = (uint64_t)p[j];
        if (j < 8) lo |= b << (8 * j); else hi |= b << (8 * (j - 8));
    }
}
inline void fp_final(uint64_t A, uint64_t B, uint64_t bytes, uint64_t seed, uint64_t out[2]) {
    const uint64_t t = fp_mix(seed ^ 0x9E3779B97F4A7C15ull);
    out[0] = fp_mix(A + t + bytes);
    out[1] = fp_mix(B + fp_rotl32(t) + bytes);
}

struct FpDesc {
    const uint8_t* data;
    uint64_t bytes, seed;
    uint32_t blocks, pad;
};

__device__ __forceinline__ uint64_t wave_sum_u64(uint64_t v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += (uint64_t)__shfl_xor((unsigned long long)v, o, 64);
    return v;
}

// grid (max blocks of any buffer in the table, buffers).  partial: [buffer][FP_MAX_BLOCKS][2]; block x of buffer y writes its slot
// when x < desc[y].blocks, and nothing else is ever read by the second pass.
__global__ __launch_bounds__(FP_THREADS) void fingerprint_kernel(const FpDesc* __restrict__ desc, uint64_t* __restrict__ partial) {
    const FpDesc d = desc[blockIdx.y];
    if (blockIdx.x >= d.blocks) return;
    const uint64_t nfull = d.bytes >> 4;
    const int tail = (int)(d.bytes & 15);
    const uint64_t stride = (uint64_t)d.blocks * FP_THREADS;
    uint64_t A = 0, B = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * FP_THREADS + threadIdx.x; i < nfull; i += stride) {
        const u32x4 v = *(const u32x4*)(d.data + i * 16);                        // one 16-byte load per chunk
        fp_term((uint64_t)v[0] | ((uint64_t)v[1] << 32), (uint64_t)v[2] | ((uint64_t)v[3] << 32), d.seed, i, A, B);
    }
    if (tail && blockIdx.x == 0 && threadIdx.x == 0) {
        uint64_t lo, hi;
        fp_tail_words(d.data + nfull * 16, tail, lo, hi);
        fp_term(lo, hi, d.seed, nfull, A, B);
    }
    A = wave_sum_u64(A);
    B = wave_sum_u64(B);
    __shared__ uint64_t red[FP_THREADS / PG_WAVE][2];
    if ((threadIdx.x & (PG_WAVE - 1)) == 0) { red[threadIdx.x / PG_WAVE][0] = A; red[threadIdx.x / PG_WAVE][1] = B; }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t a = 0, b = 0;
        for (int w = 0; w < FP_THREADS / PG_WAVE; ++w) { a += red[w][0]; b += red[w][1]; }
        uint64_t* o = partial + ((uint64_t)blockIdx.y * FP_MAX_BLOCKS + blockIdx.x) * 2;
        o[0] = a; o[1] = b;
    }
}

// grid (buffers): acc[buffer] = the sum of the buffer's desc.blocks partials (0, 0 for an empty buffer)
__global__ __launch_bounds__(FP_THREADS) void fingerprint_sum_kernel(const FpDesc* __restrict__ desc, const uint64_t* __restrict__ partial,
                                                                     uint64_t* __restrict__ acc) {
    const uint32_t nb = desc[blockIdx.x].blocks;
    const uint64_t* p = partial + (uint64_t)blockIdx.x * FP_MAX_BLOCKS * 2;
    uint64_t A = 0, B = 0;
    for (uint32_t j = threadIdx.x; j < nb; j += FP_THREADS) { A += p[2 * j]; B += p[2 * j + 1]; }
    __shared__ uint64_t red[FP_THREADS][2];
    red[threadIdx.x][0] = A; red[threadIdx.x][1] = B;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t a = 0, b = 0;
        for (int t = 0; t < FP_THREADS; ++t) { a += red[t][0]; b += red[t][1]; }
        acc[2 * blockIdx.x] = a; acc[2 * blockIdx.x + 1] = b;
    }
}

}  // namespace

void pg_fingerprint_host(const void* data, size_t bytes, uint64_t seed, uint64_t out[2]) {
    const uint8_t* p = (const uint8_t*)data;
    const uint64_t nfull = (uint64_t)bytes >> 4;
    uint64_t A = 0, B = 0, lo, hi;
    for (uint64_t i = 0; i < nfull; ++i) {
        fp_tail_words(p + i * 16, 16, lo, hi);
        fp_term(lo, hi, seed, i, A, B);
    }
    if (bytes & 15) {
        fp_tail_words(p + nfull * 16, (int)(bytes & 15), lo, hi);
        fp_term(lo, hi, seed, nfull, A, B);
    }
    fp_final(A, B, (uint64_t)bytes, seed, out);
}

int pg_fingerprint_many(const PgFpBuf* bufs, int n, uint64_t* out, hipStream_t stream) {
    if (n < 0 || n > 65535) { pg_set_error("fingerprint: %d buffers (0..65535)", n); return PG_EINVAL; }
    std::vector<FpDesc> desc((size_t)n);
    uint32_t max_blocks = 0;
    for (int i = 0; i < n; ++i) {
        if (bufs[i].bytes && !bufs[i].data) { pg_set_error("fingerprint: buffer %d is null with %zu bytes", i, bufs[i].bytes); return PG_EINVAL; }
        if (bufs[i].bytes && ((uintptr_t)bufs[i].data & 15) != 0) {
            pg_set_error("fingerprint: buffer %d at %p is not 16-byte aligned (the kernel reads 16-byte chunks)", i, bufs[i].data);
            return PG_EINVAL;
        }
        const uint64_t nfull = (uint64_t)bufs[i].bytes >> 4;
        uint64_t nb = (nfull + (uint64_t)FP_THREADS * FP_CHUNKS_PER_LANE - 1) / ((uint64_t)FP_THREADS * FP_CHUNKS_PER_LANE);
        if (nb > FP_MAX_BLOCKS) nb = FP_MAX_BLOCKS;
        if (nb == 0 && bufs[i].bytes) nb = 1;                  // fewer than 16 bytes: the tail chunk alone
        desc[i] = {(const uint8_t*)bufs[i].data, (uint64_t)bufs[i].bytes, bufs[i].seed, (uint32_t)nb, 0u};
        if ((uint32_t)nb > max_blocks) max_blocks = (uint32_t)nb;
    }
    std::vector<uint64_t> acc((size_t)n * 2, 0);
    if (max_blocks > 0) {                                      // something to read: table | partials | sums in one scratch allocation
        const size_t desc_b = ((size_t)n * sizeof(FpDesc) + 255) / 256 * 256;
        const size_t part_b = (size_t)n * FP_MAX_BLOCKS * 2 * sizeof(uint64_t);
        const size_t acc_b = (size_t)n * 2 * sizeof(uint64_t);
        char* scratch = nullptr;
        PG_HIP(hipMalloc((void**)&scratch, desc_b + part_b + acc_b));
        FpDesc* d_desc = (FpDesc*)scratch;
        uint64_t* d_part = (uint64_t*)(scratch + desc_b);
        uint64_t* d_acc = (uint64_t*)(scratch + desc_b + part_b);
        hipError_t e = hipMemcpyAsync(d_desc, desc.data(), (size_t)n * sizeof(FpDesc), hipMemcpyHostToDevice, stream);
        if (e == hipSuccess) {
            hipLaunchKernelGGL(fingerprint_kernel, dim3(max_blocks, (unsigned)n), dim3(FP_THREADS), 0, stream, d_desc, d_part);
            hipLaunchKernelGGL(fingerprint_sum_kernel, dim3((unsigned)n), dim3(FP_THREADS), 0, stream, d_desc, d_part, d_acc);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipMemcpyAsync(acc.data(), d_acc, acc_b, hipMemcpyDeviceToHost, stream);
        const hipError_t es = hipStreamSynchronize(stream);     // also after a failure: the table on the host must outlive the copy
        if (e == hipSuccess) e = es;
        (void)hipFree(scratch);
        if (e != hipSuccess) { pg_set_error("fingerprint: %s", hipGetErrorString(e)); return PG_EHIP; }
    }
    for (int i = 0; i < n; ++i) fp_final(acc[2 * i], acc[2 * i + 1], desc[i].bytes, desc[i].seed, out + 2 * i);
    return PG_OK;
}

extern "C" int pg_fingerprint(const void* data, size_t bytes, uint64_t seed, uint64_t out[2], void* stream) {
    if (!out) { pg_set_error("fingerprint: out is null"); return PG_EINVAL; }
    if (bytes && !data) { pg_set_error("fingerprint: data is null with %zu bytes", bytes); return PG_EINVAL; }
    if (bytes && ((uintptr_t)data & 15) != 0) {
        pg_set_error("fingerprint: data at %p is not 16-byte aligned (the kernel reads 16-byte chunks)", data);
        return PG_EINVAL;
    }
    const PgFpBuf b = {data, bytes, seed};
    uint64_t r[2];
    const int rc = pg_fingerprint_many(&b, 1, r, (hipStream_t)stream);
    if (rc != PG_OK) return rc;
    out[0] = r[0]; out[1] = r[1];
    return PG_OK;
}
