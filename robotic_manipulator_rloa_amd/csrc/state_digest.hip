// naf_state_digest: one 64-bit digest per device segment, in one read-only pass (include/naf_hip.h).
//
// digest(seg) = sum over i < n_words of mix(i, word_i)  (mod 2^64)
// mix(i, w)   = z ^ (z >> 32) with z = (x ^ (x >> 32)) * K2 and x = i * K1 + w
// For a fixed index the map w -> mix(i, w) is a bijection (the add, the xorshift and the odd multiply each are), so a changed
// word always changes the digest; the index in x makes the digest depend on where a word sits. The sum is commutative and
// associative: every thread, every workgroup and the one atomic per workgroup and segment may run in any order, and the result
// does not depend on the grid. tests/test_resume_cpu.py keeps the numpy twin.
#include "common.h"
#include "../../include/naf_hip.h"

namespace {

constexpr int DG_THREADS = 256;
constexpr int DG_UNROLL = 4;                  // float4 loads in flight per thread and trip
constexpr uint64_t DG_K1 = 0x9E3779B97F4A7C15ull;
constexpr uint64_t DG_K2 = 0xD6E8FEB86659FD93ull;

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));      // (the nontemporal builtin takes clang vectors, not uint4)

struct DigestSegs {
    const uint32_t* ptr[NAF_DIGEST_MAX_SEGS];
    uint64_t n[NAF_DIGEST_MAX_SEGS];
};

__device__ __forceinline__ uint64_t dg_mix(uint64_t key, uint32_t w) {
    uint64_t x = key + (uint64_t)w;
    x = (x ^ (x >> 32)) * DG_K2;
    return x ^ (x >> 32);
}

__device__ __forceinline__ uint64_t dg_mix4(uint64_t q, u32x4 v) {
    const uint64_t k = 4 * q * DG_K1;          // key of word 4q; the next three are + K1 each
    return dg_mix(k, v.x) + dg_mix(k + DG_K1, v.y) + dg_mix(k + 2 * DG_K1, v.z) + dg_mix(k + 3 * DG_K1, v.w);
}

__global__ __launch_bounds__(DG_THREADS) void state_digest_kernel(DigestSegs segs, unsigned long long* __restrict__ out) {
    const int s = blockIdx.y;
    const uint32_t* __restrict__ p = segs.ptr[s];
    const uint64_t n = segs.n[s];
    const uint64_t tid = threadIdx.x;
    const uint64_t gtid = (uint64_t)blockIdx.x * DG_THREADS + tid;
    const uint64_t nthreads = (uint64_t)gridDim.x * DG_THREADS;
    if ((uint64_t)blockIdx.x * DG_THREADS >= n) return;       // (uniform: this workgroup has no word of the segment)
    uint64_t acc = 0;
    uint64_t scalar_from = 0;
    if (((uintptr_t)p & 15) == 0) {
        const u32x4* __restrict__ p4 = (const u32x4*)p;
        const uint64_t n4 = n / 4;
        uint64_t q = gtid;
        for (; q + (DG_UNROLL - 1) * nthreads < n4; q += DG_UNROLL * nthreads) {
            u32x4 v[DG_UNROLL];
#pragma unroll
            for (int u = 0; u < DG_UNROLL; ++u) v[u] = __builtin_nontemporal_load(p4 + q + u * nthreads);
#pragma unroll
            for (int u = 0; u < DG_UNROLL; ++u) acc += dg_mix4(q + u * nthreads, v[u]);
        }
        for (; q < n4; q += nthreads) acc += dg_mix4(q, __builtin_nontemporal_load(p4 + q));
        scalar_from = 4 * n4;                  // the last n % 4 words
    }
    for (uint64_t i = scalar_from + gtid; i < n; i += nthreads) acc += dg_mix(i * DG_K1, p[i]);
    // workgroup sum: lanes, then the four waves through LDS; one atomic per workgroup
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) acc += __shfl_xor(acc, off, NAF_WAVE);
    __shared__ unsigned long long wsum[DG_THREADS / NAF_WAVE];
    if ((tid & (NAF_WAVE - 1)) == 0) wsum[tid / NAF_WAVE] = acc;
    __syncthreads();
    if (tid == 0) {
        unsigned long long t = 0;
#pragma unroll
        for (int w = 0; w < DG_THREADS / NAF_WAVE; ++w) t += wsum[w];
        atomicAdd(out + s, t);
    }
}

}  // namespace

extern "C" int naf_state_digest(const naf_digest_seg_t* segs, int n_seg, uint64_t* out, int blocks_per_seg, void* stream) {
    if (n_seg < 0 || (n_seg > 0 && (!segs || !out))) return NAF_ERR_ARG;
    for (int i = 0; i < n_seg; ++i)
        if ((segs[i].n_words && !segs[i].ptr) || ((uintptr_t)segs[i].ptr & 3)) return NAF_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    for (int b = 0; b < n_seg; b += NAF_DIGEST_MAX_SEGS) {
        const int cnt = n_seg - b < NAF_DIGEST_MAX_SEGS ? n_seg - b : NAF_DIGEST_MAX_SEGS;
        DigestSegs d = {};
        uint64_t most = 0;
        for (int i = 0; i < cnt; ++i) {
            d.ptr[i] = (const uint32_t*)segs[b + i].ptr;
            d.n[i] = segs[b + i].n_words;
            most = d.n[i] > most ? d.n[i] : most;
        }
        // default grid: each thread takes at least DG_UNROLL float4, at most 8 workgroups per CU of the MI355X's 256
        uint64_t blocks = blocks_per_seg > 0 ? (uint64_t)blocks_per_seg
                                             : (most + 4ull * DG_UNROLL * DG_THREADS - 1) / (4ull * DG_UNROLL * DG_THREADS);
        if (blocks_per_seg <= 0 && blocks > 2048) blocks = 2048;
        if (blocks < 1) blocks = 1;
        if (blocks > (1u << 20)) return NAF_ERR_ARG;
        hipError_t e = hipMemsetAsync(out + b, 0, sizeof(uint64_t) * cnt, st);
        if (e != hipSuccess) return (int)e;
        state_digest_kernel<<<dim3((unsigned)blocks, cnt), DG_THREADS, 0, st>>>(d, (unsigned long long*)(out + b));
        NAF_CHECK_LAUNCH();
    }
    return NAF_OK;
}
