// State digests (include/synthesis_amd.h syn_state_digest; not in the reference): a 64-bit fingerprint of a piece of
// engine state, computed where the state lives. A component is a sequence of 32-bit words w_0 .. w_{L-1} (its arrays concatenated, each
// read as it lies in memory); with T = DIGEST_TAG + what and all arithmetic unsigned 64-bit with wrap-around
//     a_i    = finalise(T + (i + 1) * GOLDEN)
//     h_i    = noise_splitmix64(a_i, w_i)
//     S      = h_0 + h_1 + ... + h_{L-1}
//     digest = sm(sm(S ^ T, hi32(L)), lo32(L))
// The sum is modulo 2^64, hence associative and commutative: the digest cannot depend on the grid and no order needs fixing. Two
// kernels: digest_sections_kernel (grid-stride over the sections, 16-byte loads where a section's alignment allows, every lane a 64-bit
// accumulator, a wave reduced by shuffles, a workgroup through LDS, one partial per workgroup) and digest_finish_kernel (one workgroup:
// the partials, then the last two sm). No atomics, and no workgroup waits for another.
#pragma once
#include <hip/hip_runtime.h>

#include "noise.cuh"

namespace syn {

constexpr uint64_t DIGEST_TAG = 0xD16E57000000AA00ull;
constexpr int DIGEST_THREADS = 256;
constexpr int DIGEST_MAX_SECTIONS = 5;

// the definition's two functions for host and device alike (the host digests SYN_DIGEST_NETWORK and the trainer's step count)
__host__ __device__ __forceinline__ uint64_t digest_finalise(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
__host__ __device__ __forceinline__ uint64_t digest_sm(uint64_t seed, uint32_t index) {
    return digest_finalise(seed + (uint64_t)(index + 1u) * NOISE_GOLDEN);
}
// h_i of word w at global index i
__host__ __device__ __forceinline__ uint64_t digest_word(uint64_t tag, uint64_t i, uint32_t w) {
    return digest_sm(digest_finalise(tag + (i + 1ull) * NOISE_GOLDEN), w);
}
__host__ __device__ __forceinline__ uint64_t digest_close(uint64_t tag, uint64_t sum, uint64_t n_words) {
    return digest_sm(digest_sm(sum ^ tag, (uint32_t)(n_words >> 32)), (uint32_t)n_words);
}

// One array of the component: `words` 32-bit words at p (4-byte aligned), the first of which is word `first` of the sequence.
struct DigestSection {
    const uint32_t* p;
    unsigned long long words;
    unsigned long long first;
};
struct DigestArgs {
    DigestSection sec[DIGEST_MAX_SECTIONS];
    int n_sections;
    unsigned long long tag;
};

// the workgroup's sum of `acc` in thread 0 (every thread calls it)
SYN_DEV uint64_t digest_block_sum(uint64_t acc) {
    __shared__ unsigned long long wave_sum[DIGEST_THREADS / 64];
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) acc += __shfl_down((unsigned long long)acc, d, 64);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) wave_sum[wave] = acc;
    __syncthreads();
    uint64_t s = 0;
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 0; w < DIGEST_THREADS / 64; w++) s += wave_sum[w];
    }
    return s;
}

// <<<grid, DIGEST_THREADS>>>: partials[blockIdx.x] = the sum of h_i over the words this workgroup read. A section is split into the
// words before its first 16-byte boundary, whole 16-byte groups and the words behind the last one; the groups are read with one
// 16-byte load per lane (a wave reads 1 KiB of consecutive memory), the at most six other words by the first threads of the grid.
__global__ void __launch_bounds__(DIGEST_THREADS) digest_sections_kernel(DigestArgs A, unsigned long long* __restrict__ partials) {
    const unsigned long long tid = (unsigned long long)blockIdx.x * DIGEST_THREADS + threadIdx.x;
    const unsigned long long stride = (unsigned long long)gridDim.x * DIGEST_THREADS;
    uint64_t acc = 0;
    for (int s = 0; s < A.n_sections; s++) {
        const uint32_t* __restrict__ p = A.sec[s].p;
        const unsigned long long n = A.sec[s].words, first = A.sec[s].first;
        unsigned long long head = (unsigned long long)((0u - (unsigned)((uintptr_t)p >> 2)) & 3u);
        if (head > n) head = n;
        const unsigned long long groups = (n - head) >> 2, tail0 = head + (groups << 2);
        const uint4* __restrict__ q = reinterpret_cast<const uint4*>(p + head);
        for (unsigned long long g = tid; g < groups; g += stride) {
            const uint4 x = q[g];
            const uint64_t i = first + head + (g << 2);
            acc += digest_word(A.tag, i, x.x);
            acc += digest_word(A.tag, i + 1, x.y);
            acc += digest_word(A.tag, i + 2, x.z);
            acc += digest_word(A.tag, i + 3, x.w);
        }
        const unsigned long long edge = head + (n - tail0);   // at most 3 + 3 words
        if (tid < edge) {
            const unsigned long long j = tid < head ? tid : tail0 + (tid - head);
            acc += digest_word(A.tag, first + j, p[j]);
        }
    }
    const uint64_t sum = digest_block_sum(acc);
    if (threadIdx.x == 0) partials[blockIdx.x] = sum;
}

// <<<1, DIGEST_THREADS>>>: out[0] = the digest of n_words words whose h_i sum to (the partials + host_sum), out[1] = n_words.
// host_sum carries the words that live on the host (the trainer's step count).
__global__ void __launch_bounds__(DIGEST_THREADS) digest_finish_kernel(const unsigned long long* __restrict__ partials, int n_partials,
                                                                       unsigned long long host_sum, unsigned long long tag,
                                                                       unsigned long long n_words, unsigned long long* __restrict__ out) {
    uint64_t acc = 0;
    for (int i = threadIdx.x; i < n_partials; i += DIGEST_THREADS) acc += partials[i];
    const uint64_t sum = digest_block_sum(acc);
    if (threadIdx.x == 0) {
        out[0] = digest_close(tag, sum + host_sum, n_words);
        out[1] = n_words;
    }
}

}  // namespace syn
