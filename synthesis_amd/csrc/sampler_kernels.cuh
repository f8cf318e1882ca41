// Device-side epoch sampler (include/synthesis_amd.h syn_train_epochs_sampled; not in the reference): an epoch's row
// order and its flip flags from a 64-bit key, without the host. Row i of an n-row data set gets the sort key
//     k_i = noise_splitmix64(K_e, i),   K_e = noise_splitmix64(key ^ SAMPLER_TAG, e)
// (pairwise distinct: the multiplier is odd and the finaliser a bijection), the rows are sorted by ascending k_i
// (hipcub::DeviceRadixSort::SortPairs over all 64 bits, engine.hip) and row i is flipped where k_i & 1. Two kernels around that sort:
// the keys, and the gather of the step-ordered batches with the flip folded in. Plain vector loads and stores, no LDS, no atomics.
#pragma once
#include <hip/hip_runtime.h>

#include "noise.cuh"
#include "replay_kernels.cuh"

namespace syn {

constexpr uint64_t SAMPLER_TAG = 0x5AD3C0DE5EED1E55ull;

// K_e on the host (one value per epoch, a kernel argument): noise_splitmix64's arithmetic, epoch + 1 in 32 bits like there
inline uint64_t sampler_epoch_key(uint64_t key, uint32_t epoch) {
    uint64_t z = (key ^ SAMPLER_TAG) + (uint64_t)(epoch + 1u) * NOISE_GOLDEN;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// keys[i] = k_i, idx[i] = i: the sort's input pairs
__global__ void __launch_bounds__(256) sampler_keys_kernel(uint64_t epoch_key, int n, unsigned long long* __restrict__ keys,
                                                           int* __restrict__ idx) {
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;   // (n <= 2^31 - 1: no wrap, and never negative)
    if (i >= (unsigned)n) return;
    keys[i] = noise_splitmix64(epoch_key, i);
    idx[i] = (int)i;
}

// train_gather_kernel from the sorted pairs: sample i of the step-ordered arrays = row perm[i], and with `flip` a row whose key is odd
// enters as (mirror(my), mirror(op), pi[8 - c], v). 16 threads per row; only the first n_take sorted rows are gathered (drop_last).
// n_rows bounds the row index: a corrupt index must not read outside the data set.
__global__ void __launch_bounds__(256) sampler_gather_kernel(
    const unsigned long long* __restrict__ sorted_keys, const int* __restrict__ perm, int n_take, int n_rows, int flip,
    const unsigned long long* __restrict__ my, const unsigned long long* __restrict__ op, const float* __restrict__ tpi,
    const float* __restrict__ tv, unsigned long long* __restrict__ g_my, unsigned long long* __restrict__ g_op,
    float* __restrict__ g_tpi, float* __restrict__ g_tv) {
    const int i = (int)((blockIdx.x * (size_t)blockDim.x + threadIdx.x) >> 4), j = threadIdx.x & 15;
    if (i >= n_take) return;
    const unsigned row = (unsigned)perm[i];
    if (row >= (unsigned)n_rows) return;
    const size_t s = row;
    const bool f = flip && (sorted_keys[i] & 1ull);
    if (j < 9) g_tpi[(size_t)i * 9 + j] = tpi[s * 9 + (f ? 8 - j : j)];
    else if (j < 12) g_tv[(size_t)i * 3 + (j - 9)] = tv[s * 3 + (j - 9)];
    else if (j == 12) g_my[i] = f ? mirror_bb(my[s]) : my[s];
    else if (j == 13) g_op[i] = f ? mirror_bb(op[s]) : op[s];
}

// syn_debug_sampler's flags in row order: flip[i] = k_i & 1
__global__ void __launch_bounds__(256) sampler_flags_kernel(uint64_t epoch_key, int n, unsigned char* __restrict__ flip) {
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < (unsigned)n) flip[i] = (unsigned char)(noise_splitmix64(epoch_key, i) & 1ull);
}

}  // namespace syn
