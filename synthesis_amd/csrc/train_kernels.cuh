// synthesis_amd — the learner step that follows the self-play path.
//
// Replaces   synthesis/src/alpha_zero.rs:72-94   forward, log_softmax, kl_div(Sum) * (1/batch), loss, backward, Adam step
//            synthesis/src/alpha_zero.rs:33-36   Adam::default() + weight decay (libtorch semantics, see oracle/train.hpp)
//            synthesis/src/data.rs:196-235       ReplayBuffer::deduplicate
//
// The reference trains with batch_size 32 on a 30,492-parameter MLP: one optimiser step is ~3 MFLOP — far too small for
// anything but latency to matter. The gradient kernels (train_mfma.cuh, train_epoch.cuh; train_conv_mfma.cuh for Connect4ConvNet)
// therefore run the whole forward + backward of a minibatch in ONE workgroup with every activation and activation-gradient
// resident in LDS and fixed-order fma chains (bit-identical to oracle/train.hpp). This file holds what they share: the LDS
// geometry of Connect4Net's learner (TrainGeom), the hyper-parameters, adam_kernel — gradients go to a caller-provided device
// buffer so that a data-parallel run can all-reduce them (RCCL, 122 KB) before it applies the update — and the kernels of the
// de-duplication and of the epoch's gather.
#pragma once
#include "device_common.cuh"

namespace syn {

struct TrainGeom {
    static constexpr int NL = 5;
    static constexpr int D[NL + 1] = {63, 128, 96, 64, 48, 12};
    static constexpr int NUM_PARAMS = 30492;
    static constexpr int CHUNK = 32;  // samples resident in LDS at a time (the reference's batch_size)
    // activation rows: width rounded up to a multiple of 4 (16-byte vector reads along k) plus 4 floats of skew, which
    // spreads the rows of the 16 sample tiles of a wave over all LDS banks
    __host__ __device__ static constexpr int kp(int l) { return (D[l] + 3) & ~3; }     // padded width of layer l's input
    __host__ __device__ static constexpr int stride(int l) { return kp(l) + 4; }
    __host__ __device__ static constexpr int w_off(int l) {
        int off = 0;
        for (int i = 0; i < l; i++) off += D[i] * D[i + 1] + D[i + 1];
        return off;
    }
    __host__ __device__ static constexpr int b_off(int l) { return w_off(l) + D[l] * D[l + 1]; }
    __host__ __device__ static constexpr int a_off(int l) {  // activations A[l] in LDS (floats)
        int off = 0;
        for (int i = 0; i < l; i++) off += CHUNK * stride(i);
        return off;
    }
    static constexpr int A_FLOATS = CHUNK * (68 + 132 + 100 + 68 + 52 + 16);
    __host__ __device__ static constexpr int d_off(int l) {  // activation gradients dZ[l], l = 1..5
        int off = A_FLOATS;
        for (int i = 1; i < l; i++) off += CHUNK * stride(i);
        return off;
    }
    static constexpr int KL_OFF = A_FLOATS + CHUNK * (132 + 100 + 68 + 52 + 16);  // per-sample KL terms [CHUNK][2]
    static constexpr int WL_OFF = (KL_OFF + 2 * CHUNK + 3) & ~3;   // end of the layout = the kernels' LDS size in floats
};

struct DevTrainHyper {
    float weight_decay, policy_weight, value_weight, beta1, beta2, eps;
};

// torch::optim::Adam (amsgrad off) on device gradients; scalars prepared on the host in double like libtorch does.
__global__ void adam_kernel(float* __restrict__ w, float* __restrict__ m, float* __restrict__ v,
                            const float* __restrict__ grads, int n, DevTrainHyper hp, float step_size,
                            float inv_sqrt_bc2, float grad_scale) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float g0 = grad_scale == 1.0f ? grads[i] : grads[i] * grad_scale;  // data-parallel mean = all-reduce sum * 1/ranks
    float g = hp.weight_decay != 0.0f ? __builtin_fmaf(hp.weight_decay, w[i], g0) : g0;
    float mi = __builtin_fmaf(1.0f - hp.beta1, g, hp.beta1 * m[i]);
    float vi = __builtin_fmaf((1.0f - hp.beta2) * g, g, hp.beta2 * v[i]);
    float denom = sqrtf(vi) * inv_sqrt_bc2 + hp.eps;
    m[i] = mi;
    v[i] = vi;
    w[i] = w[i] - step_size * (mi / denom);
}

// ---------------------------------------------------------------------------------------------- deduplicate
// After a stable sort of the buffer indices by (my_bb, op_bb): head[i] = 1 where a new state starts.
__global__ void dedup_heads_kernel(const unsigned long long* __restrict__ my_sorted,
                                   const unsigned long long* __restrict__ op_sorted, int n, unsigned* __restrict__ head) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    head[i] = (i == 0 || my_sorted[i] != my_sorted[i - 1] || op_sorted[i] != op_sorted[i - 1]) ? 1u : 0u;
}
// seg_start[s] = first sorted position of unique state s (seg_id = inclusive scan of head, minus 1)
__global__ void dedup_starts_kernel(const unsigned* __restrict__ head, const unsigned* __restrict__ seg_incl, int n,
                                    unsigned* __restrict__ seg_start) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (head[i]) seg_start[seg_incl[i] - 1] = (unsigned)i;
}
// One 16-lane row per unique state, lane j < 12 owns one target component and sums it over the duplicates in buffer
// order (the stable sort keeps buffer order inside a segment), then divides by the count (data.rs:206-226).
__global__ void dedup_reduce_kernel(const unsigned* __restrict__ order, const unsigned* __restrict__ seg_start, int m,
                                    int n, const unsigned long long* __restrict__ my_bb,
                                    const unsigned long long* __restrict__ op_bb, const float* __restrict__ pis,
                                    const float* __restrict__ vs, unsigned long long* __restrict__ out_my,
                                    unsigned long long* __restrict__ out_op, float* __restrict__ out_pi,
                                    float* __restrict__ out_v, unsigned* __restrict__ out_num) {
    int row = (blockIdx.x * blockDim.x + threadIdx.x) >> 4;
    int j = threadIdx.x & 15;
    if (row >= m) return;
    unsigned s0 = seg_start[row], s1 = row + 1 < m ? seg_start[row + 1] : (unsigned)n;
    float acc = 0.0f;
    if (j < 12) {
        for (unsigned p = s0; p < s1; p++) {
            unsigned i = order[p];
            acc += j < 9 ? pis[(size_t)i * 9 + j] : vs[(size_t)i * 3 + (j - 9)];
        }
        float avg = acc / (float)(s1 - s0);
        if (j < 9) out_pi[(size_t)row * 9 + j] = avg;
        else out_v[(size_t)row * 3 + (j - 9)] = avg;
    }
    if (j == 12) {
        unsigned i = order[s0];
        out_my[row] = my_bb[i];
        out_op[row] = op_bb[i];
        out_num[row] = s1 - s0;
    }
}
// BatchRandSampler's index_select for a whole epoch at once: sample i of the step-ordered arrays = buffer entry perm[i]
__global__ void train_gather_kernel(const int* __restrict__ perm, int n, const unsigned long long* __restrict__ my,
                                    const unsigned long long* __restrict__ op, const float* __restrict__ tpi,
                                    const float* __restrict__ tv, unsigned long long* __restrict__ g_my,
                                    unsigned long long* __restrict__ g_op, float* __restrict__ g_tpi,
                                    float* __restrict__ g_tv) {
    const int i = (blockIdx.x * blockDim.x + threadIdx.x) >> 4, j = threadIdx.x & 15;
    if (i >= n) return;
    const size_t s = (size_t)perm[i];
    if (j < 9) g_tpi[(size_t)i * 9 + j] = tpi[s * 9 + j];
    else if (j < 12) g_tv[(size_t)i * 3 + (j - 9)] = tv[s * 3 + (j - 9)];
    else if (j == 12) g_my[i] = my[s];
    else if (j == 13) g_op[i] = op[s];
}
__global__ void iota_kernel(unsigned* p, int n) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = (unsigned)i;
}
__global__ void gather_u64_kernel(const unsigned long long* __restrict__ src, const unsigned* __restrict__ idx, int n,
                                  unsigned long long* __restrict__ dst) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = src[idx[i]];
}

}  // namespace syn
