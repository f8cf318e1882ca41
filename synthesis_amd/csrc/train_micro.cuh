// synthesis_amd — the micro-batch learner step (SYN_TRAIN_BATCH_MICRO, include/synthesis_amd.h): a minibatch of B = 32 nb positions is
// nb micro-batches of 32 (sample 32 j + i = sample i of micro-batch j), and
//   g_j, l_j   = what the chained step computes for micro-batch j as a minibatch of its own (batch mean 1/32, policy_weight and
//                value_weight applied): tm_gradients / conv_grad_step_mfma / conv_grad_step_bf16 with B = 32, chain for chain
//   acc        = g_0, then acc = acc + g_j for j = 1 .. nb-1: plain f32 additions in ascending j (nothing is added to g_0, so nb = 1
//                is the chained step's bits, the sign of a zero included)
//   G          = acc * inv, inv = 1.0f / (float)nb: one rounding, fused with nothing; the two losses alike
// G is the gradient of the mean loss over the B samples (a mean of equal-size block means), evaluated in an order that does not depend
// on how many workgroups computed it. Adam is unchanged.
//
// Two kinds of launch per step, in stream order, and NO workgroup of either waits for another one: no grid barrier, no spin on memory,
// no cooperative launch — so they need no co-residency, run beside a self-play launch that holds every CU, and need none of the
// snapshot / give-up machinery of the persistent epoch kernels.
//   blocks   workgroup b takes the micro-batches j = b, b + gridDim.x, ... < nb and writes g_j, l_j to row j of the block buffer
//            (row = [g_j: P floats][l_j: 2 floats], stride padded to a multiple of 64 floats: micro_row_stride). Nothing about the
//            network changes inside a step, and the per-block device functions stage no weights (their A operands come from the
//            L2-resident images / parameter array fragment by fragment): what a workgroup sets up once for all of its blocks is the
//            kernel arguments and the row arithmetic; the weight fragments stay warm in its CU's vector L1 across its blocks.
//   reduce   thread p owns parameter p (or one of the two loss words): the ascending chain over the rows, then * inv, into the gradient
//            buffer the caller named / the loss slot. Consecutive threads read consecutive floats of a row (coalesced); the loads of
//            MICRO_AHEAD rows are issued before the additions that consume them.
#pragma once
#include "train_conv_mfma.cuh"
#include "train_mfma.cuh"

namespace syn {

constexpr int MICRO_BLOCK = 32;          // samples of a micro-batch: the reference's batch_size, = TrainGeom::CHUNK = ConvMfmaGeom::CHUNK
constexpr int MICRO_MAX_BLOCKS = 1024;   // nb above this is refused (SYN_ERR_UNSUPPORTED)
constexpr int MICRO_REDUCE_THREADS = 64;
constexpr int MICRO_AHEAD = 8;
static_assert(TrainGeom::CHUNK == MICRO_BLOCK && ConvMfmaGeom::CHUNK == MICRO_BLOCK, "a micro-batch is one chunk of either learner");

__host__ __device__ constexpr int micro_row_stride(int num_params) { return (num_params + 2 + 63) & ~63; }

// Connect4Net: <<<min(nb, cap), 1024>>>, TrainGeom::WL_OFF floats of LDS. Row j of `rows` <- g_j, l_j.
__global__ __launch_bounds__(1024) void train_micro_blocks_kernel(const float* __restrict__ wimg, const float* __restrict__ timg,
                                                                  const unsigned long long* __restrict__ my_bb,
                                                                  const unsigned long long* __restrict__ op_bb,
                                                                  const float* __restrict__ tpi, const float* __restrict__ tv, int nb,
                                                                  DevTrainHyper hp, float* __restrict__ rows) {
    constexpr int P = TrainGeom::NUM_PARAMS, STRIDE = micro_row_stride(P);
    for (int j = blockIdx.x; j < nb; j += gridDim.x) {
        const size_t o = (size_t)j * MICRO_BLOCK;
        float* row = rows + (size_t)j * STRIDE;
        // (tm_gradients ends every chunk behind a workgroup barrier: the next block's feature stores cannot overtake this block's
        // parameter-gradient reads of LDS)
        tm_gradients(wimg, timg, my_bb + o, op_bb + o, tpi + o * 9, tv + o * 3, MICRO_BLOCK, hp, row, row + P, nullptr, nullptr);
    }
}

// Connect4ConvNet, f32 or bf16: <<<min(nb, cap), 512>>>, ConvMfmaGeom::LDS_FLOATS floats of LDS (157.5 KB: one workgroup per CU).
template <bool BF16>
__global__ __launch_bounds__(CONV_TRAIN_THREADS) void train_micro_blocks_conv_kernel(const float* __restrict__ w,
                                                                                     const unsigned long long* __restrict__ my_bb,
                                                                                     const unsigned long long* __restrict__ op_bb,
                                                                                     const float* __restrict__ tpi, const float* __restrict__ tv,
                                                                                     int nb, DevTrainHyper hp, float* __restrict__ rows) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int P = ConvGeom::NUM_PARAMS, STRIDE = micro_row_stride(P), NT = CONV_TRAIN_THREADS;
    for (int j = blockIdx.x; j < nb; j += gridDim.x) {
        const size_t o = (size_t)j * MICRO_BLOCK;
        float* row = rows + (size_t)j * STRIDE;
        if (BF16) conv_grad_step_bf16<NT>(w, my_bb + o, op_bb + o, tpi + o * 9, tv + o * 3, MICRO_BLOCK, hp, row, row + P, nullptr, lds, threadIdx.x);
        else conv_grad_step_mfma<NT>(w, my_bb + o, op_bb + o, tpi + o * 9, tv + o * 3, MICRO_BLOCK, hp, row, row + P, nullptr, lds, threadIdx.x);
        // the step ends without a barrier (its last phase reads the partials in LDS): the next block's staging must not overtake it
        __syncthreads();
    }
}

// <<<ceil((P + 2) / 64), 64>>>: entry p < P -> grads[p], entries P, P + 1 -> losses[0..1]. The order of the additions is the
// definition: ascending j, nothing re-associated.
__global__ __launch_bounds__(MICRO_REDUCE_THREADS) void train_micro_reduce_kernel(const float* __restrict__ rows, int nb, int num_params,
                                                                                  int stride, float inv, float* __restrict__ grads,
                                                                                  float* __restrict__ losses) {
    const int p = blockIdx.x * MICRO_REDUCE_THREADS + threadIdx.x;
    if (p >= num_params + 2) return;
    const float* col = rows + p;
    float acc = col[0];
    int j = 1;
    for (; j + MICRO_AHEAD <= nb; j += MICRO_AHEAD) {
        float v[MICRO_AHEAD];
#pragma unroll
        for (int k = 0; k < MICRO_AHEAD; k++) v[k] = col[(size_t)(j + k) * stride];
#pragma unroll
        for (int k = 0; k < MICRO_AHEAD; k++) acc = acc + v[k];
    }
    for (; j < nb; j++) acc = acc + col[(size_t)j * stride];
    const float g = acc * inv;
    if (p < num_params) grads[p] = g;
    else losses[p - num_params] = g;
}

}  // namespace syn
