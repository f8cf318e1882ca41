// Device-resident replay buffer (synthesis/src/data.rs:107-235: extend, keep_last_n_games): the kernels between a self-play
// launch's padded outputs and the learner's data set. A buffer is five structure-of-arrays sections
//     my[cap] u64 | op[cap] u64 | gid[cap] i64 | pi[cap][9] f32 | v[cap][3] f32          (72 bytes per position)
// and every kernel here keeps buffer order (game order, then ply order), because the de-duplication sums the targets of identical
// states in buffer order (train_kernels.cuh dedup_reduce_kernel): a float sum in another order is another float.
// All of them stream: plain vector loads and stores, no LDS, no atomics.
#pragma once
#include <hip/hip_runtime.h>

namespace syn {

constexpr int REPLAY_T = 63;  // Connect4::MAX_TURNS: slots per game in syn_selfplay_run's outputs

// Compaction of a self-play launch. One wave per game: the game's pi rows are ONE span of plies x 9 floats at the source
// (pis[g][0..plies)[9]) and at the destination (pi[off .. off + plies)[9]), likewise v — the lanes stride over the spans as dwords,
// coalesced on both sides; lane = ply splits the interleaved (my, op) pairs into the two sections and writes the game id.
// off[g] = exclusive sum of plies. A game with plies == 0 (never started after syn_cancel) contributes nothing. `cap` bounds every
// store (the host has checked the total; a corrupt plies entry must still not write outside the sections).
__global__ void __launch_bounds__(256) replay_compact_kernel(
    const int* __restrict__ plies, const unsigned* __restrict__ off, int n_games, const unsigned long long* __restrict__ states,
    const float* __restrict__ pis, const float* __restrict__ vs, long long first_gid, unsigned long long cap,
    unsigned long long* __restrict__ out_my, unsigned long long* __restrict__ out_op, long long* __restrict__ out_gid,
    float* __restrict__ out_pi, float* __restrict__ out_v) {
    const int g = (int)((blockIdx.x * (size_t)blockDim.x + threadIdx.x) >> 6), lane = threadIdx.x & 63;
    if (g >= n_games) return;
    const int p = plies[g];
    const size_t o = off[g];
    if (p <= 0 || p > REPLAY_T || o + (size_t)p > cap) return;
    const size_t src = (size_t)g * REPLAY_T;
    const float* spi = pis + src * 9;
    float* dpi = out_pi + o * 9;
    for (int k = lane; k < p * 9; k += 64) dpi[k] = spi[k];
    const float* sv = vs + src * 3;
    float* dv = out_v + o * 3;
    for (int k = lane; k < p * 3; k += 64) dv[k] = sv[k];
    if (lane < p) {
        const ulonglong2 s = reinterpret_cast<const ulonglong2*>(states)[src + lane];
        out_my[o + lane] = s.x;
        out_op[o + lane] = s.y;
        out_gid[o + lane] = first_gid + g;
    }
}

// Stable keep-window (data.rs:172-194), step 1: keep[i] = 1 where the position's game is inside the window
__global__ void replay_keep_flags_kernel(const long long* __restrict__ gid, int n, long long min_gid, unsigned* __restrict__ keep) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) keep[i] = gid[i] >= min_gid ? 1u : 0u;
}

// ... step 2, after the exclusive sum `dst` of the flags: every kept position moves to its rank among the kept ones, into a second
// buffer. blockIdx.y = section; a thread moves one dword (u64 sections as two), so consecutive threads read consecutive addresses and a
// run of kept positions is written to consecutive addresses.
__global__ void replay_keep_scatter_kernel(const unsigned* __restrict__ keep, const unsigned* __restrict__ dst, int n,
                                           const unsigned* __restrict__ s_my, const unsigned* __restrict__ s_op,
                                           const unsigned* __restrict__ s_gid, const unsigned* __restrict__ s_pi,
                                           const unsigned* __restrict__ s_v, unsigned* __restrict__ d_my, unsigned* __restrict__ d_op,
                                           unsigned* __restrict__ d_gid, unsigned* __restrict__ d_pi, unsigned* __restrict__ d_v) {
    const int sec = blockIdx.y;
    const int W = sec < 3 ? 2 : (sec == 3 ? 9 : 3);
    const size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (t >= (size_t)n * W) return;
    const unsigned i = (unsigned)(t / W), c = (unsigned)(t % W);
    if (!keep[i]) return;
    const unsigned* s = sec == 0 ? s_my : sec == 1 ? s_op : sec == 2 ? s_gid : sec == 3 ? s_pi : s_v;
    unsigned* d = sec == 0 ? d_my : sec == 1 ? d_op : sec == 2 ? d_gid : sec == 3 ? d_pi : d_v;
    d[(size_t)dst[i] * W + c] = s[t];
}

}  // namespace syn
