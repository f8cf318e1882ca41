// Device-resident games (run_games in engine.hip, behind syn_match_run / syn_match_run_sides / syn_tournament_run): what runs between
// two plies' search launches. The live games are match_kernels.cuh's five parallel arrays, kept GROUPED BY MOVER — group p is the range
// [seg[p], seg[p + 1]) and holds the games player p moves in at this ply, in game order — so that a ply needs one search launch per
// player, over that player's range, whatever pairing each of its games belongs to. (A match is two players with player 0 first in
// every game: all its live games share one mover, so every ply has one group.) After a ply's searches
//     tournament_advance_kernel   the rules of one step (match_advance_job) for one group's range, and key[i]: the player that moves
//                                 next in job i's game (from device copies of the schedule, through id[i]), or n_keys when the game
//                                 ended here or its root was not searched (dropped)
//     tournament_count_kernel     per 256-job workgroup, how many of its jobs hold each key: a key-major [n_keys + 1][n_blocks] matrix
//     an exclusive sum over that matrix (hipcub): cell (k, b) becomes the position of the first job of workgroup b with key k
//     tournament_scatter_kernel   moves every surviving job to that position plus its rank among its workgroup's jobs of the same key,
//                                 into the second set of arrays, and leaves seg[0 .. n_keys] (the groups of the next ply; seg[n_keys] =
//                                 the survivors) and the ply's error word behind it — the n_keys + 2 words the host reads per ply
// The partition is stable: inside a group the input order is kept, so the job order of every ply is a function of the call's inputs
// alone. No atomics, no workgroup waits for another, LDS only inside a workgroup behind __syncthreads(). A wave finds its ranks without
// sorting: it peels its distinct keys one at a time — the first remaining lane's key, the 64-bit ballot of the lanes that hold it, a
// popcount — and since the input arrives grouped by the previous mover, a wave holds few distinct keys.
#pragma once
#include <hip/hip_runtime.h>

#include "match_kernels.cuh"

namespace syn {

constexpr int TOURNAMENT_MAX_KEYS = 64;                 // SYN_TOURNAMENT_MAX_PLAYERS
constexpr int TOURNAMENT_BLOCK = 256;                   // four wave64s
constexpr int TOURNAMENT_WAVES = TOURNAMENT_BLOCK / 64;

// match_advance_job for the jobs [lo, lo + n) of the live arrays, one thread per job: `results` is that range's own record array (job
// lo's record first). first / second: the schedule, per game.
template <class Result>
__global__ void __launch_bounds__(256) tournament_advance_kernel(
    const Result* __restrict__ results, int lo, int n, int ply, unsigned long long* __restrict__ my, unsigned long long* __restrict__ op,
    const int* __restrict__ id, const unsigned long long* __restrict__ word, const int* __restrict__ first,
    const int* __restrict__ second, int n_keys, int* __restrict__ key, int* __restrict__ stream_error, MatchOut out) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const int i = lo + j;
    const int g = id[i];
    const bool on = match_advance_job(results[j], i, g, ply, my, op, word, stream_error, out);
    // after ply `ply` an even number of moves has been played when ply is odd: the first player moves again
    key[i] = on ? ((ply & 1) ? first[g] : second[g]) : n_keys;
}

// One wave's peel: cnt[k] = lanes of this wave that hold key k (written for the keys present only: the caller zeroes cnt), and the
// return value = lanes below this one that hold this lane's key. k < 0 marks a lane without a job.
SYN_DEV int tournament_wave_ranks(int k, int lane, int* __restrict__ cnt) {
    unsigned long long todo = __ballot(k >= 0);
    int below = 0;
    while (todo != 0ull) {   // wave-uniform: every lane runs the same trips
        const int lead = __builtin_amdgcn_readfirstlane((int)__ffsll(todo) - 1);
        const int kk = __builtin_amdgcn_readlane(k, lead);
        const unsigned long long same = __ballot(k == kk);
        if (k == kk) below = __popcll(same & ((1ull << lane) - 1ull));
        if (lane == lead) cnt[kk] = __popcll(same);
        todo &= ~same;
    }
    return below;
}

// a job's key as the kernels below use it: anything outside [0, n_keys) is "dropped"
SYN_DEV int tournament_load_key(const int* __restrict__ key, int i, int n_live, int n_keys) {
    if (i >= n_live) return -1;
    const int k = key[i];
    return (unsigned)k < (unsigned)n_keys ? k : n_keys;
}

// counts[k * n_blocks + b] = jobs of workgroup b with key k, for every k in [0, n_keys] and every b: each cell by exactly one thread
__global__ void __launch_bounds__(TOURNAMENT_BLOCK) tournament_count_kernel(const int* __restrict__ key, int n_live, int n_keys,
                                                                            unsigned* __restrict__ counts) {
    __shared__ int cnt[TOURNAMENT_WAVES][TOURNAMENT_MAX_KEYS + 1];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    for (int c = t; c < TOURNAMENT_WAVES * (TOURNAMENT_MAX_KEYS + 1); c += TOURNAMENT_BLOCK) (&cnt[0][0])[c] = 0;
    __syncthreads();
    const int i = blockIdx.x * TOURNAMENT_BLOCK + t;
    tournament_wave_ranks(tournament_load_key(key, i, n_live, n_keys), lane, cnt[w]);
    __syncthreads();
    if (t <= n_keys) {
        int s = 0;
#pragma unroll
        for (int v = 0; v < TOURNAMENT_WAVES; v++) s += cnt[v][t];
        counts[(size_t)t * gridDim.x + blockIdx.x] = (unsigned)s;
    }
}

// `base` = the exclusive sum of counts. seg_out[0 .. n_keys] = base's column 0; seg_out[n_keys + 1] = the ply's error word:
// -(the search kernels' error word), -MATCH_ERR_STREAM, or 0 (search_error / stream_error may be NULL: the regroup alone).
__global__ void __launch_bounds__(TOURNAMENT_BLOCK) tournament_scatter_kernel(
    const int* __restrict__ key, int n_live, int n_keys, const unsigned* __restrict__ base, MatchLive from, MatchLive to,
    const int* __restrict__ search_error, const int* __restrict__ stream_error, int* __restrict__ seg_out) {
    __shared__ int cnt[TOURNAMENT_WAVES][TOURNAMENT_MAX_KEYS + 1];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    for (int c = t; c < TOURNAMENT_WAVES * (TOURNAMENT_MAX_KEYS + 1); c += TOURNAMENT_BLOCK) (&cnt[0][0])[c] = 0;
    __syncthreads();
    const int i = blockIdx.x * TOURNAMENT_BLOCK + t;
    const int k = tournament_load_key(key, i, n_live, n_keys);
    const int below = tournament_wave_ranks(k, lane, cnt[w]);
    __syncthreads();
    if (k >= 0 && k < n_keys) {
        unsigned d = base[(size_t)k * gridDim.x + blockIdx.x] + (unsigned)below;
        for (int v = 0; v < w; v++) d += (unsigned)cnt[v][k];
        if (d < (unsigned)n_live) {   // (always: the ranks of the survivors are a permutation of [0, survivors))
            to.id[d] = from.id[i];
            if (from.my) {   // (NULL: syn_debug_tournament_regroup permutes ids alone)
                to.my[d] = from.my[i];
                to.op[d] = from.op[i];
                to.seed[d] = from.seed[i];
                to.word[d] = from.word[i];
            }
        }
    }
    if (blockIdx.x == 0) {
        if (t <= n_keys) seg_out[t] = (int)base[(size_t)t * gridDim.x];
        if (t == TOURNAMENT_BLOCK - 1) {
            const int err = search_error ? search_error[0] : 0;
            seg_out[n_keys + 1] = err != 0 ? -err : (stream_error && stream_error[0] != 0 ? -MATCH_ERR_STREAM : 0);
        }
    }
}

}  // namespace syn
