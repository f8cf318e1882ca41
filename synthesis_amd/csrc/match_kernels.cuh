// Device-resident matches between two networks (syn_match_run, engine.hip): what runs between two plies' search launches.
// The live games of a match are three parallel arrays — my[i], op[i] (the position, mover's stones first: the roots of the
// next MODE_SEARCH launch) and id[i] (which game of the call job i is) — in game order. After a ply's search
//     match_advance_kernel   plays job i's best_action on its position and writes keep[i]: 1 = the game goes on, 0 = it ended here
//                            (its reward, ply count and final position are written to the call's outputs, indexed by game)
//     an exclusive sum of keep (hipcub, as syn_replay_keep_games_from)
//     match_compact_kernel   moves every surviving job to its rank among the survivors, into the second set of arrays, and leaves the
//                            number of survivors — the one word the host reads per ply
// A game's record depends on its own position alone, never on its job index: compaction keeps game order, and nothing here is
// indexed by job except the arrays it permutes. One thread per job, plain loads and stores, no LDS, no atomics, and no workgroup
// waits for another.
#pragma once
#include <hip/hip_runtime.h>

#include "device_common.cuh"
#include "engine_kernels.cuh"

namespace syn {

constexpr int MATCH_T = 63;                    // Connect4::MAX_TURNS: move slots per game
constexpr unsigned char MATCH_NO_MOVE = 255;   // a move slot the game never reached

// The per-game outputs of a call (device), indexed by game.
struct MatchOut {
    float* rewards;                // +1 / 0 / -1 for the player that moved first
    int* plies;                    // moves played in the match
    unsigned char* moves;          // [n][MATCH_T], MATCH_NO_MOVE where the game was over
    unsigned long long* final_bb;  // [n][2]: the first mover's stones, the second mover's
};

// game.step(&best_action) (connect4.rs:221-233) for every live job; `ply` = moves played so far (even: the first player moves).
// A job whose root was not searched (num_nodes == 0: syn_cancel kept it from starting) is dropped without a record — the call
// returns SYN_ERR_CANCELLED then. The column is checked before it is played: a record never comes from an illegal move.
__global__ void __launch_bounds__(256) match_advance_kernel(
    const DevSearchResult* __restrict__ results, int n_live, int ply, unsigned long long* __restrict__ my,
    unsigned long long* __restrict__ op, const int* __restrict__ id, unsigned* __restrict__ keep, MatchOut out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_live) return;
    const int col = results[i].best_action;
    const uint64_t m = my[i], o = op[i], occ = m | o;
    const bool searched = results[i].num_nodes != 0u && col >= 0 && col < c4::WIDTH;
    const int h = searched ? c4::col_height(occ, col) : c4::HEIGHT;
    if (h >= c4::HEIGHT) {
        keep[i] = 0u;
        return;
    }
    const int g = id[i];
    const uint64_t bit = 1ull << (h + 7 * col);
    const uint64_t mover = m | bit;
    const bool w = c4::won(mover);
    const bool full = (occ | bit) == c4::FULL;
    out.moves[(size_t)g * MATCH_T + ply] = (unsigned char)col;
    if (w || full) {
        const bool first_moved = (ply & 1) == 0;
        out.rewards[g] = w ? (first_moved ? 1.0f : -1.0f) : 0.0f;   // game.reward(first player) (evaluator.rs:160)
        out.plies[g] = ply + 1;
        out.final_bb[2 * (size_t)g + 0] = first_moved ? mover : o;
        out.final_bb[2 * (size_t)g + 1] = first_moved ? o : mover;
        keep[i] = 0u;
    } else {
        my[i] = o;      // the opponent moves next: its stones first
        op[i] = mover;
        keep[i] = 1u;
    }
}

// Stable compaction: surviving job i goes to dst[i] (= its rank among the survivors) of the second arrays. The thread of the last
// job also writes live_out[0]: the number of survivors, or -(the search kernel's error word) when the ply's search reported one
// (EngineParams::error; the host's next launch resets it).
__global__ void __launch_bounds__(256) match_compact_kernel(
    const unsigned* __restrict__ keep, const unsigned* __restrict__ dst, int n_live, const unsigned long long* __restrict__ my,
    const unsigned long long* __restrict__ op, const int* __restrict__ id, unsigned long long* __restrict__ my_next,
    unsigned long long* __restrict__ op_next, int* __restrict__ id_next, const int* __restrict__ search_error,
    int* __restrict__ live_out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_live) return;
    const unsigned k = keep[i], d = dst[i];
    if (k && d < (unsigned)n_live) {
        my_next[d] = my[i];
        op_next[d] = op[i];
        id_next[d] = id[i];
    }
    if (i == n_live - 1) {
        const int err = search_error[0];
        live_out[0] = err != 0 ? -err : (int)(d + k);
    }
}

}  // namespace syn
