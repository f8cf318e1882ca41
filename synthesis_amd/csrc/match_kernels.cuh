// Device-resident matches (syn_match_run / syn_match_run_sides, engine.hip): what runs between two plies' search launches.
// The live games of a match are five parallel arrays — my[i], op[i] (the position, mover's stones first: the roots of the next search
// launch), id[i] (which game of the call job i is), seed[i] and word[i] (the game's rollout generator, StdRng::seed_from_u64(seed), and
// its first unused output word: what a baseline side's frozen_rollout_kernel reads and advances in place) — in game order. After a
// ply's search
//     match_advance_kernel   plays job i's best_action on its position and writes keep[i]: 1 = the game goes on, 0 = it ended here
//                            (its reward, ply count, final position and stream position are written to the call's outputs, indexed by
//                            game). One template over the search's result record: DevSearchResult (a network side's MODE_SEARCH launch)
//                            or FrozenResult (a baseline side's), of which it reads best_action and num_nodes alone.
//     an exclusive sum of keep (hipcub, as syn_replay_keep_games_from)
//     match_compact_kernel   moves every surviving job to its rank among the survivors, into the second set of arrays, and leaves the
//                            number of survivors — the one word the host reads per ply
// A game's record depends on its own position and its own generator alone, never on its job index: compaction keeps game order and
// carries the generator with the game, and nothing here is indexed by job except the arrays it permutes. One thread per job, plain
// loads and stores, no LDS, no atomics, and no workgroup waits for another.
#pragma once
#include <hip/hip_runtime.h>

#include "device_common.cuh"
#include "engine_kernels.cuh"
#include "frozen_kernel.cuh"

namespace syn {

constexpr int MATCH_T = 63;                    // Connect4::MAX_TURNS: move slots per game
constexpr unsigned char MATCH_NO_MOVE = 255;   // a move slot the game never reached
// a generator's stream position beyond which the next baseline search could run past 2^32 output words (frozen_rollout_kernel keeps
// 32 bits of it): syn_frozen_search_rollout refuses such a start, a match ends with the code below
constexpr unsigned long long MATCH_WORD_LIMIT = 0xC0000000ull;
constexpr int MATCH_ERR_STREAM = 0x10000;      // live_out = -MATCH_ERR_STREAM (the search kernels' own error words are 1 and 2)

// The per-game outputs of a call (device), indexed by game.
struct MatchOut {
    float* rewards;                // +1 / 0 / -1 for the player that moved first
    int* plies;                    // moves played in the match
    unsigned char* moves;          // [n][MATCH_T], MATCH_NO_MOVE where the game was over
    unsigned long long* final_bb;  // [n][2]: the first mover's stones, the second mover's
    unsigned long long* rng_words; // the game's stream position when it ended
};

// game.step(&best_action) (connect4.rs:221-233) for every live job; `ply` = moves played so far (even: the first player moves).
// A job whose root was not searched (num_nodes == 0: syn_cancel kept it from starting) is dropped without a record — the call
// returns SYN_ERR_CANCELLED then. The column is checked before it is played: a record never comes from an illegal move.
// word[i] is the stream position the ply's search left (a network ply leaves it alone). A position past MATCH_WORD_LIMIT raises
// stream_error[0]: every thread that sees one stores the same 1, so the plain stores need no order among themselves.
// The rules for ONE job (shared with tournament_advance_kernel, tournament_kernels.cuh): job i's search record is `res`, its game g.
// Returns whether the game goes on.
template <class Result>
SYN_DEV bool match_advance_job(const Result& res, int i, int g, int ply, unsigned long long* __restrict__ my,
                               unsigned long long* __restrict__ op, const unsigned long long* __restrict__ word,
                               int* __restrict__ stream_error, const MatchOut& out) {
    const int col = res.best_action;
    const uint64_t m = my[i], o = op[i], occ = m | o;
    const unsigned long long w_pos = word[i];
    if (w_pos > MATCH_WORD_LIMIT) stream_error[0] = 1;
    const bool searched = res.num_nodes != 0u && col >= 0 && col < c4::WIDTH;
    const int h = searched ? c4::col_height(occ, col) : c4::HEIGHT;
    if (h >= c4::HEIGHT) return false;
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
        out.rng_words[g] = w_pos;
        return false;
    }
    my[i] = o;      // the opponent moves next: its stones first
    op[i] = mover;
    return true;
}

template <class Result>
__global__ void __launch_bounds__(256) match_advance_kernel(
    const Result* __restrict__ results, int n_live, int ply, unsigned long long* __restrict__ my, unsigned long long* __restrict__ op,
    const int* __restrict__ id, const unsigned long long* __restrict__ word, unsigned* __restrict__ keep, int* __restrict__ stream_error,
    MatchOut out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_live) return;
    keep[i] = match_advance_job(results[i], i, id[i], ply, my, op, word, stream_error, out) ? 1u : 0u;
}

// The live games' arrays, one set: a ply's compaction reads one set and writes the other.
struct MatchLive {
    unsigned long long* my;
    unsigned long long* op;
    int* id;
    unsigned long long* seed;
    unsigned long long* word;
};

// Stable compaction: surviving job i goes to dst[i] (= its rank among the survivors) of the second arrays, its generator with it. The
// thread of the last job also writes live_out[0]: the number of survivors, or -(the search kernel's error word) when the ply's search
// reported one (EngineParams::error / FrozenParams::error; the host's next launch resets it), or -MATCH_ERR_STREAM when a generator
// ran past MATCH_WORD_LIMIT (stream_error, written by the advance kernel that ran before this one on the same stream).
__global__ void __launch_bounds__(256) match_compact_kernel(
    const unsigned* __restrict__ keep, const unsigned* __restrict__ dst, int n_live, MatchLive from, MatchLive to,
    const int* __restrict__ search_error, const int* __restrict__ stream_error, int* __restrict__ live_out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_live) return;
    const unsigned k = keep[i], d = dst[i];
    if (k && d < (unsigned)n_live) {
        to.my[d] = from.my[i];
        to.op[d] = from.op[i];
        to.id[d] = from.id[i];
        to.seed[d] = from.seed[i];
        to.word[d] = from.word[i];
    }
    if (i == n_live - 1) {
        const int err = search_error[0];
        live_out[0] = err != 0 ? -err : (stream_error[0] != 0 ? -MATCH_ERR_STREAM : (int)(d + k));
    }
}

}  // namespace syn
