// Device-resident games (run_games in engine.hip, behind syn_match_run / syn_match_run_sides / syn_tournament_run): the live games'
// arrays, the per-game outputs and the rules of one game step. The loop's kernels are in tournament_kernels.cuh.
// The live games of a call are five parallel arrays — my[i], op[i] (the position, mover's stones first: the roots of the next search
// launch), id[i] (which game of the call job i is), seed[i] and word[i] (the game's rollout generator, StdRng::seed_from_u64(seed), and
// its first unused output word: what a baseline player's frozen_rollout_kernel reads and advances in place). After a ply's search
// match_advance_job plays job i's best_action on its position and says whether the game goes on; when it ended, its reward, ply count,
// final position and stream position are written to the call's outputs, indexed by game. One template over the search's result
// record: DevSearchResult (a network player's MODE_SEARCH launch) or FrozenResult (a baseline player's), of which it reads best_action
// and num_nodes alone.
// A game's record depends on its own position and its own generator alone, never on its job index: the loop's regroup carries the
// generator with the game, and nothing here is indexed by job except the arrays it permutes. Plain loads and stores, no LDS, no atomics.
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
constexpr int MATCH_ERR_STREAM = 0x10000;      // the ply's error word = -MATCH_ERR_STREAM (the search kernels' own error words are 1 and 2)

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
// The rules for ONE job (tournament_advance_kernel, tournament_kernels.cuh, runs them per group): job i's search record is `res`,
// its game g. Returns whether the game goes on.
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

// The live games' arrays, one set: a ply's regroup reads one set and writes the other.
struct MatchLive {
    unsigned long long* my;
    unsigned long long* op;
    int* id;
    unsigned long long* seed;
    unsigned long long* word;
};

}  // namespace syn
