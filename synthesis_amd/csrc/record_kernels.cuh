// Recorded device games (syn_games_run_recorded, engine.hip; include/synthesis_amd.h "Recorded games"): run_games' loop with
// run_game's per-move tail (alpha_zero.rs:243-264) and its game end (fill_state_info / store_rewards, 295-338) computed from what
// the loop already holds after a ply — the job's DevSearchResult, its position and its generator — instead of from a tree:
//     record_advance_kernel   takes tournament_advance_kernel's place: one thread per job of a group's range. Writes the row (when
//                             the mover is recorded), chooses the action as selfplay_move_step does (engine_kernels.cuh), advances the
//                             game's stream position, applies mcts.solution(action) and the stop rule, steps the position, and at the
//                             game's end writes the per-game outputs
//     record_finish_kernel    once after the last ply, one thread per (game, row): z by parity from the game's last position, t, and
//                             store_rewards in place over the q the advance kernel staged in vs
// What the tree gave selfplay_move_step comes from the record: pi = target_pi, q = target_q, best = best_action (the player's action
// selection went into the search), T.next_node = num_nodes, and mcts.solution(a) = child_sol[a] (all zero for a column that is no
// child). The legal mask comes from the position. The float expressions are selfplay_move_step's, operand for operand, under the
// translation unit's -ffp-contract=off.
// A game's record depends on its own position and generator alone, never on its job index: rows are indexed by game, and the regroup
// carries seed and word with the game. Plain vector loads and stores, no LDS, no atomics: game g belongs to one job per ply, so its
// row counter has one writer per launch, and launches are ordered by the stream.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

#include "device_common.cuh"
#include "engine_kernels.cuh"
#include "match_kernels.cuh"

namespace syn {

// DevSearchResult has a 372-byte stride (not a multiple of 8 or 16): its fields are read as dwords
constexpr int RECORD_RES_DWORDS = (int)(sizeof(DevSearchResult) / 4);
constexpr int RECORD_RES_SOL = (int)(offsetof(DevSearchResult, child_sol) / 4);
constexpr int RECORD_RES_NODES = (int)(offsetof(DevSearchResult, num_nodes) / 4);
constexpr int RECORD_RES_BEST = (int)(offsetof(DevSearchResult, best_action) / 4);
constexpr int RECORD_RES_PI = (int)(offsetof(DevSearchResult, target_pi) / 4);
constexpr int RECORD_RES_Q = (int)(offsetof(DevSearchResult, target_q) / 4);
static_assert(sizeof(DevSearchResult) % 4 == 0 && offsetof(DevSearchResult, child_sol) % 4 == 0, "DevSearchResult is read as dwords");

// the call's sample_action / stop rule (RolloutConfig, alpha_zero.rs:270-293); turns count from the start position
struct RecordRules {
    int random_until;
    int sample_until;
    int stop_when_solved;
};

// The rows of a call (device): the engine's self-play output buffers, slot = game, row r = the r-th recorded ply of the game.
struct RecordOut {
    int* rows;                     // [n] rows of game g so far
    unsigned long long* states_bb; // [n][63][2]
    float* pis;                    // [n][63][9]
    float* vs;                     // [n][63][3]: target_q until record_finish_kernel has run
    unsigned char* actions;        // [n][63]
    uint32_t* root_nodes;          // [n][63]
    unsigned char* final_kind;     // [n]
    unsigned char* row_ply;        // [n][63] the ply (from the start position) a row was recorded at
};

// jobs [lo, lo + n) of the live arrays, one thread per job; `results` = that range's own record array as dwords (job lo's record
// first). `recorded`: the group's mover has its bit in the call's record_mask. A job whose root was not searched (num_nodes == 0:
// syn_cancel kept it from starting) or whose chosen column cannot be played is dropped without a record, as match_advance_job drops it.
__global__ void __launch_bounds__(256) record_advance_kernel(
    const unsigned* __restrict__ results, int lo, int n, int ply, int recorded, RecordRules rules, unsigned long long* __restrict__ my,
    unsigned long long* __restrict__ op, const int* __restrict__ id, const unsigned long long* __restrict__ seed,
    unsigned long long* __restrict__ word, const int* __restrict__ first, const int* __restrict__ second, int n_keys,
    int* __restrict__ key, int* __restrict__ stream_error, MatchOut out, RecordOut rec) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const int i = lo + j;
    const int g = id[i];
    const unsigned* r = results + (size_t)j * RECORD_RES_DWORDS;
    const uint32_t num_nodes = r[RECORD_RES_NODES];
    const int best = (int)r[RECORD_RES_BEST];
    const uint64_t m = my[i], o = op[i], occ = m | o;
    unsigned long long w_pos = word[i];
    if (w_pos > MATCH_WORD_LIMIT) stream_error[0] = 1;   // (the generator's block counter keeps 32 bits of the position)
    key[i] = n_keys;
    if (num_nodes == 0u || best < 0 || best >= c4::WIDTH) return;

    uint32_t lmask = 0;
#pragma unroll
    for (int c = 0; c < 9; c++) lmask |= c4::col_height(occ, c) < c4::HEIGHT ? (1u << c) : 0u;
    float pi[9];
#pragma unroll
    for (int c = 0; c < 9; c++) pi[c] = __uint_as_float(r[RECORD_RES_PI + c]);

    // sample_action (alpha_zero.rs:270-294), as selfplay_move_step takes its draws
    const bool want_random = ply < rules.random_until;
    const bool maybe_sample = !want_random && ply < rules.sample_until;
    const bool best_solved = r[RECORD_RES_SOL + 3 * best] != 0u;
    StdRng rng;
    uint32_t rnd = 0;
    if (want_random || maybe_sample) {
        rng.seed_from_u64(seed[i]);
        rnd = rng.word((uint32_t)w_pos);
    }
    int action;
    if (want_random) {
        // Rng::gen_range(0..n) for u8 (device_common.cuh StdRng::gen_range_u8), first candidate = rnd
        const uint32_t nl = (uint32_t)__popc(lmask);
        const uint32_t zone = 0xFFFFFFFFu - (0xFFFFFFFFu - nl + 1u) % nl;
        uint64_t mm = (uint64_t)rnd * (uint64_t)nl;
        w_pos += 1;
        while ((uint32_t)mm > zone) {   // rejected (probability ~1e-9): draw again
            mm = (uint64_t)rng.word((uint32_t)w_pos) * (uint64_t)nl;
            w_pos += 1;
        }
        const uint32_t nth = (uint32_t)(mm >> 32);
        uint32_t lm = lmask;
        for (uint32_t k = 0; k < nth; k++) lm &= lm - 1u;   // iter_actions().nth(r)
        action = __ffs((int)lm) - 1;
    } else if (maybe_sample && (!best_solved || !rules.stop_when_solved)) {
        // WeightedIndex::new(search_policy).sample(rng): 9 weights by column
        float cum[8];
        float total = pi[0];
#pragma unroll
        for (int c = 1; c < 9; c++) {
            cum[c - 1] = total;
            total += pi[c];
        }
        // Uniform<f32>::new(0, total).sample: [1,2) from the top 23 bits, minus 1, times total
        const float chosen = (__uint_as_float((rnd >> 9) | 0x3F800000u) - 1.0f) * total + 0.0f;
        w_pos += 1;
        int idx = 0;
#pragma unroll
        for (int c = 0; c < 8; c++) idx = cum[c] <= chosen ? c + 1 : idx;
        action = idx;
    } else {
        action = best;
    }
    if (action < 0 || action >= c4::WIDTH) return;
    const int hgt = c4::col_height(occ, action);
    if (hgt >= c4::HEIGHT) return;   // a record never comes from an illegal move

    // buffer.add(&game, &search_policy, ..) + StateInfo::q (alpha_zero.rs:248-250)
    if (recorded) {
        const int row = rec.rows[g];
        if (row >= 0 && row < MATCH_T) {
            const size_t pos = (size_t)g * MATCH_T + (size_t)row;
            rec.states_bb[pos * 2 + 0] = m;
            rec.states_bb[pos * 2 + 1] = o;
            rec.root_nodes[pos] = num_nodes;
#pragma unroll
            for (int c = 0; c < 9; c++) rec.pis[pos * 9 + c] = pi[c];
#pragma unroll
            for (int c = 0; c < 3; c++) rec.vs[pos * 3 + c] = __uint_as_float(r[RECORD_RES_Q + c]);
            rec.actions[pos] = (unsigned char)action;
            rec.row_ply[pos] = (unsigned char)ply;
            rec.rows[g] = row + 1;
        }
    }

    // solution = mcts.solution(&action) (alpha_zero.rs:254, mcts.rs:296-306): child_sol is all zero for a column that is no child
    bool sol_some = r[RECORD_RES_SOL + 3 * action] != 0u;
    uint32_t sol_kind = r[RECORD_RES_SOL + 3 * action + 1];

    // game.step(&action) (connect4.rs:221-233)
    const uint64_t bit = 1ull << (hgt + 7 * action);
    const uint64_t mover = m | bit;
    const bool w = c4::won(mover);
    const bool full = (occ | bit) == c4::FULL;
    if (w || full) {
        sol_some = true;
        sol_kind = w ? 0u : 1u;   // reward(player to move).into(): the mover won -> Lose(0); else Draw(0)
    } else if (!rules.stop_when_solved) {
        sol_some = false;
    }
    out.moves[(size_t)g * MATCH_T + ply] = (unsigned char)action;
    if (!sol_some) {
        my[i] = o;   // the opponent moves next: its stones first
        op[i] = mover;
        word[i] = w_pos;
        // after ply `ply` an even number of moves has been played when ply is odd: the first player moves again
        key[i] = (ply & 1) ? first[g] : second[g];
        return;
    }
    // the game is over (or solved, with stop_games_when_solved): sol_kind is the outcome for the player that would move next
    const bool first_moved = (ply & 1) == 0;
    const float mover_reward = sol_kind == 1u ? 0.0f : (sol_kind == 0u ? 1.0f : -1.0f);
    out.rewards[g] = first_moved ? mover_reward : 0.0f - mover_reward;
    out.plies[g] = ply + 1;
    out.final_bb[2 * (size_t)g + 0] = first_moved ? mover : o;
    out.final_bb[2 * (size_t)g + 1] = first_moved ? o : mover;
    out.rng_words[g] = w_pos;
    rec.final_kind[g] = (unsigned char)sol_kind;
}

// fill_state_info(solution.reversed()) + store_rewards for every row of the call: thread (g, row) over n_games * 63. `plies` = all
// moves of the game, recorded or not; a row's turn is its ply + 1.
__global__ void __launch_bounds__(256) record_finish_kernel(int n_games, const int* __restrict__ plies, int value_target, float vt_p,
                                                            float vt_from, float vt_to, RecordOut rec) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)n_games * MATCH_T) return;
    const int g = (int)(idx / MATCH_T), row = (int)(idx % MATCH_T);
    if (row >= rec.rows[g]) return;
    const int n = plies[g];
    const int i = (int)rec.row_ply[idx];
    if (n <= 0 || i >= n) return;   // (a game that did not end: the call fails)
    const uint32_t sol_kind = rec.final_kind[g];
    const uint32_t last_kind = sol_kind == 1u ? 1u : 2u - sol_kind;   // kind of solution.reversed()
    // outcome seen from position i: reversed once per step back from the last position
    const bool flip = ((n - 1 - i) & 1) != 0;
    const uint32_t zk = (flip && last_kind != 1u) ? 2u - last_kind : last_kind;
    const float z0 = zk == 0u ? 1.0f : 0.0f, z1 = zk == 1u ? 1.0f : 0.0f, z2 = zk == 2u ? 1.0f : 0.0f;
    const float t = (float)(i + 1) / (float)n;
    float* v = rec.vs + idx * 3;
    const float a0 = v[0], a1 = v[1], a2 = v[2];
    float o0, o1, o2;
    if (value_target == 1) { o0 = a0; o1 = a1; o2 = a2; }
    else if (value_target == 0) { o0 = z0; o1 = z1; o2 = z2; }
    else if (value_target == 2) {
        const float p = vt_p;
        o0 = a0 * p + z0 * (1.0f - p);
        o1 = a1 * p + z1 * (1.0f - p);
        o2 = a2 * p + z2 * (1.0f - p);
    } else {
        const float p = (1.0f - t) * vt_from + t * vt_to;
        o0 = a0 * (1.0f - p) + z0 * p;
        o1 = a1 * (1.0f - p) + z1 * p;
        o2 = a2 * (1.0f - p) + z2 * p;
    }
    v[0] = o0; v[1] = o1; v[2] = o2;
}

}  // namespace syn
