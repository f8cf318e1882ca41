// Host check of the two LDS tables behind layer 1's operands (synthesis_amd/csrc/l1_tables.cuh): the spread table that
// transposes a board to feature order, the quad table that holds whole f32x4 operands, and the composed path the lane
// kernel and policy_eval_kernel run (transpose once, four quad lookups per lane group). The reference is the cell-by-cell
// definition of Game::features (connect4.rs:235-258) in the bits mlp.cuh's feature_from_boards states:
//   mine +1.0 | theirs -1.0 | lowest empty cell of a column +0.1 | any other empty cell -0.1 | padding feature 63: -0.1
// Prints one line per part and exits 0 only if every part matched.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../../synthesis_amd/csrc/l1_tables.cuh"

using namespace syn;

static const uint32_t ONE = 0x3F800000u, TENTH = 0x3DCCCCCDu, NEG = 0x80000000u;
static const uint64_t FULL = (1ull << 63) - 1;

// the tables exactly as build_l1_tables (mlp.cuh) fills them
static std::vector<uint64_t> g_spread;
static std::vector<uint32_t> g_quad;
static void build_tables() {
    g_spread.resize(L1Tables::SPREAD_ENTRIES);
    g_quad.resize(L1Tables::QUAD_WORDS);
    for (int i = 0; i < L1Tables::SPREAD_ENTRIES; i++) g_spread[i] = l1_spread_entry((uint32_t)i);
    for (int i = 0; i < L1Tables::QUAD_WORDS; i++) g_quad[i] = l1_quad_word((uint32_t)i >> 2, i & 3);
}
static uint64_t spread_at(uint32_t p) { return g_spread.at(p); }

// ---- the reference, cell by cell
static uint32_t ref_feature_bits(uint64_t my, uint64_t op, int f) {
    if (f == 63) return TENTH | NEG;
    const int row = f / 9, col = f % 9;
    const uint64_t bit = 1ull << (row + 7 * col);
    if (my & bit) return ONE;
    if (op & bit) return ONE | NEG;
    int height = 0;
    while (height < 7 && ((my | op) >> (height + 7 * col) & 1ull)) height++;
    return row == height ? TENTH : (TENTH | NEG);
}

// mlp.cuh feature_boards, restated: hi = occupied, lo = mine | next-free
static void feature_boards(uint64_t my, uint64_t op, uint64_t& hi, uint64_t& lo) {
    uint64_t fab_row = 0;
    for (int c = 0; c < 9; c++) fab_row |= 1ull << (7 * c);
    hi = my | op;
    lo = my | (((hi << 1) | fab_row) & ~hi & FULL);
}

static long check_spread() {
    long bad = 0;
    for (uint32_t p = 0; p < 128; p++)
        for (int col = 0; col < 9; col++) {
            uint64_t want = 0;
            for (int row = 0; row < 7; row++)
                if ((p >> row) & 1u) want |= 1ull << (9 * row + col);
            const uint64_t got = l1_transpose((uint64_t)p << (7 * col), spread_at);
            if (got != want) bad++;
        }
    return bad;
}

// entry idx of the quad table as lane group q reads it: element i is feature 16*s4 + 4*i + q, whose (hi, lo) pair stands at
// l1_quad_pair_shift(i) of the index; the values do not depend on q or s4 (the padding feature's pair is (0,0) by construction)
static long check_quad() {
    long bad = 0;
    for (uint32_t idx = 0; idx < 256; idx++)
        for (int q = 0; q < 4; q++) {
            // a pair of transposed boards whose quad 3 (the one that holds the padding on q = 3) has exactly these bits
            uint64_t hi_t = 0, lo_t = 0;
            bool representable = true;
            for (int i = 0; i < 4; i++) {
                const uint32_t pair = (idx >> l1_quad_pair_shift(i)) & 3u;
                const int f = 48 + 4 * i + q;
                if (f == 63) { representable = representable && pair == 0; continue; }
                if (pair & 1u) hi_t |= 1ull << f;
                if (pair & 2u) lo_t |= 1ull << f;
            }
            uint32_t got_idx[4];
            l1_quad_indices(hi_t, lo_t, q, got_idx);
            if (representable && got_idx[3] != idx) bad++;
            if (representable && (got_idx[0] | got_idx[1] | got_idx[2]) != 0) bad++;
            for (int i = 0; i < 4; i++) {
                const uint32_t pair = (idx >> l1_quad_pair_shift(i)) & 3u;
                const uint32_t want = ((pair & 1u) ? ONE : TENTH) | ((pair & 2u) ? 0u : NEG);
                if (g_quad.at(idx * 4 + i) != want) bad++;
            }
        }
    return bad;
}

// all 64 operands of one position through the composed path against the reference
static long check_position(uint64_t my, uint64_t op) {
    uint64_t hi, lo;
    feature_boards(my, op, hi, lo);
    const uint64_t hi_t = l1_transpose(hi, spread_at), lo_t = l1_transpose(lo, spread_at);
    long bad = 0;
    for (int q = 0; q < 4; q++) {
        uint32_t idx[4];
        l1_quad_indices(hi_t, lo_t, q, idx);
        for (int s4 = 0; s4 < 4; s4++)
            for (int i = 0; i < 4; i++)
                if (g_quad.at(idx[s4] * 4 + i) != ref_feature_bits(my, op, 16 * s4 + 4 * i + q)) bad++;
    }
    return bad;
}

static bool won(uint64_t bb) {
    uint64_t fab_row = 0, cols0to5 = 0;
    for (int c = 0; c < 9; c++) fab_row |= 1ull << (7 * c);
    for (int c = 0; c < 6; c++) cols0to5 |= 0x7Full << (7 * c);
    auto rows = [&](int a, int b) { uint64_t r = 0; for (int i = a; i <= b; i++) r |= fab_row << i; return r; };
    const uint64_t d1 = bb & (bb >> 6) & (bb >> 12) & (bb >> 18) & cols0to5 & rows(3, 6);
    const uint64_t d2 = bb & (bb >> 8) & (bb >> 16) & (bb >> 24) & cols0to5 & rows(0, 3);
    const uint64_t h = bb & (bb >> 7) & (bb >> 14) & (bb >> 21) & cols0to5;
    const uint64_t v = bb & (bb >> 1) & (bb >> 2) & (bb >> 3) & rows(0, 3);
    return (v | h | d1 | d2) != 0;
}

int main() {
    build_tables();
    const long bad_spread = check_spread();
    printf("spread %d patterns x 9 columns: %ld mismatches\n", 128, bad_spread);
    const long bad_quad = check_quad();
    printf("quad 256 indices x 4 lane groups: %ld mismatches\n", bad_quad);

    // the empty board, full boards (alternating columns of stones, both ways round), then every position of random games
    long n_pos = 0, bad_pos = 0;
    bad_pos += check_position(0, 0); n_pos++;
    uint64_t a = 0;
    for (int col = 0; col < 9; col++)
        for (int row = 0; row < 7; row++)
            if ((col + row / 2) & 1) a |= 1ull << (row + 7 * col);
    bad_pos += check_position(a, FULL & ~a); n_pos++;
    bad_pos += check_position(FULL & ~a, a); n_pos++;
    std::mt19937_64 rng(20261019);
    while (n_pos < 120000) {
        uint64_t my = 0, op = 0;
        for (;;) {
            const uint64_t occ = my | op;
            int legal[9], n_legal = 0;
            for (int c = 0; c < 9; c++)
                if (!((occ >> (6 + 7 * c)) & 1ull)) legal[n_legal++] = c;
            if (n_legal == 0) break;
            const int col = legal[rng() % (uint64_t)n_legal];
            int height = 0;
            while ((occ >> (height + 7 * col)) & 1ull) height++;
            const uint64_t mover = my | (1ull << (height + 7 * col));
            my = op;
            op = mover;
            bad_pos += check_position(my, op); n_pos++;
            if (won(mover)) break;
        }
    }
    printf("composed path, %ld reachable positions x 64 operands: %ld mismatches\n", n_pos, bad_pos);
    return (bad_spread | bad_quad | bad_pos) == 0 ? 0 : 1;
}
