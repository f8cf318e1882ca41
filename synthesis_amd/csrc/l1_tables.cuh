// synthesis_amd — layer-1 B operands of the Connect4Net tile from two small LDS tables.
//
// The network's first layer reads 63 cell features, f = 9*row + col, each one of four constants chosen by two bits of the
// derived boards (mlp.cuh feature_boards: hi = occupied, lo = mine | next-free):
//   (hi,lo) = (1,1) +1.0 | (1,0) -1.0 | (0,1) +0.1 | (0,0) -0.1      magnitude = hi ? 1.0 : 0.1, sign bit = !lo
// Lane (j,q) of a tile consumes features 4m + q, m = 0..15 (feature 63 is padding: its weight column is zero). The boards
// arrive in the game's column-major layout, bit row + 7*col, so feature 4m + q sits at a different bit on every lane and for
// every m. Instead of two variable 64-bit shifts and a select per feature:
//   1. the boards are transposed ONCE to feature order (bit f = cell f) through the SPREAD table: entry p is the 7-bit
//      column pattern p with its rows at stride 9, and column c's entry goes in shifted left by c;
//   2. lane (j,q) shifts both transposed boards right by q (feature 4m + q is then bit 4m), interleaves them
//      (bit 4m = hi, bit 4m + 1 = lo), and folds each 32-bit half once (y = c | c << 6): the eight bits of operand quad s4
//      (features 16*s4 + 4*i + q, i = 0..3) are then the contiguous byte at bit 6 + 16*(s4 & 1) of half s4 >> 1;
//   3. that byte indexes the QUAD table, whose 16-byte entry is the whole f32x4 operand: one ds_read_b128 per quad.
// Everything here is plain integer code for host and device alike, so a host program checks the very functions the
// kernels run (tests/cpp/l1_tables_check.cpp).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define SYN_L1_HD __host__ __device__ inline
#else
#define SYN_L1_HD inline
#endif

namespace syn {

struct L1Tables {
    static constexpr int SPREAD_ENTRIES = 128;                       // 7-bit column patterns, 8 bytes each
    static constexpr int QUAD_ENTRIES = 256;                         // 8-bit quad indices, 16 bytes each
    static constexpr int SPREAD_BYTES = SPREAD_ENTRIES * 8;          // 1 KB
    static constexpr int QUAD_BYTES = QUAD_ENTRIES * 16;             // 4 KB
    static constexpr int BYTES = SPREAD_BYTES + QUAD_BYTES;          // the spread table first, then the quad table
    static constexpr int QUAD_WORDS = QUAD_ENTRIES * 4;
};

// SPREAD entry p: bit `row` of the column pattern -> bit 9*row.
SYN_L1_HD uint64_t l1_spread_entry(uint32_t p) {
    uint64_t r = 0;
    for (int row = 0; row < 7; row++)
        if ((p >> row) & 1u) r |= 1ull << (9 * row);
    return r;
}

// Where the fold leaves the (hi, lo) bit pair of element i of a quad inside the 8-bit index: elements 0 and 1 come from the
// shifted copy, 2 and 3 from the original, so the pairs stand in the order 0, 2, 1, 3.
SYN_L1_HD int l1_quad_pair_shift(int i) { return 2 * (((i & 1) << 1) | (i >> 1)); }

// QUAD table word: the f32 bits of element i (0..3) of entry idx (0..255).
SYN_L1_HD uint32_t l1_quad_word(uint32_t idx, int i) {
    const uint32_t pair = (idx >> l1_quad_pair_shift(i)) & 3u;
    const uint32_t hi = pair & 1u, lo = pair >> 1;
    return (hi ? 0x3F800000u : 0x3DCCCCCDu) | ((lo ^ 1u) << 31);
}

// A column-major board (bit row + 7*col, 9 columns of 7) to feature order (bit 9*row + col). `spread(p)` returns SPREAD entry p.
template <class Spread>
SYN_L1_HD uint64_t l1_transpose(uint64_t board, Spread spread) {
    uint64_t r = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int col = 0; col < 9; col++) r |= spread((uint32_t)(board >> (7 * col)) & 0x7Fu) << col;
    return r;
}

// The QUAD table indices of the four layer-1 operand quads of lane group q (0..3) from the two transposed boards.
SYN_L1_HD void l1_quad_indices(uint64_t hi_t, uint64_t lo_t, int q, uint32_t (&idx)[4]) {
    const uint64_t m = 0x1111111111111111ull;
    const uint64_t c = ((hi_t >> q) & m) | (((lo_t >> q) & m) << 1);
    const uint32_t c0 = (uint32_t)c, c1 = (uint32_t)(c >> 32);
    const uint32_t y0 = c0 | (c0 << 6), y1 = c1 | (c1 << 6);
    idx[0] = (y0 >> 6) & 0xFFu;
    idx[1] = (y0 >> 22) & 0xFFu;
    idx[2] = (y1 >> 6) & 0xFFu;
    idx[3] = (y1 >> 22) & 0xFFu;
}

}  // namespace syn
