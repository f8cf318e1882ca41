// synthesis_amd — where stored positions and the scratch areas of the replay / data-set host code lie: byte sizes, column pointers and
// carved layouts, as pure functions of plain numbers. Host-only C++17 without a HIP header, so the layouts are read and tested on a
// CPU (tests/test_position_layout.py). engine.hip allocates what a layout asks for and hands the pointers to the kernels.
#pragma once
#include <cstddef>
#include <cstdint>

namespace syn {

// One stored position, column by column: two boards, an optional game id, the policy target and the value target.
constexpr size_t POS_BOARD_BYTES = 8;
constexpr size_t POS_GID_BYTES = 8;
constexpr size_t POS_PI_FLOATS = 9, POS_PI_BYTES = POS_PI_FLOATS * 4;
constexpr size_t POS_V_FLOATS = 3, POS_V_BYTES = POS_V_FLOATS * 4;
constexpr size_t POS_ROW_BYTES = 2 * POS_BOARD_BYTES + POS_PI_BYTES + POS_V_BYTES;   // 64: the learner's and the evaluation's data sets
constexpr size_t POS_ROW_GID_BYTES = POS_ROW_BYTES + POS_GID_BYTES;                  // 72: the replay buffer
constexpr size_t SEARCH_RESULT_BYTES = 372;   // engine_kernels.cuh DevSearchResult (engine.hip static_asserts it)

// One device allocation carved into sections, each 256-byte aligned: take() returns the next section's byte offset, `at` ends as the total.
inline size_t align256(size_t bytes) { return (bytes + 255) & ~(size_t)255; }
struct Carve {
    size_t at = 0;
    size_t take(size_t bytes) {
        const size_t o = at;
        at += align256(bytes);
        return o;
    }
};
constexpr size_t ABSENT = ~(size_t)0;   // the offset of a section that a layout does not have

// n positions stored as columns my | op | [gid] | pi | v. A column that is not there (or that a caller does not want) is null.
struct PositionColumns {
    unsigned long long* my;
    unsigned long long* op;
    long long* gid;
    float* pi;
    float* v;
};
// The columns of one allocation of `capacity` rows at `base`: the replay buffer (with_gid) or a data set / staged batch (without).
inline PositionColumns columns_at(void* base, size_t capacity, bool with_gid) {
    unsigned char* b = static_cast<unsigned char*>(base);
    const size_t o_pi = capacity * (2 * POS_BOARD_BYTES + (with_gid ? POS_GID_BYTES : 0));
    return {reinterpret_cast<unsigned long long*>(b), reinterpret_cast<unsigned long long*>(b + capacity * POS_BOARD_BYTES),
            with_gid ? reinterpret_cast<long long*>(b + capacity * 2 * POS_BOARD_BYTES) : nullptr, reinterpret_cast<float*>(b + o_pi),
            reinterpret_cast<float*>(b + o_pi + capacity * POS_PI_BYTES)};
}
// the same columns from row `at` on
inline PositionColumns columns_from(const PositionColumns& s, size_t at) {
    return {s.my + at, s.op + at, s.gid ? s.gid + at : nullptr, s.pi + at * POS_PI_FLOATS, s.v + at * POS_V_FLOATS};
}
// a caller's five arrays (the C ABI's types); a source that is only read enters here too
inline PositionColumns columns_of(const uint64_t* my, const uint64_t* op, const int64_t* gid, const float* pi, const float* v) {
    return {reinterpret_cast<unsigned long long*>(const_cast<uint64_t*>(my)), reinterpret_cast<unsigned long long*>(const_cast<uint64_t*>(op)),
            reinterpret_cast<long long*>(const_cast<int64_t*>(gid)), const_cast<float*>(pi), const_cast<float*>(v)};
}

// A data set of the engine's own (the learner's, the evaluation's): an allocation with room for `cap` rows that holds n of them as
// columns_at(d, n, false) — the columns are packed for the set's size, not for the capacity.
struct PositionRows {
    void* d = nullptr;
    size_t cap = 0, n = 0;
};

// Four columns of `rows` positions as carved sections of their own (no game id); pi and v can be left out.
struct ColumnOffsets {
    size_t my, op, pi, v;
};
inline ColumnOffsets carve_columns(Carve& c, size_t rows, bool with_pi = true, bool with_v = true) {
    ColumnOffsets o;
    o.my = c.take(rows * POS_BOARD_BYTES);
    o.op = c.take(rows * POS_BOARD_BYTES);
    o.pi = with_pi ? c.take(rows * POS_PI_BYTES) : ABSENT;
    o.v = with_v ? c.take(rows * POS_V_BYTES) : ABSENT;
    return o;
}
inline PositionColumns columns_in(void* base, const ColumnOffsets& o) {
    unsigned char* b = static_cast<unsigned char*>(base);
    return {reinterpret_cast<unsigned long long*>(b + o.my), reinterpret_cast<unsigned long long*>(b + o.op), nullptr,
            o.pi != ABSENT ? reinterpret_cast<float*>(b + o.pi) : nullptr, o.v != ABSENT ? reinterpret_cast<float*>(b + o.v) : nullptr};
}

// The de-duplication core's work area for n positions (replay_kernels.cuh), in carve order:
//   sort keys and buffer indices (double buffers) | heads | their scan | segment starts | the output rows and their counts | cub temp
// and for the symmetric form, whose outputs have 2n rows: | canonical boards | flip flags | expand flags | their scan
struct DedupLayout {
    size_t k0, k1, i0, i1, head, scan, start;
    size_t rows;         // output rows: n, with mirror 2n
    ColumnOffsets out;
    size_t out_num, tmp;
    size_t c_my, c_op, flip, expand, dst;   // ABSENT without mirror
    size_t total;
};
inline DedupLayout dedup_layout(size_t n, size_t tmp_bytes, bool mirror) {
    DedupLayout L{};
    Carve c;
    L.k0 = c.take(n * 8); L.k1 = c.take(n * 8); L.i0 = c.take(n * 4); L.i1 = c.take(n * 4);
    L.head = c.take(n * 4); L.scan = c.take(n * 4); L.start = c.take(n * 4);
    L.rows = mirror ? 2 * n : n;
    L.out = carve_columns(c, L.rows);
    L.out_num = c.take(L.rows * 4);
    L.tmp = c.take(tmp_bytes);
    L.c_my = L.c_op = L.flip = L.expand = L.dst = ABSENT;
    if (mirror) { L.c_my = c.take(n * 8); L.c_op = c.take(n * 8); L.flip = c.take(n * 4); L.expand = c.take(n * 4); L.dst = c.take(n * 4); }
    L.total = c.at;
    return L;
}

// syn_replay_reanalyse's and syn_replay_select_positions' scratch (reanalyse_kernels.cuh):
//   [sel n][skip n][dst n][job_my n][job_op n][job_row n][moved n][done n][counts: skipped, moved, done][cub temp][results of one chunk]
// (the job arrays are sized for every row: the scratch is laid out before the number of selected rows is known)
struct ReanalyseLayout {
    size_t sel, skip, dst, job_my, job_op, job_row, moved, done, counts, tmp, results, total;
};
inline ReanalyseLayout reanalyse_layout(size_t n, size_t tmp_bytes, size_t chunk) {
    ReanalyseLayout L{};
    Carve c;
    L.sel = c.take(n * 4); L.skip = c.take(n * 4); L.dst = c.take(n * 4);
    L.job_my = c.take(n * 8); L.job_op = c.take(n * 8); L.job_row = c.take(n * 4);
    L.moved = c.take(n * 4); L.done = c.take(n * 4);
    L.counts = c.take(16);
    L.tmp = c.take(tmp_bytes);
    L.results = c.take(chunk * SEARCH_RESULT_BYTES);
    L.total = c.at;
    return L;
}

}  // namespace syn
