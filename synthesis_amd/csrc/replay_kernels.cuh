// Device-resident replay buffer (synthesis/src/data.rs:107-235: extend, keep_last_n_games): the kernels between a self-play
// launch's padded outputs and the learner's data set. A buffer is five structure-of-arrays sections
//     my[cap] u64 | op[cap] u64 | gid[cap] i64 | pi[cap][9] f32 | v[cap][3] f32          (72 bytes per position)
// and every kernel here keeps buffer order (game order, then ply order), because the de-duplication sums the targets of identical
// states in buffer order (train_kernels.cuh dedup_reduce_kernel): a float sum in another order is another float.
// All of them stream: plain vector loads and stores, no LDS, no atomics.
#pragma once
#include <hip/hip_runtime.h>

#include "noise.cuh"

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

// ---------------------------------------------------------------------------------------------- holding games out
// syn_replay_set_holdout (include/synthesis_amd.h "Holding games out"): game gid is held out iff
//     (sm(sm(key ^ HOLDOUT_TAG, (uint32)(gid >> 32)), (uint32)gid) >> 32) < threshold,     sm = noise_splitmix64
// — by game, not by position: the positions of one game are correlated. Step 1: held[i] = 1 where position i's game is held out.
constexpr unsigned long long HOLDOUT_TAG = 0x401D0075E7C0FFEEull;
__global__ void replay_holdout_flags_kernel(const long long* __restrict__ gid, int n, unsigned long long tagged_key,
                                            unsigned long long threshold, unsigned* __restrict__ held) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const unsigned long long g = (unsigned long long)gid[i];
    const unsigned long long hash = noise_splitmix64(noise_splitmix64(tagged_key, (uint32_t)(g >> 32)), (uint32_t)g) >> 32;
    held[i] = hash < threshold ? 1u : 0u;
}

// Stable two-way partition of n rows of four sections (my u64 | op u64 | pi [9] f32 | v [3] f32), step 2 after the exclusive sum `rank`
// of the flags: a row with flag 0 moves to its rank among the flag-0 rows (i - rank[i]), a row with flag 1 to n_first + rank[i], where
// n_first = the number of flag-0 rows. Order is kept inside both parts. blockIdx.y = section, a thread moves one dword (as
// replay_keep_scatter_kernel). Destination indices are bounded by n: a corrupt rank must not write outside the sections.
__global__ void replay_partition_scatter_kernel(const unsigned* __restrict__ flag, const unsigned* __restrict__ rank, int n, unsigned n_first,
                                                const unsigned* __restrict__ s_my, const unsigned* __restrict__ s_op,
                                                const unsigned* __restrict__ s_pi, const unsigned* __restrict__ s_v,
                                                unsigned* __restrict__ d_my, unsigned* __restrict__ d_op, unsigned* __restrict__ d_pi,
                                                unsigned* __restrict__ d_v) {
    const int sec = blockIdx.y;
    const int W = sec < 2 ? 2 : (sec == 2 ? 9 : 3);
    const size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (t >= (size_t)n * W) return;
    const unsigned i = (unsigned)(t / W), c = (unsigned)(t % W);
    const unsigned to = flag[i] ? n_first + rank[i] : i - rank[i];
    if (to >= (unsigned)n) return;
    const unsigned* s = sec == 0 ? s_my : sec == 1 ? s_op : sec == 2 ? s_pi : s_v;
    unsigned* d = sec == 0 ? d_my : sec == 1 ? d_op : sec == 2 ? d_pi : d_v;
    d[(size_t)to * W + c] = s[t];
}

__device__ __forceinline__ unsigned long long mirror_bb(unsigned long long b);
// seen[i] = 1 where row i's state — with `mirror` its canonical form (the smaller of the pair and its mirror image, my first) — is
// among the n_t rows (t_my, t_op), which are sorted ascending by (my, op): one binary search per row.
__global__ void replay_seen_flags_kernel(const unsigned long long* __restrict__ my, const unsigned long long* __restrict__ op, int n,
                                         const unsigned long long* __restrict__ t_my, const unsigned long long* __restrict__ t_op, int n_t,
                                         int mirror, unsigned* __restrict__ seen) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    unsigned long long a = my[i], b = op[i];
    if (mirror) {
        const unsigned long long ma = mirror_bb(a), mb = mirror_bb(b);
        if (ma < a || (ma == a && mb < b)) {
            a = ma;
            b = mb;
        }
    }
    int lo = 0, hi = n_t;   // first row not below (a, b)
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        const unsigned long long x = t_my[mid], y = t_op[mid];
        if (x < a || (x == a && y < b)) lo = mid + 1;
        else hi = mid;
    }
    seen[i] = (lo < n_t && t_my[lo] == a && t_op[lo] == b) ? 1u : 0u;
}

// ---------------------------------------------------------------------------------------------- mirror symmetry
// The 9x7 board is left-right symmetric: a record (my, op, pi, v) implies (mirror(my), mirror(op), reverse(pi), v). Bit index of a
// bitboard = row + 7 * col (device_common.cuh), so a column is a group of 7 bits and mirroring exchanges the groups c and 8 - c: four
// delta-swaps at distances 56 / 42 / 28 / 14; the middle column (bits 28..34) and bit 63 stay where they are.
__device__ __forceinline__ unsigned long long mirror_bb(unsigned long long b) {
    unsigned long long x;
    x = ((b >> 56) ^ b) & 0x7Full;          b ^= x ^ (x << 56);
    x = ((b >> 42) ^ b) & (0x7Full << 7);   b ^= x ^ (x << 42);
    x = ((b >> 28) ^ b) & (0x7Full << 14);  b ^= x ^ (x << 28);
    x = ((b >> 14) ^ b) & (0x7Full << 21);  b ^= x ^ (x << 14);
    return b;
}

// syn_positions_mirror: a thread moves one dword of pi (out_pi[i][c] = pi[i][8 - c]; pi == nullptr: boards only, n threads), the first
// n threads also mirror position i's two boards.
__global__ void __launch_bounds__(256) replay_mirror_kernel(
    const unsigned long long* __restrict__ my, const unsigned long long* __restrict__ op, const float* __restrict__ pi, int n,
    unsigned long long* __restrict__ out_my, unsigned long long* __restrict__ out_op, float* __restrict__ out_pi) {
    const size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (t < (size_t)n) {
        out_my[t] = mirror_bb(my[t]);
        out_op[t] = mirror_bb(op[t]);
    }
    if (pi != nullptr && t < (size_t)n * 9) {
        const size_t i = t / 9, c = t % 9;
        out_pi[t] = pi[i * 9 + (8 - c)];
    }
}

// Symmetric de-duplication, step 1: the canonical orientation of every record. (mirror(my), mirror(op)) < (my, op) as pairs of
// unsigned numbers, my first (the order the de-duplication emits states in) -> the record is flipped and its keys are the mirrored
// boards; otherwise the keys are its own. The sort then runs over these n keys: a position and its mirror image meet in one segment.
__global__ void __launch_bounds__(256) replay_canonicalise_kernel(
    const unsigned long long* __restrict__ my, const unsigned long long* __restrict__ op, int n,
    unsigned long long* __restrict__ key_my, unsigned long long* __restrict__ key_op, unsigned* __restrict__ flip) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const unsigned long long a = my[i], b = op[i], ma = mirror_bb(a), mb = mirror_bb(b);
    const bool f = ma < a || (ma == a && mb < b);
    key_my[i] = f ? ma : a;
    key_op[i] = f ? mb : b;
    flip[i] = f ? 1u : 0u;
}

// ... step 2, after the stable sort by the canonical keys: dedup_reduce_kernel's shape (train_kernels.cuh: one 16-lane row per class,
// lane j < 12 owns one target component and sums it over the members in buffer order, then divides by the count), except that the pi
// lane j reads component 8 - j of a flipped member. Lane 12 writes the canonical state and the count, lane 13 whether the class has a
// mirror image of its own (expand[row] = 0 for a self-symmetric state).
__global__ void __launch_bounds__(256) dedup_reduce_mirror_kernel(
    const unsigned* __restrict__ order, const unsigned* __restrict__ seg_start, int m, int n,
    const unsigned long long* __restrict__ key_my, const unsigned long long* __restrict__ key_op, const unsigned* __restrict__ flip,
    const float* __restrict__ pis, const float* __restrict__ vs, unsigned long long* __restrict__ out_my,
    unsigned long long* __restrict__ out_op, float* __restrict__ out_pi, float* __restrict__ out_v, unsigned* __restrict__ out_num,
    unsigned* __restrict__ expand) {
    const int row = (blockIdx.x * blockDim.x + threadIdx.x) >> 4;
    const int j = threadIdx.x & 15;
    if (row >= m) return;
    const unsigned s0 = seg_start[row], s1 = row + 1 < m ? seg_start[row + 1] : (unsigned)n;
    if (j < 12) {
        float acc = 0.0f;
        for (unsigned p = s0; p < s1; p++) {
            const unsigned i = order[p];
            acc += j < 9 ? pis[(size_t)i * 9 + (flip[i] ? 8 - j : j)] : vs[(size_t)i * 3 + (j - 9)];
        }
        const float avg = acc / (float)(s1 - s0);
        if (j < 9) out_pi[(size_t)row * 9 + j] = avg;
        else out_v[(size_t)row * 3 + (j - 9)] = avg;
    } else if (j == 12) {
        const unsigned i = order[s0];
        out_my[row] = key_my[i];
        out_op[row] = key_op[i];
        out_num[row] = s1 - s0;
    } else if (j == 13) {
        const unsigned i = order[s0];
        const unsigned long long a = key_my[i], b = key_op[i];
        expand[row] = (mirror_bb(a) != a || mirror_bb(b) != b) ? 1u : 0u;
    }
}

// ... step 3, after the exclusive sum `dst` of the expand flags: class `row` with a mirror image writes it to row m + dst[row] —
// (mirror(my), mirror(op), reverse(pi_avg), v_avg, num): a permutation of the averaged row, so the two rows agree bit for bit.
// Rows [0, m) are only read, rows [m, rows_cap) only written (the arrays are the same: no __restrict__ on them).
__global__ void __launch_bounds__(256) dedup_expand_mirror_kernel(
    const unsigned* __restrict__ expand, const unsigned* __restrict__ dst, int m, size_t rows_cap, unsigned long long* out_my,
    unsigned long long* out_op, float* out_pi, float* out_v, unsigned* out_num) {
    const int row = (blockIdx.x * blockDim.x + threadIdx.x) >> 4;
    const int j = threadIdx.x & 15;
    if (row >= m || !expand[row]) return;
    const size_t d = (size_t)m + dst[row];
    if (d >= rows_cap) return;
    if (j < 9) out_pi[d * 9 + j] = out_pi[(size_t)row * 9 + (8 - j)];
    else if (j < 12) out_v[d * 3 + (j - 9)] = out_v[(size_t)row * 3 + (j - 9)];
    else if (j == 12) out_my[d] = mirror_bb(out_my[row]);
    else if (j == 13) out_op[d] = mirror_bb(out_op[row]);
    else if (j == 14) out_num[d] = out_num[row];
}

}  // namespace syn
