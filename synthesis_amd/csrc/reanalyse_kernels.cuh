// Device-resident reanalyse (syn_replay_reanalyse, engine.hip; include/synthesis_amd.h "Reanalyse"): what runs around the search
// launches that refresh stored targets. A call selects rows of the replay buffer by a hash of (key, gid, my, op), compacts the selected
// positions into job arrays in buffer order, searches them chunk by chunk with the engine's MODE_SEARCH kernels and writes the new
// targets back over the old ones:
//     reanalyse_flags_kernel      the hash, the gid bound and the searchable test per row: sel[i] / skip[i]
//     an exclusive sum of sel (hipcub, as syn_replay_keep_games_from) and a sum of skip
//     reanalyse_compact_kernel    selected row i goes to job dst[i]: job_my | job_op | job_row
//     reanalyse_writeback_kernel  one 16-lane group per job of a chunk (dedup_reduce_kernel's shape): pi, v and the moved flag
// All of them stream: plain vector loads and stores, no LDS, no atomics, and no workgroup waits for another.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

#include "device_common.cuh"
#include "engine_kernels.cuh"
#include "noise.cuh"

namespace syn {

constexpr unsigned long long REANALYSE_TAG = 0x2EA7A1F5E5EA2C40ull;
// v write-back: value_mix == 0 keeps v, == 1 stores target_q, otherwise v_old * (1 - w) + q * w
enum { REANALYSE_V_KEEP = 0, REANALYSE_V_STORE = 1, REANALYSE_V_MIX = 2 };

// DevSearchResult has a 372-byte stride (not a multiple of 8 or 16): its fields are read as dwords
constexpr int REANALYSE_RES_DWORDS = (int)(sizeof(DevSearchResult) / 4);
constexpr int REANALYSE_RES_NODES = (int)(offsetof(DevSearchResult, num_nodes) / 4);
constexpr int REANALYSE_RES_PI = (int)(offsetof(DevSearchResult, target_pi) / 4);
constexpr int REANALYSE_RES_Q = (int)(offsetof(DevSearchResult, target_q) / 4);
static_assert(sizeof(DevSearchResult) % 4 == 0 && offsetof(DevSearchResult, target_pi) % 4 == 0, "DevSearchResult is read as dwords");

// engine.hip valid_root (disjoint boards inside the 63 cells, every column filled from the bottom, a free column) and neither side
// with four in a row: what syn_mcts_search and syn_match_run check on the host before a root reaches a search kernel
__device__ __forceinline__ bool reanalyse_searchable(unsigned long long my, unsigned long long op) {
    if ((my & op) != 0 || ((my | op) >> 63) != 0) return false;
    const unsigned long long occ = my | op;
    bool any_free = false;
    for (int c = 0; c < 9; c++) {
        const unsigned col = (unsigned)((occ >> (7 * c)) & 0x7F);
        if ((col & (col + 1)) != 0) return false;
        any_free |= col != 0x7F;
    }
    return any_free && !c4::won(my) && !c4::won(op);
}

__device__ __forceinline__ unsigned long long reanalyse_hash(unsigned long long tagged_key, unsigned long long gid, unsigned long long my,
                                                             unsigned long long op) {
    unsigned long long h = tagged_key;
    h = noise_splitmix64(noise_splitmix64(h, (uint32_t)(gid >> 32)), (uint32_t)gid);
    h = noise_splitmix64(noise_splitmix64(h, (uint32_t)(my >> 32)), (uint32_t)my);
    h = noise_splitmix64(noise_splitmix64(h, (uint32_t)(op >> 32)), (uint32_t)op);
    return h >> 32;
}

// sel[i] = 1: row i is reanalysed; skip[i] = 1: it passed the gid bound and the hash but is not a searchable position
__global__ void __launch_bounds__(256) reanalyse_flags_kernel(
    const long long* __restrict__ gid, const unsigned long long* __restrict__ my, const unsigned long long* __restrict__ op, int n,
    unsigned long long tagged_key, unsigned long long threshold, long long before_gid, unsigned* __restrict__ sel,
    unsigned* __restrict__ skip) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const long long g = gid[i];
    const unsigned long long a = my[i], b = op[i];
    const bool drawn = g < before_gid && reanalyse_hash(tagged_key, (unsigned long long)g, a, b) < threshold;
    const bool ok = reanalyse_searchable(a, b);
    sel[i] = drawn && ok ? 1u : 0u;
    skip[i] = drawn && !ok ? 1u : 0u;
}

// Stable compaction after the exclusive sum `dst` of sel: the j-th selected row, in buffer order, becomes job j. `cap` = the job
// arrays' size (a corrupt rank must not write outside them).
__global__ void __launch_bounds__(256) reanalyse_compact_kernel(
    const unsigned* __restrict__ sel, const unsigned* __restrict__ dst, int n, unsigned cap, const unsigned long long* __restrict__ my,
    const unsigned long long* __restrict__ op, unsigned long long* __restrict__ job_my, unsigned long long* __restrict__ job_op,
    unsigned* __restrict__ job_row) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || !sel[i]) return;
    const unsigned d = dst[i];
    if (d >= cap) return;
    job_my[d] = my[i];
    job_op[d] = op[i];
    job_row[d] = (unsigned)i;
}

// The write-back of one searched chunk: job j of the chunk (results[j], job_row[j]) rewrites buffer row job_row[j]. Lanes 0-8 store
// pi, lanes 9-11 v, lane 12 the moved flag (arg-max column of the old pi against the new one, the first maximum wins) and lane 13
// the done flag. Every lane loads what it reads of the old row BEFORE any lane stores (the old pi reaches lane 12 through the
// lanes that own its columns), so the flag never sees a half-written row. Nothing is written when the chunk's search reported an
// error (search_error[0] != 0: the chunk stays wholly old) or for a root a syn_cancel kept from being searched (num_nodes == 0).
__global__ void __launch_bounds__(256) reanalyse_writeback_kernel(
    const unsigned* __restrict__ results, int n_jobs, const unsigned* __restrict__ job_row, unsigned n_rows, int v_mode, float w,
    const int* __restrict__ search_error, float* __restrict__ pi, float* __restrict__ v, unsigned* __restrict__ moved,
    unsigned* __restrict__ done) {
    const int job = (int)((blockIdx.x * (size_t)blockDim.x + threadIdx.x) >> 4);
    const int j = threadIdx.x & 15;
    bool active = job < n_jobs && search_error[0] == 0;
    const unsigned* r = results + (size_t)(active ? job : 0) * REANALYSE_RES_DWORDS;
    unsigned row = 0;
    if (active) {
        row = job_row[job];
        active = r[REANALYSE_RES_NODES] != 0u && row < n_rows;
    }
    const float old_pi = active && j < 9 ? pi[(size_t)row * 9 + j] : 0.0f;
    // (uniform over the 16-lane group: `active` is the same in all of its lanes)
    int best_old = 0, best_new = 0;
    float max_old = 0.0f, max_new = 0.0f;
    for (int c = 0; c < 9; c++) {
        const float o = __shfl(old_pi, c, 16);
        const float q = active ? __uint_as_float(r[REANALYSE_RES_PI + c]) : 0.0f;
        if (c == 0 || o > max_old) {
            max_old = o;
            best_old = c;
        }
        if (c == 0 || q > max_new) {
            max_new = q;
            best_new = c;
        }
    }
    if (!active) return;
    if (j < 9) {
        pi[(size_t)row * 9 + j] = __uint_as_float(r[REANALYSE_RES_PI + j]);
    } else if (j < 12) {
        const int k = j - 9;
        const float q = __uint_as_float(r[REANALYSE_RES_Q + k]);
        if (v_mode == REANALYSE_V_STORE) {
            v[(size_t)row * 3 + k] = q;
        } else if (v_mode == REANALYSE_V_MIX) {
            const float old_v = v[(size_t)row * 3 + k];
            v[(size_t)row * 3 + k] = old_v * (1.0f - w) + q * w;
        }
    } else if (j == 12) {
        moved[job] = best_old != best_new ? 1u : 0u;
    } else if (j == 13) {
        done[job] = 1u;
    }
}

}  // namespace syn
