// synthesis_amd — held-out evaluation (syn_dataset_evaluate, include/synthesis_amd.h): the losses of a set of parameters on a data set,
// forward only, nothing of the learner touched. The rows [first, first + n) of a TrainSections data set are n_blocks = ceil(n / 32)
// blocks of 32 rows (the last one n mod 32 rows when that is not zero), and per block j
//   pi_loss_j, v_loss_j = what the f32 learner reports for the block's rows as a minibatch of rows_j samples: the forward and the
//                         log_softmax / kl_div statements of tm_gradients (train_mfma.cuh) resp. of phases F and H of conv_grad_step_mfma
//                         (train_conv_mfma.cuh), chain for chain, then bm * (kl_0 + kl_1 + ...) in row order by one thread with
//                         bm = 1.0f / rows_j. policy_weight / value_weight do not enter (they do not enter the learner's losses).
//   pi_hit_j            = rows whose first maximum of the nine policy logits over the LEGAL columns (top cell of the column free) is
//                         the first maximum of the target pi; a row without a legal column counts as a miss
//   v_hit_j             = rows whose first maximum of the three value logits is the first maximum of the target v
// ("first maximum": best = entry 0 resp. the first legal entry; a later entry replaces it only when it compares greater.)
// What is left out of the learner's step: dz, every backward phase, every gradient store, and with them the LDS they live in:
//   Connect4Net      TrainGeom::A_FLOATS activations + 128 floats = 56,320 B   (the learner: TrainGeom::WL_OFF floats = 103,680 B)
//   Connect4ConvNet  boards + head partials + 128 floats        = 25,600 B   (the learner: ConvMfmaGeom::LDS_FLOATS = 157,568 B); the
//                    ReLU outputs go from the conv accumulators straight into the head's MFMAs and are never stored
// Launches, in stream order; NO workgroup waits for another one (no grid barrier, no spin, no cooperative launch, no atomics):
//   blocks   workgroup b takes the blocks j = b, b + gridDim.x, ... and writes record j (DsBlockRecord) — and, where asked for, the
//            rows' twelve logits and two KL values. A record depends on its rows and the parameters only: any grid gives the same bytes.
//   reduce   ONE workgroup of DS_REDUCE_THREADS threads. Chunk c = the records [256 c, 256 c + 256): thread t sums the chunks t,
//            t + DS_REDUCE_THREADS, ... each as an ascending chain in f64 from 0.0 of (double)rows_j * (double)loss_j (the product
//            is exact: 6 x 24 bits), integer sums of the hits; after a barrier thread 0 adds the chunk sums from 0.0 in ascending c.
//            The order is a function of n alone. The host divides the two f64 sums by n.
// The other arithmetics (syn_dataset_evaluate_arith): blocks, rows_j, the head's statements, the hit rules, the record and the reduce are
// the ones above; only what produces a row's twelve raw outputs differs.
//   f16x2   dataset_eval_blocks_f16x2_kernel<NET>: the engine's f16x2 inference (f16x2_tile16<3> resp. conv_f16x2_tile16 times the
//           image's output scale, as policy_eval_f16x2_kernel / policy_eval_conv_f16x2_kernel), the image staged into LDS once per
//           workgroup; a wave computes a tile of 16 rows, a block is two tiles, four blocks are in flight per pass.
//   bf16    dataset_eval_blocks_conv_bf16_kernel: phases F (without the activation store) and H (without dz) of conv_grad_step_bf16.
#pragma once
#include "conv_f16x2_tile.cuh"
#include "train_conv_mfma.cuh"
#include "train_mfma.cuh"

namespace syn {

constexpr int DS_BLOCK = 32;            // rows of a block: TrainGeom::CHUNK = ConvMfmaGeom::CHUNK = MICRO_BLOCK
constexpr int DS_CHUNK_BLOCKS = 256;    // records of a reduction chunk
constexpr int DS_REDUCE_THREADS = 256;
static_assert(TrainGeom::CHUNK == DS_BLOCK && ConvMfmaGeom::CHUNK == DS_BLOCK, "a block is one chunk of either learner");

struct DsBlockRecord {   // 32 bytes
    float pi_loss, v_loss;
    unsigned rows, pi_hit, v_hit;
    unsigned pad[3];
};
struct DsTotals {        // what the reduce leaves for the host
    double sum_pi, sum_v;             // sums over the blocks of rows_j * loss_j
    unsigned long long pi_hits, v_hits, rows;
};
struct DsChunkSum {
    double pi, v;
    unsigned long long pi_hits, v_hits, rows;
};

struct DsArgs {
    const unsigned long long* my_bb;   // the first row of the range
    const unsigned long long* op_bb;
    const float* tpi;                  // [n][9]
    const float* tv;                   // [n][3]
    long long n;                       // rows, >= 1
    long long n_blocks;
    DsBlockRecord* records;            // [n_blocks]
    float* block_losses;               // [n_blocks][2] or NULL
    float* row_logits;                 // [n][12] or NULL
    float* row_kl;                     // [n][2] or NULL
};

struct DsMlpGeom {
    static constexpr int KL_OFF = TrainGeom::A_FLOATS;   // [32][2] KL terms
    static constexpr int HIT_OFF = KL_OFF + 2 * DS_BLOCK; // [32][2] hit flags (as unsigned)
    static constexpr int LDS_FLOATS = HIT_OFF + 2 * DS_BLOCK;
};
struct DsConvGeom {
    static constexpr int BB_OFF = 0;                                 // [32][2] u64 boards; rows >= the block's: zero
    static constexpr int PART_OFF = BB_OFF + DS_BLOCK * 4;           // [wave 16][sample 32][12] head partials
    static constexpr int KL_OFF = PART_OFF + 16 * DS_BLOCK * 12;
    static constexpr int HIT_OFF = KL_OFF + 2 * DS_BLOCK;
    static constexpr int LDS_FLOATS = HIT_OFF + 2 * DS_BLOCK;
};

// first maximum of x[0..9) over the columns of `occ` (= my | op) whose top cell (bit 6 + 7 c) is free; 9 when there is none
SYN_DEV int ds_argmax_legal(const float (&x)[9], unsigned long long occ) {
    int best = 9;
    float bv = 0.0f;
#pragma unroll
    for (int c = 0; c < 9; c++) {
        const bool legal = ((occ >> (6 + 7 * c)) & 1ull) == 0ull;
        if (legal && (best == 9 || x[c] > bv)) {
            best = c;
            bv = x[c];
        }
    }
    return best;
}
template <int N>
SYN_DEV int ds_argmax_first(const float* x) {
    int best = 0;
    float bv = x[0];
#pragma unroll
    for (int c = 1; c < N; c++)
        if (x[c] > bv) {
            best = c;
            bv = x[c];
        }
    return best;
}

// record j from the block's 32 x 2 KL terms and hit flags in LDS: one thread, row order (tm_gradients' pi_acc / v_acc)
SYN_DEV void ds_write_record(const float* kl, const unsigned* hit, int nb, long long j, const DsArgs& A) {
    const float bm = 1.0f / (float)nb;
    float pi_acc = 0.0f, v_acc = 0.0f;
    unsigned ph = 0u, vh = 0u;
    for (int b = 0; b < nb; b++) {
        pi_acc += kl[b * 2 + 0];
        v_acc += kl[b * 2 + 1];
        ph += hit[b * 2 + 0];
        vh += hit[b * 2 + 1];
    }
    DsBlockRecord r;
    r.pi_loss = bm * pi_acc;
    r.v_loss = bm * v_acc;
    r.rows = (unsigned)nb;
    r.pi_hit = ph;
    r.v_hit = vh;
    r.pad[0] = r.pad[1] = r.pad[2] = 0u;
    A.records[j] = r;
    if (A.block_losses) {
        A.block_losses[2 * j + 0] = r.pi_loss;
        A.block_losses[2 * j + 1] = r.v_loss;
    }
}

// Connect4Net: <<<min(n_blocks, cap), 512>>>, DsMlpGeom::LDS_FLOATS floats of LDS. wimg = the inference fragment image (mlp.cuh).
// Eight waves, not the learner's sixteen: the forward has 16, 12, 8, 6 and 2 tiles per layer (the learner's sixteen waves are there
// for its 119 parameter tiles), and two such workgroups fit a CU's LDS and registers, so one block's barriers hide behind the other's
// tiles. Which wave computes a tile changes no bit of it.
constexpr int DS_MLP_THREADS = 512;
__global__ __launch_bounds__(DS_MLP_THREADS) void dataset_eval_blocks_kernel(const float* __restrict__ wimg, DsArgs A) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    using G = TrainGeom;
    using E = DsMlpGeom;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    unsigned* hit = reinterpret_cast<unsigned*>(lds + E::HIT_OFF);
    for (long long j = blockIdx.x; j < A.n_blocks; j += gridDim.x) {
        const size_t c0 = (size_t)j * DS_BLOCK;
        const int nb = A.n - (long long)c0 < DS_BLOCK ? (int)(A.n - (long long)c0) : DS_BLOCK;
        float tgt[9];
#pragma unroll
        for (int k = 0; k < 9; k++) tgt[k] = 0.0f;
        unsigned long long occ = 0ull;
        if (tid < 2 * DS_BLOCK && (tid >> 1) < nb) {
            const size_t si = c0 + (size_t)(tid >> 1);
            if ((tid & 1) == 0) {
#pragma unroll
                for (int k = 0; k < 9; k++) tgt[k] = A.tpi[si * 9 + k];
                occ = A.my_bb[si] | A.op_bb[si];
            } else {
#pragma unroll
                for (int k = 0; k < 3; k++) tgt[k] = A.tv[si * 3 + k];
            }
        }
        // features -> A[0] (columns 63.. of the padded rows are zero; rows of samples past nb are zero) — tm_gradients' statements
        {
            constexpr int NIT = DS_BLOCK * 64 / DS_MLP_THREADS;
            uint64_t bmy[NIT], bop[NIT];
#pragma unroll
            for (int it = 0; it < NIT; it++) {
                const int b = (tid + it * DS_MLP_THREADS) >> 6;
                const size_t s = b < nb ? c0 + (size_t)b : c0;
                bmy[it] = b < nb ? A.my_bb[s] : 0ull;
                bop[it] = b < nb ? A.op_bb[s] : 0ull;
            }
#pragma unroll
            for (int it = 0; it < NIT; it++) {
                const int i = tid + it * DS_MLP_THREADS, b = i >> 6, f = i & 63;
                float x = 0.0f;
                if (b < nb && f < 63) x = c4::feature(bmy[it], bop[it], c4::next_free_cells(bmy[it] | bop[it]), f);
                lds[G::a_off(0) + b * G::stride(0) + f] = x;
            }
        }
        __syncthreads();
#define DS_FWD(L)                                                                                                              \
    for (int t = wave; t < MlpGeom::NOB[L] * 2; t += DS_MLP_THREADS / 64) tm_forward_tile<L>(wimg, lds, t >> 1, t & 1, lane); \
    __syncthreads();
        DS_FWD(0) DS_FWD(1) DS_FWD(2) DS_FWD(3) DS_FWD(4)
#undef DS_FWD
        // ---- heads: tm_gradients' log_softmax + kl_div, one thread per (sample, head); the arg-maxes beside them
        if (tid < 2 * DS_BLOCK) {
            const int b = tid >> 1, head = tid & 1;
            const int off = head == 0 ? 0 : 9, n = head == 0 ? 9 : 3;
            float kl = 0.0f;
            unsigned h = 0u;
            if (b < nb) {
                const float* x = lds + G::a_off(5) + b * G::stride(5) + off;
                float xv[9];
#pragma unroll
                for (int k = 0; k < 9; k++) xv[k] = k < n ? x[k] : 0.0f;
                float mx = xv[0];
#pragma unroll
                for (int k = 1; k < 9; k++) mx = (k < n && xv[k] > mx) ? xv[k] : mx;
                float se = 0.0f;
#pragma unroll
                for (int k = 0; k < 9; k++)
                    if (k < n) se += det_expf(xv[k] - mx);
                const float lse = mx + det_logf(se);
#pragma unroll
                for (int k = 0; k < 9; k++) {
                    if (k < n) {
                        const float logp = xv[k] - lse;
                        if (tgt[k] > 0.0f) kl += tgt[k] * (det_logf(tgt[k]) - logp);
                    }
                }
                const size_t si = c0 + (size_t)b;
                if (head == 0) {
                    h = ds_argmax_legal(xv, occ) == ds_argmax_first<9>(tgt) ? 1u : 0u;
                    if (A.row_logits) {
#pragma unroll
                        for (int k = 0; k < 9; k++) A.row_logits[si * 12 + k] = xv[k];
                    }
                } else {
                    h = ds_argmax_first<3>(xv) == ds_argmax_first<3>(tgt) ? 1u : 0u;
                    if (A.row_logits) {
#pragma unroll
                        for (int k = 0; k < 3; k++) A.row_logits[si * 12 + 9 + k] = xv[k];
                    }
                }
                if (A.row_kl) A.row_kl[si * 2 + head] = kl;
            }
            lds[E::KL_OFF + b * 2 + head] = kl;
            hit[b * 2 + head] = h;
        }
        __syncthreads();
        // (the next block's first writes to the KL / hit words come five barriers from here, which thread 0 has to pass as well)
        if (tid == 0) ds_write_record(lds + E::KL_OFF, hit, nb, j, A);
    }
}

// Connect4ConvNet: <<<min(n_blocks, cap), 512>>>, DsConvGeom::LDS_FLOATS floats of LDS. w = the canonical parameters (12,412 floats).
// Phases F (without the activation store) and H (without dz) of conv_grad_step_mfma<512>.
__global__ __launch_bounds__(CONV_TRAIN_THREADS) void dataset_eval_blocks_conv_kernel(const float* __restrict__ w, DsArgs A) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    using G = ConvMfmaGeom;
    using E = DsConvGeom;
    constexpr int NT = CONV_TRAIN_THREADS, NWV = NT / 64;
    static_assert(NT == 16 * DS_BLOCK, "the heads phase maps thread -> (sample tid >> 4, entry tid & 15)");
    const int tid = threadIdx.x, lane = tid & 63, rw = tid >> 6, j = lane & 15, q = lane >> 4;
    float* part = lds + E::PART_OFF;
    uint64_t* bb = reinterpret_cast<uint64_t*>(lds + E::BB_OFF);
    unsigned* hit = reinterpret_cast<unsigned*>(lds + E::HIT_OFF);
    for (long long blk = blockIdx.x; blk < A.n_blocks; blk += gridDim.x) {
        const size_t c0 = (size_t)blk * DS_BLOCK;
        const int B = A.n - (long long)c0 < DS_BLOCK ? (int)(A.n - (long long)c0) : DS_BLOCK;
        if (tid < 2 * DS_BLOCK) {
            const int b = tid >> 1;
            unsigned long long v = 0ull;
            if (b < B) v = (tid & 1) ? A.op_bb[c0 + b] : A.my_bb[c0 + b];
            bb[tid] = v;
        }
        const int hb = tid >> 4, jx = tid & 15;
        float tgt = 0.0f;
        if (hb < B && jx < 12) {
            const size_t si = c0 + (size_t)hb;
            tgt = jx < 9 ? A.tpi[si * 9 + jx] : A.tv[si * 3 + (jx - 9)];
        }
        const float ltgt = tgt > 0.0f ? det_logf(tgt) : 0.0f;
        __syncthreads();

        // ---- F: conv forward + ReLU + head partials
        for (int wv = rw; wv < 16; wv += NWV) {
            float ca[5];
#pragma unroll
            for (int s = 0; s < 5; s++) ca[s] = 4 * s + q < 18 ? w[G::P_CW + j * 18 + 4 * s + q] : 0.0f;   // A[channel j][tap 4 s + q]
            const f32x4 cbv = *reinterpret_cast<const f32x4*>(w + G::P_CB + 4 * q);                         // D rows: channels 4 q + r
            float hwv[4][4];
#pragma unroll
            for (int c = 0; c < 4; c++)
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const int p = wv + 16 * c;
                    hwv[c][r] = (j < 12 && p < G::HW) ? w[G::P_HW + (size_t)j * G::FLAT + (4 * q + r) * G::HW + p] : 0.0f;
                }
#pragma unroll 1
            for (int t = 0; t < 2; t++) {
                const int sample = 16 * t + j;
                const uint64_t my = bb[2 * sample], op = bb[2 * sample + 1];
                uint64_t S[5];
#pragma unroll
                for (int s = 0; s < 5; s++) S[s] = conv_tap_board(my, op, 4 * s + q);
                f32x4 hacc = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
                for (int c = 0; c < 4; c++) {
                    const int p = wv + 16 * c;
                    if (p < G::HW) {   // (wave-uniform: only wave 15 has three cells)
                        const int row = p / 9, col = p - 9 * row, pos = row + 7 * col;
                        f32x4 acc = cbv;
#pragma unroll
                        for (int s = 0; s < 5; s++)
                            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(ca[s], (float)((uint32_t)(S[s] >> pos) & 1u), acc, 0, 0, 0);
#pragma unroll
                        for (int r = 0; r < 4; r++) {
                            const float a = acc[r] > 0.0f ? acc[r] : 0.0f;
                            hacc = __builtin_amdgcn_mfma_f32_16x16x4f32(hwv[c][r], a, hacc, 0, 0, 0);
                        }
                    }
                }
                if (q < 3) {
#pragma unroll
                    for (int r = 0; r < 4; r++) part[(wv * DS_BLOCK + sample) * 12 + 4 * q + r] = hacc[r];
                }
            }
        }
        __syncthreads();

        // ---- H: the 12 outputs (bias + the sixteen partials in order), log_softmax + kl_div; the arg-maxes beside them
        {
            const bool pol = jx < 9;
            const bool live = jx < 12 && hb < B;
            float xo = 0.0f;
            if (jx < 12) {
                xo = w[G::P_HB + jx];
#pragma unroll
                for (int g = 0; g < 16; g++) xo += part[(g * DS_BLOCK + hb) * 12 + jx];
            }
            xo = live ? xo : 0.0f;
            float xs[12], ts[12];
            ep_row_gather(xo, xs);
            ep_row_gather(tgt, ts);
            float mxp = xs[0], mxv = xs[9];
#pragma unroll
            for (int t = 1; t < 9; t++) mxp = xs[t] > mxp ? xs[t] : mxp;
#pragma unroll
            for (int t = 10; t < 12; t++) mxv = xs[t] > mxv ? xs[t] : mxv;
            const float mx = pol ? mxp : mxv;
            const float e = live ? det_expf(xo - mx) : 0.0f;
            const float se = ep_row_sum(e, pol);
            const float lse = mx + det_logf(live ? se : 1.0f);
            const float logp = xo - lse;
            const float term = (live && tgt > 0.0f) ? tgt * (ltgt - logp) : 0.0f;
            const float kl = ep_row_sum(term, pol);
            if (jx == 0 || jx == 9) {
                unsigned h = 0u;
                if (hb < B) {
                    if (pol) {
                        float xp[9];
#pragma unroll
                        for (int t = 0; t < 9; t++) xp[t] = xs[t];
                        h = ds_argmax_legal(xp, bb[2 * hb] | bb[2 * hb + 1]) == ds_argmax_first<9>(ts) ? 1u : 0u;
                    } else {
                        h = ds_argmax_first<3>(xs + 9) == ds_argmax_first<3>(ts + 9) ? 1u : 0u;
                    }
                    if (A.row_kl) A.row_kl[(c0 + (size_t)hb) * 2 + (pol ? 0 : 1)] = kl;
                }
                lds[E::KL_OFF + hb * 2 + (pol ? 0 : 1)] = hb < B ? kl : 0.0f;
                hit[hb * 2 + (pol ? 0 : 1)] = h;
            }
            if (live && A.row_logits) A.row_logits[(c0 + (size_t)hb) * 12 + jx] = xo;
        }
        __syncthreads();
        // (the next block's KL / hit / partial words are written two barriers from here; its boards overwrite words nobody reads now)
        if (tid == 0) ds_write_record(lds + E::KL_OFF, hit, B, blk, A);
    }
}

// ---------------------------------------------------------------------------------------------- the f16x2 arithmetic
// <<<min(ceil(n_blocks / 4), cap), 512>>>, DsF16Geom<NET>::LDS_WORDS words of LDS. g_img = the f16x2 image of the parameters (NET 0:
// F16Geom, Connect4Net; NET 1: ConvF16Geom, Connect4ConvNet). Workgroup b takes the blocks b, b + grid, ... four per pass: wave w
// computes tile w & 1 (rows 16 (w & 1) ..) of the pass's block w >> 1 and leaves the raw outputs [32][12] in LDS; after a barrier the
// head runs as in dataset_eval_blocks_kernel, one thread per (block of the pass, sample, head); after another barrier one thread per
// block writes its record. Which pass and wave a block falls to changes no bit of it. A tile without a row of the range is not
// computed; rows past n in the last tile enter as zero boards and nothing of them leaves LDS.
constexpr int DS_F16_THREADS = 512;
constexpr int DS_F16_SLOTS = DS_F16_THREADS / 128;   // blocks in flight per pass: two waves (tiles) each
template <int NET>
struct DsF16Geom {
    static constexpr int IMG_WORDS = NET == 0 ? F16Geom::IMG_WORDS : ConvF16Geom::IMG_WORDS;
    static constexpr int RAW_OFF = IMG_WORDS;                                  // [slot][32][12] raw outputs (f32)
    static constexpr int KL_OFF = RAW_OFF + DS_F16_SLOTS * DS_BLOCK * 12;      // [slot][32][2] KL terms
    static constexpr int HIT_OFF = KL_OFF + DS_F16_SLOTS * DS_BLOCK * 2;       // [slot][32][2] hit flags
    static constexpr int LDS_WORDS = HIT_OFF + DS_F16_SLOTS * DS_BLOCK * 2;
};
static_assert(DsF16Geom<0>::IMG_WORDS % 4 == 0 && DsF16Geom<1>::IMG_WORDS % 4 == 0, "the image is staged in 16-byte pieces");
static_assert((size_t)DsF16Geom<0>::LDS_WORDS * 4 <= 160u * 1024u, "one workgroup per CU for Connect4Net");
static_assert((size_t)DsF16Geom<1>::LDS_WORDS * 4 * 2 <= 160u * 1024u, "Connect4ConvNet: the LDS of two workgroups fits a CU");

// the head of one row for thread (sample, head): dataset_eval_blocks_kernel's statements on the row's twelve raw outputs x (LDS)
SYN_DEV void ds_head_thread(const float* x12, int head, size_t si, const DsArgs& A, float& kl_out, unsigned& hit_out) {
    const int off = head == 0 ? 0 : 9, n = head == 0 ? 9 : 3;
    float tgt[9];
#pragma unroll
    for (int k = 0; k < 9; k++) tgt[k] = 0.0f;
    unsigned long long occ = 0ull;
    if (head == 0) {
#pragma unroll
        for (int k = 0; k < 9; k++) tgt[k] = A.tpi[si * 9 + k];
        occ = A.my_bb[si] | A.op_bb[si];
    } else {
#pragma unroll
        for (int k = 0; k < 3; k++) tgt[k] = A.tv[si * 3 + k];
    }
    const float* x = x12 + off;
    float xv[9];
#pragma unroll
    for (int k = 0; k < 9; k++) xv[k] = k < n ? x[k] : 0.0f;
    float mx = xv[0];
#pragma unroll
    for (int k = 1; k < 9; k++) mx = (k < n && xv[k] > mx) ? xv[k] : mx;
    float se = 0.0f;
#pragma unroll
    for (int k = 0; k < 9; k++)
        if (k < n) se += det_expf(xv[k] - mx);
    const float lse = mx + det_logf(se);
    float kl = 0.0f;
#pragma unroll
    for (int k = 0; k < 9; k++) {
        if (k < n) {
            const float logp = xv[k] - lse;
            if (tgt[k] > 0.0f) kl += tgt[k] * (det_logf(tgt[k]) - logp);
        }
    }
    unsigned h;
    if (head == 0) {
        h = ds_argmax_legal(xv, occ) == ds_argmax_first<9>(tgt) ? 1u : 0u;
        if (A.row_logits) {
#pragma unroll
            for (int k = 0; k < 9; k++) A.row_logits[si * 12 + k] = xv[k];
        }
    } else {
        h = ds_argmax_first<3>(xv) == ds_argmax_first<3>(tgt) ? 1u : 0u;
        if (A.row_logits) {
#pragma unroll
            for (int k = 0; k < 3; k++) A.row_logits[si * 12 + 9 + k] = xv[k];
        }
    }
    if (A.row_kl) A.row_kl[si * 2 + head] = kl;
    kl_out = kl;
    hit_out = h;
}

template <int NET>
__global__ __launch_bounds__(DS_F16_THREADS) void dataset_eval_blocks_f16x2_kernel(const uint32_t* __restrict__ g_img, DsArgs A) {
    extern __shared__ __attribute__((aligned(16))) uint32_t ds16[];
    using E = DsF16Geom<NET>;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, q = lane >> 4;
    for (int i = tid; i < E::IMG_WORDS / 4; i += DS_F16_THREADS) reinterpret_cast<uint4*>(ds16)[i] = reinterpret_cast<const uint4*>(g_img)[i];
    float* raw = reinterpret_cast<float*>(ds16 + E::RAW_OFF);
    float* klw = reinterpret_cast<float*>(ds16 + E::KL_OFF);
    unsigned* hit = ds16 + E::HIT_OFF;
    __syncthreads();
    const int slot = wave >> 1, tile = wave & 1;
    const long long pass_stride = (long long)gridDim.x * DS_F16_SLOTS;
    for (long long j0 = blockIdx.x; j0 < A.n_blocks; j0 += pass_stride) {
        // ---- tiles: the raw outputs of the pass's rows
        {
            const long long blk = j0 + (long long)slot * gridDim.x;
            const long long r0 = blk * DS_BLOCK + 16 * tile;
            if (blk < A.n_blocks && r0 < A.n) {   // (wave-uniform)
                uint32_t img_off = 0;   // opaque per pass: the image reads stay LDS reads next to their MFMAs
                asm volatile("" : "+v"(img_off));
                const uint32_t* img = ds16 + img_off;
                const long long pos = r0 + j;
                const bool valid = pos < A.n;
                const uint64_t my = valid ? A.my_bb[pos] : 0ull, op = valid ? A.op_bb[pos] : 0ull;
                f32x4_ o;
                float os;
                if constexpr (NET == 0) {
                    uint64_t hi, lo;
                    feature_boards(my, op, hi, lo);
                    o = f16x2_tile16<3>(img, lane, hi, lo);
                    os = reinterpret_cast<const float*>(img + F16Geom::SCALE_WORD0)[4];
                } else {
                    o = conv_f16x2_tile16(img, lane, my, op);
                    os = reinterpret_cast<const float*>(img + ConvF16Geom::SCALE_W0)[1];
                }
#pragma unroll
                for (int r = 0; r < 4; r++) o[r] *= os;
                if (q < 3) {
#pragma unroll
                    for (int r = 0; r < 4; r++) raw[((slot * DS_BLOCK) + 16 * tile + j) * 12 + 4 * q + r] = o[r];
                }
            }
        }
        __syncthreads();
        // ---- heads: one thread per (slot, sample, head)
        if (tid < DS_F16_SLOTS * 2 * DS_BLOCK) {
            const int hs = tid >> 6, b = (tid >> 1) & (DS_BLOCK - 1), head = tid & 1;
            const long long blk = j0 + (long long)hs * gridDim.x;
            float kl = 0.0f;
            unsigned h = 0u;
            if (blk < A.n_blocks && blk * DS_BLOCK + b < A.n)
                ds_head_thread(raw + (hs * DS_BLOCK + b) * 12, head, (size_t)(blk * DS_BLOCK + b), A, kl, h);
            klw[(hs * DS_BLOCK + b) * 2 + head] = kl;
            hit[(hs * DS_BLOCK + b) * 2 + head] = h;
        }
        __syncthreads();
        // (the next pass's raw outputs are written behind this barrier, its KL / hit words behind the next one, which these threads pass too)
        if (tid < DS_F16_SLOTS) {
            const long long blk = j0 + (long long)tid * gridDim.x;
            if (blk < A.n_blocks) {
                const long long c0 = blk * DS_BLOCK;
                const int nb = A.n - c0 < DS_BLOCK ? (int)(A.n - c0) : DS_BLOCK;
                ds_write_record(klw + tid * 2 * DS_BLOCK, hit + tid * 2 * DS_BLOCK, nb, blk, A);
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------- the conv learner's bf16 precision
// Connect4ConvNet: <<<min(n_blocks, cap), 512>>>, DsConvGeom::LDS_FLOATS floats of LDS. w = the canonical parameters in f32 (what the
// bf16 learner reads: it rounds its operands itself). Phases F (without the activation store) and H (without dz) of
// conv_grad_step_bf16<512>; H is dataset_eval_blocks_conv_kernel's.
__global__ __launch_bounds__(CONV_TRAIN_THREADS) void dataset_eval_blocks_conv_bf16_kernel(const float* __restrict__ w, DsArgs A) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    using G = ConvMfmaGeom;
    using E = DsConvGeom;
    constexpr int NT = CONV_TRAIN_THREADS, NWV = NT / 64;
    static_assert(NT == 16 * DS_BLOCK, "the heads phase maps thread -> (sample tid >> 4, entry tid & 15)");
    const int tid = threadIdx.x, lane = tid & 63, rw = tid >> 6, j = lane & 15, q = lane >> 4;
    float* part = lds + E::PART_OFF;
    uint64_t* bb = reinterpret_cast<uint64_t*>(lds + E::BB_OFF);
    unsigned* hit = reinterpret_cast<unsigned*>(lds + E::HIT_OFF);
    for (long long blk = blockIdx.x; blk < A.n_blocks; blk += gridDim.x) {
        const size_t c0 = (size_t)blk * DS_BLOCK;
        const int B = A.n - (long long)c0 < DS_BLOCK ? (int)(A.n - (long long)c0) : DS_BLOCK;
        if (tid < 2 * DS_BLOCK) {
            const int b = tid >> 1;
            unsigned long long v = 0ull;
            if (b < B) v = (tid & 1) ? A.op_bb[c0 + b] : A.my_bb[c0 + b];
            bb[tid] = v;
        }
        const int hb = tid >> 4, jx = tid & 15;
        float tgt = 0.0f;
        if (hb < B && jx < 12) {
            const size_t si = c0 + (size_t)hb;
            tgt = jx < 9 ? A.tpi[si * 9 + jx] : A.tv[si * 3 + (jx - 9)];
        }
        const float ltgt = tgt > 0.0f ? det_logf(tgt) : 0.0f;
        __syncthreads();

        // ---- F: conv (k = tap 16 h + 4 q + e) + ReLU + head partials (k = channel 4 q + e), operands rounded to bf16
        for (int wv = rw; wv < 16; wv += NWV) {
            bf16x4 ca[2];
#pragma unroll
            for (int h = 0; h < 2; h++) {
                float t4[4];
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    const int tap = 16 * h + 4 * q + e;
                    t4[e] = tap < 18 ? w[G::P_CW + j * 18 + tap] : 0.0f;
                }
                ca[h] = pack_bf16(t4[0], t4[1], t4[2], t4[3]);
            }
            const f32x4 cbv = *reinterpret_cast<const f32x4*>(w + G::P_CB + 4 * q);
            bf16x4 hwb[4];
#pragma unroll
            for (int c = 0; c < 4; c++) {
                const int p = wv + 16 * c;
                float h4[4];
#pragma unroll
                for (int r = 0; r < 4; r++) h4[r] = (j < 12 && p < G::HW) ? w[G::P_HW + (size_t)j * G::FLAT + (4 * q + r) * G::HW + p] : 0.0f;
                hwb[c] = pack_bf16(h4[0], h4[1], h4[2], h4[3]);
            }
#pragma unroll 1
            for (int t = 0; t < 2; t++) {
                const int sample = 16 * t + j;
                const uint64_t my = bb[2 * sample], op = bb[2 * sample + 1];
                uint64_t S[2][4];
#pragma unroll
                for (int h = 0; h < 2; h++)
#pragma unroll
                    for (int e = 0; e < 4; e++) S[h][e] = conv_tap_board(my, op, 16 * h + 4 * q + e);   // (taps >= 18: empty boards)
                f32x4 hacc = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
                for (int c = 0; c < 4; c++) {
                    const int p = wv + 16 * c;
                    if (p < G::HW) {   // (wave-uniform: only wave 15 has three cells)
                        const int row = p / 9, col = p - 9 * row, pos = row + 7 * col;
                        f32x4 acc = cbv;
#pragma unroll
                        for (int h = 0; h < 2; h++) {
                            const bf16x4 xb = pack_bf16((float)((uint32_t)(S[h][0] >> pos) & 1u), (float)((uint32_t)(S[h][1] >> pos) & 1u),
                                                        (float)((uint32_t)(S[h][2] >> pos) & 1u), (float)((uint32_t)(S[h][3] >> pos) & 1u));
                            acc = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(ca[h], xb, acc, 0, 0, 0);
                        }
                        float a4[4];
#pragma unroll
                        for (int r = 0; r < 4; r++) a4[r] = acc[r] > 0.0f ? acc[r] : 0.0f;
                        hacc = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(hwb[c], pack_bf16(a4[0], a4[1], a4[2], a4[3]), hacc, 0, 0, 0);
                    }
                }
                if (q < 3) {
#pragma unroll
                    for (int r = 0; r < 4; r++) part[(wv * DS_BLOCK + sample) * 12 + 4 * q + r] = hacc[r];
                }
            }
        }
        __syncthreads();

        // ---- H (f32): the 12 outputs (bias + the sixteen partials in order), log_softmax + kl_div; the arg-maxes beside them
        {
            const bool pol = jx < 9;
            const bool live = jx < 12 && hb < B;
            float xo = 0.0f;
            if (jx < 12) {
                xo = w[G::P_HB + jx];
#pragma unroll
                for (int g = 0; g < 16; g++) xo += part[(g * DS_BLOCK + hb) * 12 + jx];
            }
            xo = live ? xo : 0.0f;
            float xs[12], ts[12];
            ep_row_gather(xo, xs);
            ep_row_gather(tgt, ts);
            float mxp = xs[0], mxv = xs[9];
#pragma unroll
            for (int t = 1; t < 9; t++) mxp = xs[t] > mxp ? xs[t] : mxp;
#pragma unroll
            for (int t = 10; t < 12; t++) mxv = xs[t] > mxv ? xs[t] : mxv;
            const float mx = pol ? mxp : mxv;
            const float e = live ? det_expf(xo - mx) : 0.0f;
            const float se = ep_row_sum(e, pol);
            const float lse = mx + det_logf(live ? se : 1.0f);
            const float logp = xo - lse;
            const float term = (live && tgt > 0.0f) ? tgt * (ltgt - logp) : 0.0f;
            const float kl = ep_row_sum(term, pol);
            if (jx == 0 || jx == 9) {
                unsigned h = 0u;
                if (hb < B) {
                    if (pol) {
                        float xp[9];
#pragma unroll
                        for (int t = 0; t < 9; t++) xp[t] = xs[t];
                        h = ds_argmax_legal(xp, bb[2 * hb] | bb[2 * hb + 1]) == ds_argmax_first<9>(ts) ? 1u : 0u;
                    } else {
                        h = ds_argmax_first<3>(xs + 9) == ds_argmax_first<3>(ts + 9) ? 1u : 0u;
                    }
                    if (A.row_kl) A.row_kl[(c0 + (size_t)hb) * 2 + (pol ? 0 : 1)] = kl;
                }
                lds[E::KL_OFF + hb * 2 + (pol ? 0 : 1)] = hb < B ? kl : 0.0f;
                hit[hb * 2 + (pol ? 0 : 1)] = h;
            }
            if (live && A.row_logits) A.row_logits[(c0 + (size_t)hb) * 12 + jx] = xo;
        }
        __syncthreads();
        // (the next block's KL / hit / partial words are written two barriers from here; its boards overwrite words nobody reads now)
        if (tid == 0) ds_write_record(lds + E::KL_OFF, hit, B, blk, A);
    }
}

// <<<1, DS_REDUCE_THREADS>>>: the order of the additions is the definition (top of this file). chunk_sums: ceil(n_blocks / 256) entries.
__global__ __launch_bounds__(DS_REDUCE_THREADS) void dataset_eval_reduce_kernel(const DsBlockRecord* __restrict__ records, long long n_blocks,
                                                                                DsChunkSum* __restrict__ chunk_sums,
                                                                                DsTotals* __restrict__ totals) {
    const long long n_chunks = (n_blocks + DS_CHUNK_BLOCKS - 1) / DS_CHUNK_BLOCKS;
    for (long long c = threadIdx.x; c < n_chunks; c += DS_REDUCE_THREADS) {
        const long long j0 = c * DS_CHUNK_BLOCKS;
        const long long j1 = j0 + DS_CHUNK_BLOCKS < n_blocks ? j0 + DS_CHUNK_BLOCKS : n_blocks;
        DsChunkSum s{0.0, 0.0, 0ull, 0ull, 0ull};
        for (long long j = j0; j < j1; j++) {
            const DsBlockRecord r = records[j];
            s.pi = s.pi + (double)r.rows * (double)r.pi_loss;
            s.v = s.v + (double)r.rows * (double)r.v_loss;
            s.pi_hits += r.pi_hit;
            s.v_hits += r.v_hit;
            s.rows += r.rows;
        }
        chunk_sums[c] = s;
    }
    __syncthreads();   // (one workgroup: its own global stores are visible to its threads behind the barrier)
    if (threadIdx.x == 0) {
        DsTotals t{0.0, 0.0, 0ull, 0ull, 0ull};
        for (long long c = 0; c < n_chunks; c++) {
            const DsChunkSum s = chunk_sums[c];
            t.sum_pi = t.sum_pi + s.pi;
            t.sum_v = t.sum_v + s.v;
            t.pi_hits += s.pi_hits;
            t.v_hits += s.v_hits;
            t.rows += s.rows;
        }
        *totals = t;
    }
}

}  // namespace syn
