// synthesis_amd — host side of the engine and the C ABI (include/synthesis_amd.h).
//
// Host role (what the reference's Rust driver does around the hot path, synthesis/src/alpha_zero.rs:181-209):
// own the device node pool and the weight image, turn the plain-C configs into kernel parameters, launch ONE fused
// kernel per call and hand results back. No torch, no CPU fallback: every entry point either runs the HIP kernels on
// the handle's GPU or returns an error code.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstdlib>
#include <cstdio>
#include <atomic>
#include <cstring>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "../../include/synthesis_amd.h"
#include "engine_kernels.cuh"
#include "eval_small.cuh"
#include "lane_kernel.cuh"
#ifdef SYN_DEBUG_SHAPES   // measured dead ends kept as parity-tested debug shapes: `make DEBUG_SHAPES=1` (default: not in the library)
#include "lane2_kernel.cuh"
#include "pc_kernel.cuh"
#endif
#include "frozen_kernel.cuh"
#include "train_kernels.cuh"
#include "replay_kernels.cuh"
#include "reanalyse_kernels.cuh"
#include "sampler_kernels.cuh"
#include "match_kernels.cuh"
#include "tournament_kernels.cuh"
#include "record_kernels.cuh"
#include "train_mfma.cuh"
#include "train_epoch.cuh"
#include "convnet.cuh"
#include "conv_f16x2_tile.cuh"
#include "layer_kernels.cuh"
#include "train_conv.cuh"
#include "train_conv_mfma.cuh"
#include "train_micro.cuh"
#include "dataset_eval.cuh"
#include "digest_kernels.cuh"
#include "lane_instances.h"
#include "launch_plan.hpp"
#include "position_layout.hpp"
#include "free_kernel.cuh"
#ifdef SYN_DEBUG_SHAPES
#include "pool_kernel.cuh"   // round 6's measured dead end (trees unbound from the lanes): a debug shape like the two above
#endif

#include <hipcub/hipcub.hpp>
#include <chrono>
#include <cmath>
#include <thread>

using namespace syn;

// The lane-per-tree, free-running, pool and two-trees-per-lane instantiations are compiled in the side translation units (engine_conv.hip,
// engine_lanes_*.hip, engine_free.hip, ...: built in parallel); here they are only declared, from the lists those units define them
// from (lane_instances.h).
#define SYN_LANES_ALL_LISTS(X)                                                                                           \
    SYN_LANES_FAST_LIST(X) SYN_LANES_GEN_LIST(X) SYN_LANES_REF_LIST(X) SYN_LANES_F16_LIST(X) SYN_LANES_F16_GEN_LIST(X) \
    SYN_LANES_CONV_LIST(X) SYN_LANES_CONV_F16_LIST(X)
namespace syn {
#define SYN_X(MODE, COUNT, FAST, NW, PROF, POLICY) \
    extern template __global__ void selfplay_kernel_lanes<MODE, COUNT, FAST, NW, PROF, POLICY>(EngineParams);
SYN_LANES_ALL_LISTS(SYN_X)
#undef SYN_X
#define SYN_X(MODE, COUNT, FAST, PROF) extern template __global__ void selfplay_kernel_free<MODE, COUNT, FAST, PROF>(EngineParams);
SYN_FREE_LIST(SYN_X)
#undef SYN_X
#ifdef SYN_DEBUG_SHAPES   // ... and (DEBUG_SHAPES=1 builds only) engine_lanes2.hip and engine_pool.hip / engine_pool_f16.hip
#define SYN_X(MODE, COUNT, FAST, NW, POLICY, TILE) \
    extern template __global__ void selfplay_kernel_lanes2<MODE, COUNT, FAST, NW, POLICY, TILE>(EngineParams);
SYN_LANES2_LIST(SYN_X)
#undef SYN_X
#define SYN_X(MODE, COUNT, FAST, NW, POLICY) extern template __global__ void selfplay_kernel_pool<MODE, COUNT, FAST, NW, POLICY>(EngineParams);
SYN_POOL_F32_LIST(SYN_X)
SYN_POOL_F16_LIST(SYN_X)
#undef SYN_X
#endif
}  // namespace syn

static_assert(sizeof(DevSearchResult) == sizeof(syn_search_result), "search result layout must match the C ABI");
static_assert(sizeof(syn_counters) == sizeof(unsigned long long) * CTR_COUNT, "counter layout must match the C ABI");

static thread_local std::string g_create_error;

// Developer knobs (launch-shape overrides, in-kernel phase stamps) are read from the environment ONLY when SYN_DEBUG=1 is
// set as well: a stray variable must never change the launch shape of a production call.
static const char* debug_env(const char* name) {
    const char* on = std::getenv("SYN_DEBUG");
    if (!on || on[0] != '1') return nullptr;
    return std::getenv(name);
}

struct syn_engine {
    int device = 0;
    int num_cus = 256;
    hipStream_t stream = nullptr;
    hipStream_t aux_stream = nullptr;  // syn_progress / syn_cancel: independent of the launch stream
    int* h_pin = nullptr;              // 512 pinned bytes for their transfers: [0..1] syn_progress, [8] syn_cancel's word, [9] its pre-read;
                                       // [16 .. 16 + K + 2) (the launch stream's, not theirs) the game loop's group starts and error word
    // The call in flight (syn_selfplay_run / syn_mcts_search* / syn_frozen_search_rollout) as syn_progress / syn_cancel see it.
    // call_mu orders their state changes and serialises the users of aux_stream and h_pin.
    std::mutex call_mu;
    int call_state = 0;                // 0 idle, 1 launching (the job counter's reset is not enqueued yet), 2 running
    int cancel_pending = 0;            // a syn_cancel that arrived while launching: applied right behind the counter's reset
    int cancel_applied = 0;            // the running call's job counter was raised past its job count
    int started_at_cancel = 0;         // jobs handed out when that happened (read just before the write)
    int running_jobs = 0;              // job count of the call in flight (0 = none)
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    int slots = 0;
    int last_shape = 0, last_grid = 0, last_threads = 0;
    int pool_trees = 0;  // (DEBUG_SHAPES builds) > 64: the pool kernel with that many trees per wave; never set: the kernel is forced by SYN_POOL only
    int last_pool_trees = 0;
    int pool_slots = 0;  // tree slabs actually allocated (slots rounded up to the largest workgroup + slack)
    int max_explores = 0;
    uint32_t cap = 0;
    float4* d_stat = nullptr;
    uint4* d_edge = nullptr;
    // The network the engine evaluates, in which arithmetic, and its images. Written by install_network (syn_load_weights*,
    // syn_trainer_publish_weights) and syn_set_network_arithmetic only.
    // Invariant: an engine with weights in the f16x2 arithmetic holds a current f16x2 image (img16_current, of host_blob, which is the
    // network d_wimg holds). A load or a switch that is refused for want of an f16x2 plan returns before anything here, or the policy
    // cache, changes. Two corners leave arith == F16X2 with img16_current == false, and every evaluation is then refused
    // (require_f16x2_image, SYN_ERR_UNSUPPORTED) until a load, a publish or a switch succeeds: a publish of parameters that have no
    // plan (the f32 image and host_blob are the new network's by then), and a HIP error in the middle of an image upload.
    struct Network {
        int kind = 0;   // which network d_wimg holds: 0 = Connect4Net (mlp.cuh), 1 = Connect4ConvNet (convnet.cuh); index of g_net_desc
        int arith = SYN_NET_ARITH_F32;   // syn_set_network_arithmetic (Connect4Net: f16x2_tile.cuh, Connect4ConvNet: conv_f16x2_tile.cuh)
        bool has_weights = false;
        float* d_wimg = nullptr;         // the f32 image (allocated with the engine, sized for Connect4Net's, the larger one)
        uint32_t* d_wimg16 = nullptr;    // the f16x2 image (allocated on first use, likewise)
        std::vector<float> host_blob;    // the current network's parameters: what the f16x2 image and plan are built from
        bool img16_current = false;      // d_wimg16 is the image of host_blob
        bool f16x2() const { return arith == SYN_NET_ARITH_F16X2; }
        // the image the current arithmetic evaluates
        const float* image() const { return f16x2() ? reinterpret_cast<const float*>(d_wimg16) : d_wimg; }
    } net;
    // The game loop's own device memory (run_games: syn_match_run, syn_match_run_sides, syn_tournament_run): one network image per
    // network player of the call, a match's in entries 0 and 1 (never the engine's: a call leaves `net` and the policy cache as they
    // were), and one allocation for the live-game arrays, the per-ply results and the per-game outputs (GamesLayout), laid out
    // afresh by every call
    struct Games {
        void* d_img[SYN_TOURNAMENT_MAX_PLAYERS] = {};   // allocated on demand, each sized for the largest image of either network in either arithmetic
        unsigned char* d_buf = nullptr;
        size_t buf_bytes = 0;
    } games;
    int* d_job_next = nullptr;
    uint4* d_cache = nullptr;      // PolicyWithCache table (policy_cache_log2 > 0)
    int cache_log2 = 0;
    unsigned long long* d_cache_stats = nullptr;
    unsigned long long last_cache_hits = 0, last_cache_misses = 0;
    // the device-resident replay buffer (syn_replay_*; replay_kernels.cuh): sections my | op | gid | pi | v of replay_cap positions each
    // in ONE allocation; d_replay_alt is the keep-window's second buffer (same size, allocated when a keep first drops something)
    unsigned char* d_replay = nullptr;
    unsigned char* d_replay_alt = nullptr;
    size_t replay_cap = 0, replay_n = 0;
    int last_selfplay_games = -1;  // games of the last syn_selfplay_run whose outputs are in d_plies / d_states / d_pis / d_vs (-1: none yet)
    uint4* d_path = nullptr;   // lane kernel's per-wave descent logs
    size_t path_bytes = 0;
    unsigned char* d_vw = nullptr;  // producer/consumer kernel: per-virtual-wave parked state + network outputs
    size_t vw_bytes = 0;
    unsigned long long* d_counters = nullptr;
    // self-play output buffers (device), grown on demand
    int out_games = 0;
    int* d_plies = nullptr;
    unsigned long long* d_states = nullptr;
    float* d_pis = nullptr;
    float* d_vs = nullptr;
    unsigned char* d_actions = nullptr;
    uint32_t* d_root_nodes = nullptr;
    unsigned char* d_final = nullptr;
    // scratch for host-pointer entry points
    void* d_scratch = nullptr;
    size_t scratch_bytes = 0;
    std::atomic<bool> eval_attr_set[EVAL_KERNELS] = {};   // launch_eval: the kernel's LDS attribute is set (indexed by EvalKernel)
    size_t eval_poll_max = 1024;       // contexts: batches up to this size signal completion through pinned memory (SYN_DEBUG=1 SYN_EVAL_POLL_MAX)
    size_t eval_zero_copy_out = 4096;  // contexts: results of up to this many positions are written into the pinned buffer by the kernel itself
    bool eval_throughput_only = false;   // syn_policy_eval_batch_device: the throughput kernel at every size (SYN_DEBUG=1 SYN_EVAL_THROUGHPUT=1: tests of its tile)
    struct syn_eval_ctx* eval_ctx = nullptr;   // syn_policy_eval_batch's own evaluation context (created on first use)
    std::string err;
    float last_kernel_ms = 0.0f;
    int last_launches = 0;
    // The learner (syn_trainer_init / syn_trainer_init_conv). Both networks' trainers share it; the buffers are sized for Connect4Net, the
    // larger one (learner_buffers).
    struct Learner {
        // parameters, Adam moments, gradient + loss scratch
        float* d_tw = nullptr;
        float* d_tm = nullptr;
        float* d_tv = nullptr;
        float* d_tgrad = nullptr;
        float* d_tloss = nullptr;
        float* d_twimg = nullptr;  // the trainer's weights in the inference fragment order (forward A operands; = the published image)
        float* d_ttimg = nullptr;  // ... and transposed fragments for the activation gradients (train_mfma.cuh)
        float* d_timg2 = nullptr;  // the second buffer of both images for the persistent epoch kernel (train_epoch.cuh): [fwd][transposed]
        unsigned* d_tsync = nullptr;  // its arrival counter and status word
        float* d_tsnap = nullptr;     // snapshot of [w][m][v][fwd image][transposed image] taken before an epoch launch (restored if it aborts)
        float* d_cxbuf = nullptr;     // Connect4ConvNet learner on four workgroups: the exchange buffer (train_conv_mfma.cuh ConvMwGeom)
        PositionRows data;  // syn_train_set_data: the learner's data set
        long long train_step = 0;
        DevTrainHyper train_hp{};
        bool has_trainer = false;
        int trainer_kind = 0;  // 0 = Connect4Net (train_mfma.cuh / train_epoch.cuh), 1 = Connect4ConvNet (train_conv_mfma.cuh)
        int train_bf16 = 0;    // Connect4ConvNet learner: 1 = the bf16 matrix-core variant of the gradient step (syn_trainer_set_precision)
        bool epoch_barrier_checked = false;  // syn_trainer_init's self-check of the epoch kernel's one-XCD barrier has run on this engine
        bool epoch_device_scope = false;     // ... and it failed (or is running its second half): the epoch kernel uses the device-scope barrier
        long long epoch_fallbacks = 0;  // syn_train_epoch calls whose persistent kernel gave up and ran through the queued launches
        bool conv_mw_checked = false;   // syn_trainer_init_conv's self-check of the four-workgroup kernel against the one-workgroup kernel has run
        bool conv_mw_disabled = false;  // ... and it failed: this engine keeps the one-workgroup epoch kernel
        int conv_mw_force = -1;         // self-check only: 0 = one workgroup, 1 = four
        // syn_trainer_set_batch_mode (train_micro.cuh); every syn_trainer_init* puts the first two back to chained / 0
        int batch_mode = SYN_TRAIN_BATCH_CHAINED;
        int micro_max_wgs = 0;          // cap on the blocks launch's workgroups; 0 = the device's CU count
        int micro_last_grid = 0;        // grid of the last blocks launch (0: none yet)
        float* d_micro_rows = nullptr;  // the block buffer: row j = [g_j][l_j] of micro-batch j (MicroPlan::row_stride); grown on demand
        size_t micro_rows_bytes = 0;
    } learner;
    // The evaluation set (syn_dataset_set / syn_dataset_get / syn_dataset_evaluate): a second data set in the learner's layout that
    // no trainer call reads or writes, and the image buffer a syn_dataset_evaluate with a blob of its own builds into.
    struct EvalSet {
        PositionRows rows;
        size_t n_unseen = 0;      // rows [0, n_unseen): states that are not in the learner's data set (syn_dataset_counts); syn_dataset_set: n
        uint64_t holdout_key = 0, holdout_threshold = 0;   // syn_replay_set_holdout; threshold 0 = nothing is held out
        float* d_img = nullptr;   // sized for the larger of Connect4Net's f32 image and Connect4ConvNet's parameters; allocated on first use
        uint32_t* d_img16 = nullptr;   // the f16x2 image a syn_dataset_evaluate_arith in SYN_EVAL_ARITH_F16X2 builds (F16Geom::IMG_WORDS); on first use
    } evalset;
};

// The learner's eleven device buffers: the one description used to allocate them (alloc_trainer_buffers: all of them or none) and to
// free them (syn_engine_destroy).
struct LearnerBuffers {
    struct {
        void** p;
        size_t bytes;
    } all[11];
};
static LearnerBuffers learner_buffers(syn_engine::Learner& L) {
    const size_t bytes = (size_t)TrainGeom::NUM_PARAMS * 4;
    const size_t img = (size_t)MlpGeom::IMG_FLOATS * 4, timg = (size_t)TrainImg::T_FLOATS * 4;
    const auto at = [](auto& field) { return reinterpret_cast<void**>(&field); };
    return {{{at(L.d_tw), bytes}, {at(L.d_tm), bytes}, {at(L.d_tv), bytes}, {at(L.d_tgrad), bytes}, {at(L.d_tloss), 64},
             {at(L.d_twimg), img}, {at(L.d_ttimg), timg}, {at(L.d_timg2), img + timg}, {at(L.d_tsync), 256},
             {at(L.d_tsnap), 3 * bytes + img + timg}, {at(L.d_cxbuf), (size_t)ConvMwGeom::FLOATS * 4}}};
}

static int fail(syn_engine* h, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    if (h) h->err = buf;
    else g_create_error = buf;
    return code;
}

// for the library's host-only translation units (lockstep_capi.cpp)
extern "C" int syn_internal_fail(syn_engine* h, int code, const char* msg) { return fail(h, code, "%s", msg); }
extern "C" int syn_internal_concurrent_games(const syn_engine* h) { return h ? h->slots : 0; }
#ifdef SYN_DEBUG_SHAPES
// present only in `make DEBUG_SHAPES=1` builds: the tests of the two debug launch shapes skip when it is absent
extern "C" int syn_internal_debug_shapes(void) { return 1; }
#endif

#define HIP_TRY(h, call)                                                                          \
    do {                                                                                          \
        hipError_t e_ = (call);                                                                   \
        if (e_ != hipSuccess)                                                                     \
            return fail(h, SYN_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

static int ensure_scratch(syn_engine* h, size_t bytes) {
    if (bytes <= h->scratch_bytes) return SYN_OK;
    if (h->d_scratch) HIP_TRY(h, hipFree(h->d_scratch));
    h->d_scratch = nullptr;
    h->scratch_bytes = 0;
    size_t want = bytes + bytes / 4 + 4096;
    HIP_TRY(h, hipMalloc(&h->d_scratch, want));
    h->scratch_bytes = want;
    return SYN_OK;
}

// The search kernels' error word (EngineParams::error) as a call's refusal: 0 = none (SYN_OK), 2 = a tree's node blocks ran out, anything
// else = a bounded spin gave up. `suffix` is appended to the capacity message.
static int fail_search_error(syn_engine* h, int kerr, const char* suffix = "") {
    if (kerr == 0) return SYN_OK;
    if (kerr == 2)
        return fail(h, SYN_ERR_CAPACITY, "a tree ran out of node blocks (lane-per-tree kernel: %u blocks per tree for max_explores %d)%s",
                    h->cap / 4, h->max_explores, suffix);
    return fail(h, SYN_ERR_HIP, "kernel reported a synchronisation timeout (bounded spin gave up)");
}

// ------------------------------------------------------------------------------------------------ weight image
// blob order: l_k.weight[O][I] then l_k.bias[O] for k = 1..5 (study-connect4/src/policies.rs:20-24)
static void build_weight_image(const float* blob, std::vector<float>& img) {
    img.assign(MlpGeom::IMG_FLOATS, 0.0f);
    size_t off = 0;
    for (int l = 0; l < MlpGeom::NL; l++) {
        const int K = MlpGeom::K[l], O = MlpGeom::O[l], S4 = MlpGeom::S4[l], NOB = MlpGeom::NOB[l];
        const float* W = blob + off;
        const float* b = W + (size_t)K * O;
        off += (size_t)K * O + O;
        for (int s4 = 0; s4 < S4; s4++)
            for (int ob = 0; ob < NOB; ob++)
                for (int lane = 0; lane < 64; lane++)
                    for (int r = 0; r < 4; r++) {
                        int i = lane & 15, q = lane >> 4;
                        int unit = mlp_unit_of_row(l, ob, i);
                        int k = 16 * s4 + 4 * r + q;
                        float v = (unit < O && k < K) ? W[(size_t)unit * K + k] : 0.0f;
                        img[MlpGeom::W_OFF[l] + ((s4 * NOB + ob) * 64 + lane) * 4 + r] = v;
                    }
        for (int ob = 0; ob < NOB; ob++)
            for (int q = 0; q < 4; q++)
                for (int r = 0; r < 4; r++) {
                    int unit = mlp_unit_of_row(l, ob, 4 * q + r);
                    img[MlpGeom::W_FLOATS + MlpGeom::B_OFF[l] + (ob * 4 + q) * 4 + r] = unit < O ? b[unit] : 0.0f;
                }
    }
}


// ------------------------------------------------------------------------------------------------ progress / cancel bracket
// Every entry point that plays jobs from the device-side job counter (d_job_next[0]) brackets its launch with a CallScope:
//   CallScope scope(h, n_jobs);          state = launching: a syn_cancel from another thread is remembered, nothing touches the device
//   ... enqueue the counter's reset ...
//   scope.armed();                       state = running; a remembered cancel is enqueued right behind the reset (same stream)
//   ... launch, copies, synchronise ...
//   scope.cancelled()                    did a cancel reach this call?  (the caller then decides from what actually finished)
// and the destructor returns the engine to idle. syn_cancel on an idle engine is an error: there is nothing to cancel.
constexpr int CANCEL_WORD = 0x40000000;
struct CallScope {
    syn_engine* e;
    CallScope(syn_engine* h, int n_jobs) : e(h) {
        std::lock_guard<std::mutex> g(e->call_mu);
        e->call_state = 1;
        e->cancel_pending = 0;
        e->cancel_applied = 0;
        e->started_at_cancel = 0;
        e->running_jobs = n_jobs;
    }
    hipError_t armed() {
        std::lock_guard<std::mutex> g(e->call_mu);
        e->call_state = 2;
        if (!e->cancel_pending) return hipSuccess;
        e->cancel_pending = 0;
        e->cancel_applied = 1;
        e->started_at_cancel = 0;
        e->h_pin[8] = CANCEL_WORD;
        return hipMemcpyAsync(e->d_job_next, e->h_pin + 8, 4, hipMemcpyHostToDevice, e->stream);
    }
    bool cancelled() {
        std::lock_guard<std::mutex> g(e->call_mu);
        return e->cancel_applied != 0;
    }
    ~CallScope() {
        std::lock_guard<std::mutex> g(e->call_mu);
        e->call_state = 0;
        e->cancel_pending = 0;
        e->running_jobs = 0;
    }
};

// ------------------------------------------------------------------------------------------------ config checks
static int convert_mcts(syn_engine* h, const syn_mcts_config* c, DevMctsCfg& d) {
    if (!c) return fail(h, SYN_ERR_INVALID_ARGUMENT, "mcts config is NULL");
    if (c->exploration != SYN_EXPLORATION_UCT && c->exploration != SYN_EXPLORATION_POLYNOMIAL_UCT)
        return fail(h, SYN_ERR_INVALID_ARGUMENT, "unknown exploration %d", c->exploration);
    if (c->fpu == SYN_FPU_FUNC)
        return fail(h, SYN_ERR_UNSUPPORTED, "SYN_FPU_FUNC (Fpu::Func(fn() -> f32), config.rs:25) is a host function: a device kernel cannot call it. "
                                            "It runs on the host trees (syn_mcts_search_lockstep / syn_selfplay_run_lockstep); on the device, "
                                            "SYN_FPU_NORMAL is the reference's own Normal(mean, std) closure");
    if (c->fpu != SYN_FPU_CONST && c->fpu != SYN_FPU_PARENT_Q && c->fpu != SYN_FPU_NORMAL)
        return fail(h, SYN_ERR_INVALID_ARGUMENT, "unknown fpu %d", c->fpu);
    if (c->fpu == SYN_FPU_NORMAL && !(c->fpu_std >= 0.0f && c->fpu_std < 1e30f && c->fpu_value == c->fpu_value))
        return fail(h, SYN_ERR_INVALID_ARGUMENT, "SYN_FPU_NORMAL needs a finite mean and a standard deviation >= 0 (Normal::new)");
    if (c->root_policy_noise != SYN_NOISE_NONE && c->root_policy_noise != SYN_NOISE_EQUAL && c->root_policy_noise != SYN_NOISE_DIRICHLET)
        return fail(h, SYN_ERR_INVALID_ARGUMENT, "unknown root policy noise %d", c->root_policy_noise);
    if (c->root_policy_noise != SYN_NOISE_NONE && !(c->noise_weight >= 0.0f))
        return fail(h, SYN_ERR_INVALID_ARGUMENT, "PolicyNoise weight must be >= 0");
    if (c->root_policy_noise == SYN_NOISE_DIRICHLET && !(c->noise_alpha > 0.0f && c->noise_alpha < 1e30f))
        return fail(h, SYN_ERR_INVALID_ARGUMENT, "PolicyNoise::Dirichlet alpha must be > 0 (Dirichlet::new_with_size)");
    d.exploration = c->exploration;
    d.c = c->c;
    d.solve = c->solve != 0;
    d.correct_values = c->correct_values_on_solve != 0;
    d.select_solved = c->select_solved_nodes != 0;
    d.auto_extend = c->auto_extend != 0;
    d.fpu = c->fpu;
    d.fpu_value = c->fpu_value;
    d.noise = c->root_policy_noise;
    d.noise_weight = c->noise_weight;
    d.fpu_std = c->fpu_std;
    d.noise_alpha = c->noise_alpha;
    // (c * prior * sqrt(N)) / (1 + n) goes through div2_safe_range only when the numerator stays inside its exact range
    d.fast_div = (c->c >= 0x1p-10f && c->c <= 0x1p10f) ? 1 : 0;
    return SYN_OK;
}

// ------------------------------------------------------------------------------------------------ launches
// Which kernel plays a call and on what shape is decided in launch_plan.hpp (plan_launch: a pure function, tested on a CPU). Here:
// the table of the instantiations the library ships, the lookup of a plan's kernel in it and the one place that launches.
static_assert(PLAN_LANE_MAX_CAP == LANE_MAX_CAP && PLAN_PATH_ENTRIES == PATH_ENTRIES, "launch_plan.hpp restates lane_kernel.cuh");
static_assert(MODE_SELFPLAY == 0 && MODE_SEARCH == 1, "launch_plan.hpp restates engine_kernels.cuh's MODE_*");
#ifdef SYN_DEBUG_SHAPES
static_assert(PLAN_PC_TREE_WAVES == PcGeom::TREE_WAVES && PLAN_PC_NT == PcGeom::NT && PLAN_PC_NV_MAX == PcGeom::NV_MAX &&
              PLAN_PC_VW_BYTES == PcGeom::VW_BYTES, "launch_plan.hpp restates pc_kernel.cuh");
static_assert(PLAN_POOL_M_MAX == PoolGeom::M_MAX && PLAN_POOL_WAVE_BYTES == PoolGeom::WAVE_BYTES, "launch_plan.hpp restates pool_kernel.cuh");
#endif

struct KernelEntry {
    int shape;   // LaunchPlan::shape
    int mode, count, fast, n, prof, policy, tile;
    void (*fn)(EngineParams);
    size_t lds;
};
// the row-per-tree, quad and producer/consumer kernels are instantiated by this translation unit, for the four kinds of call
#define SYN_CALL_LIST(X) X(MODE_SEARCH, false, false) X(MODE_SELFPLAY, false, false) X(MODE_SELFPLAY, true, false) X(MODE_SELFPLAY, false, true)
#define SYN_ROW(MODE, COUNT, PROF, WPS, FAST) \
    {WPS, MODE, COUNT, FAST, WPS, PROF, 0, 0, selfplay_kernel<MODE, COUNT, WPS, FAST, PROF>, WPS == 1 ? EngineLds::BYTES_WPS1 : EngineLds::BYTES_WPS2},
#define SYN_QUAD(MODE, COUNT, PROF, NQ, FAST) {3, MODE, COUNT, FAST, NQ, PROF, 0, 0, selfplay_kernel_quads<MODE, COUNT, FAST, NQ, PROF>, QuadLds<NQ>::BYTES},
#ifdef SYN_DEBUG_SHAPES
#define SYN_PC(MODE, COUNT, PROF, FAST) {5, MODE, COUNT, FAST, 0, PROF, 0, 0, selfplay_kernel_pc<MODE, COUNT, FAST, PROF>, PcLds::BYTES},
#else
#define SYN_PC(MODE, COUNT, PROF, FAST)
#endif
static const KernelEntry g_kernels[] = {
#define SYN_X(MODE, COUNT, PROF)                                                                                                    \
    SYN_ROW(MODE, COUNT, PROF, 1, false) SYN_ROW(MODE, COUNT, PROF, 1, true) SYN_ROW(MODE, COUNT, PROF, 2, false) SYN_ROW(MODE, COUNT, PROF, 2, true) \
    SYN_QUAD(MODE, COUNT, PROF, 2, false) SYN_QUAD(MODE, COUNT, PROF, 2, true) SYN_QUAD(MODE, COUNT, PROF, 3, false)                \
    SYN_QUAD(MODE, COUNT, PROF, 3, true) SYN_QUAD(MODE, COUNT, PROF, 4, false) SYN_QUAD(MODE, COUNT, PROF, 4, true)                 \
    SYN_PC(MODE, COUNT, PROF, false) SYN_PC(MODE, COUNT, PROF, true)
    SYN_CALL_LIST(SYN_X)
#undef SYN_X
#define SYN_X(MODE, COUNT, FAST, NW, PROF, POLICY) \
    {4, MODE, COUNT, FAST, NW, PROF, POLICY, 0, selfplay_kernel_lanes<MODE, COUNT, FAST, NW, PROF, POLICY>, LaneLds<NW>::BYTES},
    SYN_LANES_ALL_LISTS(SYN_X)
#undef SYN_X
#define SYN_X(MODE, COUNT, FAST, PROF) {7, MODE, COUNT, FAST, 0, PROF, 0, 0, selfplay_kernel_free<MODE, COUNT, FAST, PROF>, FreeLds::BYTES},
    SYN_FREE_LIST(SYN_X)
#undef SYN_X
#ifdef SYN_DEBUG_SHAPES
#define SYN_X(MODE, COUNT, FAST, NW, POLICY, TILE) \
    {6, MODE, COUNT, FAST, NW, false, POLICY, TILE, selfplay_kernel_lanes2<MODE, COUNT, FAST, NW, POLICY, TILE>, Lane2Lds<NW>::BYTES},
    SYN_LANES2_LIST(SYN_X)
#undef SYN_X
#define SYN_X(MODE, COUNT, FAST, NW, POLICY) \
    {8, MODE, COUNT, FAST, NW, false, POLICY, 0, selfplay_kernel_pool<MODE, COUNT, FAST, NW, POLICY>, PoolLds<NW, FAST>::BYTES},
    SYN_POOL_F32_LIST(SYN_X) SYN_POOL_F16_LIST(SYN_X)
#undef SYN_X
#endif
};
#undef SYN_ROW
#undef SYN_QUAD
#undef SYN_PC
#undef SYN_CALL_LIST

// The plan's instantiation; where a profile is requested and no profiled instantiation ships, the plain one. nullptr: not in the library.
static const KernelEntry* find_kernel(const LaunchPlan& p) {
    for (int prof = p.prof ? 1 : 0; prof >= 0; prof--)
        for (const KernelEntry& e : g_kernels)
            if (e.shape == p.shape && e.mode == p.mode && e.count == (int)p.count && e.fast == p.fast && e.n == p.n && e.prof == prof &&
                e.policy == p.policy && e.tile == p.tile)
                return &e;
    return nullptr;
}

// the developer knobs of the launch selection (honoured with SYN_DEBUG=1 only: debug_env)
static LaunchKnobs read_launch_knobs() {
    LaunchKnobs k;
    const auto num = [](const char* name, int& v) { if (const char* ev = debug_env(name)) v = std::atoi(ev); };
    num("SYN_LANES", k.lanes); num("SYN_FREE", k.free_run); num("SYN_QUADS", k.quads);
    num("SYN_LANE_THRESH", k.lane_thresh); num("SYN_SCAN_MIN", k.scan_min); num("SYN_ABLATE", k.ablate);
#ifdef SYN_DEBUG_SHAPES
    const auto flag = [](const char* name, int& v) { if (debug_env(name)) v = 1; };
    num("SYN_PC", k.pc); num("SYN_PC_PRIO", k.pc_prio); flag("SYN_PC_STUB", k.pc_stub);
    num("SYN_LANES2", k.lanes2); flag("SYN_L2_TILE", k.l2_tile);
    num("SYN_POOL", k.pool); num("SYN_POOL_NW", k.pool_nw); num("SYN_POOL_FIRE", k.pool_fire); num("SYN_POOL_SCAN", k.pool_scan);
#endif
    return k;
}

// a device buffer that only grows: at least `need` bytes behind buf
template <class T>
static hipError_t ensure_device_buffer(T*& buf, size_t& have, size_t need) {
    if (need <= have) return hipSuccess;
    if (buf) (void)hipFree(buf);
    buf = nullptr;
    have = 0;
    hipError_t e = hipMalloc(&buf, need);
    if (e == hipSuccess) have = need;
    return e;
}

// Grows the buffers the plan needs, fills the EngineParams fields it fixes, looks its kernel up and launches it.
static int launch_planned(syn_engine* h, const LaunchPlan& plan, EngineParams P) {
    if (plan.error)
        return fail(h, SYN_ERR_HIP, "launch failed: %s (this configuration runs in the lane-per-tree kernels only: at most %u nodes per tree, this engine: %u)",
                    hipGetErrorString(hipErrorInvalidValue), LANE_MAX_CAP, h->cap);
    const KernelEntry* k = find_kernel(plan);
    if (!k)
        return fail(h, SYN_ERR_UNSUPPORTED, "this library ships no kernel for launch shape %d with (mode %d, count %d, fast %d, n %d, prof %d, policy %d, tile %d)",
                    plan.shape, plan.mode, (int)plan.count, plan.fast, plan.n, (int)plan.prof, plan.policy, plan.tile);
    HIP_TRY(h, ensure_device_buffer(h->d_path, h->path_bytes, plan.path_entries * sizeof(uint4)));
    HIP_TRY(h, ensure_device_buffer(h->d_vw, h->vw_bytes, plan.vw_bytes));
    P.path = h->d_path;
    P.vw_buf = h->d_vw;
    P.lane_thresh = plan.lane_thresh;
    P.nv = plan.nv;
    P.debug_prio = plan.debug_prio;
    P.debug_stub = plan.debug_stub;
    if (plan.no_cache) P.cache = nullptr;
    HIP_TRY(h, hipFuncSetAttribute(reinterpret_cast<const void*>(k->fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)k->lds));
    hipLaunchKernelGGL(k->fn, dim3(plan.grid), dim3(plan.threads), k->lds, h->stream, P);
    h->last_shape = plan.shape; h->last_grid = plan.grid; h->last_threads = plan.threads;
    if (plan.shape == 8) h->last_pool_trees = plan.pool_trees;
    HIP_TRY(h, hipGetLastError());
    return SYN_OK;
}

// `arith`: PLAN_ARITH_* of the image P.wimg points at (launch_plan.hpp). The engine's own calls leave the default; a match side passes
// the arithmetic its image was built in, so an f32 engine launches the f16x2 kernels for an f16x2 side and the reverse.
static int launch_engine(syn_engine* h, const EngineParams& P, int jobs, int mode, bool count, bool prof, int arith = PLAN_ARITH_ENGINE) {
    LaunchEngine e;
    e.num_cus = h->num_cus;
    e.slots = h->slots;
    e.cap = h->cap;
    e.net_kind = h->net.kind;
    e.f16 = h->net.f16x2();
    e.pool_trees = h->pool_trees;
    const LaunchQuery q = launch_query(e, arith, jobs, mode, count, prof, P.mcts.fpu, P.mcts.noise, cfg_family(P.mcts));
    return launch_planned(h, plan_launch(q, read_launch_knobs()), P);
}

extern "C" {

void syn_default_rollout_config(syn_rollout_config* cfg) {
    if (!cfg) return;
    std::memset(cfg, 0, sizeof(*cfg));
    cfg->num_explores = 800;
    cfg->random_actions_until = 1;
    cfg->sample_actions_until = 30;
    cfg->stop_games_when_solved = 0;
    cfg->value_target = SYN_VALUE_Q;
    cfg->action = SYN_ACTION_NUM_VISITS;
    cfg->mcts_cfg.exploration = SYN_EXPLORATION_POLYNOMIAL_UCT;
    cfg->mcts_cfg.c = 3.0f;
    cfg->mcts_cfg.solve = 1;
    cfg->mcts_cfg.correct_values_on_solve = 1;
    cfg->mcts_cfg.select_solved_nodes = 1;
    cfg->mcts_cfg.auto_extend = 1;
    cfg->mcts_cfg.fpu = SYN_FPU_CONST;
    cfg->mcts_cfg.fpu_value = 1.0f;
    cfg->mcts_cfg.root_policy_noise = SYN_NOISE_NONE;
}

const char* syn_last_error(const syn_engine* h) { return h ? h->err.c_str() : g_create_error.c_str(); }

int syn_engine_create(const syn_engine_config* cfg, int device, syn_engine** out) {
    if (!cfg || !out) return fail(nullptr, SYN_ERR_INVALID_ARGUMENT, "cfg/out is NULL");
    *out = nullptr;
    if (cfg->concurrent_games < 1 || cfg->max_explores < 1)
        return fail(nullptr, SYN_ERR_INVALID_ARGUMENT, "concurrent_games and max_explores must be >= 1");
    if (cfg->policy_cache_log2 != 0 && (cfg->policy_cache_log2 < 10 || cfg->policy_cache_log2 > 30))
        return fail(nullptr, SYN_ERR_INVALID_ARGUMENT, "policy_cache_log2 must be 0 (off) or 10..30");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(nullptr, SYN_ERR_NO_DEVICE, "no HIP device visible (the engine has no CPU fallback)");
    if (device < 0 || device >= ndev)
        return fail(nullptr, SYN_ERR_NO_DEVICE, "device %d out of range (%d visible)", device, ndev);
    syn_engine* h = new (std::nothrow) syn_engine();
    if (!h) return fail(nullptr, SYN_ERR_HIP, "out of host memory");
    h->device = device;
    auto bail = [&](const char* what, hipError_t e) {
        int rc = fail(nullptr, SYN_ERR_HIP, "%s failed: %s", what, hipGetErrorString(e));
        syn_engine_destroy(h);
        return rc;
    };
    hipError_t e;
    if ((e = hipSetDevice(device)) != hipSuccess) return bail("hipSetDevice", e);
    hipDeviceProp_t prop;
    if ((e = hipGetDeviceProperties(&prop, device)) != hipSuccess) return bail("hipGetDeviceProperties", e);
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        int rc = fail(nullptr, SYN_ERR_NO_DEVICE, "device %d is %s; this library is built for gfx950 only", device,
                      prop.gcnArchName);
        syn_engine_destroy(h);
        return rc;
    }
    h->num_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    h->slots = ((cfg->concurrent_games + 15) / 16) * 16;
    h->max_explores = cfg->max_explores;
    if (const char* ev = debug_env("SYN_EVAL_POLL_MAX")) h->eval_poll_max = (size_t)std::atoll(ev);
    if (const char* ev = debug_env("SYN_EVAL_ZC_OUT")) h->eval_zero_copy_out = (size_t)std::atoll(ev);
    if (const char* ev = debug_env("SYN_EVAL_THROUGHPUT")) h->eval_throughput_only = ev[0] == '1';
    // nodes.len() <= 1 + 9*(explores+1), rounded up to keep slabs 16-byte-record aligned per 4 nodes
    h->cap = (uint32_t)(1 + 9 * (cfg->max_explores + 1));
    h->cap = (h->cap + 3u) & ~3u;
    if ((e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking)) != hipSuccess) return bail("hipStreamCreate", e);
    {
        // the progress / cancel stream must never share a hardware queue with the launch stream (it would wait behind the running
        // kernel): the runtime deals streams of one priority round-robin over a few queues, so after enough streams in a process
        // two of them coincide — a different priority class has its own queues
        int lo = 0, hi = 0;
        if ((e = hipDeviceGetStreamPriorityRange(&lo, &hi)) != hipSuccess) return bail("hipDeviceGetStreamPriorityRange", e);
        if ((e = hipStreamCreateWithPriority(&h->aux_stream, hipStreamNonBlocking, hi)) != hipSuccess) return bail("hipStreamCreate", e);
    }
    if ((e = hipHostMalloc(reinterpret_cast<void**>(&h->h_pin), 512)) != hipSuccess) return bail("hipHostMalloc", e);
    if ((e = hipEventCreate(&h->ev0)) != hipSuccess) return bail("hipEventCreate", e);
    if ((e = hipEventCreate(&h->ev1)) != hipSuccess) return bail("hipEventCreate", e);
    // the launch may round the slot count up to a whole workgroup (<= 1024 trees: lane kernel)
    // + 48: the 3-quad launch rounds to multiples of 48 slots
    // (768: the 12-wave lane kernel rounds to multiples of 768 slots)
    // (2304: the producer/consumer kernel rounds to multiples of 768 x NV slots, NV <= 3)
    // (1536: the two-trees-per-lane kernel with 12 waves rounds to multiples of 1,536 slots)
    h->pool_slots = ((h->slots + 1023) / 1024) * 1024 + 2304;
    size_t nodes = (size_t)h->pool_slots * h->cap;
    if ((e = hipMalloc(&h->d_stat, nodes * 32)) != hipSuccess) return bail("hipMalloc(node pool)", e);
    h->d_edge = reinterpret_cast<uint4*>(h->d_stat);  // same records, edge half = odd 16-byte elements
    if (cfg->policy_cache_log2 != 0) {
        h->cache_log2 = cfg->policy_cache_log2;
        const size_t bytes = (size_t)64 << h->cache_log2;
        if ((e = hipMalloc(&h->d_cache, bytes)) != hipSuccess) return bail("hipMalloc(policy cache)", e);
        // empty: an all-zero entry never verifies. (On the engine's own stream: a memset on the null stream is asynchronous to the host
        // and not ordered against a non-blocking stream's launches.)
        if ((e = hipMemsetAsync(h->d_cache, 0, bytes, h->stream)) != hipSuccess) return bail("hipMemsetAsync(policy cache)", e);
    }
    if ((e = hipMalloc(&h->d_cache_stats, 16)) != hipSuccess) return bail("hipMalloc(cache stats)", e);
    if ((e = hipMalloc(&h->net.d_wimg, MlpGeom::IMG_FLOATS * sizeof(float))) != hipSuccess) return bail("hipMalloc(wimg)", e);
    if ((e = hipMalloc(&h->d_job_next, 64)) != hipSuccess) return bail("hipMalloc(job)", e);
    if ((e = hipMemsetAsync(h->d_job_next, 0, 64, h->stream)) != hipSuccess) return bail("hipMemsetAsync(job)", e);  // syn_progress before the first launch reads zeros
    if ((e = hipStreamSynchronize(h->stream)) != hipSuccess) return bail("hipStreamSynchronize", e);
    if ((e = hipMalloc(&h->d_counters, sizeof(DevCounters))) != hipSuccess) return bail("hipMalloc(counters)", e);
    *out = h;
    return SYN_OK;
}

int syn_engine_destroy(syn_engine* h) {
    if (!h) return SYN_OK;
    hipSetDevice(h->device);
    if (h->eval_ctx) syn_eval_ctx_destroy(h->eval_ctx);
    if (h->stream) hipStreamSynchronize(h->stream);
    hipFree(h->d_stat);
    hipFree(h->net.d_wimg);
    hipFree(h->net.d_wimg16);
    for (void* img : h->games.d_img) hipFree(img);
    hipFree(h->games.d_buf);
    hipFree(h->d_job_next);
    hipFree(h->d_path);
    hipFree(h->d_vw);
    hipFree(h->learner.data.d);
    hipFree(h->learner.d_micro_rows);
    hipFree(h->evalset.rows.d);
    hipFree(h->evalset.d_img);
    hipFree(h->evalset.d_img16);
    hipFree(h->d_replay);
    hipFree(h->d_replay_alt);
    hipFree(h->d_cache);
    hipFree(h->d_cache_stats);
    hipFree(h->d_counters);
    hipFree(h->d_plies);
    hipFree(h->d_states);
    hipFree(h->d_pis);
    hipFree(h->d_vs);
    hipFree(h->d_actions);
    hipFree(h->d_root_nodes);
    hipFree(h->d_final);
    hipFree(h->d_scratch);
    const LearnerBuffers learner_bufs = learner_buffers(h->learner);
    for (const auto& b : learner_bufs.all) hipFree(*b.p);
    if (h->ev0) hipEventDestroy(h->ev0);
    if (h->ev1) hipEventDestroy(h->ev1);
    if (h->stream) hipStreamDestroy(h->stream);
    if (h->aux_stream) hipStreamDestroy(h->aux_stream);
    if (h->h_pin) hipHostFree(h->h_pin);
    delete h;
    return SYN_OK;
}

// ------------------------------------------------------------------------------------------------ the engine's network
// (state and invariant: syn_engine::Network)
// What differs between the two networks on the host, indexed by Network::kind.
struct NetDesc {
    const char* name;   // as messages say it
    int num_params;
    bool lane_only;     // evaluated by the lane-per-tree kernels only: engines of more than LANE_MAX_CAP nodes per tree cannot hold it
    void (*build_f32)(const float* blob, std::vector<float>& img);          // the f32 fragment image of a blob
    bool (*build_f16x2)(const float* blob, std::vector<uint32_t>& words);   // its f16x2 image; false = the blob has no f16x2 plan
    size_t param_bytes() const { return (size_t)num_params * 4; }
};
static bool build_mlp_f16x2_words(const float* blob, std::vector<uint32_t>& words) {
    F16Image im;
    if (!build_f16x2_image(blob, im)) return false;
    words.swap(im.words);
    return true;
}
static bool build_conv_f16x2_words(const float* blob, std::vector<uint32_t>& words) {
    ConvF16Image im;
    if (!build_conv_f16x2_image(blob, im)) return false;
    words.swap(im.words);
    return true;
}
static void build_conv_image_vec(const float* blob, std::vector<float>& img) {
    img.resize((size_t)ConvGeom::IMG_FLOATS);
    build_conv_image(blob, img.data());
}
static const NetDesc g_net_desc[2] = {
    {"Connect4Net", MlpGeom::NUM_PARAMS, false, build_weight_image, build_mlp_f16x2_words},
    {"Connect4ConvNet", ConvGeom::NUM_PARAMS, true, build_conv_image_vec, build_conv_f16x2_words},
};
static_assert(TrainGeom::NUM_PARAMS == MlpGeom::NUM_PARAMS, "the learner's Connect4Net is the engine's");
static_assert(ConvGeom::IMG_FLOATS <= MlpGeom::IMG_FLOATS && ConvF16Geom::IMG_WORDS <= F16Geom::IMG_WORDS,
              "both image buffers are sized for Connect4Net");

// The one text and status of each refusal in this section; the evaluation contexts put the same texts into their own error slot.
static const char* const MSG_NO_WEIGHTS = "call syn_load_weights first";
static const char* const MSG_NO_F16X2_IMAGE = "the engine is in the f16x2 arithmetic but holds no f16x2 image of its parameters";
static bool lacks_f16x2_image(const syn_engine* h) { return h->net.f16x2() && (!h->net.img16_current || !h->net.d_wimg16); }
static int require_weights(syn_engine* h) { return h->net.has_weights ? SYN_OK : fail(h, SYN_ERR_NO_WEIGHTS, "%s", MSG_NO_WEIGHTS); }
// every path that evaluates a network in the f16x2 arithmetic checks this first
static int require_f16x2_image(syn_engine* h) { return lacks_f16x2_image(h) ? fail(h, SYN_ERR_UNSUPPORTED, "%s", MSG_NO_F16X2_IMAGE) : SYN_OK; }
// Fpu::Func, PolicyNoise::Dirichlet, Connect4ConvNet and the f16x2 arithmetic exist in the lane-per-tree kernels only, whose block ids
// are 14 bits: an engine created for more than 7,280 explores cannot run them. Said before anything is enqueued or changed.
static int require_lane_cap(syn_engine* h, const char* what) {
    if (h->cap <= LANE_MAX_CAP) return SYN_OK;
    return fail(h, SYN_ERR_UNSUPPORTED, "%s runs in the lane-per-tree kernels only: max_explores must be <= %u (this engine: %d)", what,
                (LANE_MAX_CAP - 1u) / 9u - 1u, h->max_explores);
}
static int require_lane_cap_of_network(syn_engine* h, int kind) {
    return g_net_desc[kind].lane_only ? require_lane_cap(h, g_net_desc[kind].name) : SYN_OK;
}
// the f16x2 image of `blob`, parameters of network `kind`, or the one refusal of parameters that have no plan
static int f16x2_image_of(syn_engine* h, int kind, const float* blob, std::vector<uint32_t>& words) {
    if (g_net_desc[kind].build_f16x2(blob, words)) return SYN_OK;
    return fail(h, SYN_ERR_UNSUPPORTED, "these parameters have no f16x2 plan (non-finite values or scales outside the f32-safe window): a load "
                                        "or a switch leaves the engine as it was, a publish leaves it without an f16x2 image");
}
// PolicyWithCache entries belong to the network and the arithmetic that produced them (the reference builds a fresh cache per
// run_n_games, alpha_zero.rs:196-198; the two arithmetics differ in the last bits): an all-zero entry never verifies. Stream-ordered
// before every launch that reads the table.
static int empty_policy_cache(syn_engine* h) {
    if (h->d_cache) HIP_TRY(h, hipMemsetAsync(h->d_cache, 0, (size_t)64 << h->cache_log2, h->stream));
    return SYN_OK;
}

// Parameters become something a kernel reads in two steps: the image of the blob that one arithmetic evaluates is built on the host,
// then uploaded into a device buffer. install_network and ensure_f16x2_image run them for the engine's own buffers, syn_match_run for
// the two buffers a match owns.
struct HostImage {
    bool f16x2 = false;
    std::vector<float> f32;         // !f16x2: the f32 fragment image
    std::vector<uint32_t> words;    // f16x2: the f16x2 image
    const void* data() const { return f16x2 ? static_cast<const void*>(words.data()) : static_cast<const void*>(f32.data()); }
    size_t bytes() const { return (f16x2 ? words.size() : f32.size()) * 4; }
};
// a device buffer that holds any image of either network
constexpr size_t NET_IMAGE_MAX_BYTES = (size_t)(MlpGeom::IMG_FLOATS > F16Geom::IMG_WORDS ? MlpGeom::IMG_FLOATS : F16Geom::IMG_WORDS) * 4;
// (f16x2: parameters without a plan are refused, SYN_ERR_UNSUPPORTED, before anything has been touched)
static int build_host_image(syn_engine* h, int kind, const float* blob, bool f16x2, HostImage& im) {
    im.f16x2 = f16x2;
    if (f16x2) return f16x2_image_of(h, kind, blob, im.words);
    g_net_desc[kind].build_f32(blob, im.f32);
    return SYN_OK;
}
// enqueued on the engine's stream: the caller synchronises before `im` goes away
static int enqueue_image_upload(syn_engine* h, const HostImage& im, void* d_dst) {
    HIP_TRY(h, hipMemcpyAsync(d_dst, im.data(), im.bytes(), hipMemcpyHostToDevice, h->stream));
    return SYN_OK;
}

// (Connect4ConvNet's f16x2 image, conv_f16x2_tile.cuh, lives in the same buffer as Connect4Net's: it is the smaller of the two)
static int upload_f16x2_image(syn_engine* h, const HostImage& im) {
    HIP_TRY(h, hipSetDevice(h->device));   // (every caller has selected it by now; kept because this helper allocates: test_abi_and_host.py)
    if (!h->net.d_wimg16) HIP_TRY(h, hipMalloc(&h->net.d_wimg16, (size_t)F16Geom::IMG_WORDS * 4));
    const int rc = enqueue_image_upload(h, im, h->net.d_wimg16);
    if (rc != SYN_OK) return rc;
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return SYN_OK;
}
// the plan of a blob, selected by its size (30,492 floats: Connect4Net, five layers; 12,412: Connect4ConvNet, layer 0 = the conv
// layer whose inputs enter unscaled, layer 1 = the head, entries 2..4 zero); plan->valid = 0 when it has none
static void fill_f16x2_plan(const float* blob, size_t n_floats, syn_f16x2_plan* plan) {
    std::memset(plan, 0, sizeof(*plan));
    if (n_floats == (size_t)MlpGeom::NUM_PARAMS) {
        F16Image im;
        if (build_f16x2_image(blob, im)) {
            plan->valid = 1;
            for (int l = 0; l < 5; l++) { plan->activation_exp[l] = im.s[l]; plan->weight_exp[l] = im.t[l]; plan->bound[l] = im.bound[l]; }
            plan->out_exp = im.out_exp;
        }
    } else if (n_floats == (size_t)ConvGeom::NUM_PARAMS) {
        ConvF16Image im;
        if (build_conv_f16x2_image(blob, im)) {
            plan->valid = 1;
            plan->activation_exp[0] = 0; plan->weight_exp[0] = im.tc; plan->bound[0] = im.bound[0];
            plan->activation_exp[1] = im.s1; plan->weight_exp[1] = im.th; plan->bound[1] = im.bound[1];
            plan->out_exp = im.out_exp;
        }
    }
}
// builds the f16x2 image from the engine's own copy of the parameters when it is not current (a switch into the arithmetic; a publish
// while in it) and commits it; a refusal leaves everything as it was
static int ensure_f16x2_image(syn_engine* h) {
    auto& N = h->net;
    if (N.img16_current) return SYN_OK;
    if (N.host_blob.size() != (size_t)g_net_desc[N.kind].num_params)
        return fail(h, SYN_ERR_UNSUPPORTED, "the engine holds no host copy of its parameters to build the f16x2 image from");
    HostImage im;
    int rc = build_host_image(h, N.kind, N.host_blob.data(), true, im);
    if (rc == SYN_OK) rc = upload_f16x2_image(h, im);
    if (rc != SYN_OK) return rc;
    N.img16_current = true;
    return SYN_OK;
}

// The one way a network becomes the engine's (the caller has selected the engine's device and checked require_lane_cap_of_network): `blob` = its parameters on the host (syn_load_weights*), or NULL = the learner's, on the
// device (syn_trainer_publish_weights). Order: (host parameters, f16x2 arithmetic) the f16x2 image is built first and a blob without a
// plan is refused before anything of the engine changes; the images; the policy cache; then the state is committed. A publish cannot
// know whether its parameters have a plan before it has read them back, by which time the f32 image is the new network's: it commits,
// then builds the f16x2 image, and a refusal there is the corner Network's invariant names.
static int install_network(syn_engine* h, int kind, const float* blob) {
    auto& N = h->net;
    const NetDesc& d = g_net_desc[kind];
    const bool want16 = N.f16x2();
    if (blob) {
        HostImage im16, img;
        if (want16) { const int rc = build_host_image(h, kind, blob, true, im16); if (rc != SYN_OK) return rc; }
        build_host_image(h, kind, blob, false, img);
        if (want16) {
            N.img16_current = false;
            const int rc = upload_f16x2_image(h, im16);
            if (rc != SYN_OK) return rc;
        }
        { const int rc = enqueue_image_upload(h, img, N.d_wimg); if (rc != SYN_OK) return rc; }
        HIP_TRY(h, hipStreamSynchronize(h->stream));
    } else if (kind == 1) {
        // Connect4ConvNet: the fragment image of convnet.cuh is rebuilt from the canonical parameters on the device
        hipLaunchKernelGGL(conv_image_kernel, dim3((ConvGeom::IMG_FLOATS + 255) / 256), dim3(256), 0, h->stream, h->learner.d_tw, N.d_wimg);
        HIP_TRY(h, hipGetLastError());
    } else {
        // Connect4Net: the trainer keeps its weights in the inference fragment order as well (train_mfma.cuh): publishing is one device copy
        HIP_TRY(h, hipMemcpyAsync(N.d_wimg, h->learner.d_twimg, (size_t)MlpGeom::IMG_FLOATS * 4, hipMemcpyDeviceToDevice, h->stream));
    }
    { const int rc = empty_policy_cache(h); if (rc != SYN_OK) return rc; }
    if (blob) {
        N.host_blob.assign(blob, blob + d.num_params);
    } else {
        // the f16x2 image is built on the host from the canonical parameters: keep a copy of what was published
        N.host_blob.resize((size_t)d.num_params);
        HIP_TRY(h, hipMemcpyAsync(N.host_blob.data(), h->learner.d_tw, d.param_bytes(), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
    }
    N.has_weights = true;
    N.kind = kind;
    N.img16_current = blob && want16;
    return !blob && want16 ? ensure_f16x2_image(h) : SYN_OK;   // an engine in the f16x2 arithmetic stays in it
}

static int check_blob(syn_engine* h, int kind, const float* blob, size_t n_floats) {
    if (!h) return SYN_ERR_INVALID_ARGUMENT;
    if (!blob) return fail(h, SYN_ERR_INVALID_ARGUMENT, "blob is NULL");
    const NetDesc& d = g_net_desc[kind];
    if (n_floats != (size_t)d.num_params) return fail(h, SYN_ERR_INVALID_ARGUMENT, "%s has %d parameters, got %zu", d.name, d.num_params, n_floats);
    return require_lane_cap_of_network(h, kind);
}
int syn_load_weights(syn_engine* h, const float* blob, size_t n_floats) {
    const int rc = check_blob(h, 0, blob, n_floats);
    if (rc != SYN_OK) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    return install_network(h, 0, blob);
}
int syn_load_weights_conv(syn_engine* h, const float* blob, size_t n_floats) {
    const int rc = check_blob(h, 1, blob, n_floats);
    if (rc != SYN_OK) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    return install_network(h, 1, blob);
}

int syn_set_network_arithmetic(syn_engine* h, int arithmetic) {
    if (!h) return SYN_ERR_INVALID_ARGUMENT;
    if (arithmetic != SYN_NET_ARITH_F32 && arithmetic != SYN_NET_ARITH_F16X2)
        return fail(h, SYN_ERR_INVALID_ARGUMENT, "unknown network arithmetic %d", arithmetic);
    if (arithmetic == h->net.arith) return SYN_OK;
    if (arithmetic == SYN_NET_ARITH_F16X2) { const int rc = require_lane_cap(h, "the f16x2 arithmetic"); if (rc != SYN_OK) return rc; }
    HIP_TRY(h, hipSetDevice(h->device));
    // the image first (of whichever network the engine holds); the switch is committed only when it exists
    if (arithmetic == SYN_NET_ARITH_F16X2 && h->net.has_weights) { const int rc = ensure_f16x2_image(h); if (rc != SYN_OK) return rc; }
    h->net.arith = arithmetic;
    return empty_policy_cache(h);
}

int syn_get_network_arithmetic(syn_engine* h, int* arithmetic, syn_f16x2_plan* plan) {
    if (!h) return SYN_ERR_INVALID_ARGUMENT;
    if (arithmetic) *arithmetic = h->net.arith;
    if (plan) {
        std::memset(plan, 0, sizeof(*plan));
        if (h->net.has_weights && !h->net.host_blob.empty()) fill_f16x2_plan(h->net.host_blob.data(), h->net.host_blob.size(), plan);
    }
    return SYN_OK;
}

int syn_f16x2_plan_of_blob(const float* blob, size_t n_floats, syn_f16x2_plan* plan) {
    if (!blob || !plan || (n_floats != (size_t)MlpGeom::NUM_PARAMS && n_floats != (size_t)ConvGeom::NUM_PARAMS))
        return SYN_ERR_INVALID_ARGUMENT;
    fill_f16x2_plan(blob, n_floats, plan);
    return SYN_OK;
}

// ------------------------------------------------------------------------------------------------ policy evaluation
// Which kernel evaluates a batch is decided in launch_plan.hpp (plan_eval: a pure function, tested on a CPU). Here: the table from its
// kernel ids to the functions and the one place that launches them.
using EvalFnF32 = void (*)(const float*, const unsigned long long*, const unsigned long long*, int, float*, float*);
using EvalFnF16 = void (*)(const uint32_t*, const unsigned long long*, const unsigned long long*, int, float*, float*);
using EvalFnTile = void (*)(const float*, const unsigned long long*, const unsigned long long*, int, float*, float*, unsigned*, unsigned*, unsigned);
struct EvalKernelEntry {
    EvalFnF32 f32;     // exactly one of the three is set: the kernel reads the f32 image,
    EvalFnF16 f16;     // ... the f16x2 image,
    EvalFnTile tile;   // ... or is the latency kernel (f32 image + the completion protocol's three arguments)
};
static const EvalKernelEntry g_eval_kernels[EVAL_KERNELS] = {
    /* EVAL_TILE */ {nullptr, nullptr, policy_eval_tile_kernel},
    /* EVAL_MLP_512 */ {policy_eval_kernel<512>, nullptr, nullptr},
    /* EVAL_MLP_768 */ {policy_eval_kernel<768>, nullptr, nullptr},
    /* EVAL_CONV_512 */ {policy_eval_conv_kernel<512>, nullptr, nullptr},
    /* EVAL_F16_512 */ {nullptr, policy_eval_f16x2_kernel<512>, nullptr},
    /* EVAL_F16_1024 */ {nullptr, policy_eval_f16x2_kernel<1024>, nullptr},
    /* EVAL_CONV_F16_512 */ {nullptr, policy_eval_conv_f16x2_kernel<512>, nullptr},
};
static_assert(EVAL_TILE == 0 && EVAL_MLP_512 == 1 && EVAL_MLP_768 == 2 && EVAL_CONV_512 == 3 && EVAL_F16_512 == 4 && EVAL_F16_1024 == 5 &&
              EVAL_CONV_F16_512 == 6 && EVAL_KERNELS == 7, "g_eval_kernels is in EvalKernel's order");
static_assert(PLAN_MLP_IMG_BYTES == (size_t)MlpGeom::IMG_FLOATS * 4 && PLAN_CONV_IMG_BYTES == (size_t)ConvGeom::IMG_FLOATS * 4 &&
              PLAN_F16_IMG_BYTES == (size_t)F16Geom::IMG_WORDS * 4 && PLAN_CONV_F16_IMG_BYTES == (size_t)ConvF16Geom::IMG_WORDS * 4,
              "launch_plan.hpp restates mlp.cuh, convnet.cuh, f16x2_tile.cuh and conv_f16x2_tile.cuh");
constexpr size_t EVAL_TILE_LDS = 14 * 64 * 16;   // policy_eval_tile_kernel (eval_small.cuh): exA 8 x 64 x 16 B + exB 6 x 64 x 16 B
static_assert(PLAN_EVAL_TILE_LDS == EVAL_TILE_LDS && EVAL_TILE_LDS <= 64 * 1024, "launch_plan.hpp restates the tile kernel's LDS; it needs no attribute");

// the completion protocol of a polled call (eval_small.cuh): workgroups finished, the pinned word, this call's number
struct EvalCompletion {
    unsigned* done_blocks = nullptr;
    unsigned* host_flag = nullptr;
    unsigned seq = 0u;
};
static EvalQuery eval_query(const syn_engine* h, int n) {
    EvalQuery q;
    q.net_kind = h->net.kind;
    q.f16 = h->net.f16x2();
    q.n = n;
    q.num_cus = h->num_cus;
    return q;
}
// The plan's kernel over the engine's network on `st` (any stream of the engine's device): n positions, pointers the device can
// read / write (device memory or pinned, device-mapped host memory).
static hipError_t launch_eval(syn_engine* h, const EvalPlan& p, hipStream_t st, const uint64_t* d_my, const uint64_t* d_op, int n,
                              float* d_logits, float* d_value, const EvalCompletion& done = EvalCompletion()) {
    const EvalKernelEntry& k = g_eval_kernels[p.kernel];
    const void* fn = k.tile ? reinterpret_cast<const void*>(k.tile) : k.f16 ? reinterpret_cast<const void*>(k.f16) : reinterpret_cast<const void*>(k.f32);
    // above the 64 KB a kernel gets unasked (all but the tile kernel), the function's attribute is set once per engine: the call costs a microsecond
    if (p.lds > 64 * 1024 && !h->eval_attr_set[p.kernel].load(std::memory_order_acquire)) {
        const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds);
        if (e != hipSuccess) return e;
        h->eval_attr_set[p.kernel].store(true, std::memory_order_release);
    }
    const unsigned long long* my = reinterpret_cast<const unsigned long long*>(d_my);
    const unsigned long long* op = reinterpret_cast<const unsigned long long*>(d_op);
    const dim3 grid((unsigned)p.grid), threads((unsigned)p.threads);
    if (k.tile) hipLaunchKernelGGL(k.tile, grid, threads, p.lds, st, h->net.d_wimg, my, op, n, d_logits, d_value, done.done_blocks, done.host_flag, done.seq);
    else if (p.f16_image) hipLaunchKernelGGL(k.f16, grid, threads, p.lds, st, h->net.d_wimg16, my, op, n, d_logits, d_value);
    else hipLaunchKernelGGL(k.f32, grid, threads, p.lds, st, h->net.d_wimg, my, op, n, d_logits, d_value);
    return hipGetLastError();
}

int syn_policy_eval_batch_device(syn_engine* h, const uint64_t* d_my, const uint64_t* d_op, int n, float* d_logits,
                                 float* d_value, int sync) {
    if (!h) return SYN_ERR_INVALID_ARGUMENT;
    if (n < 0 || (n > 0 && (!d_my || !d_op || !d_logits || !d_value)))
        return fail(h, SYN_ERR_INVALID_ARGUMENT, "bad arguments to syn_policy_eval_batch_device");
    { const int rc = require_weights(h); if (rc != SYN_OK) return rc; }
    if (n == 0) return SYN_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipEventRecord(h->ev0, h->stream));
    { const int rc16 = require_f16x2_image(h); if (rc16 != SYN_OK) return rc16; }
    EvalQuery q = eval_query(h, n);
    // (the debug knob plans as for a batch just past the latency kernel's range: the throughput kernels take any n, idle workgroups return)
    if (h->eval_throughput_only && (size_t)q.n <= PLAN_EVAL_TILE_MAX) q.n = (int)PLAN_EVAL_TILE_MAX + 1;
    HIP_TRY(h, launch_eval(h, plan_eval(q), h->stream, d_my, d_op, n, d_logits, d_value));
    HIP_TRY(h, hipEventRecord(h->ev1, h->stream));
    h->last_launches = 1;
    if (sync) {
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        HIP_TRY(h, hipEventElapsedTime(&h->last_kernel_ms, h->ev0, h->ev1));
    }
    return SYN_OK;
}

// ---- evaluation contexts: one worker's policy (alpha_zero.rs:192-198 gives every worker thread of gather_experience its own) ----
// A context owns a stream, pinned staging and device scratch, and reads the engine's weight image; contexts of one engine run
// side by side from different host threads. Errors stay in the context (the engine's error slot belongs to the engine's thread).
// one polite spin-wait step on the host CPU
static inline void spin_pause() {
#if defined(__x86_64__) || defined(__i386__)
    __builtin_ia32_pause();
#elif defined(__aarch64__)
    asm volatile("yield" ::: "memory");
#else
    std::this_thread::yield();
#endif
}

struct syn_eval_ctx {
    syn_engine* h = nullptr;
    hipStream_t stream = nullptr;
    void* h_stage = nullptr;   // [my n][op n][logits 9n][value 3n]
    void* d_out = nullptr;     // results of batches too large to be written across the host link in place
    size_t cap = 0;            // positions the two buffers hold
    int pending = 0;           // positions of the submitted batch (0 = none)
    bool out_in_place = false;
    unsigned* d_done = nullptr;   // the latency kernels' completion protocol (eval_small.cuh): workgroups finished, device word
    unsigned* h_flag = nullptr;   // ... and the word in pinned host memory the last one stores the call's sequence number into
    unsigned seq = 0;
    bool polled = false;          // the submitted batch signals through h_flag
    bool poll_broken = false;     // a completion word went missing once: stream synchronisation from then on
    std::string err;
};
static int ctx_fail(syn_eval_ctx* c, int code, const char* what, hipError_t e = hipSuccess) {
    c->err = what;
    if (e != hipSuccess) c->err += std::string(": ") + hipGetErrorString(e);
    return code;
}
#define CTX_TRY(c, call)                                                  \
    do {                                                                  \
        hipError_t e_ = (call);                                           \
        if (e_ != hipSuccess) return ctx_fail(c, SYN_ERR_HIP, #call, e_); \
    } while (0)

int syn_eval_ctx_create(syn_engine* h, syn_eval_ctx** out) {
    if (!h) return SYN_ERR_INVALID_ARGUMENT;
    if (!out) return fail(h, SYN_ERR_INVALID_ARGUMENT, "syn_eval_ctx_create: out is NULL");
    *out = nullptr;
    HIP_TRY(h, hipSetDevice(h->device));
    syn_eval_ctx* c = new (std::nothrow) syn_eval_ctx;
    if (!c) return fail(h, SYN_ERR_HIP, "out of host memory");
    c->h = h;
    hipError_t e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&c->d_done), 64);
    // (stream-ordered in front of the context's kernels; SYN_DEBUG=1 SYN_EVAL_BREAK_COUNTER=1 starts the counter off wrong: the test of
    // syn_eval_ctx_wait's way out when a completion word goes missing)
    if (e == hipSuccess) e = hipMemsetAsync(c->d_done, debug_env("SYN_EVAL_BREAK_COUNTER") ? 1 : 0, 64, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) e = hipHostMalloc(reinterpret_cast<void**>(&c->h_flag), 64, hipHostMallocDefault);
    if (e != hipSuccess) {
        syn_eval_ctx_destroy(c);
        return fail(h, SYN_ERR_HIP, "syn_eval_ctx_create: %s", hipGetErrorString(e));
    }
    *c->h_flag = 0u;
    *out = c;
    return SYN_OK;
}

int syn_eval_ctx_destroy(syn_eval_ctx* c) {
    if (!c) return SYN_OK;
    hipSetDevice(c->h->device);
    if (c->stream) {
        hipStreamSynchronize(c->stream);
        hipStreamDestroy(c->stream);
    }
    if (c->h_stage) hipHostFree(c->h_stage);
    if (c->d_out) hipFree(c->d_out);
    if (c->d_done) hipFree(c->d_done);
    if (c->h_flag) hipHostFree(c->h_flag);
    delete c;
    return SYN_OK;
}

const char* syn_eval_ctx_last_error(const syn_eval_ctx* c) { return c ? c->err.c_str() : "context is NULL"; }

int syn_eval_ctx_submit(syn_eval_ctx* c, const uint64_t* my_bb, const uint64_t* op_bb, int n) {
    if (!c) return SYN_ERR_INVALID_ARGUMENT;
    if (n < 0 || (n > 0 && (!my_bb || !op_bb))) return ctx_fail(c, SYN_ERR_INVALID_ARGUMENT, "bad arguments to syn_eval_ctx_submit");
    if (c->pending != 0) return ctx_fail(c, SYN_ERR_INVALID_ARGUMENT, "syn_eval_ctx_submit: the previous batch has not been waited for");
    syn_engine* h = c->h;
    if (!h->net.has_weights) return ctx_fail(c, SYN_ERR_NO_WEIGHTS, MSG_NO_WEIGHTS);
    if (lacks_f16x2_image(h)) return ctx_fail(c, SYN_ERR_UNSUPPORTED, MSG_NO_F16X2_IMAGE);
    if (n == 0) return SYN_OK;
    CTX_TRY(c, hipSetDevice(h->device));
    const size_t nb = (size_t)n;
    if (nb > c->cap) {
        CTX_TRY(c, hipStreamSynchronize(c->stream));
        if (c->h_stage) CTX_TRY(c, hipHostFree(c->h_stage));
        if (c->d_out) CTX_TRY(c, hipFree(c->d_out));
        c->h_stage = c->d_out = nullptr;
        c->cap = 0;
        const size_t want = nb + nb / 4 + 256;
        CTX_TRY(c, hipHostMalloc(&c->h_stage, want * 64, hipHostMallocDefault));
        CTX_TRY(c, hipMalloc(&c->d_out, want * 48));
        c->cap = want;
    }
    uint64_t* s_my = static_cast<uint64_t*>(c->h_stage);
    uint64_t* s_op = s_my + nb;
    float* s_logits = reinterpret_cast<float*>(s_op + nb);
    std::memcpy(s_my, my_bb, nb * 8);
    std::memcpy(s_op, op_bb, nb * 8);
    EvalQuery q = eval_query(h, n);
    q.poll_max = h->eval_poll_max;
    q.zero_copy_out = h->eval_zero_copy_out;
    q.poll_broken = c->poll_broken;
    const EvalPlan plan = plan_eval(q);
    c->out_in_place = plan.in_place;
    c->polled = plan.polled;
    float* o_logits = c->out_in_place ? s_logits : static_cast<float*>(c->d_out);
    EvalCompletion done;
    if (c->polled) done = EvalCompletion{c->d_done, c->h_flag, c->seq += 1u};   // syn_eval_ctx_wait polls h_flag for this call's number
    CTX_TRY(c, launch_eval(h, plan, c->stream, s_my, s_op, n, o_logits, o_logits + nb * 9, done));
    if (!c->out_in_place) CTX_TRY(c, hipMemcpyAsync(s_logits, c->d_out, nb * 48, hipMemcpyDeviceToHost, c->stream));
    c->pending = n;
    return SYN_OK;
}

int syn_eval_ctx_wait(syn_eval_ctx* c, float* logits, float* value) {
    if (!c) return SYN_ERR_INVALID_ARGUMENT;
    if (c->pending == 0) return SYN_OK;
    if (!logits || !value) return ctx_fail(c, SYN_ERR_INVALID_ARGUMENT, "bad arguments to syn_eval_ctx_wait");
    const size_t nb = (size_t)c->pending;
    c->pending = 0;
    // (under CombiningPolicy the wait runs on whichever worker thread finishes the batch: that thread may never have selected the device)
    CTX_TRY(c, hipSetDevice(c->h->device));
    bool done = false;
    if (c->polled) {
        // at most ~300 us of polling (a call is tens of microseconds; behind a long self-play launch the kernel is far away and a
        // burning core buys nothing); a kernel that has not reported by then falls through to the stream, where a fault shows as an error
        const volatile unsigned* flag = c->h_flag;
        const auto t_poll = std::chrono::steady_clock::now();
        for (int spin = 0; !done; spin++) {
            done = *flag == c->seq;
            if (done) break;
            spin_pause();
            if ((spin & 255) == 255 && std::chrono::steady_clock::now() - t_poll > std::chrono::microseconds(300)) break;
        }
        std::atomic_thread_fence(std::memory_order_acquire);
    }
    if (!done) {
        CTX_TRY(c, hipStreamSynchronize(c->stream));
        if (c->polled && *static_cast<const volatile unsigned*>(c->h_flag) != c->seq) {
            // The stream is drained, so the kernel has finished and its results are complete — only the completion word is missing
            // (the workgroup counter was disturbed). Not an error for the caller: note it, put the counter back and let this context
            // wait on its stream from now on.
            unsigned done_word = 0xFFFFFFFFu;
            if (hipMemcpy(&done_word, c->d_done, 4, hipMemcpyDeviceToHost) != hipSuccess) done_word = 0xFFFFFFFFu;   // (diagnostic only)
            char msg[256];
            std::snprintf(msg, sizeof msg, "note: an evaluation kernel finished without reporting completion (n %zu, call %u, word in pinned "
                          "memory %u, workgroups counted %u); this context now waits on its stream", nb, c->seq,
                          *static_cast<const volatile unsigned*>(c->h_flag), done_word);
            c->err = msg;
            c->poll_broken = true;
            CTX_TRY(c, hipMemsetAsync(c->d_done, 0, 64, c->stream));
            CTX_TRY(c, hipStreamSynchronize(c->stream));
        }
    }
    const float* s_logits = reinterpret_cast<const float*>(static_cast<const uint64_t*>(c->h_stage) + 2 * nb);
    std::memcpy(logits, s_logits, nb * 36);
    std::memcpy(value, s_logits + nb * 9, nb * 12);
    return SYN_OK;
}

int syn_eval_ctx_eval(syn_eval_ctx* c, const uint64_t* my_bb, const uint64_t* op_bb, int n, float* logits, float* value) {
    const int rc = syn_eval_ctx_submit(c, my_bb, op_bb, n);
    return rc != SYN_OK ? rc : syn_eval_ctx_wait(c, logits, value);
}

int syn_policy_eval_batch(syn_engine* h, const uint64_t* my_bb, const uint64_t* op_bb, int n, float* logits,
                          float* value) {
    if (!h) return SYN_ERR_INVALID_ARGUMENT;
    if (n < 0 || (n > 0 && (!my_bb || !op_bb || !logits || !value)))
        return fail(h, SYN_ERR_INVALID_ARGUMENT, "bad arguments to syn_policy_eval_batch");
    { const int rc = require_weights(h); if (rc != SYN_OK) return rc; }
    if (n == 0) return SYN_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t nb = (size_t)n;
    constexpr size_t EVAL_STAGE_MAX = 32768;  // beyond it two host copies cost more than the runtime's pageable path (measured)
    if (nb <= EVAL_STAGE_MAX && debug_env("SYN_EVAL_PAGEABLE") == nullptr) {
        // A call of this size is latency, not bandwidth (a Rust `impl Policy` adaptor calls with n = 1, a host-tree driver with the
        // leaves of one round): the engine's own evaluation context — positions read and small results written in pinned host
        // memory in place, the latency kernel, completion polled (syn_eval_ctx_* above). Pageable transfers cost a staging copy and
        // a synchronisation each inside the runtime, four per call.
        if (!h->eval_ctx) {
            const int rc = syn_eval_ctx_create(h, &h->eval_ctx);
            if (rc != SYN_OK) return rc;
        }
        const int rc = syn_eval_ctx_eval(h->eval_ctx, my_bb, op_bb, n, logits, value);
        if (rc != SYN_OK) return fail(h, rc, "%s", h->eval_ctx->err.c_str());
        h->last_launches = 1;
        h->last_kernel_ms = 0.0f;   // (not measured on this path: no events in a latency call)
        return SYN_OK;
    }
    // large batches: the runtime's own chunked transfers from / to the pageable buffers around the throughput kernel
    int rc = ensure_scratch(h, nb * (8 + 8 + 36 + 12) + 256);
    if (rc != SYN_OK) return rc;
    char* base = static_cast<char*>(h->d_scratch);
    uint64_t* d_my = reinterpret_cast<uint64_t*>(base);
    uint64_t* d_op = d_my + nb;
    float* d_logits = reinterpret_cast<float*>(d_op + nb);
    float* d_value = d_logits + nb * 9;
    HIP_TRY(h, hipMemcpyAsync(d_my, my_bb, nb * 8, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipMemcpyAsync(d_op, op_bb, nb * 8, hipMemcpyHostToDevice, h->stream));
    rc = syn_policy_eval_batch_device(h, d_my, d_op, n, d_logits, d_value, 0);
    if (rc != SYN_OK) return rc;
    HIP_TRY(h, hipMemcpyAsync(logits, d_logits, nb * 36, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipMemcpyAsync(value, d_value, nb * 12, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    HIP_TRY(h, hipEventElapsedTime(&h->last_kernel_ms, h->ev0, h->ev1));
    return SYN_OK;
}

int syn_features_batch(syn_engine* h, const uint64_t* my_bb, const uint64_t* op_bb, int n, float* out) {
    if (!h) return SYN_ERR_INVALID_ARGUMENT;
    if (n < 0 || (n > 0 && (!my_bb || !op_bb || !out))) return fail(h, SYN_ERR_INVALID_ARGUMENT, "bad arguments");
    if (n == 0) return SYN_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    size_t nb = (size_t)n;
    int rc = ensure_scratch(h, nb * (16 + 252) + 256);
    if (rc != SYN_OK) return rc;
    uint64_t* d_my = reinterpret_cast<uint64_t*>(h->d_scratch);
    uint64_t* d_op = d_my + nb;
    float* d_out = reinterpret_cast<float*>(d_op + nb);
    HIP_TRY(h, hipMemcpyAsync(d_my, my_bb, nb * 8, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipMemcpyAsync(d_op, op_bb, nb * 8, hipMemcpyHostToDevice, h->stream));
    size_t total = nb * 63;
    int grid = (int)((total + 255) / 256);
    if (grid > 2048) grid = 2048;
    HIP_TRY(h, hipEventRecord(h->ev0, h->stream));
    if (n <= (1 << 25)) {
        grid = (int)((total / 4 + 256) / 256);
        if (grid > 16 * h->num_cus) grid = 16 * h->num_cus;
        hipLaunchKernelGGL(features4_kernel, dim3(grid), dim3(256), 0, h->stream,   // four features per thread, 16-byte stores
                           reinterpret_cast<const unsigned long long*>(d_my),
                           reinterpret_cast<const unsigned long long*>(d_op), n, d_out);
    } else {
        hipLaunchKernelGGL(features_kernel, dim3(grid), dim3(256), 0, h->stream,
                           reinterpret_cast<const unsigned long long*>(d_my),
                           reinterpret_cast<const unsigned long long*>(d_op), n, d_out);
    }
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipEventRecord(h->ev1, h->stream));
    HIP_TRY(h, hipMemcpyAsync(out, d_out, total * 4, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    HIP_TRY(h, hipEventElapsedTime(&h->last_kernel_ms, h->ev0, h->ev1));
    h->last_launches = 1;
    return SYN_OK;
}

int syn_linear_forward(syn_engine* h, int I, int O, const float* W, const float* b, const float* x, int batch,
                       float* y, int relu) {
    if (!h) return SYN_ERR_INVALID_ARGUMENT;
    if (I < 1 || O < 1 || batch < 0 || !W || !b || (batch > 0 && (!x || !y)))
        return fail(h, SYN_ERR_INVALID_ARGUMENT, "bad arguments to syn_linear_forward");
    if (batch == 0) return SYN_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    size_t nW = (size_t)I * O, nx = (size_t)batch * I, ny = (size_t)batch * O;
    int rc = ensure_scratch(h, (nW + O + nx + ny) * 4 + 256);
    if (rc != SYN_OK) return rc;
    float* dW = static_cast<float*>(h->d_scratch);
    float* db = dW + nW;
    float* dx = db + O;
    float* dy = dx + nx;
    HIP_TRY(h, hipMemcpyAsync(dW, W, nW * 4, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipMemcpyAsync(db, b, (size_t)O * 4, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipMemcpyAsync(dx, x, nx * 4, hipMemcpyHostToDevice, h->stream));
    int grid = (int)((ny + 255) / 256);
    if (grid > 2048) grid = 2048;
    HIP_TRY(h, hipEventRecord(h->ev0, h->stream));
    if (linear_tiled_lds_bytes(I, O) + 16 <= 64 * 1024 && batch >= LIN_SB) {
        // weights and a 64-sample input tile in LDS, 8 samples per thread (layer_kernels.cuh): VALU-bound, as slimnn's two-rounding
        // multiply-add demands
        int g2 = (batch + LIN_SB - 1) / LIN_SB;
        if (g2 > 4 * h->num_cus) g2 = 4 * h->num_cus;
        hipLaunchKernelGGL(linear_tiled_kernel, dim3(g2), dim3(256), linear_tiled_lds_bytes(I, O) + 16, h->stream, I, O, dW, db, dx,
                           batch, dy, relu);
    } else if (nW * 4 <= 64 * 1024) {
        // weights in LDS, transposed (the usual case: every layer of Connect4Net is <= 48 KB); few, long-lived workgroups so
        // that the staging is amortised
        if (grid > 4 * h->num_cus) grid = 4 * h->num_cus;
        hipLaunchKernelGGL(linear_kernel_lds, dim3(grid), dim3(256), nW * 4, h->stream, I, O, dW, db, dx, batch, dy, relu);
    } else {
        hipLaunchKernelGGL(linear_kernel, dim3(grid), dim3(256), 0, h->stream, I, O, dW, db, dx, batch, dy, relu);
    }
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipEventRecord(h->ev1, h->stream));
    HIP_TRY(h, hipMemcpyAsync(y, dy, ny * 4, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    HIP_TRY(h, hipEventElapsedTime(&h->last_kernel_ms, h->ev0, h->ev1));
    h->last_launches = 1;
    return SYN_OK;
}

int syn_conv2d_forward(syn_engine* h, int CIN, int COUT, int K, int RP, int CP, int S, int H_IN, int W_IN, int H_OUT,
                       int W_OUT, const float* W, const float* b, const float* x, int batch, float* y, int relu) {
    if (!h) return SYN_ERR_INVALID_ARGUMENT;
    if (CIN < 1 || COUT < 1 || K < 1 || RP < 0 || CP < 0 || S < 1 || H_IN < 1 || W_IN < 1 || batch < 0 || !W || !b ||
        (batch > 0 && (!x || !y)))
        return fail(h, SYN_ERR_INVALID_ARGUMENT, "bad arguments to syn_conv2d_forward");
    // slimnn asserts these (conv.rs:50-51)
    if (W_IN + 2 * CP < K || H_IN + 2 * RP < K || W_OUT != ((W_IN + 2 * CP - K) / S) + 1 ||
        H_OUT != ((H_IN + 2 * RP - K) / S) + 1)
        return fail(h, SYN_ERR_INVALID_ARGUMENT, "output dims must be ((IN + 2*PAD - K) / STRIDE) + 1");
    if (batch == 0) return SYN_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    size_t nW = (size_t)COUT * CIN * K * K, nx = (size_t)batch * CIN * H_IN * W_IN,
           ny = (size_t)batch * COUT * H_OUT * W_OUT;
    int rc = ensure_scratch(h, (nW + COUT + nx + ny) * 4 + 256);
    if (rc != SYN_OK) return rc;
    float* dW = static_cast<float*>(h->d_scratch);
    float* db = dW + nW;
    float* dx = db + COUT;
    float* dy = dx + nx;
    HIP_TRY(h, hipMemcpyAsync(dW, W, nW * 4, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipMemcpyAsync(db, b, (size_t)COUT * 4, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipMemcpyAsync(dx, x, nx * 4, hipMemcpyHostToDevice, h->stream));
    int grid = (int)((ny + 255) / 256);
    if (grid > 2048) grid = 2048;
    HIP_TRY(h, hipEventRecord(h->ev0, h->stream));
    {
        // input planes of SB samples + the weights in LDS (layer_kernels.cuh) when they fit 64 KB, else element-per-thread from global
        const size_t per_in = (size_t)CIN * H_IN * W_IN;
        size_t sb = (60 * 1024 - nW * 4) / (per_in * 4);
        if (nW * 4 < 48 * 1024 && sb >= 4) {
            if (sb > 64) sb = 64;
            int g2 = (int)(((size_t)batch + sb - 1) / sb);
            if (g2 > 8 * h->num_cus) g2 = 8 * h->num_cus;
            hipLaunchKernelGGL(conv2d_tiled_kernel, dim3(g2), dim3(256), (nW + sb * per_in) * 4, h->stream, CIN, COUT, K, RP, CP, S,
                               H_IN, W_IN, H_OUT, W_OUT, (int)sb, dW, db, dx, batch, dy, relu);
        } else {
            hipLaunchKernelGGL(conv2d_kernel, dim3(grid), dim3(256), 0, h->stream, CIN, COUT, K, RP, CP, S, H_IN, W_IN, H_OUT,
                               W_OUT, dW, db, dx, batch, dy, relu);
        }
    }
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipEventRecord(h->ev1, h->stream));
    HIP_TRY(h, hipMemcpyAsync(y, dy, ny * 4, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    HIP_TRY(h, hipEventElapsedTime(&h->last_kernel_ms, h->ev0, h->ev1));
    h->last_launches = 1;
    return SYN_OK;
}

// A searchable Connect4 position (connect4.rs:3-13): disjoint bitboards inside the 63 cells, every column filled
// from the bottom without holes, at least one free column. (The reference would panic in best_action().unwrap() on a
// root without legal moves, mcts.rs:293.)
static bool valid_root(uint64_t my, uint64_t op) {
    if ((my & op) != 0 || ((my | op) >> 63) != 0) return false;
    uint64_t occ = my | op;
    bool any_free = false;
    for (int c = 0; c < 9; c++) {
        unsigned col = (unsigned)((occ >> (7 * c)) & 0x7F);
        if ((col & (col + 1)) != 0) return false;  // must be 0b0..01..1
        any_free |= col != 0x7F;
    }
    return any_free;
}

static int common_params(syn_engine* h, EngineParams& P, int explores, bool need_weights = true) {
    if (need_weights) {
        int rc = require_weights(h);
        if (rc == SYN_OK) rc = require_f16x2_image(h);
        if (rc != SYN_OK) return rc;
    }
    if (explores < 0) return fail(h, SYN_ERR_INVALID_ARGUMENT, "explores must be >= 0");
    if (explores > h->max_explores)
        return fail(h, SYN_ERR_CAPACITY, "explores %d exceeds the engine's max_explores %d", explores, h->max_explores);
    std::memset(&P, 0, sizeof(P));
    P.wimg = h->net.image();
    P.stat = h->d_stat;
    P.edge = h->d_edge;
    P.cap = h->cap;
    P.job_next = h->d_job_next;
    P.error = h->d_job_next + 8;  // same 64-byte block, zeroed before every launch
    P.path = nullptr;
    P.lane_thresh = 48;
    P.cache = h->d_cache;
    P.cache_shift = (uint32_t)(64 - h->cache_log2);
    P.cache_stats = h->d_cache_stats;
    P.counters = h->d_counters;
    return SYN_OK;
}

// a search or self-play call whose configuration or network lives in the lane-per-tree kernels only (require_lane_cap)
static int check_lane_only(syn_engine* h, const DevMctsCfg& m) {
    if (m.fpu == 2) return require_lane_cap(h, "Fpu::Func");
    if (m.noise == 2) return require_lane_cap(h, "PolicyNoise::Dirichlet");
    return require_lane_cap_of_network(h, h->net.kind);
}

static int mcts_search_impl(syn_engine* h, const syn_mcts_config* cfg, const uint64_t* my_bb, const uint64_t* op_bb, int n,
                            int explores, int action_selection, syn_search_result* results, bool rollout, uint64_t seed) {
    if (!h) return SYN_ERR_INVALID_ARGUMENT;
    if (n < 0 || (n > 0 && (!my_bb || !op_bb || !results)))
        return fail(h, SYN_ERR_INVALID_ARGUMENT, "bad arguments to syn_mcts_search");
    if (action_selection != SYN_ACTION_Q && action_selection != SYN_ACTION_NUM_VISITS)
        return fail(h, SYN_ERR_INVALID_ARGUMENT, "unknown action selection %d", action_selection);
    EngineParams P;
    int rc = common_params(h, P, explores, /*need_weights=*/!rollout);
    if (rc != SYN_OK) return rc;
    rc = convert_mcts(h, cfg, P.mcts);
    if (rc != SYN_OK) return rc;
    if (!rollout && (rc = check_lane_only(h, P.mcts)) != SYN_OK) return rc;
    if (n == 0) return SYN_OK;
    for (int i = 0; i < n; i++)
        if (!valid_root(my_bb[i], op_bb[i]))
            return fail(h, SYN_ERR_INVALID_ARGUMENT, "root %d is not a searchable Connect4 position "
                        "(overlapping / floating stones, bit 63 set, or no free column)", i);
    HIP_TRY(h, hipSetDevice(h->device));
    size_t nb = (size_t)n;
    rc = ensure_scratch(h, nb * (16 + sizeof(DevSearchResult)) + 256);
    if (rc != SYN_OK) return rc;
    unsigned long long* d_my = static_cast<unsigned long long*>(h->d_scratch);
    unsigned long long* d_op = d_my + nb;
    DevSearchResult* d_res = reinterpret_cast<DevSearchResult*>(d_op + nb);
    CallScope scope(h, n);
    HIP_TRY(h, hipMemcpyAsync(d_my, my_bb, nb * 8, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipMemcpyAsync(d_op, op_bb, nb * 8, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipMemsetAsync(h->d_job_next, 0, 64, h->stream));
    HIP_TRY(h, scope.armed());
    HIP_TRY(h, hipMemsetAsync(h->d_cache_stats, 0, 16, h->stream));
    // a root that syn_cancel kept from being searched reads as all zeros (num_nodes == 0: a searched root has at least its own node)
    HIP_TRY(h, hipMemsetAsync(d_res, 0, nb * sizeof(DevSearchResult), h->stream));
    P.roll.num_explores = explores;
    P.n_jobs = n;
    P.in_my = d_my;
    P.in_op = d_op;
    P.results = d_res;
    P.action_selection = action_selection;
    HIP_TRY(h, hipEventRecord(h->ev0, h->stream));
    P.base_seed = seed;
    P.first_game = 0;
    if (int rc = rollout ? launch_planned(h, plan_rollout_search(h->slots, n, h->cap), P) : launch_engine(h, P, n, MODE_SEARCH, false, false))
        return rc;
    HIP_TRY(h, hipEventRecord(h->ev1, h->stream));
    HIP_TRY(h, hipMemcpyAsync(results, d_res, nb * sizeof(DevSearchResult), hipMemcpyDeviceToHost, h->stream));
    int kerr = 0;
    unsigned long long cstats[2] = {0, 0};
    HIP_TRY(h, hipMemcpyAsync(&kerr, h->d_job_next + 8, 4, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipMemcpyAsync(cstats, h->d_cache_stats, 16, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    h->last_cache_hits = cstats[0];
    h->last_cache_misses = cstats[1];
    if (const int rc = fail_search_error(h, kerr)) return rc;
    HIP_TRY(h, hipEventElapsedTime(&h->last_kernel_ms, h->ev0, h->ev1));
    h->last_launches = 1;
    if (scope.cancelled()) {
        int missing = 0;
        for (int i = 0; i < n; i++) missing += results[i].num_nodes == 0u ? 1 : 0;
        if (missing)
            return fail(h, SYN_ERR_CANCELLED, "cancelled by syn_cancel: %d of %d roots were not searched (their results are all zero)",
                        missing, n);
    }
    return SYN_OK;
}

int syn_mcts_search(syn_engine* h, const syn_mcts_config* cfg, const uint64_t* my_bb, const uint64_t* op_bb, int n,
                    int explores, int action_selection, syn_search_result* results) {
    return mcts_search_impl(h, cfg, my_bb, op_bb, n, explores, action_selection, results, false, 0);
}

int syn_mcts_search_rollout(syn_engine* h, const syn_mcts_config* cfg, uint64_t seed, const uint64_t* my_bb,
                            const uint64_t* op_bb, int n, int explores, int action_selection, syn_search_result* results) {
    return mcts_search_impl(h, cfg, my_bb, op_bb, n, explores, action_selection, results, true, seed);
}

// ------------------------------------------------------------------------------------------------ the evaluator's baseline
// FrozenMCTS over RolloutPolicy (frozen_kernel.cuh). The baseline's trees live in the engine's node pool, re-partitioned for a call:
// every tree gets the record capacity the largest search of the call can need (1 + 9 nodes per visit), and the pool holds as many
// trees at once as fit. syn_frozen_search_rollout and a match's baseline sides (syn_match_run_sides) share the partition, the checks
// of the configuration and the launch.
struct FrozenPartition {
    size_t nodes_per_tree = 0;   // record capacity of one tree
    size_t lanes_max = 0;        // trees the pool holds at that capacity
};
static size_t frozen_worst_records(int explores) { return 1 + 9 * ((size_t)explores + 1); }
static int frozen_partition(syn_engine* h, size_t max_need, FrozenPartition& part) {
    const size_t nodes_per_tree = (max_need + 7) & ~(size_t)7;
    const size_t pool_records = (size_t)h->pool_slots * h->cap * 2;  // 16-byte records in the 32-byte-per-node pool
    if (max_need > 0x1FFFFFu || nodes_per_tree > pool_records)
        return fail(h, SYN_ERR_CAPACITY, "a baseline search of %zu explores needs up to %zu node records; the engine's pool holds %zu "
                    "and a tree at most 2,097,151", (max_need - 1) / 9 - 1, max_need, pool_records);
    part.nodes_per_tree = nodes_per_tree;
    part.lanes_max = pool_records / nodes_per_tree;
    return SYN_OK;
}
// the baseline panics on anything else (evaluator.rs:418-421, 429-436)
static int check_frozen_config(syn_engine* h, const syn_mcts_config* cfg) {
    if (cfg->exploration != SYN_EXPLORATION_UCT)
        return fail(h, SYN_ERR_UNSUPPORTED, "FrozenMCTS supports Exploration::Uct only (evaluator.rs:429-436)");
    if (cfg->fpu != SYN_FPU_CONST)
        return fail(h, SYN_ERR_UNSUPPORTED, "FrozenMCTS supports Fpu::Const only (evaluator.rs:418-421)");
    return SYN_OK;
}
// One launch over P.n_roots roots: the caller has filled the roots, seeds, stream positions, explores, results and n_roots (device
// arrays); the pool, the partition, the descent logs (grown here), the configuration and the error word are filled in.
static size_t frozen_lanes(const FrozenPartition& part, int n_roots) {
    return part.lanes_max < (size_t)n_roots ? part.lanes_max : (size_t)n_roots;
}
// the descent logs of a launch over n_roots roots, grown before the call's first enqueue (the buffer never shrinks)
static int ensure_frozen_path(syn_engine* h, const FrozenPartition& part, int n_roots) {
    const size_t grid = (frozen_lanes(part, n_roots) + 63) / 64;
    HIP_TRY(h, ensure_device_buffer(h->d_path, h->path_bytes, grid * 4096 * sizeof(uint32_t)));
    return SYN_OK;
}
static int launch_frozen(syn_engine* h, const FrozenPartition& part, const syn_mcts_config* cfg, int action_selection, FrozenParams P) {
    const size_t n_lanes = frozen_lanes(part, P.n_roots);
    const int grid = (int)((n_lanes + 63) / 64);  // one wave per workgroup
    if (const int rc = ensure_frozen_path(h, part, P.n_roots)) return rc;
    P.pool = reinterpret_cast<uint4*>(h->d_stat);
    P.nodes_per_tree = part.nodes_per_tree;
    P.path = reinterpret_cast<uint32_t*>(h->d_path);
    P.n_lanes = (int)n_lanes;
    P.c = cfg->c;
    P.fpu_value = cfg->fpu_value;
    P.solve = cfg->solve ? 1 : 0;
    P.action_selection = action_selection;
    P.error = h->d_job_next + 8;
    hipLaunchKernelGGL(frozen_rollout_kernel, dim3(grid), dim3(64), 0, h->stream, P);
    HIP_TRY(h, hipGetLastError());
    h->last_shape = 5; h->last_grid = grid; h->last_threads = 64;
    return SYN_OK;
}

// ------------------------------------------------------------------------------------------------ device-resident games
// syn_match_run / syn_match_run_sides / syn_tournament_run (match_kernels.cuh, tournament_kernels.cuh): ONE loop, run_games, in which
// every game of a schedule between K players is searched, stepped and retired on the device. A match is the schedule of two players
// with player 0 first in every game. The live games are kept grouped by mover; per ply every non-empty group gets its player's search
// over its range of the arrays — one MODE_SEARCH launch with the player's image in the player's arithmetic, or one
// frozen_rollout_kernel launch on the re-partitioned pool for a baseline player — and the advance kernel, then one stable regroup by
// next mover (count, scan, scatter), and the host reads the groups' starts and the error word back: K + 2 words. All games of a match
// share their mover, so its ply has one group: four launches. Nothing is uploaded inside the loop; the outputs come back once, after
// the last ply. Both kinds of search use the engine's node pool and alternate on one stream: nothing runs concurrently. The job
// counter is reset before every search launch; the search kernels' error word sits in the same 64-byte block and is reset once per ply
// only, so what the first group raised is still there after the last.
// The searches never touch the policy cache (P.cache = nullptr): its entries are keyed by position alone and belong to the engine's own
// network, so a call neither reads another network's evaluations nor leaves its own behind.

// c4::won (device_common.cuh, device code) for the host's check of the start positions: the same four anchored lines, its masks
static bool host_won(uint64_t bb) {
    const uint64_t d1 = bb & (bb >> 6) & (bb >> 12) & (bb >> 18) & c4::D1_MASK;
    const uint64_t d2 = bb & (bb >> 8) & (bb >> 16) & (bb >> 24) & c4::D2_MASK;
    const uint64_t hz = bb & (bb >> 7) & (bb >> 14) & (bb >> 21) & c4::H_MASK;
    const uint64_t vt = bb & (bb >> 1) & (bb >> 2) & (bb >> 3) & c4::V_MASK;
    return (d1 | d2 | hz | vt) != 0;
}
// a game's start: a position the first search can take as its root, and not a finished game
static int check_start(syn_engine* h, int g, uint64_t my, uint64_t op) {
    if (!valid_root(my, op))
        return fail(h, SYN_ERR_INVALID_ARGUMENT, "start %d is not a searchable Connect4 position "
                    "(overlapping / floating stones, bit 63 set, or no free column)", g);
    if (host_won(my) || host_won(op))
        return fail(h, SYN_ERR_INVALID_ARGUMENT, "start %d is a finished game: one side has four in a row", g);
    return SYN_OK;
}

// a network side of a match: its configuration must be one whose search is a function of the root alone
static int check_match_player(syn_engine* h, const char* who, const syn_match_player* p, DevMctsCfg& m) {
    if (p->action != SYN_ACTION_Q && p->action != SYN_ACTION_NUM_VISITS)
        return fail(h, SYN_ERR_INVALID_ARGUMENT, "syn_match_run: the %s player's action selection %d is unknown", who, p->action);
    if (p->mcts_cfg.fpu == SYN_FPU_NORMAL || p->mcts_cfg.fpu == SYN_FPU_FUNC || p->mcts_cfg.root_policy_noise == SYN_NOISE_DIRICHLET)
        return fail(h, SYN_ERR_UNSUPPORTED, "syn_match_run: the %s player draws random numbers (SYN_FPU_NORMAL / SYN_FPU_FUNC / "
                                            "SYN_NOISE_DIRICHLET); their streams are keyed by job index, which changes as games end: "
                                            "a match takes deterministic players only", who);
    if (p->explores < 0) return fail(h, SYN_ERR_INVALID_ARGUMENT, "syn_match_run: the %s player's explores must be >= 0", who);
    if (p->explores > h->max_explores)
        return fail(h, SYN_ERR_CAPACITY, "syn_match_run: the %s player's explores %d exceed the engine's max_explores %d", who,
                    p->explores, h->max_explores);
    return convert_mcts(h, &p->mcts_cfg, m);
}

// One player as the loop uses it: a network side's MODE_SEARCH parameters, its blob and the arithmetic of its image, or a baseline
// side's partition of the pool.
struct MatchSide {
    bool baseline = false;
    int arith = PLAN_ARITH_ENGINE;   // network: the image's arithmetic, carried to launch_engine with every ply
    bool f16 = false;                // ... resolved against the engine's
    EngineParams P;                  // network
    FrozenPartition part;            // baseline
    const syn_match_player* player = nullptr;
    const float* blob = nullptr;     // network
};

// ---- everything that can refuse a side, before anything of the engine or the device changes
static int check_match_side(syn_engine* h, const char* who, const syn_match_side* s, bool have_seeds, MatchSide& out) {
    if (!s) return fail(h, SYN_ERR_INVALID_ARGUMENT, "syn_match_run: the %s player is NULL", who);
    out.player = &s->player;
    if (s->kind == SYN_MATCH_SIDE_BASELINE) {
        out.baseline = true;
        const syn_match_player& p = s->player;
        if (p.action != SYN_ACTION_Q && p.action != SYN_ACTION_NUM_VISITS)
            return fail(h, SYN_ERR_INVALID_ARGUMENT, "syn_match_run: the %s player's action selection %d is unknown", who, p.action);
        if (const int rc = check_frozen_config(h, &p.mcts_cfg)) return rc;
        if (p.explores < 0) return fail(h, SYN_ERR_INVALID_ARGUMENT, "syn_match_run: the %s player's explores must be >= 0", who);
        if (!have_seeds)
            return fail(h, SYN_ERR_INVALID_ARGUMENT, "syn_match_run: the %s player is a baseline side, whose playouts need seeds: seeds is NULL", who);
        return frozen_partition(h, frozen_worst_records(p.explores), out.part);
    }
    if (s->kind != SYN_MATCH_SIDE_NETWORK)
        return fail(h, SYN_ERR_INVALID_ARGUMENT, "syn_match_run: the %s side's kind %d is unknown", who, s->kind);
    if (s->arithmetic != SYN_MATCH_ARITH_ENGINE && s->arithmetic != SYN_MATCH_ARITH_F32 && s->arithmetic != SYN_MATCH_ARITH_F16X2)
        return fail(h, SYN_ERR_INVALID_ARGUMENT, "syn_match_run: the %s side's arithmetic %d is unknown", who, s->arithmetic);
    out.blob = s->blob;
    static_assert(SYN_MATCH_ARITH_ENGINE == PLAN_ARITH_ENGINE && SYN_MATCH_ARITH_F32 == PLAN_ARITH_F32 && SYN_MATCH_ARITH_F16X2 == PLAN_ARITH_F16X2,
                  "launch_plan.hpp restates the header's SYN_MATCH_ARITH_*");
    out.arith = s->arithmetic;
    out.f16 = plan_call_f16(h->net.f16x2(), s->arithmetic);
    DevMctsCfg m{};
    int rc = check_match_player(h, who, &s->player, m);
    if (rc == SYN_OK) rc = check_blob(h, h->net.kind, s->blob, s->n_floats);
    if (rc == SYN_OK && out.f16) rc = require_lane_cap(h, "the f16x2 arithmetic");
    if (rc == SYN_OK) rc = common_params(h, out.P, s->player.explores, /*need_weights=*/false);
    if (rc != SYN_OK) return rc;
    out.P.mcts = m;
    out.P.cache = nullptr;
    out.P.roll.num_explores = s->player.explores;
    out.P.action_selection = s->player.action;
    return SYN_OK;
}

struct RegroupBuffers {   // device
    unsigned* counts;   // [n_keys + 1][n_blocks]
    unsigned* base;     // their exclusive sum
    void* temp;         // the scan's temporary storage
    size_t temp_bytes;
};
static size_t regroup_cells(size_t n, int n_keys) { return (size_t)(n_keys + 1) * ((n + TOURNAMENT_BLOCK - 1) / TOURNAMENT_BLOCK); }
// count, scan, scatter over key[0 .. n_live) on the engine's stream; seg_out holds n_keys + 2 words
static int enqueue_regroup(syn_engine* h, const int* key, int n_live, int n_keys, const RegroupBuffers& B, const MatchLive& from,
                           const MatchLive& to, const int* search_error, const int* stream_error, int* seg_out) {
    const dim3 grid((unsigned)((n_live + TOURNAMENT_BLOCK - 1) / TOURNAMENT_BLOCK)), block(TOURNAMENT_BLOCK);
    size_t temp_bytes = B.temp_bytes;
    hipLaunchKernelGGL(tournament_count_kernel, grid, block, 0, h->stream, key, n_live, n_keys, B.counts);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipcub::DeviceScan::ExclusiveSum(B.temp, temp_bytes, B.counts, B.base, (int)regroup_cells((size_t)n_live, n_keys), h->stream));
    hipLaunchKernelGGL(tournament_scatter_kernel, grid, block, 0, h->stream, key, n_live, n_keys, B.base, from, to, search_error,
                       stream_error, seg_out);
    HIP_TRY(h, hipGetLastError());
    return SYN_OK;
}

struct GamesLayout {   // byte offsets into syn_engine::Games::d_buf
    size_t my[2], op[2], id[2], seed[2], word[2];   // the live games, two sets: a ply's regroup reads one and writes the other
    size_t key, counts, base, scan;                 // the regroup's
    size_t results;                                 // GAMES_RESULT_STRIDE bytes per live job: group [lo, hi) owns the bytes from lo * stride
    size_t explores;                                // baseline players' explores per root: player p's run starts at its own offset
    size_t first, second;                           // the schedule, per game
    size_t rewards, plies, moves, final_bb, rng_words;   // MatchOut, per game
    size_t seg;                                     // [0 .. K] group starts, [K + 1] error word, [K + 2] the advance kernels' stream-position flag
    size_t row_ply;                                 // a recording call's [n][63] plies of its rows (record_kernels.cuh); no bytes otherwise
    size_t total;
};
constexpr size_t GAMES_RESULT_STRIDE =
    ((sizeof(DevSearchResult) > sizeof(FrozenResult) ? sizeof(DevSearchResult) : sizeof(FrozenResult)) + 15) & ~(size_t)15;
static GamesLayout games_layout(size_t n, int n_players, size_t cells, size_t scan_bytes, size_t n_explores, bool recording) {
    GamesLayout L{};
    Carve c;
    for (int k = 0; k < 2; k++) {
        L.my[k] = c.take(n * 8); L.op[k] = c.take(n * 8); L.id[k] = c.take(n * 4); L.seed[k] = c.take(n * 8); L.word[k] = c.take(n * 8);
    }
    L.key = c.take(n * 4); L.counts = c.take(cells * 4); L.base = c.take(cells * 4); L.scan = c.take(scan_bytes);
    L.results = c.take(n * GAMES_RESULT_STRIDE);
    L.explores = c.take(n_explores * 4);
    L.first = c.take(n * 4); L.second = c.take(n * 4);
    L.rewards = c.take(n * 4); L.plies = c.take(n * 4); L.moves = c.take(n * MATCH_T); L.final_bb = c.take(n * 16); L.rng_words = c.take(n * 8);
    L.seg = c.take((size_t)(n_players + 3) * 4);
    L.row_ply = c.take(recording ? n * MATCH_T : 0);
    L.total = c.at;
    return L;
}

// What makes a call of the loop a recording one (syn_games_run_recorded; record_kernels.cuh): the rules of run_game's tail, which
// players' plies become rows, the value target, and where the rows go on the host.
struct RecordCall {
    RecordRules rules;
    uint64_t mask;
    int value_target;
    float vt_p, vt_from, vt_to;
    const syn_record_outputs* out;   // may be NULL
};
static int ensure_outputs(syn_engine* h, int n_games);

// The loop. S: the call's K checked players; first / second: the schedule (host). `noun` names the call in messages ("match",
// "tournament"). Everything that can still refuse the call — the schedule, the starts, an image without a plan — comes before anything
// of the engine or the device changes; the entry point has selected the engine's device. `rec` (may be NULL) makes the call a recording
// one: record_advance_kernel takes the advance kernel's place, the rows go to the engine's self-play output buffers, and
// record_finish_kernel runs once after the last ply. With rec == NULL the function enqueues exactly what it enqueued before there was one.
static int run_games(syn_engine* h, MatchSide* S, int K, const int32_t* first, const int32_t* second, const uint64_t* start_my,
                     const uint64_t* start_op, const uint64_t* seeds, int n_games, float* rewards, int32_t* plies, uint8_t* moves,
                     uint64_t* final_bb, uint64_t* rng_words, const char* noun, const RecordCall* rec = nullptr) {
    const std::string fn_name = rec ? std::string("syn_games_run_recorded") : "syn_" + std::string(noun) + "_run";
    const char* const fn = fn_name.c_str();
    for (int g = 0; g < n_games; g++) {
        if (first[g] < 0 || first[g] >= K || second[g] < 0 || second[g] >= K)
            return fail(h, SYN_ERR_INVALID_ARGUMENT, "%s: game %d names players %d and %d; there are %d", fn, g, first[g],
                        second[g], K);
        if (const int rc = check_start(h, g, start_my[g], start_op[g])) return rc;
    }
    std::vector<HostImage> im((size_t)K);
    for (int p = 0; p < K; p++) {
        if (S[p].baseline) continue;
        const int rc = build_host_image(h, h->net.kind, S[p].blob, S[p].f16, im[p]);   // (f16x2: SYN_ERR_UNSUPPORTED for a blob without a plan)
        if (rc != SYN_OK) return rc;
    }
    if (n_games == 0) return SYN_OK;
    // ---- the schedule: how many games each player appears in, and the games in their first ply's order (grouped by first mover)
    const size_t n = (size_t)n_games;
    std::vector<int> appears((size_t)K, 0), seg((size_t)K + 1, 0);
    for (size_t g = 0; g < n; g++) {
        appears[first[g]]++;
        if (second[g] != first[g]) appears[second[g]]++;
        seg[first[g] + 1]++;
    }
    for (int p = 0; p < K; p++) seg[p + 1] += seg[p];
    std::vector<int> order(n);
    {
        std::vector<int> at(seg.begin(), seg.end() - 1);
        for (size_t g = 0; g < n; g++) order[at[first[g]]++] = (int)g;
    }
    std::vector<size_t> expl_at((size_t)K, 0);
    size_t n_explores = 0;
    for (int p = 0; p < K; p++)
        if (S[p].baseline) { expl_at[p] = n_explores; n_explores += (size_t)appears[p]; }
    // ---- device memory
    const size_t cells = regroup_cells(n, K);
    size_t scan_bytes = 0;
    HIP_TRY(h, hipcub::DeviceScan::ExclusiveSum(nullptr, scan_bytes, (const unsigned*)nullptr, (unsigned*)nullptr, (int)cells, h->stream));
    const GamesLayout L = games_layout(n, K, cells, scan_bytes, n_explores, rec != nullptr);
    for (int p = 0; p < K; p++)
        if (!S[p].baseline && !h->games.d_img[p]) HIP_TRY(h, hipMalloc(&h->games.d_img[p], NET_IMAGE_MAX_BYTES));
    HIP_TRY(h, ensure_device_buffer(h->games.d_buf, h->games.buf_bytes, L.total));
    for (int p = 0; p < K; p++)
        if (S[p].baseline && appears[p] > 0)
            if (const int rc = ensure_frozen_path(h, S[p].part, appears[p])) return rc;
    if (rec)
        if (const int rc = ensure_outputs(h, n_games)) return rc;
    unsigned char* const base = h->games.d_buf;
    const auto u64_at = [base](size_t o) { return reinterpret_cast<unsigned long long*>(base + o); };
    MatchLive live_set[2];
    for (int k = 0; k < 2; k++)
        live_set[k] = MatchLive{u64_at(L.my[k]), u64_at(L.op[k]), reinterpret_cast<int*>(base + L.id[k]), u64_at(L.seed[k]), u64_at(L.word[k])};
    int* const d_key = reinterpret_cast<int*>(base + L.key);
    const RegroupBuffers R{reinterpret_cast<unsigned*>(base + L.counts), reinterpret_cast<unsigned*>(base + L.base), base + L.scan, scan_bytes};
    unsigned char* const d_res = base + L.results;
    int* const d_expl = reinterpret_cast<int*>(base + L.explores);
    int* const d_first = reinterpret_cast<int*>(base + L.first);
    int* const d_second = reinterpret_cast<int*>(base + L.second);
    int* const d_seg = reinterpret_cast<int*>(base + L.seg);
    int* const d_stream_error = d_seg + K + 2;
    MatchOut out;
    out.rewards = reinterpret_cast<float*>(base + L.rewards);
    out.plies = reinterpret_cast<int*>(base + L.plies);
    out.moves = base + L.moves;
    out.final_bb = u64_at(L.final_bb);
    out.rng_words = u64_at(L.rng_words);
    RecordOut rows{};
    if (rec) {
        rows.rows = h->d_plies;
        rows.states_bb = reinterpret_cast<unsigned long long*>(h->d_states);
        rows.pis = h->d_pis;
        rows.vs = h->d_vs;
        rows.actions = h->d_actions;
        rows.root_nodes = h->d_root_nodes;
        rows.final_kind = h->d_final;
        rows.row_ply = base + L.row_ply;
    }

    CallScope scope(h, n_games);
    std::vector<unsigned long long> s_my(n), s_op(n), s_seed(n, 0ull);
    for (size_t i = 0; i < n; i++) {
        s_my[i] = start_my[order[i]];
        s_op[i] = start_op[order[i]];
        if (seeds) s_seed[i] = seeds[order[i]];
    }
    std::vector<int> expl(n_explores);
    for (int p = 0; p < K; p++) {
        if (S[p].baseline) {
            std::fill(expl.begin() + (ptrdiff_t)expl_at[p], expl.begin() + (ptrdiff_t)(expl_at[p] + (size_t)appears[p]), S[p].player->explores);
            continue;
        }
        const int rc = enqueue_image_upload(h, im[p], h->games.d_img[p]);
        if (rc != SYN_OK) return rc;
        S[p].P.wimg = static_cast<const float*>(h->games.d_img[p]);
    }
    if (n_explores) HIP_TRY(h, hipMemcpyAsync(d_expl, expl.data(), n_explores * 4, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipMemcpyAsync(live_set[0].my, s_my.data(), n * 8, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipMemcpyAsync(live_set[0].op, s_op.data(), n * 8, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipMemcpyAsync(live_set[0].id, order.data(), n * 4, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipMemcpyAsync(live_set[0].seed, s_seed.data(), n * 8, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipMemcpyAsync(d_first, first, n * 4, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipMemcpyAsync(d_second, second, n * 4, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipMemsetAsync(live_set[0].word, 0, n * 8, h->stream));   // every game's generator starts at output word 0
    HIP_TRY(h, hipMemsetAsync(base + L.rewards, 0, L.moves - L.rewards, h->stream));   // rewards and plies
    HIP_TRY(h, hipMemsetAsync(out.moves, MATCH_NO_MOVE, n * MATCH_T, h->stream));
    HIP_TRY(h, hipMemsetAsync(out.final_bb, 0, n * 16, h->stream));
    HIP_TRY(h, hipMemsetAsync(out.rng_words, 0, n * 8, h->stream));
    HIP_TRY(h, hipMemsetAsync(d_seg, 0, (size_t)(K + 3) * 4, h->stream));
    if (rec) {   // no rows yet; the slots no row reaches read as zeros
        const size_t slots = n * MATCH_T;
        HIP_TRY(h, hipMemsetAsync(rows.rows, 0, n * 4, h->stream));
        HIP_TRY(h, hipMemsetAsync(rows.states_bb, 0, slots * 16, h->stream));
        HIP_TRY(h, hipMemsetAsync(rows.pis, 0, slots * 36, h->stream));
        HIP_TRY(h, hipMemsetAsync(rows.vs, 0, slots * 12, h->stream));
        HIP_TRY(h, hipMemsetAsync(rows.actions, 0, slots, h->stream));
        HIP_TRY(h, hipMemsetAsync(rows.root_nodes, 0, slots * 4, h->stream));
        HIP_TRY(h, hipMemsetAsync(rows.final_kind, 0, n, h->stream));
        HIP_TRY(h, hipMemsetAsync(rows.row_ply, 0, slots, h->stream));
    }
    HIP_TRY(h, hipStreamSynchronize(h->stream));   // the last upload from host memory: the loop below only launches and reads K + 2 words

    float kernel_ms = 0.0f;
    int launches = 0, live = n_games, ply = 0;
    int* const h_seg = h->h_pin + 16;
    for (; live > 0 && ply < MATCH_T; ply++) {
        const int cur = ply & 1, nxt = cur ^ 1;
        const MatchLive& A = live_set[cur];
        bool any_launch = false, any_baseline = false, any_network = false;
        // (a syn_cancel's word does not survive the next reset: the loop itself stops at the first ply that ends after it)
        HIP_TRY(h, hipMemsetAsync(h->d_job_next, 0, 64, h->stream));   // the counters and, once per ply, the error word
        if (ply == 0) HIP_TRY(h, scope.armed());
        HIP_TRY(h, hipEventRecord(h->ev0, h->stream));
        for (int p = 0; p < K; p++) {
            const int lo = seg[p], cnt = seg[p + 1] - seg[p];
            if (cnt == 0) continue;
            if (any_launch) HIP_TRY(h, hipMemsetAsync(h->d_job_next, 0, 32, h->stream));   // the counters alone: the error word stays
            any_launch = true;
            const dim3 grid((unsigned)((cnt + 255) / 256)), block(256);
            unsigned char* const res = d_res + (size_t)lo * GAMES_RESULT_STRIDE;
            // a root that syn_cancel kept from being searched reads as all zeros: the advance kernel drops it
            if (S[p].baseline) {
                any_baseline = true;
                HIP_TRY(h, hipMemsetAsync(res, 0, (size_t)cnt * sizeof(FrozenResult), h->stream));
                FrozenParams F{};
                F.in_my = A.my + lo; F.in_op = A.op + lo; F.seeds = A.seed + lo; F.rng_words = A.word + lo; F.explores = d_expl + expl_at[p];
                F.n_roots = cnt;
                F.results = reinterpret_cast<FrozenResult*>(res);
                if (const int rc = launch_frozen(h, S[p].part, &S[p].player->mcts_cfg, S[p].player->action, F)) return rc;
                hipLaunchKernelGGL(tournament_advance_kernel<FrozenResult>, grid, block, 0, h->stream, reinterpret_cast<const FrozenResult*>(res),
                                   lo, cnt, ply, A.my, A.op, A.id, A.word, d_first, d_second, K, d_key, d_stream_error, out);
            } else {
                any_network = true;
                HIP_TRY(h, hipMemsetAsync(res, 0, (size_t)cnt * sizeof(DevSearchResult), h->stream));
                EngineParams Q = S[p].P;
                Q.n_jobs = cnt;
                Q.in_my = A.my + lo;
                Q.in_op = A.op + lo;
                Q.results = reinterpret_cast<DevSearchResult*>(res);
                if (const int rc = launch_engine(h, Q, cnt, MODE_SEARCH, false, false, S[p].arith)) return rc;
                if (rec)
                    hipLaunchKernelGGL(record_advance_kernel, grid, block, 0, h->stream, reinterpret_cast<const unsigned*>(res), lo, cnt, ply,
                                       (int)((rec->mask >> p) & 1ull), rec->rules, A.my, A.op, A.id, A.seed, A.word, d_first, d_second, K, d_key,
                                       d_stream_error, out, rows);
                else
                    hipLaunchKernelGGL(tournament_advance_kernel<DevSearchResult>, grid, block, 0, h->stream,
                                       reinterpret_cast<const DevSearchResult*>(res), lo, cnt, ply, A.my, A.op, A.id, A.word, d_first, d_second, K,
                                       d_key, d_stream_error, out);
            }
            HIP_TRY(h, hipGetLastError());
            launches += 2;   // the search and the advance
        }
        if (const int rc = enqueue_regroup(h, d_key, live, K, R, A, live_set[nxt], h->d_job_next + 8, d_stream_error, d_seg)) return rc;
        launches += 2;       // the count and the scatter (the scan between them is the library's)
        HIP_TRY(h, hipEventRecord(h->ev1, h->stream));
        HIP_TRY(h, hipMemcpyAsync(h_seg, d_seg, (size_t)(K + 2) * 4, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        float ms = 0.0f;
        HIP_TRY(h, hipEventElapsedTime(&ms, h->ev0, h->ev1));
        kernel_ms += ms;
        h->last_kernel_ms = kernel_ms;
        h->last_launches = launches;
        if (scope.cancelled())
            return fail(h, SYN_ERR_CANCELLED, "cancelled by syn_cancel at ply %d of the %s: the outputs are unspecified", ply, noun);
        const int err = h_seg[K + 1];
        if (err == -MATCH_ERR_STREAM)
            return fail(h, SYN_ERR_CAPACITY, "a game's rollout generator passed output word 0xC0000000 at ply %d of the %s: the "
                                             "baseline search supports no longer stream", ply, noun);
        if (err < 0 && any_baseline && !any_network) return fail(h, SYN_ERR_CAPACITY, "a baseline tree ran out of node records");
        // (both kinds of search raise 2 for a full tree: after a ply of both it may have been a baseline player's)
        if (const int rc = fail_search_error(h, -err, any_baseline ? "; or a baseline tree of the same ply ran out of node records" : "")) return rc;
        bool sane = h_seg[0] == 0 && h_seg[K] <= live;
        for (int p = 0; p < K && sane; p++) sane = h_seg[p] <= h_seg[p + 1];
        if (!sane) return fail(h, SYN_ERR_HIP, "%s: the regroup of ply %d returned group starts that are no partition of "
                                               "at most %d games", fn, ply, live);
        for (int p = 0; p <= K; p++) seg[p] = h_seg[p];
        live = seg[K];
    }
    if (live > 0) return fail(h, SYN_ERR_HIP, "%s: %d games are unfinished after %d plies", fn, live, MATCH_T);
    if (rec) {   // z, t and store_rewards over the staged q of every row
        const size_t slots = n * MATCH_T;
        HIP_TRY(h, hipEventRecord(h->ev0, h->stream));
        hipLaunchKernelGGL(record_finish_kernel, dim3((unsigned)((slots + 255) / 256)), dim3(256), 0, h->stream, n_games, out.plies,
                           rec->value_target, rec->vt_p, rec->vt_from, rec->vt_to, rows);
        HIP_TRY(h, hipGetLastError());
        HIP_TRY(h, hipEventRecord(h->ev1, h->stream));
        if (const syn_record_outputs* o = rec->out) {
            if (o->rows) HIP_TRY(h, hipMemcpyAsync(o->rows, rows.rows, n * 4, hipMemcpyDeviceToHost, h->stream));
            if (o->states_bb) HIP_TRY(h, hipMemcpyAsync(o->states_bb, rows.states_bb, slots * 16, hipMemcpyDeviceToHost, h->stream));
            if (o->pis) HIP_TRY(h, hipMemcpyAsync(o->pis, rows.pis, slots * 36, hipMemcpyDeviceToHost, h->stream));
            if (o->vs) HIP_TRY(h, hipMemcpyAsync(o->vs, rows.vs, slots * 12, hipMemcpyDeviceToHost, h->stream));
            if (o->actions) HIP_TRY(h, hipMemcpyAsync(o->actions, rows.actions, slots, hipMemcpyDeviceToHost, h->stream));
            if (o->root_nodes) HIP_TRY(h, hipMemcpyAsync(o->root_nodes, rows.root_nodes, slots * 4, hipMemcpyDeviceToHost, h->stream));
            if (o->final_kind) HIP_TRY(h, hipMemcpyAsync(o->final_kind, rows.final_kind, n, hipMemcpyDeviceToHost, h->stream));
        }
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        float ms = 0.0f;
        HIP_TRY(h, hipEventElapsedTime(&ms, h->ev0, h->ev1));
        h->last_kernel_ms = kernel_ms + ms;
        h->last_launches = launches + 1;
    }
    HIP_TRY(h, hipMemcpyAsync(rewards, out.rewards, n * 4, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipMemcpyAsync(plies, out.plies, n * 4, hipMemcpyDeviceToHost, h->stream));
    if (moves) HIP_TRY(h, hipMemcpyAsync(moves, out.moves, n * MATCH_T, hipMemcpyDeviceToHost, h->stream));
    if (final_bb) HIP_TRY(h, hipMemcpyAsync(final_bb, out.final_bb, n * 16, hipMemcpyDeviceToHost, h->stream));
    if (rng_words) HIP_TRY(h, hipMemcpyAsync(rng_words, out.rng_words, n * 8, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    h->last_cache_hits = h->last_cache_misses = 0;   // the game loop does not use the policy cache
    return SYN_OK;
}

// A match: two players, `first` moving first in every game. (n_games == 0 is answered here, once the sides have passed.)
static int match_run_impl(syn_engine* h, const syn_match_side* first, const syn_match_side* second, const uint64_t* start_my,
                          const uint64_t* start_op, const uint64_t* seeds, int n_games, float* rewards, int32_t* plies, uint8_t* moves,
                          uint64_t* final_bb, uint64_t* rng_words) {
    if (n_games < 0 || (n_games > 0 && (!start_my || !start_op || !rewards || !plies)))
        return fail(h, SYN_ERR_INVALID_ARGUMENT, "bad arguments to syn_match_run");
    MatchSide S[2];
    if (const int rc = check_match_side(h, "first", first, seeds != nullptr, S[0])) return rc;
    if (const int rc = check_match_side(h, "second", second, seeds != nullptr, S[1])) return rc;
    if (n_games == 0) return SYN_OK;
    const std::vector<int32_t> zeros((size_t)n_games, 0), ones((size_t)n_games, 1);
    return run_games(h, S, 2, zeros.data(), ones.data(), start_my, start_op, seeds, n_games, rewards, plies, moves, final_bb, rng_words, "match");
}

int syn_match_run_sides(syn_engine* h, const syn_match_side* first, const syn_match_side* second, const uint64_t* start_my,
                        const uint64_t* start_op, const uint64_t* seeds, int n_games, float* rewards, int32_t* plies, uint8_t* moves,
                        uint64_t* final_bb, uint64_t* rng_words) {
    if (!h) return SYN_ERR_INVALID_ARGUMENT;
    HIP_TRY(h, hipSetDevice(h->device));   // (selecting the device changes nothing of the engine: the refusals come first in match_run_impl)
    return match_run_impl(h, first, second, start_my, start_op, seeds, n_games, rewards, plies, moves, final_bb, rng_words);
}

// two network sides in the engine's arithmetic
int syn_match_run(syn_engine* h, const syn_match_player* first, const syn_match_player* second, const float* blob_first,
                  const float* blob_second, size_t n_floats, const uint64_t* start_my, const uint64_t* start_op, int n_games,
                  float* rewards, int32_t* plies, uint8_t* moves, uint64_t* final_bb) {
    if (!h) return SYN_ERR_INVALID_ARGUMENT;
    if (n_games < 0 || (n_games > 0 && (!start_my || !start_op || !rewards || !plies)))
        return fail(h, SYN_ERR_INVALID_ARGUMENT, "bad arguments to syn_match_run");
    const syn_match_player* const players[2] = {first, second};
    const float* const blobs[2] = {blob_first, blob_second};
    syn_match_side sides[2];
    for (int s = 0; s < 2; s++) {
        if (!players[s]) return fail(h, SYN_ERR_INVALID_ARGUMENT, "syn_match_run: the %s player is NULL", s == 0 ? "first" : "second");
        sides[s] = syn_match_side{SYN_MATCH_SIDE_NETWORK, SYN_MATCH_ARITH_ENGINE, *players[s], blobs[s], n_floats};
    }
    HIP_TRY(h, hipSetDevice(h->device));
    return match_run_impl(h, &sides[0], &sides[1], start_my, start_op, nullptr, n_games, rewards, plies, moves, final_bb, nullptr);
}

int syn_tournament_run(syn_engine* h, const syn_match_side* players, int n_players, const int32_t* first, const int32_t* second,
                       const uint64_t* start_my, const uint64_t* start_op, const uint64_t* seeds, int n_games, float* rewards,
                       int32_t* plies, uint8_t* moves, uint64_t* final_bb, uint64_t* rng_words) {
    if (!h) return SYN_ERR_INVALID_ARGUMENT;
    if (n_games < 0 || (n_games > 0 && (!first || !second || !start_my || !start_op || !rewards || !plies)))
        return fail(h, SYN_ERR_INVALID_ARGUMENT, "bad arguments to syn_tournament_run");
    if (n_players < 1 || n_players > SYN_TOURNAMENT_MAX_PLAYERS)
        return fail(h, SYN_ERR_INVALID_ARGUMENT, "syn_tournament_run: n_players %d is outside 1 .. %d", n_players, SYN_TOURNAMENT_MAX_PLAYERS);
    if (!players) return fail(h, SYN_ERR_INVALID_ARGUMENT, "syn_tournament_run: players is NULL");
    HIP_TRY(h, hipSetDevice(h->device));   // (selecting the device changes nothing of the engine)
    // ---- everything that can refuse the call, before anything of the engine or the device changes
    const int K = n_players;
    std::vector<MatchSide> S((size_t)K);
    for (int p = 0; p < K; p++) {
        char who[24];
        std::snprintf(who, sizeof(who), "tournament's #%d", p);
        if (const int rc = check_match_side(h, who, &players[p], seeds != nullptr, S[p])) return rc;
    }
    return run_games(h, S.data(), K, first, second, start_my, start_op, seeds, n_games, rewards, plies, moves, final_bb, rng_words, "tournament");
}

// Recorded games (include/synthesis_amd.h "Recorded games"): syn_tournament_run's arguments and refusals, network sides only, and the
// loop in its recording form. The rows stay in the engine's self-play output buffers: for syn_replay_append_selfplay and
// syn_selfplay_positions_device the call is a self-play launch of n_games games.
int syn_games_run_recorded(syn_engine* h, const syn_match_side* players, int n_players, const int32_t* first, const int32_t* second,
                           const uint64_t* start_my, const uint64_t* start_op, const uint64_t* seeds, int n_games,
                           const syn_record_config* rec, float* rewards, int32_t* plies, uint8_t* moves, uint64_t* final_bb,
                           uint64_t* rng_words, const syn_record_outputs* out) {
    if (!h) return SYN_ERR_INVALID_ARGUMENT;
    h->last_selfplay_games = -1;   // what a failed syn_selfplay_run leaves: nothing to compact until this call has ended without an error
    if (n_games < 0 || (n_games > 0 && (!first || !second || !start_my || !start_op || !rewards || !plies)))
        return fail(h, SYN_ERR_INVALID_ARGUMENT, "bad arguments to syn_games_run_recorded");
    if (n_players < 1 || n_players > SYN_TOURNAMENT_MAX_PLAYERS)
        return fail(h, SYN_ERR_INVALID_ARGUMENT, "syn_games_run_recorded: n_players %d is outside 1 .. %d", n_players, SYN_TOURNAMENT_MAX_PLAYERS);
    if (!players) return fail(h, SYN_ERR_INVALID_ARGUMENT, "syn_games_run_recorded: players is NULL");
    if (!rec) return fail(h, SYN_ERR_INVALID_ARGUMENT, "syn_games_run_recorded: the record configuration is NULL");
    if (rec->value_target < SYN_VALUE_Z || rec->value_target > SYN_VALUE_Q_TO_Z)
        return fail(h, SYN_ERR_INVALID_ARGUMENT, "syn_games_run_recorded: unknown value target %d", rec->value_target);
    if (rec->random_actions_until < 0 || rec->sample_actions_until < 0)
        return fail(h, SYN_ERR_INVALID_ARGUMENT, "syn_games_run_recorded: random_actions_until / sample_actions_until must be >= 0");
    if (n_players < 64 && (rec->record_mask >> n_players) != 0)
        return fail(h, SYN_ERR_INVALID_ARGUMENT, "syn_games_run_recorded: record_mask 0x%llx has a bit at or above n_players %d",
                    (unsigned long long)rec->record_mask, n_players);
    if (!seeds && (rec->random_actions_until > 0 || rec->sample_actions_until > 0))
        return fail(h, SYN_ERR_INVALID_ARGUMENT, "syn_games_run_recorded: seeds is NULL, but actions are drawn (random_actions_until %d, "
                                                 "sample_actions_until %d)", rec->random_actions_until, rec->sample_actions_until);
    HIP_TRY(h, hipSetDevice(h->device));   // (selecting the device changes nothing of the engine)
    // ---- everything that can refuse the call, before anything of the engine or the device changes
    const int K = n_players;
    std::vector<MatchSide> S((size_t)K);
    for (int p = 0; p < K; p++) {
        if (players[p].kind == SYN_MATCH_SIDE_BASELINE)
            return fail(h, SYN_ERR_UNSUPPORTED, "syn_games_run_recorded: player #%d is a baseline side, whose search record has no target_pi / "
                                                "target_q: recorded games take network sides only", p);
        char who[24];
        std::snprintf(who, sizeof(who), "recorded games' #%d", p);
        if (const int rc = check_match_side(h, who, &players[p], seeds != nullptr, S[p])) return rc;
    }
    RecordCall R{};
    R.rules.random_until = rec->random_actions_until;
    R.rules.sample_until = rec->sample_actions_until;
    R.rules.stop_when_solved = rec->stop_games_when_solved != 0;
    R.mask = rec->record_mask;
    R.value_target = rec->value_target;
    R.vt_p = rec->value_target_p;
    R.vt_from = rec->value_target_from;
    R.vt_to = rec->value_target_to;
    R.out = out;
    const int rc = run_games(h, S.data(), K, first, second, start_my, start_op, seeds, n_games, rewards, plies, moves, final_bb, rng_words,
                             "recorded games", &R);
    if (rc == SYN_OK) h->last_selfplay_games = n_games;
    return rc;
}

int syn_debug_tournament_regroup(syn_engine* h, const int32_t* keys, int n, int n_keys, int32_t* perm_out, int32_t* seg_out) {
    if (!h) return SYN_ERR_INVALID_ARGUMENT;
    if (n < 0 || n_keys < 1 || n_keys > TOURNAMENT_MAX_KEYS || !seg_out || (n > 0 && (!keys || !perm_out)))
        return fail(h, SYN_ERR_INVALID_ARGUMENT, "bad arguments to syn_debug_tournament_regroup");
    for (int i = 0; i < n; i++)
        if (keys[i] < 0 || keys[i] > n_keys)
            return fail(h, SYN_ERR_INVALID_ARGUMENT, "syn_debug_tournament_regroup: key %d of job %d is outside [0, %d]", keys[i], i, n_keys);
    for (int k = 0; k <= n_keys; k++) seg_out[k] = 0;
    if (n == 0) return SYN_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t nb = (size_t)n, cells = regroup_cells(nb, n_keys);
    size_t scan_bytes = 0;
    HIP_TRY(h, hipcub::DeviceScan::ExclusiveSum(nullptr, scan_bytes, (const unsigned*)nullptr, (unsigned*)nullptr, (int)cells, h->stream));
    Carve c;
    const size_t o_key = c.take(nb * 4), o_in = c.take(nb * 4), o_out = c.take(nb * 4), o_counts = c.take(cells * 4),
                 o_base = c.take(cells * 4), o_seg = c.take((size_t)(n_keys + 2) * 4), o_scan = c.take(scan_bytes);
    if (const int rc = ensure_scratch(h, c.at)) return rc;
    unsigned char* const base = static_cast<unsigned char*>(h->d_scratch);
    int* const d_key = reinterpret_cast<int*>(base + o_key);
    int* const d_seg = reinterpret_cast<int*>(base + o_seg);
    const MatchLive from{nullptr, nullptr, reinterpret_cast<int*>(base + o_in), nullptr, nullptr};
    const MatchLive to{nullptr, nullptr, reinterpret_cast<int*>(base + o_out), nullptr, nullptr};
    const RegroupBuffers R{reinterpret_cast<unsigned*>(base + o_counts), reinterpret_cast<unsigned*>(base + o_base), base + o_scan, scan_bytes};
    std::vector<int> iota(nb);
    for (size_t i = 0; i < nb; i++) iota[i] = (int)i;
    HIP_TRY(h, hipMemcpyAsync(d_key, keys, nb * 4, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipMemcpyAsync(from.id, iota.data(), nb * 4, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipMemsetAsync(to.id, 0xFF, nb * 4, h->stream));
    HIP_TRY(h, hipEventRecord(h->ev0, h->stream));
    if (const int rc = enqueue_regroup(h, d_key, n, n_keys, R, from, to, nullptr, nullptr, d_seg)) return rc;
    HIP_TRY(h, hipEventRecord(h->ev1, h->stream));
    HIP_TRY(h, hipMemcpyAsync(perm_out, to.id, nb * 4, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipMemcpyAsync(seg_out, d_seg, (size_t)(n_keys + 1) * 4, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    HIP_TRY(h, hipEventElapsedTime(&h->last_kernel_ms, h->ev0, h->ev1));
    h->last_launches = 2;
    return SYN_OK;
}

// evaluator.rs:308-319 FrozenMCTS::exploit over RolloutPolicy for n roots (frozen_kernel.cuh)
int syn_frozen_search_rollout(syn_engine* h, const syn_mcts_config* cfg, const uint64_t* seeds, uint64_t* rng_words,
                              const uint64_t* my_bb, const uint64_t* op_bb, const int32_t* explores, int n,
                              int action_selection, syn_frozen_result* results) {
    if (!h) return SYN_ERR_INVALID_ARGUMENT;
    if (!cfg || n < 0 || (n > 0 && (!seeds || !rng_words || !my_bb || !op_bb || !explores || !results)))
        return fail(h, SYN_ERR_INVALID_ARGUMENT, "bad arguments to syn_frozen_search_rollout");
    if (action_selection != SYN_ACTION_Q && action_selection != SYN_ACTION_NUM_VISITS)
        return fail(h, SYN_ERR_INVALID_ARGUMENT, "unknown action selection %d", action_selection);
    if (const int rc = check_frozen_config(h, cfg)) return rc;
    if (n == 0) return SYN_OK;
    size_t max_need = 0;
    for (int i = 0; i < n; i++) {
        if (!valid_root(my_bb[i], op_bb[i]))
            return fail(h, SYN_ERR_INVALID_ARGUMENT, "root %d is not a searchable Connect4 position", i);
        if (explores[i] < 0) return fail(h, SYN_ERR_INVALID_ARGUMENT, "explores[%d] must be >= 0", i);
        const size_t worst = frozen_worst_records(explores[i]);
        if (worst > max_need) max_need = worst;
        if (rng_words[i] > MATCH_WORD_LIMIT)
            return fail(h, SYN_ERR_INVALID_ARGUMENT, "rng_words[%d] is beyond the supported stream length", i);
    }
    FrozenPartition part;
    if (const int rc = frozen_partition(h, max_need, part)) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t nb = (size_t)n;
    int rc = ensure_scratch(h, nb * (8 * 4 + 4 + sizeof(FrozenResult)) + 256);
    if (rc != SYN_OK) return rc;
    unsigned long long* d_my = static_cast<unsigned long long*>(h->d_scratch);
    unsigned long long* d_op = d_my + nb;
    unsigned long long* d_seed = d_op + nb;
    unsigned long long* d_words = d_seed + nb;
    FrozenResult* d_res = reinterpret_cast<FrozenResult*>(d_words + nb);
    int* d_expl = reinterpret_cast<int*>(d_res + nb);
    if (const int prc = ensure_frozen_path(h, part, n)) return prc;
    HIP_TRY(h, hipMemcpyAsync(d_my, my_bb, nb * 8, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipMemcpyAsync(d_op, op_bb, nb * 8, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipMemcpyAsync(d_seed, seeds, nb * 8, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipMemcpyAsync(d_words, rng_words, nb * 8, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipMemcpyAsync(d_expl, explores, nb * 4, hipMemcpyHostToDevice, h->stream));
    CallScope scope(h, n);
    HIP_TRY(h, hipMemsetAsync(h->d_job_next, 0, 64, h->stream));
    HIP_TRY(h, scope.armed());  // (this kernel takes its roots in a grid-stride loop, not from the job counter: a syn_cancel
                                //  during the call is accepted and has no effect — every root is searched)
    FrozenParams P{};
    P.in_my = d_my; P.in_op = d_op; P.seeds = d_seed; P.rng_words = d_words; P.explores = d_expl;
    P.n_roots = n;
    P.results = d_res;
    HIP_TRY(h, hipEventRecord(h->ev0, h->stream));
    if (const int lrc = launch_frozen(h, part, cfg, action_selection, P)) return lrc;
    HIP_TRY(h, hipEventRecord(h->ev1, h->stream));
    static_assert(sizeof(FrozenResult) == sizeof(syn_frozen_result), "device and ABI result records must match");
    int kerr = 0;
    HIP_TRY(h, hipMemcpyAsync(results, d_res, nb * sizeof(FrozenResult), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipMemcpyAsync(rng_words, d_words, nb * 8, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipMemcpyAsync(&kerr, h->d_job_next + 8, 4, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (kerr) return fail(h, SYN_ERR_CAPACITY, "a baseline tree ran out of node records");
    HIP_TRY(h, hipEventElapsedTime(&h->last_kernel_ms, h->ev0, h->ev1));
    h->last_launches = 1;
    return SYN_OK;
}

static int ensure_outputs(syn_engine* h, int n_games) {
    if (n_games <= h->out_games) return SYN_OK;
    hipFree(h->d_plies); hipFree(h->d_states); hipFree(h->d_pis); hipFree(h->d_vs);
    hipFree(h->d_actions); hipFree(h->d_root_nodes); hipFree(h->d_final);
    h->d_plies = nullptr; h->d_states = nullptr; h->d_pis = nullptr; h->d_vs = nullptr;
    h->d_actions = nullptr; h->d_root_nodes = nullptr; h->d_final = nullptr;
    h->out_games = 0;
    size_t g = (size_t)n_games, p = g * 63;
    HIP_TRY(h, hipMalloc(&h->d_plies, g * 4));
    HIP_TRY(h, hipMalloc(&h->d_states, p * 16));
    HIP_TRY(h, hipMalloc(&h->d_pis, p * 36));
    HIP_TRY(h, hipMalloc(&h->d_vs, p * 12));
    HIP_TRY(h, hipMalloc(&h->d_actions, p));
    HIP_TRY(h, hipMalloc(&h->d_root_nodes, p * 4));
    HIP_TRY(h, hipMalloc(&h->d_final, g));
    h->out_games = n_games;
    return SYN_OK;
}

int syn_selfplay_run(syn_engine* h, const syn_rollout_config* cfg, uint64_t base_seed, uint64_t first_game,
                     int n_games, int32_t* plies, uint64_t* states_bb, float* pis, float* vs, uint8_t* actions,
                     uint32_t* root_nodes, uint8_t* final_kind, syn_counters* counters) {
    if (!h) return SYN_ERR_INVALID_ARGUMENT;
    if (!cfg) return fail(h, SYN_ERR_INVALID_ARGUMENT, "rollout config is NULL");
    if (n_games < 0) return fail(h, SYN_ERR_INVALID_ARGUMENT, "n_games must be >= 0");
    if (cfg->value_target < SYN_VALUE_Z || cfg->value_target > SYN_VALUE_Q_TO_Z)
        return fail(h, SYN_ERR_INVALID_ARGUMENT, "unknown value target %d", cfg->value_target);
    if (cfg->action != SYN_ACTION_Q && cfg->action != SYN_ACTION_NUM_VISITS)
        return fail(h, SYN_ERR_INVALID_ARGUMENT, "unknown action selection %d", cfg->action);
    if (cfg->random_actions_until < 0 || cfg->sample_actions_until < 0)
        return fail(h, SYN_ERR_INVALID_ARGUMENT, "random_actions_until / sample_actions_until must be >= 0");
    EngineParams P;
    int rc = common_params(h, P, cfg->num_explores);
    if (rc != SYN_OK) return rc;
    rc = convert_mcts(h, &cfg->mcts_cfg, P.mcts);
    if (rc != SYN_OK) return rc;
    if ((rc = check_lane_only(h, P.mcts)) != SYN_OK) return rc;
    if (counters) std::memset(counters, 0, sizeof(*counters));
    // what syn_replay_append_selfplay / syn_selfplay_positions_device compact: nothing until this launch has ended without an error
    h->last_selfplay_games = n_games == 0 ? 0 : -1;
    if (n_games == 0) return SYN_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    rc = ensure_outputs(h, n_games);
    if (rc != SYN_OK) return rc;
    P.roll.num_explores = cfg->num_explores;
    P.roll.random_until = cfg->random_actions_until;
    P.roll.sample_until = cfg->sample_actions_until;
    P.roll.stop_when_solved = cfg->stop_games_when_solved != 0;
    P.roll.value_target = cfg->value_target;
    P.roll.vt_p = cfg->value_target_p;
    P.roll.vt_from = cfg->value_target_from;
    P.roll.vt_to = cfg->value_target_to;
    P.roll.action = cfg->action;
    P.n_jobs = n_games;
    P.base_seed = base_seed;
    P.first_game = first_game;
    P.plies = h->d_plies;
    P.states_bb = h->d_states;
    P.pis = h->d_pis;
    P.vs = h->d_vs;
    P.actions = h->d_actions;
    P.root_nodes = h->d_root_nodes;
    P.final_kind = h->d_final;
    CallScope scope(h, n_games);
    HIP_TRY(h, hipMemsetAsync(h->d_job_next, 0, 64, h->stream));
    HIP_TRY(h, scope.armed());
    HIP_TRY(h, hipMemsetAsync(h->d_cache_stats, 0, 16, h->stream));
    HIP_TRY(h, hipMemsetAsync(h->d_counters, 0, sizeof(DevCounters), h->stream));
    HIP_TRY(h, hipMemsetAsync(h->d_plies, 0, (size_t)n_games * 4, h->stream));  // plies = 0: a game that never started (syn_cancel)
    // SYN_PROFILE=1: diagnostic build of the kernel with s_memtime stamps around each phase (never timed/benched)
    const bool prof = !counters && debug_env("SYN_PROFILE") != nullptr;
    unsigned long long* d_prof = nullptr;
    if (prof) {
        HIP_TRY(h, hipMalloc(&d_prof, (size_t)4096 * 16 * 6 * 8));
        HIP_TRY(h, hipMemsetAsync(d_prof, 0, (size_t)4096 * 16 * 6 * 8, h->stream));
        P.prof = d_prof;
    }
    HIP_TRY(h, hipEventRecord(h->ev0, h->stream));
    if (int rc = launch_engine(h, P, n_games, MODE_SELFPLAY, counters != nullptr, prof)) return rc;
    const int pgrid = h->last_grid, pnt = h->last_threads;
    HIP_TRY(h, hipEventRecord(h->ev1, h->stream));
    if (prof) {
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        if (h->last_shape == 7) {  // free-running rows: per wave [A, B, C, iterations, tiles, leaves] (free_kernel.cuh)
            const int nwv = pgrid * 4;
            std::vector<unsigned long long> hp((size_t)nwv * FP_FIELDS);
            HIP_TRY(h, hipMemcpy(hp.data(), d_prof, hp.size() * 8, hipMemcpyDeviceToHost));
            HIP_TRY(h, hipFree(d_prof));
            d_prof = nullptr;
            double s7[FP_FIELDS] = {0};
            for (int w = 0; w < nwv; w++)
                for (int j = 0; j < FP_FIELDS; j++) s7[j] += (double)hp[(size_t)w * FP_FIELDS + j];
            const double it7 = s7[FP_ITERS] + 1e-9;
            fprintf(stderr, "[syn profile free] grid=%d waves=%d rounds/wave=%.0f | cycles per round (one explore on each of a wave's four trees): "
                            "A=%.0f B=%.0f C=%.0f total=%.0f | tiles per round=%.3f, leaves per tile=%.2f, cycles per tile=%.0f\n",
                    pgrid, nwv, it7 / nwv, s7[FP_A] / it7, s7[FP_B] / it7, s7[FP_C] / it7, (s7[FP_A] + s7[FP_B] + s7[FP_C]) / it7,
                    s7[FP_TILES] / it7, s7[FP_LEAVES] / (s7[FP_TILES] + 1e-9), s7[FP_B] / (s7[FP_TILES] + 1e-9));
        } else
        if (h->last_shape == 5) {  // producer/consumer kernel: per wave [role, ...] (pc_kernel.cuh)
            const int nwv = pgrid * 16;
            std::vector<unsigned long long> hp((size_t)nwv * 8);
            HIP_TRY(h, hipMemcpy(hp.data(), d_prof, hp.size() * 8, hipMemcpyDeviceToHost));
            HIP_TRY(h, hipFree(d_prof));
            d_prof = nullptr;
            double mw = 0, mb = 0, mt = 0, nm = 0, tw = 0, ta = 0, tc = 0, tr = 0, tf = 0, ntw = 0;
            for (int w = 0; w < nwv; w++) {
                const unsigned long long* o = &hp[(size_t)w * 8];
                if (o[0] == 1) { nm++; mw += (double)o[1]; mb += (double)o[2]; mt += (double)o[3]; }
                else if (o[0] == 2) { ntw++; tw += (double)o[1]; ta += (double)o[2]; tc += (double)o[3]; tr += (double)o[4]; tf += (double)o[5]; }
            }
            fprintf(stderr, "[syn profile pc] grid=%d | matrix waves=%.0f: busy %.1f%% of (busy+wait), %.0f cycles per tile, %.0f tiles per wave | "
                            "tree waves=%.0f: per visit: wait=%.0f C=%.0f A+submit=%.0f cycles, explores finished=%.2f, visits per wave=%.0f\n",
                    pgrid, nm, 100.0 * mb / (mb + mw + 1e-9), mb / (mt + 1e-9), mt / (nm + 1e-9), ntw, tw / (tr + 1e-9), tc / (tr + 1e-9),
                    ta / (tr + 1e-9), tf / (tr + 1e-9), tr / (ntw + 1e-9));
        } else if (h->last_shape == 4) {  // lane kernel: per wave [A, B, C, move, rounds, tiles, active lanes, evals, then the LP_* fields]
            int nwv = pgrid * (pnt / 64);
            constexpr int F = LP_FIELDS;
            std::vector<unsigned long long> hp((size_t)nwv * F);
            HIP_TRY(h, hipMemcpy(hp.data(), d_prof, hp.size() * 8, hipMemcpyDeviceToHost));
            unsigned long long* d_prof_keep = d_prof;
            double s[F];
            for (int j = 0; j < F; j++) s[j] = 0;
            for (int w = 0; w < nwv; w++)
                for (int j = 0; j < F; j++) s[j] += (double)hp[(size_t)w * F + j];
            fprintf(stderr, "[syn profile lanes] grid=%d nt=%d waves=%d rounds/wave=%.0f | cycles per round: A=%.0f B=%.0f C: children=%.0f "
                            "solver walk=%.0f sweep=%.0f move=%.0f total=%.0f | per round: tiles=%.3f explores finished=%.2f evals=%.2f "
                            "(%.2f per tile) | cycles per finished explore=%.0f\n",
                    pgrid, pnt, nwv, s[4] / nwv, s[0] / s[4], s[1] / s[4], s[6] / s[4], s[7] / s[4], s[2] / s[4], s[3] / s[4],
                    (s[0] + s[1] + s[2] + s[3] + s[6] + s[7]) / s[4], s[5] / s[4], s[8] / s[4], s[9] / s[4], s[9] / s[5],
                    (s[0] + s[1] + s[2] + s[3] + s[6] + s[7]) / s[8]);
            const double R = s[4];  // rounds (all waves)
            fprintf(stderr, "[syn profile lanes, inside the phases; cycles per round and wave] A: %.2f iterations (%.1f lanes each), line wait %.0f "
                            "(%.0f per iteration), level arithmetic %.0f (%.0f per iteration), arrive %.0f | B: tiles %.0f (%.0f per tile), "
                            "scatter %.0f | C children: softmaxes %.0f, records %.0f (%.1f lanes) | solver walk: %.2f iterations (%.1f lanes each), "
                            "line wait %.0f (%.0f per iteration) | sweep: %.2f steps, %.1f lane-levels per step, log wait %.0f (%.0f per step), "
                            "arithmetic + stores %.0f (%.0f per step) | end of search: %.3f calls per round, %.1f lanes per call, cycles per call %.0f = "
                            "root line + generator %.0f, targets %.0f, sample %.0f, step %.0f, game end / reset %.0f\n",
                    s[LP_A_ITERS] / R, s[LP_A_LANES] / (s[LP_A_ITERS] + 1e-9), s[LP_A_WAIT] / R, s[LP_A_WAIT] / (s[LP_A_ITERS] + 1e-9),
                    s[LP_A_ALU] / R, s[LP_A_ALU] / (s[LP_A_ITERS] + 1e-9), s[LP_A_ARRIVE] / R, s[LP_B_TILE] / R,
                    s[LP_B_TILE] / (s[5] + 1e-9), s[LP_B_SCATTER] / R, s[LP_C_SOFT] / R, (s[LP_C_WRITE] - s[LP_C_SOFT]) / R,
                    s[LP_C_LANES] / R, s[LP_W_ITERS] / R, s[LP_W_LANES] / (s[LP_W_ITERS] + 1e-9), s[LP_W_WAIT] / R,
                    s[LP_W_WAIT] / (s[LP_W_ITERS] + 1e-9), s[LP_S_STEPS] / R, s[LP_S_LANES] / (s[LP_S_STEPS] + 1e-9), s[LP_S_WAIT] / R,
                    s[LP_S_WAIT] / (s[LP_S_STEPS] + 1e-9), s[LP_S_ALU] / R, s[LP_S_ALU] / (s[LP_S_STEPS] + 1e-9), s[LP_M_CALLS] / R,
                    s[LP_M_LANES] / (s[LP_M_CALLS] + 1e-9), s[LP_M_TOTAL] / (s[LP_M_CALLS] + 1e-9), s[LP_M_T1] / (s[LP_M_CALLS] + 1e-9),
                    s[LP_M_T2] / (s[LP_M_CALLS] + 1e-9), s[LP_M_T3] / (s[LP_M_CALLS] + 1e-9), s[LP_M_T4] / (s[LP_M_CALLS] + 1e-9),
                    s[LP_M_T5] / (s[LP_M_CALLS] + 1e-9));
            {
                std::vector<unsigned long long> tlv(4 * 16 * 3);
                (void)hipMemcpy(tlv.data(), d_prof_keep + PROF_TIMELINE_OFF, tlv.size() * 8, hipMemcpyDeviceToHost);
                unsigned long long t0 = ~0ull;
                for (auto v : tlv) if (v && v < t0) t0 = v;
                for (int w = 0; w < pnt / 256; w++) {
                    fprintf(stderr, "[timeline wave %d of SIMD 0] (B start, B end, round end) kilo-cycles:", w * 4);
                    for (int r = 0; r < 8; r++)
                        fprintf(stderr, " (%.0f %.0f %.0f)", (tlv[(w * 16 + r) * 3] - t0) / 1e3, (tlv[(w * 16 + r) * 3 + 1] - t0) / 1e3,
                                (tlv[(w * 16 + r) * 3 + 2] - t0) / 1e3);
                    fprintf(stderr, "\n");
                }
                (void)hipFree(d_prof_keep);
            }
            d_prof = nullptr;
        }
    }
    if (prof && d_prof) {
        int nw = pgrid * (pnt / 64);
        std::vector<unsigned long long> hp((size_t)nw * 6);
        HIP_TRY(h, hipMemcpy(hp.data(), d_prof, hp.size() * 8, hipMemcpyDeviceToHost));
        HIP_TRY(h, hipFree(d_prof));
        double sum[6] = {0, 0, 0, 0, 0, 0};
        unsigned long long max_it = 0;
        for (int w = 0; w < nw; w++) {
            for (int j = 0; j < 6; j++) sum[j] += (double)hp[(size_t)w * 6 + j];
            if (hp[(size_t)w * 6 + 5] > max_it) max_it = hp[(size_t)w * 6 + 5];
        }
        double its = sum[5] / nw;
        fprintf(stderr, "[syn profile] grid=%d nt=%d waves=%d iterations avg=%.0f max=%llu | cycles/iteration per wave (100 MHz s_memtime ticks x?): "
                        "A=%.0f wait1=%.0f B=%.0f wait2=%.0f C=%.0f total=%.0f\n",
                pgrid, pnt, nw, its, max_it, sum[0] / sum[5], sum[1] / sum[5], sum[2] / sum[5], sum[3] / sum[5],
                sum[4] / sum[5], (sum[0] + sum[1] + sum[2] + sum[3] + sum[4]) / sum[5]);
    }
    size_t g = (size_t)n_games, p = g * 63;
    if (plies) HIP_TRY(h, hipMemcpyAsync(plies, h->d_plies, g * 4, hipMemcpyDeviceToHost, h->stream));
    if (states_bb) HIP_TRY(h, hipMemcpyAsync(states_bb, h->d_states, p * 16, hipMemcpyDeviceToHost, h->stream));
    if (pis) HIP_TRY(h, hipMemcpyAsync(pis, h->d_pis, p * 36, hipMemcpyDeviceToHost, h->stream));
    if (vs) HIP_TRY(h, hipMemcpyAsync(vs, h->d_vs, p * 12, hipMemcpyDeviceToHost, h->stream));
    if (actions) HIP_TRY(h, hipMemcpyAsync(actions, h->d_actions, p, hipMemcpyDeviceToHost, h->stream));
    if (root_nodes) HIP_TRY(h, hipMemcpyAsync(root_nodes, h->d_root_nodes, p * 4, hipMemcpyDeviceToHost, h->stream));
    if (final_kind) HIP_TRY(h, hipMemcpyAsync(final_kind, h->d_final, g, hipMemcpyDeviceToHost, h->stream));
    if (counters)
        HIP_TRY(h, hipMemcpyAsync(counters, h->d_counters, sizeof(DevCounters), hipMemcpyDeviceToHost, h->stream));
    int kerr = 0, games_finished = 0;
    unsigned long long cstats[2] = {0, 0};
    HIP_TRY(h, hipMemcpyAsync(&kerr, h->d_job_next + 8, 4, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipMemcpyAsync(&games_finished, h->d_job_next + 1, 4, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipMemcpyAsync(cstats, h->d_cache_stats, 16, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    h->last_cache_hits = cstats[0];
    h->last_cache_misses = cstats[1];
    if (const int rc = fail_search_error(h, kerr)) return rc;
    HIP_TRY(h, hipEventElapsedTime(&h->last_kernel_ms, h->ev0, h->ev1));
    h->last_launches = 1;
    h->last_selfplay_games = n_games;
    // decided by what finished, not by the flag: a cancel that arrives after the last game was handed out cancels nothing
    if (scope.cancelled() && games_finished < n_games)
        return fail(h, SYN_ERR_CANCELLED, "cancelled by syn_cancel: %d of %d games were played (to the end); the others have plies == 0",
                    games_finished, n_games);
    return SYN_OK;
}

int syn_progress(syn_engine* h, int* started, int* finished) {
    if (!h) return SYN_ERR_INVALID_ARGUMENT;
    std::lock_guard<std::mutex> g(h->call_mu);
    if (hipSetDevice(h->device) != hipSuccess) return SYN_ERR_HIP;
    if (hipMemcpyAsync(h->h_pin, h->d_job_next, 8, hipMemcpyDeviceToHost, h->aux_stream) != hipSuccess) return SYN_ERR_HIP;
    if (hipStreamSynchronize(h->aux_stream) != hipSuccess) return SYN_ERR_HIP;
    const int jobs = h->running_jobs;
    int st = h->h_pin[0];
    if (st >= CANCEL_WORD) st = h->started_at_cancel;  // the counter was raised by syn_cancel: what had been handed out before
    if (jobs > 0 && st > jobs) st = jobs;              // (every lane's last fetch overshoots the job count)
    if (started) *started = st;
    if (finished) *finished = h->h_pin[1];
    return SYN_OK;
}

int syn_cancel(syn_engine* h) {
    if (!h) return SYN_ERR_INVALID_ARGUMENT;
    std::lock_guard<std::mutex> g(h->call_mu);
    if (h->call_state == 0) return SYN_ERR_INVALID_ARGUMENT;  // no call in flight: nothing to cancel (the error string belongs to the calling thread's entry points and is not touched here)
    if (h->call_state == 1) {  // the call has not reset the job counter yet: it applies the cancel itself, right behind the reset
        h->cancel_pending = 1;
        return SYN_OK;
    }
    if (h->cancel_applied) return SYN_OK;
    if (hipSetDevice(h->device) != hipSuccess) return SYN_ERR_HIP;
    // jobs handed out so far (a lower bound of what will have started: a fetch between this read and the write below still counts)
    if (hipMemcpyAsync(h->h_pin + 9, h->d_job_next, 4, hipMemcpyDeviceToHost, h->aux_stream) != hipSuccess) return SYN_ERR_HIP;
    // every later job fetch (an atomic add on this word) now returns an index past the call's job count: no new game starts
    h->h_pin[8] = CANCEL_WORD;
    if (hipMemcpyAsync(h->d_job_next, h->h_pin + 8, 4, hipMemcpyHostToDevice, h->aux_stream) != hipSuccess) return SYN_ERR_HIP;
    if (hipStreamSynchronize(h->aux_stream) != hipSuccess) return SYN_ERR_HIP;
    h->started_at_cancel = h->h_pin[9] < h->running_jobs ? h->h_pin[9] : h->running_jobs;
    h->cancel_applied = 1;
    return SYN_OK;
}

// ------------------------------------------------------------------------------------------------ learner
// Every learner entry point opens with this: the handle, then the learner. (Its own argument check and the selection of the engine's
// device follow in the entry point, in the order its errors have always had.)
static int learner_check(syn_engine* h) {
    if (!h) return SYN_ERR_INVALID_ARGUMENT;
    if (!h->learner.has_trainer) return fail(h, SYN_ERR_NO_WEIGHTS, "call syn_trainer_init first");
    return SYN_OK;
}

// the developer knobs of the learner (honoured with SYN_DEBUG=1 only: debug_env), read once per process where one is first needed: the
// first syn_train_epoch or gradient launch, which is inside the first syn_trainer_init*'s self-check.
// (SYN_TRAIN_FORCE_ABORT is not among them: epoch_force_abort)
struct LearnerKnobs {
    bool queued;        // SYN_TRAIN_QUEUED=1: syn_train_epoch keeps the two launches per step (A/B, same bits)
    bool profile;       // SYN_TRAIN_PROFILE=1: diagnostic stamps of the kernels' phases, printed to stderr
    bool device_scope;  // SYN_TRAIN_DEVICE_SCOPE=1: the epoch kernels use the device-scope barrier
    bool conv_mw_off;   // SYN_TRAIN_CONV_MW=0: the conv epoch runs in the one-workgroup kernel
};
static const LearnerKnobs& learner_knobs() {
    static const LearnerKnobs knobs = [] {
        const char* mw = debug_env("SYN_TRAIN_CONV_MW");
        return LearnerKnobs{debug_env("SYN_TRAIN_QUEUED") != nullptr, debug_env("SYN_TRAIN_PROFILE") != nullptr,
                            debug_env("SYN_TRAIN_DEVICE_SCOPE") != nullptr, mw && std::atoi(mw) == 0};
    }();
    return knobs;
}
// test hook, read at every syn_train_epoch call: the persistent kernel's result is thrown away and the recovery path taken
static bool epoch_force_abort() { return debug_env("SYN_TRAIN_FORCE_ABORT") != nullptr; }

// All of the learner's device buffers or none: a failed allocation frees what was taken, so that a retry starts from scratch instead
// of skipping the allocation block.
static int alloc_trainer_buffers(syn_engine* h) {
    static_assert(ConvGeom::NUM_PARAMS <= TrainGeom::NUM_PARAMS, "trainer buffers are sized for Connect4Net");
    auto& L = h->learner;
    if (L.d_tw) return SYN_OK;
    const LearnerBuffers want = learner_buffers(L);
    for (const auto& w : want.all) {
        hipError_t e = hipMalloc(w.p, w.bytes);
        if (e != hipSuccess) {
            for (const auto& u : want.all) {
                if (*u.p) (void)hipFree(*u.p);
                *u.p = nullptr;
            }
            L.has_trainer = false;
            return fail(h, SYN_ERR_HIP, "hipMalloc(trainer buffers) failed: %s", hipGetErrorString(e));
        }
    }
    return SYN_OK;
}

// The learner of network `kind` at its start: (Connect4Net) both fragment images uploaded, then the parameters, zero moments and
// gradients (all three over the buffers' whole size, whichever network used them before), step 0.
struct LearnerStart {
    int kind;
    const float* blob;
    const std::vector<float>* img;   // Connect4Net: the forward and the transposed fragment image of `blob`; else NULL
    const std::vector<float>* timg;
};
static int learner_load_state(syn_engine* h, const LearnerStart& s) {
    auto& L = h->learner;
    const size_t cap_bytes = (size_t)TrainGeom::NUM_PARAMS * 4;
    if (s.kind == 0) {
        HIP_TRY(h, hipMemcpyAsync(L.d_twimg, s.img->data(), s.img->size() * 4, hipMemcpyHostToDevice, h->stream));
        HIP_TRY(h, hipMemcpyAsync(L.d_ttimg, s.timg->data(), s.timg->size() * 4, hipMemcpyHostToDevice, h->stream));
    }
    HIP_TRY(h, hipMemcpyAsync(L.d_tw, s.blob, g_net_desc[s.kind].param_bytes(), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipMemsetAsync(L.d_tm, 0, cap_bytes, h->stream));
    HIP_TRY(h, hipMemsetAsync(L.d_tv, 0, cap_bytes, h->stream));
    HIP_TRY(h, hipMemsetAsync(L.d_tgrad, 0, cap_bytes, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    L.train_step = 0;
    return SYN_OK;
}

// Optimiser step `step`'s (1-based) bias corrections folded into the two scalars the Adam kernels take, in double on the host like
// libtorch.
struct AdamScalars {
    float step_size, inv_sqrt_bc2;
};
static AdamScalars adam_scalars(const DevTrainHyper& hp, float lr, long long step) {
    const double bc1 = 1.0 - std::pow((double)hp.beta1, (double)step);
    const double bc2 = 1.0 - std::pow((double)hp.beta2, (double)step);
    return {(float)((double)lr / bc1), (float)(1.0 / std::sqrt(bc2))};
}

// The start-up self-checks of the two learners run eight steps of batch 8 over this synthetic data set of 64 positions.
struct SelfCheckBatch {
    static constexpr int N = 64, STEPS = 8, B = 8;
    std::vector<uint64_t> my, op;
    std::vector<float> tpi, tv;
    std::vector<int32_t> perm;
};
static SelfCheckBatch self_check_batch() {
    using S = SelfCheckBatch;
    S b{std::vector<uint64_t>(S::N), std::vector<uint64_t>(S::N), std::vector<float>((size_t)S::N * 9, 1.0f / 9.0f),
        std::vector<float>((size_t)S::N * 3, 0.0f), std::vector<int32_t>(S::STEPS * S::B)};
    for (int i = 0; i < S::N; i++) {
        b.my[i] = (0x0000040810204081ull * (uint64_t)(i % 7 + 1)) & 0x00003F7EFDFBF7EFull & ~(0x7Full << (7 * (i % 9)));
        b.op[i] = (0x7Full << (7 * (i % 9))) & (0x0101010101010101ull * (uint64_t)(i % 5 + 1));
        b.op[i] &= ~b.my[i];
        b.tv[(size_t)i * 3 + i % 3] = 1.0f;
    }
    for (int i = 0; i < S::STEPS * S::B; i++) b.perm[i] = (i * 37) % S::N;
    return b;
}
// The two-mode loop of a self-check: from the caller's state `start`, mode 0 then mode 1 run the synthetic epoch, the weights are
// read and the caller's state is put back. A mode is the barrier for Connect4Net (1 = device scope) and the kernel for Connect4ConvNet
// (0 = one workgroup, 1 = four). Returns whether all of it could run (h->err says what could not); *same_bits: it could, and the two
// modes left the same weights bit for bit.
static bool learner_self_check(syn_engine* h, const LearnerStart& start, bool* same_bits) {
    auto& L = h->learner;
    const SelfCheckBatch b = self_check_batch();
    const size_t nw = (size_t)g_net_desc[start.kind].num_params;
    std::vector<float> w[2] = {std::vector<float>(nw), std::vector<float>(nw)};
    bool ok = true;
    for (int mode = 0; mode < 2 && ok; mode++) {
        if (start.kind == 0) L.epoch_device_scope = mode == 1;
        else L.conv_mw_force = mode;
        ok = syn_train_set_data(h, b.my.data(), b.op.data(), b.tpi.data(), b.tv.data(), b.N) == SYN_OK &&
             syn_train_epoch(h, b.perm.data(), b.STEPS, b.B, 1e-3f, nullptr) == SYN_OK &&
             syn_trainer_get_state(h, w[mode].data(), nullptr, nullptr, nullptr, nullptr) == SYN_OK && learner_load_state(h, start) == SYN_OK;
    }
    L.conv_mw_force = -1;
    L.train_step = 0;
    L.data.n = 0;   // the synthetic batch replaced whatever syn_train_set_data had uploaded: the caller uploads again (once per engine)
    *same_bits = ok && std::memcmp(w[0].data(), w[1].data(), nw * 4) == 0;
    return ok;
}

// The two fragment-order images the matrix-core Connect4Net learner reads its A operands from (train_mfma.cuh); adam_image_kernel
// keeps them in step with the canonical weights afterwards. The slot table is checked by its bit patterns: a restored state may hold NaNs.
static int build_trainer_images(syn_engine* h, const float* blob, std::vector<float>& img, std::vector<float>& timg) {
    timg.assign((size_t)TrainImg::T_FLOATS, 0.0f);
    build_weight_image(blob, img);
    for (int p = 0; p < TrainGeom::NUM_PARAMS; p++) {
        int fwd, tr;
        train_image_slots(p, fwd, tr);
        if (std::memcmp(&img[(size_t)fwd], &blob[p], 4) != 0)
            return fail(h, SYN_ERR_HIP, "internal: image slot table disagrees with build_weight_image at %d", p);
        if (tr >= 0) timg[(size_t)tr] = blob[p];
    }
    return SYN_OK;
}

int syn_trainer_init(syn_engine* h, const float* blob, size_t n_floats, const syn_train_config* cfg) {
    if (!h) return SYN_ERR_INVALID_ARGUMENT;
    if (!blob || !cfg) return fail(h, SYN_ERR_INVALID_ARGUMENT, "blob/cfg is NULL");
    if (n_floats != (size_t)TrainGeom::NUM_PARAMS)
        return fail(h, SYN_ERR_INVALID_ARGUMENT, "Connect4Net has %d parameters, got %zu", TrainGeom::NUM_PARAMS, n_floats);
    HIP_TRY(h, hipSetDevice(h->device));
    int rc = alloc_trainer_buffers(h);
    if (rc != SYN_OK) return rc;
    auto& L = h->learner;
    std::vector<float> img, timg;
    rc = build_trainer_images(h, blob, img, timg);
    if (rc != SYN_OK) return rc;
    const LearnerStart start{0, blob, &img, &timg};
    rc = learner_load_state(h, start);
    if (rc != SYN_OK) return rc;
    L.train_hp = DevTrainHyper{cfg->weight_decay, cfg->policy_weight, cfg->value_weight, cfg->beta1, cfg->beta2, cfg->eps};
    L.has_trainer = true;
    L.trainer_kind = 0;
    L.train_bf16 = 0;
    L.batch_mode = SYN_TRAIN_BATCH_CHAINED;
    L.micro_max_wgs = 0;
    // ---- the epoch kernel's one-XCD step barrier rests on observed hardware behaviour (train_epoch.cuh: `buffer_inv sc0` empties
    //      the vector L1 outside threadgroup-split mode). Once per engine: eight steps on a synthetic batch through that barrier and
    //      through the device-scope barrier from the same state; any differing bit switches this engine to the device-scope barrier.
    if (!L.epoch_barrier_checked) {
        L.epoch_barrier_checked = true;
        bool same = false;
        const bool ok = learner_self_check(h, start, &same);
        L.epoch_device_scope = !same;
        if (!ok) return fail(h, SYN_ERR_HIP, "the learner's start-up self-check could not run: %s", h->err.c_str());
    }
    return SYN_OK;
}

int syn_trainer_init_conv(syn_engine* h, const float* blob, size_t n_floats, const syn_train_config* cfg) {
    if (!h) return SYN_ERR_INVALID_ARGUMENT;
    if (!blob || !cfg) return fail(h, SYN_ERR_INVALID_ARGUMENT, "blob/cfg is NULL");
    if (n_floats != (size_t)ConvGeom::NUM_PARAMS)
        return fail(h, SYN_ERR_INVALID_ARGUMENT, "Connect4ConvNet has %d parameters, got %zu", ConvGeom::NUM_PARAMS, n_floats);
    HIP_TRY(h, hipSetDevice(h->device));
    int rc = alloc_trainer_buffers(h);
    if (rc != SYN_OK) return rc;
    auto& L = h->learner;
    const LearnerStart start{1, blob, nullptr, nullptr};
    rc = learner_load_state(h, start);
    if (rc != SYN_OK) return rc;
    L.train_hp = DevTrainHyper{cfg->weight_decay, cfg->policy_weight, cfg->value_weight, cfg->beta1, cfg->beta2, cfg->eps};
    L.has_trainer = true;
    L.trainer_kind = 1;
    L.train_bf16 = 0;
    L.batch_mode = SYN_TRAIN_BATCH_CHAINED;
    L.micro_max_wgs = 0;
    // ---- the four-workgroup epoch kernel exchanges its intermediates through L2 behind the one-XCD barrier of train_epoch.cuh (observed
    //      hardware behaviour, see there). Once per engine: eight steps on a synthetic batch through it and through the one-workgroup
    //      kernel from the same state; any differing bit (or a launch that cannot run) keeps this engine on the one-workgroup kernel.
    if (!L.conv_mw_checked) {
        L.conv_mw_checked = true;
        const long long fallbacks0 = L.epoch_fallbacks;
        bool same = false;
        const bool ok = learner_self_check(h, start, &same);
        L.conv_mw_disabled = !(same && L.epoch_fallbacks == fallbacks0);
        L.epoch_fallbacks = fallbacks0;
        if (!ok) return fail(h, SYN_ERR_HIP, "the conv learner's start-up self-check could not run: %s", h->err.c_str());
    }
    return SYN_OK;
}

int syn_trainer_set_precision(syn_engine* h, int precision) {
    if (!h) return SYN_ERR_INVALID_ARGUMENT;
    auto& L = h->learner;
    if (!L.has_trainer) return fail(h, SYN_ERR_NO_WEIGHTS, "call syn_trainer_init_conv first");
    if (precision != SYN_TRAIN_F32 && precision != SYN_TRAIN_BF16) return fail(h, SYN_ERR_INVALID_ARGUMENT, "unknown training precision %d", precision);
    if (precision == SYN_TRAIN_BF16 && L.trainer_kind != 1)
        return fail(h, SYN_ERR_UNSUPPORTED, "the bf16 training variant exists for Connect4ConvNet only (BASELINE configs[4]: \"bf16 conv\"); "
                                            "Connect4Net trains in f32, bit-exact with the oracle");
    L.train_bf16 = precision == SYN_TRAIN_BF16 ? 1 : 0;
    return SYN_OK;
}

int syn_trainer_set_batch_mode(syn_engine* h, int mode, int max_workgroups) {
    const int rc = learner_check(h);
    if (rc != SYN_OK) return rc;
    if (mode != SYN_TRAIN_BATCH_CHAINED && mode != SYN_TRAIN_BATCH_MICRO) return fail(h, SYN_ERR_INVALID_ARGUMENT, "unknown batch mode %d", mode);
    if (max_workgroups < 0) return fail(h, SYN_ERR_INVALID_ARGUMENT, "max_workgroups is negative (%d); 0 means one workgroup per CU", max_workgroups);
    HIP_TRY(h, hipSetDevice(h->device));
    h->learner.batch_mode = mode;
    h->learner.micro_max_wgs = max_workgroups;
    return SYN_OK;
}

int syn_trainer_get_batch_mode(syn_engine* h, int* mode, int* max_workgroups, int* last_grid) {
    const int rc = learner_check(h);
    if (rc != SYN_OK) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    if (mode) *mode = h->learner.batch_mode;
    if (max_workgroups) *max_workgroups = h->learner.micro_max_wgs;
    if (last_grid) *last_grid = h->learner.micro_last_grid;
    return SYN_OK;
}

// ------------------------------------------------------------------------------------------------ learner step
// Stored positions (position_layout.hpp): the replay buffer is columns_at(.., capacity, true); the learner's data set, the evaluation
// set and every staged batch are columns_at(.., n, false), 64 bytes a position.
static_assert(sizeof(DevSearchResult) == SEARCH_RESULT_BYTES, "position_layout.hpp restates engine_kernels.cuh's search result");
// n positions from `src` to `dst` on h->stream: one block copy per column, a column that is null on either side is skipped
static int copy_positions(syn_engine* h, const PositionColumns& dst, const PositionColumns& src, size_t n, hipMemcpyKind kind) {
    if (n == 0) return SYN_OK;
    if (dst.my && src.my) HIP_TRY(h, hipMemcpyAsync(dst.my, src.my, n * POS_BOARD_BYTES, kind, h->stream));
    if (dst.op && src.op) HIP_TRY(h, hipMemcpyAsync(dst.op, src.op, n * POS_BOARD_BYTES, kind, h->stream));
    if (dst.gid && src.gid) HIP_TRY(h, hipMemcpyAsync(dst.gid, src.gid, n * POS_GID_BYTES, kind, h->stream));
    if (dst.pi && src.pi) HIP_TRY(h, hipMemcpyAsync(dst.pi, src.pi, n * POS_PI_BYTES, kind, h->stream));
    if (dst.v && src.v) HIP_TRY(h, hipMemcpyAsync(dst.v, src.v, n * POS_V_BYTES, kind, h->stream));
    return SYN_OK;
}
// Room for `need` positions in a data set of the engine's. A buffer that has to grow is allocated for `grow_to` >= need positions (the
// caller's growth policy) once the stream's work on the old one is done; the data set it held is gone then (R.n == 0).
static int ensure_position_rows(syn_engine* h, PositionRows& R, size_t need, size_t grow_to) {
    if (need <= R.cap) return SYN_OK;
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    (void)hipFree(R.d);
    R = PositionRows{};
    HIP_TRY(h, hipMalloc(&R.d, grow_to * POS_ROW_BYTES));
    R.cap = grow_to;
    return SYN_OK;
}

// SYN_TRAIN_BATCH_MICRO's refusals, before anything is staged or launched: the learner is left as it was
static_assert(PLAN_MICRO_BLOCK == MICRO_BLOCK && PLAN_MICRO_MAX_BLOCKS == MICRO_MAX_BLOCKS && PLAN_MLP_NUM_PARAMS == TrainGeom::NUM_PARAMS &&
                  PLAN_CONV_NUM_PARAMS == ConvGeom::NUM_PARAMS && PLAN_MICRO_MLP_LDS == (size_t)TrainGeom::WL_OFF * 4 &&
                  PLAN_MICRO_CONV_LDS == (size_t)ConvMfmaGeom::LDS_FLOATS * 4,
              "launch_plan.hpp restates train_micro.cuh and the learners' geometry");
static int check_micro_batch(syn_engine* h, int batch) {
    if (h->learner.batch_mode != SYN_TRAIN_BATCH_MICRO) return SYN_OK;
    if (batch < MICRO_BLOCK || batch % MICRO_BLOCK != 0)
        return fail(h, SYN_ERR_INVALID_ARGUMENT, "SYN_TRAIN_BATCH_MICRO takes minibatches that are a multiple of %d positions (got %d)", MICRO_BLOCK, batch);
    if (batch / MICRO_BLOCK > MICRO_MAX_BLOCKS)
        return fail(h, SYN_ERR_UNSUPPORTED, "SYN_TRAIN_BATCH_MICRO takes at most %d micro-batches of %d positions (got %d positions)",
                    MICRO_MAX_BLOCKS, MICRO_BLOCK, batch);
    return SYN_OK;
}

// The micro-batch gradient (train_micro.cuh): the blocks kernel over plan_micro_grads' grid, then the reduce, both on `st`.
static int launch_grads_micro(syn_engine* h, hipStream_t st, const PositionColumns& b, int batch, float* d_grads, float* d_losses) {
    auto& L = h->learner;
    const int rc = check_micro_batch(h, batch);
    if (rc != SYN_OK) return rc;
    MicroQuery q;
    q.net_kind = L.trainer_kind; q.nb = batch / MICRO_BLOCK; q.max_workgroups = L.micro_max_wgs; q.num_cus = h->num_cus;
    const MicroPlan p = plan_micro_grads(q);
    if (p.buffer_bytes > L.micro_rows_bytes) {
        // (hipFree waits for the device: nothing still reads the old rows)
        if (L.d_micro_rows) HIP_TRY(h, hipFree(L.d_micro_rows));
        L.d_micro_rows = nullptr;
        L.micro_rows_bytes = 0;
        HIP_TRY(h, hipMalloc(&L.d_micro_rows, p.buffer_bytes));
        L.micro_rows_bytes = p.buffer_bytes;
    }
    int num_params;
    if (L.trainer_kind == 1) {
        auto kb = L.train_bf16 ? train_micro_blocks_conv_kernel<true> : train_micro_blocks_conv_kernel<false>;
        HIP_TRY(h, hipFuncSetAttribute(reinterpret_cast<const void*>(kb), hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds));
        hipLaunchKernelGGL(kb, dim3(p.grid), dim3(p.threads), p.lds, st, L.d_tw, b.my, b.op, b.pi, b.v, q.nb, L.train_hp, L.d_micro_rows);
        num_params = ConvGeom::NUM_PARAMS;
    } else {
        HIP_TRY(h, hipFuncSetAttribute(reinterpret_cast<const void*>(train_micro_blocks_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds));
        hipLaunchKernelGGL(train_micro_blocks_kernel, dim3(p.grid), dim3(p.threads), p.lds, st, L.d_twimg, L.d_ttimg, b.my, b.op, b.pi, b.v, q.nb,
                           L.train_hp, L.d_micro_rows);
        num_params = TrainGeom::NUM_PARAMS;
    }
    HIP_TRY(h, hipGetLastError());
    L.micro_last_grid = p.grid;
    hipLaunchKernelGGL(train_micro_reduce_kernel, dim3(p.reduce_grid), dim3(p.reduce_threads), 0, st, L.d_micro_rows, q.nb, num_params, p.row_stride,
                       1.0f / (float)q.nb, d_grads, d_losses);
    HIP_TRY(h, hipGetLastError());
    return SYN_OK;
}

// (the *_enqueue entry points run the step on the caller's stream `st` — which may be the null stream: torch's default)
static int launch_grads(syn_engine* h, hipStream_t st, const PositionColumns& b, int batch, float* d_grads, float* d_losses = nullptr) {
    auto& L = h->learner;
    if (!d_losses) d_losses = L.d_tloss;
    if (L.batch_mode == SYN_TRAIN_BATCH_MICRO) return launch_grads_micro(h, st, b, batch, d_grads, d_losses);
    if (L.trainer_kind == 1) {
        // Connect4ConvNet (train_conv_mfma.cuh): one workgroup, the minibatch's activations resident in LDS, every chain on the
        // f32 matrix cores
        if (batch > ConvTrainGeom::CHUNK)
            return fail(h, SYN_ERR_UNSUPPORTED, "the Connect4ConvNet learner takes minibatches of at most %d positions (got %d)",
                        ConvTrainGeom::CHUNK, batch);
        const size_t clds = (size_t)ConvMfmaGeom::LDS_FLOATS * 4;
        auto kg = L.train_bf16 ? train_conv_grad_kernel_mfma<true> : train_conv_grad_kernel_mfma<false>;
        HIP_TRY(h, hipFuncSetAttribute(reinterpret_cast<const void*>(kg), hipFuncAttributeMaxDynamicSharedMemorySize, (int)clds));
        hipLaunchKernelGGL(kg, dim3(1), dim3(CONV_TRAIN_THREADS), clds, st, L.d_tw, b.my, b.op, b.pi, b.v, batch, L.train_hp, d_grads,
                           d_losses, (const int*)nullptr);
        HIP_TRY(h, hipGetLastError());
        return SYN_OK;
    }
    // Connect4Net: the matrix-core kernel (train_mfma.cuh)
    const size_t lds = (size_t)TrainGeom::WL_OFF * 4;
    HIP_TRY(h, hipFuncSetAttribute(reinterpret_cast<const void*>(train_grad_kernel_mfma), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    // SYN_TRAIN_PROFILE=1: diagnostic stamps of the kernel's phases (first chunk), printed to stderr
    const bool prof = learner_knobs().profile;
    unsigned long long* d_prof = nullptr;
    if (prof) {
        HIP_TRY(h, hipMalloc(&d_prof, 4096));
        HIP_TRY(h, hipMemsetAsync(d_prof, 0, 4096, st));
    }
    hipLaunchKernelGGL(train_grad_kernel_mfma, dim3(1), dim3(1024), lds, st, L.d_tw, L.d_twimg, L.d_ttimg, b.my, b.op, b.pi, b.v, batch,
                       L.train_hp, d_grads, d_losses, (const int*)nullptr, d_prof);
    HIP_TRY(h, hipGetLastError());
    if (prof) {
        unsigned long long t[8] = {0};
        HIP_TRY(h, hipStreamSynchronize(st));
        HIP_TRY(h, hipMemcpy(t, d_prof, sizeof(t), hipMemcpyDeviceToHost));
        HIP_TRY(h, hipFree(d_prof));
        fprintf(stderr, "[syn train profile] cycles: features %llu forward %llu heads %llu backward %llu param-grads %llu\n",
                t[1] - t[0], t[2] - t[1], t[3] - t[2], t[4] - t[3], t[5] - t[4]);
    }
    return SYN_OK;
}

static int launch_adam(syn_engine* h, hipStream_t st, const float* d_grads, float lr, float grad_scale) {
    auto& L = h->learner;
    L.train_step += 1;
    const AdamScalars a = adam_scalars(L.train_hp, lr, L.train_step);
    if (L.trainer_kind == 1) {
        const int nc = ConvGeom::NUM_PARAMS;
        hipLaunchKernelGGL(adam_kernel, dim3((nc + 255) / 256), dim3(256), 0, st, L.d_tw, L.d_tm, L.d_tv, d_grads, nc, L.train_hp,
                           a.step_size, a.inv_sqrt_bc2, grad_scale);
    } else {
        const int n = TrainGeom::NUM_PARAMS;
        hipLaunchKernelGGL(adam_image_kernel, dim3((n + 255) / 256), dim3(256), 0, st, L.d_tw, L.d_tm, L.d_tv, d_grads, n, L.train_hp,
                           a.step_size, a.inv_sqrt_bc2, grad_scale, L.d_twimg, L.d_ttimg);
    }
    HIP_TRY(h, hipGetLastError());
    return SYN_OK;
}

int syn_train_gradients_device(syn_engine* h, const uint64_t* d_my_bb, const uint64_t* d_op_bb, const float* d_target_pi,
                               const float* d_target_v, int batch, float* d_grads, float* losses) {
    int rc = learner_check(h);
    if (rc != SYN_OK) return rc;
    if (batch < 1 || !d_my_bb || !d_op_bb || !d_target_pi || !d_target_v || !d_grads)
        return fail(h, SYN_ERR_INVALID_ARGUMENT, "bad arguments to syn_train_gradients_device");
    HIP_TRY(h, hipSetDevice(h->device));
    rc = launch_grads(h, h->stream, columns_of(d_my_bb, d_op_bb, nullptr, d_target_pi, d_target_v), batch, d_grads);
    if (rc != SYN_OK) return rc;
    if (losses) HIP_TRY(h, hipMemcpyAsync(losses, h->learner.d_tloss, 8, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return SYN_OK;
}

int syn_train_apply_device(syn_engine* h, const float* d_grads, float lr, float grad_scale) {
    int rc = learner_check(h);
    if (rc != SYN_OK) return rc;
    if (!d_grads) return fail(h, SYN_ERR_INVALID_ARGUMENT, "d_grads is NULL");
    HIP_TRY(h, hipSetDevice(h->device));
    rc = launch_adam(h, h->stream, d_grads, lr, grad_scale);
    if (rc != SYN_OK) return rc;
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return SYN_OK;
}

// The same two halves of a data-parallel step WITHOUT the host in between: both are enqueued on the caller's stream (the stream the
// batch was prepared on and the all-reduce runs on), nothing is synchronised, the two loss sums go to device memory — a step is
// gradients -> all-reduce -> Adam in one stream order. The caller keeps other trainer calls of this engine off other streams meanwhile.
int syn_train_gradients_enqueue(syn_engine* h, void* stream, const uint64_t* d_my_bb, const uint64_t* d_op_bb, const float* d_target_pi,
                                const float* d_target_v, int batch, float* d_grads, float* d_losses) {
    const int rc = learner_check(h);
    if (rc != SYN_OK) return rc;
    if (batch < 1 || !d_my_bb || !d_op_bb || !d_target_pi || !d_target_v || !d_grads)
        return fail(h, SYN_ERR_INVALID_ARGUMENT, "bad arguments to syn_train_gradients_enqueue");
    HIP_TRY(h, hipSetDevice(h->device));
    return launch_grads(h, static_cast<hipStream_t>(stream), columns_of(d_my_bb, d_op_bb, nullptr, d_target_pi, d_target_v), batch, d_grads, d_losses);
}

int syn_train_apply_enqueue(syn_engine* h, void* stream, const float* d_grads, float lr, float grad_scale) {
    const int rc = learner_check(h);
    if (rc != SYN_OK) return rc;
    if (!d_grads) return fail(h, SYN_ERR_INVALID_ARGUMENT, "d_grads is NULL");
    HIP_TRY(h, hipSetDevice(h->device));
    return launch_adam(h, static_cast<hipStream_t>(stream), d_grads, lr, grad_scale);
}

int syn_train_step(syn_engine* h, const uint64_t* my_bb, const uint64_t* op_bb, const float* target_pi,
                   const float* target_v, int batch, float lr, float* losses) {
    int rc = learner_check(h);
    if (rc != SYN_OK) return rc;
    if (batch < 1 || !my_bb || !op_bb || !target_pi || !target_v) return fail(h, SYN_ERR_INVALID_ARGUMENT, "bad arguments to syn_train_step");
    rc = check_micro_batch(h, batch);
    if (rc != SYN_OK) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    auto& L = h->learner;
    const size_t nb = (size_t)batch;
    rc = ensure_scratch(h, nb * POS_ROW_BYTES + 256);
    if (rc != SYN_OK) return rc;
    const PositionColumns staged = columns_at(h->d_scratch, nb, false);
    rc = copy_positions(h, staged, columns_of(my_bb, op_bb, nullptr, target_pi, target_v), nb, hipMemcpyHostToDevice);
    if (rc != SYN_OK) return rc;
    rc = launch_grads(h, h->stream, staged, batch, L.d_tgrad);
    if (rc != SYN_OK) return rc;
    rc = launch_adam(h, h->stream, L.d_tgrad, lr, 1.0f);
    if (rc != SYN_OK) return rc;
    if (losses) HIP_TRY(h, hipMemcpyAsync(losses, L.d_tloss, 8, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return SYN_OK;
}

// ---- epochs without the host in the loop: the de-duplicated buffer is uploaded once per iteration, an epoch is one call
int syn_train_set_data(syn_engine* h, const uint64_t* my_bb, const uint64_t* op_bb, const float* target_pi,
                       const float* target_v, size_t n) {
    int rc = learner_check(h);
    if (rc != SYN_OK) return rc;
    if (n < 1 || n > 0x7FFFFFFFu || !my_bb || !op_bb || !target_pi || !target_v)
        return fail(h, SYN_ERR_INVALID_ARGUMENT, "bad arguments to syn_train_set_data");
    HIP_TRY(h, hipSetDevice(h->device));
    rc = ensure_position_rows(h, h->learner.data, n, n);
    if (rc != SYN_OK) return rc;
    rc = copy_positions(h, columns_at(h->learner.data.d, n, false), columns_of(my_bb, op_bb, nullptr, target_pi, target_v), n, hipMemcpyHostToDevice);
    if (rc != SYN_OK) return rc;
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    h->learner.data.n = n;
    return SYN_OK;
}

// What syn_train_epoch's paths work on, all of it in d_scratch: the permutation, the per-step losses (2 per step), the epoch's batches
// in step order, the per-step Adam scalars' slot ([step_size n_steps][inv_sqrt_bc2 n_steps]) and 4 KB for diagnostic stamps.
struct EpochStage {
    int* d_perm;
    float* d_losses;
    PositionColumns batches;
    float* d_adam;
    unsigned long long* d_stamps;
};
// an epoch's arguments (n_steps == 0 is valid: the caller returns before it selects the device)
static int check_epoch(syn_engine* h, const int32_t* perm, size_t n_steps, int batch) {
    const int rc = learner_check(h);
    if (rc != SYN_OK) return rc;
    const size_t n = h->learner.data.n, ni = n_steps * (size_t)batch;
    if (n == 0) return fail(h, SYN_ERR_INVALID_ARGUMENT, "call syn_train_set_data first");
    if (batch < 1 || (n_steps > 0 && !perm) || ni > 0x7FFFFFFFu) return fail(h, SYN_ERR_INVALID_ARGUMENT, "bad arguments to syn_train_epoch");
    if (n_steps == 0) return SYN_OK;
    for (size_t i = 0; i < ni; i++)
        if (perm[i] < 0 || (size_t)perm[i] >= n)
            return fail(h, SYN_ERR_INVALID_ARGUMENT, "perm[%zu] = %d is outside the %zu uploaded states", i, perm[i], n);
    return SYN_OK;
}
// scratch: [perm ni x 4][losses n_steps x 8][step-ordered batches: my, op (8 B each), pi (36 B), v (12 B) per sample]
//          [per-step Adam scalars n_steps x 8][diagnostic stamps 4 KB]
struct EpochStageLayout {
    size_t perm_bytes, loss_bytes, batch_bytes;
    size_t bytes() const { return perm_bytes + loss_bytes + batch_bytes + loss_bytes + 4096; }
};
static EpochStageLayout epoch_stage_layout(size_t n_steps, int batch) {
    const size_t ni = n_steps * (size_t)batch;
    return {(ni * 4 + 255) & ~(size_t)255, (n_steps * 8 + 255) & ~(size_t)255, (ni * POS_ROW_BYTES + 255) & ~(size_t)255};
}
// the stage's pointers into the scratch at `base` (derived after ensure_scratch: the buffer may have moved)
static EpochStage epoch_stage_at(void* base, const EpochStageLayout& lay, size_t ni) {
    unsigned char* sc = static_cast<unsigned char*>(base);
    EpochStage st{};
    st.d_perm = reinterpret_cast<int*>(sc);
    st.d_losses = reinterpret_cast<float*>(sc + lay.perm_bytes);
    st.batches = columns_at(sc + lay.perm_bytes + lay.loss_bytes, ni, false);
    st.d_adam = reinterpret_cast<float*>(sc + lay.perm_bytes + lay.loss_bytes + lay.batch_bytes);
    st.d_stamps = reinterpret_cast<unsigned long long*>(sc + lay.perm_bytes + lay.loss_bytes + lay.batch_bytes + lay.loss_bytes);
    return st;
}
// "stage the step-ordered batches" from the caller's permutation: lays the scratch out and gathers the epoch's batches
static int stage_epoch(syn_engine* h, const int32_t* perm, size_t n_steps, int batch, EpochStage* st) {
    const size_t n = h->learner.data.n, ni = n_steps * (size_t)batch;
    const EpochStageLayout lay = epoch_stage_layout(n_steps, batch);
    const int rc = ensure_scratch(h, lay.bytes() + 256);
    if (rc != SYN_OK) return rc;
    *st = epoch_stage_at(h->d_scratch, lay, ni);
    HIP_TRY(h, hipMemcpyAsync(st->d_perm, perm, ni * 4, hipMemcpyHostToDevice, h->stream));
    // one gather for the whole epoch (the sampler's index_select), so a step reads its batch from consecutive addresses
    // instead of chasing perm -> sample inside the latency-bound step kernel
    const PositionColumns data = columns_at(h->learner.data.d, n, false);
    const PositionColumns g = st->batches;
    hipLaunchKernelGGL(train_gather_kernel, dim3((unsigned)((ni * 16 + 255) / 256)), dim3(256), 0, h->stream, st->d_perm, (int)ni, data.my,
                       data.op, data.pi, data.v, g.my, g.op, g.pi, g.v);
    HIP_TRY(h, hipGetLastError());
    return SYN_OK;
}

// the Adam scalars of the epoch's steps, as the persistent kernels read them from EpochStage::d_adam
static std::vector<float> epoch_adam_scalars(const syn_engine::Learner& L, float lr, size_t n_steps) {
    std::vector<float> sc(2 * n_steps);
    for (size_t s = 0; s < n_steps; s++) {
        const AdamScalars a = adam_scalars(L.train_hp, lr, L.train_step + (long long)s + 1);
        sc[s] = a.step_size;
        sc[n_steps + s] = a.inv_sqrt_bc2;
    }
    return sc;
}

// d_tsnap holds the learner as it was before a persistent epoch launch that may give up: [w][m][v] of the current network, then
// (Connect4Net only) its two fragment images.
struct SnapshotLayout {
    float* live[5];
    size_t bytes[5];
    int parts;
};
static SnapshotLayout snapshot_layout(const syn_engine::Learner& L) {
    const size_t pb = g_net_desc[L.trainer_kind].param_bytes();
    return {{L.d_tw, L.d_tm, L.d_tv, L.d_twimg, L.d_ttimg},
            {pb, pb, pb, (size_t)MlpGeom::IMG_FLOATS * 4, (size_t)TrainImg::T_FLOATS * 4},
            L.trainer_kind == 1 ? 3 : 5};
}
static int learner_snapshot(syn_engine* h) {
    const SnapshotLayout s = snapshot_layout(h->learner);
    unsigned char* sn = reinterpret_cast<unsigned char*>(h->learner.d_tsnap);
    for (int i = 0; i < s.parts; sn += s.bytes[i++])
        HIP_TRY(h, hipMemcpyAsync(sn, s.live[i], s.bytes[i], hipMemcpyDeviceToDevice, h->stream));
    return SYN_OK;
}
// the persistent launch gave up: the learner is put back for the path that runs the epoch instead, and the fallback is counted
static int learner_restore(syn_engine* h) {
    const SnapshotLayout s = snapshot_layout(h->learner);
    const unsigned char* sn = reinterpret_cast<const unsigned char*>(h->learner.d_tsnap);
    for (int i = 0; i < s.parts; sn += s.bytes[i++])
        HIP_TRY(h, hipMemcpyAsync(s.live[i], sn, s.bytes[i], hipMemcpyDeviceToDevice, h->stream));
    h->learner.epoch_fallbacks++;
    return SYN_OK;
}

// ---- SYN_TRAIN_PROFILE=1: the stamps of an epoch kernel's step 2, printed to stderr
// Connect4Net, workgroup g at [16 g ..]: top, features, forward L0..L4, heads, act-grads L4..L1, parameter jobs, step barrier
static void print_epoch_stamps(const unsigned long long* stamps, bool one_xcd) {
    fprintf(stderr, "[syn train profile] epoch kernel (%s), step 2, cycles per phase\n", one_xcd ? "workers on one XCD" : "device-scope barrier");
    for (int g = 0; g < EP_WGS; g++) {
        fprintf(stderr, "  wg %d (start %+lld):", g, (long long)(stamps[16 * g] - stamps[0]));
        for (int i = 1; i < 14; i++) fprintf(stderr, " %llu", stamps[16 * g + i] - stamps[16 * g + i - 1]);
        fprintf(stderr, " | probe fresh line %llu, cold line %llu\n", stamps[16 * g + 14], stamps[16 * g + 15]);
    }
}
static int print_conv_mw_stamps(syn_engine* h, const unsigned long long* d_stamps, bool one_xcd) {
    unsigned long long t[16 * CONV_MW_WGS] = {0};
    HIP_TRY(h, hipMemcpy(t, d_stamps, sizeof(t), hipMemcpyDeviceToHost));
    fprintf(stderr, "[syn train profile] conv epoch kernel on %d workgroups (%s), step 2, cycles: stage | F | barrier | H | G1 | G2 | Adam (own head weights, inside the barrier) | rest of the barrier | dY in | G3 | barrier | G4 + Adam (shared)\n",
            CONV_MW_WGS, one_xcd ? "one XCD" : "device-scope barrier");
    for (int g = 0; g < CONV_MW_WGS; g++) {
        fprintf(stderr, "  wg %d (start %+lld):", g, (long long)(t[16 * g] - t[0]));
        for (int i = 1; i < 13; i++) fprintf(stderr, " %llu", t[16 * g + i] - t[16 * g + i - 1]);
        fprintf(stderr, " | total %llu\n", t[16 * g + 12] - t[16 * g]);
    }
    return SYN_OK;
}
static int print_conv_stamps(syn_engine* h, const unsigned long long* d_stamps) {
    unsigned long long t[16] = {0};
    HIP_TRY(h, hipMemcpy(t, d_stamps, sizeof(t), hipMemcpyDeviceToHost));
    fprintf(stderr, "[syn train profile] conv epoch kernel, step 2, cycles: stage %llu | F %llu | H %llu | losses+G1 %llu | G2 %llu | G3 %llu | G4 %llu | Adam %llu | total %llu\n",
            t[1] - t[0], t[2] - t[1], t[3] - t[2], t[4] - t[3], t[5] - t[4], t[6] - t[5], t[7] - t[6], t[15] - t[7], t[15] - t[0]);
    return SYN_OK;
}

// Connect4Net, batch <= 32: ONE persistent launch for the whole epoch (train_epoch.cuh). *done = false: the kernel gave up, the learner
// is as it was before the call and the epoch is still to run.
static int epoch_persistent_mlp(syn_engine* h, const EpochStage& st, size_t n_steps, int batch, float lr, float* step_losses, bool* done) {
    auto& L = h->learner;
    *done = false;
    const bool prof = learner_knobs().profile;
    const std::vector<float> adam_sc = epoch_adam_scalars(L, lr, n_steps);
    unsigned status[4] = {0u, 0u, 0u, 0u};
    unsigned long long stamps[16 * EP_WGS] = {0};
    HIP_TRY(h, hipMemcpyAsync(st.d_adam, adam_sc.data(), adam_sc.size() * 4, hipMemcpyHostToDevice, h->stream));
    // snapshot of the learner (parameters, moments, both images: 0.85 MB of device copies): the launch below needs its 16
    // workgroups resident together; if it gives up (another kernel holds the CUs) the state is put back and the epoch runs
    // through the queued per-step launches instead — same bits, no co-residency requirement
    int rc = learner_snapshot(h);
    if (rc != SYN_OK) return rc;
    HIP_TRY(h, hipMemsetAsync(st.d_stamps, 0, 2048, h->stream));
    HIP_TRY(h, hipMemsetAsync(L.d_tsync, 0, 256, h->stream));
    float* img2 = L.d_timg2;
    float* timg2 = L.d_timg2 + MlpGeom::IMG_FLOATS;
    // both buffers start as the current network: the kernel rewrites every parameter's slot, never the padding
    HIP_TRY(h, hipMemcpyAsync(img2, L.d_twimg, (size_t)MlpGeom::IMG_FLOATS * 4, hipMemcpyDeviceToDevice, h->stream));
    HIP_TRY(h, hipMemcpyAsync(timg2, L.d_ttimg, (size_t)TrainImg::T_FLOATS * 4, hipMemcpyDeviceToDevice, h->stream));
    EpochParams ep{};
    ep.w = L.d_tw; ep.m = L.d_tm; ep.v = L.d_tv;
    ep.img[0] = L.d_twimg; ep.img[1] = img2;
    ep.timg[0] = L.d_ttimg; ep.timg[1] = timg2;
    ep.my_bb = st.batches.my; ep.op_bb = st.batches.op; ep.tpi = st.batches.pi; ep.tv = st.batches.v;
    ep.step_size = st.d_adam; ep.inv_sqrt_bc2 = st.d_adam + n_steps;
    ep.losses = st.d_losses; ep.grads = L.d_tgrad; ep.sync = L.d_tsync;
    ep.prof = prof ? st.d_stamps : nullptr;
    ep.n_steps = (int)n_steps; ep.batch = batch; ep.hp = L.train_hp;
    ep.force_device_scope = (learner_knobs().device_scope || L.epoch_device_scope) ? 1 : 0;
    const size_t lds = (size_t)TrainGeom::WL_OFF * 4;
    HIP_TRY(h, hipFuncSetAttribute(reinterpret_cast<const void*>(train_epoch_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(train_epoch_kernel, dim3(EP_WGS * EP_XCDS), dim3(EP_THREADS), lds, h->stream, ep);
    HIP_TRY(h, hipGetLastError());
    if (n_steps & 1) {  // the final network sits in the second buffer: bring the first one (the published image) up to date
        HIP_TRY(h, hipMemcpyAsync(L.d_twimg, img2, (size_t)MlpGeom::IMG_FLOATS * 4, hipMemcpyDeviceToDevice, h->stream));
        HIP_TRY(h, hipMemcpyAsync(L.d_ttimg, timg2, (size_t)TrainImg::T_FLOATS * 4, hipMemcpyDeviceToDevice, h->stream));
    }
    if (step_losses) HIP_TRY(h, hipMemcpyAsync(step_losses, st.d_losses, n_steps * 8, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipMemcpyAsync(status, L.d_tsync, 16, hipMemcpyDeviceToHost, h->stream));
    if (prof) HIP_TRY(h, hipMemcpyAsync(stamps, st.d_stamps, sizeof(stamps), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    // the workers were not resident together: put the learner back, the caller runs the epoch through the queued launches
    if (status[1] != 0u || epoch_force_abort()) return learner_restore(h);
    if (prof) print_epoch_stamps(stamps, status[3] != 0u);
    L.train_step += (long long)n_steps;
    *done = true;
    return SYN_OK;
}

// Connect4ConvNet, batch <= 32: gradients and Adam of every step in ONE launch (train_conv_mfma.cuh) — on four workgroups of one XCD
// where that kernel may run and does not give up, else in the one-workgroup kernel, which has no co-residency requirement.
static int epoch_persistent_conv(syn_engine* h, const EpochStage& st, size_t n_steps, int batch, float lr, float* step_losses) {
    auto& L = h->learner;
    const LearnerKnobs& knobs = learner_knobs();
    const std::vector<float> adam_sc = epoch_adam_scalars(L, lr, n_steps);
    HIP_TRY(h, hipMemcpyAsync(st.d_adam, adam_sc.data(), adam_sc.size() * 4, hipMemcpyHostToDevice, h->stream));
    ConvEpochParams ep{};
    ep.w = L.d_tw; ep.m = L.d_tm; ep.v = L.d_tv;
    ep.my_bb = st.batches.my; ep.op_bb = st.batches.op; ep.tpi = st.batches.pi; ep.tv = st.batches.v;
    ep.step_size = st.d_adam; ep.inv_sqrt_bc2 = st.d_adam + n_steps;
    ep.losses = st.d_losses; ep.grads = L.d_tgrad;
    ep.n_steps = (int)n_steps; ep.batch = batch; ep.hp = L.train_hp;
    const bool prof = knobs.profile && n_steps > 2;
    if (prof) HIP_TRY(h, hipMemsetAsync(st.d_stamps, 0, 128, h->stream));
    ep.prof = prof ? st.d_stamps : nullptr;
    // the step spread over four workgroups of one XCD (train_conv_epoch_kernel_mw: same chains, same bits, f32 and bf16). They must be
    // resident together: the learner is snapshotted first, and a launch that gives up (or SYN_DEBUG=1 SYN_TRAIN_CONV_MW=0, or a
    // failed start-up self-check) runs the one-workgroup kernel below instead.
    const bool want_mw = L.conv_mw_force >= 0 ? L.conv_mw_force == 1 : (!knobs.conv_mw_off && !L.conv_mw_disabled);
    if (want_mw) {
        int rc = learner_snapshot(h);
        if (rc != SYN_OK) return rc;
        HIP_TRY(h, hipMemsetAsync(L.d_tsync, 0, 256, h->stream));
        if (prof) HIP_TRY(h, hipMemsetAsync(st.d_stamps, 0, 512, h->stream));
        ConvMwParams mp{};
        mp.e = ep;
        mp.xbuf = L.d_cxbuf;
        mp.sync = L.d_tsync;
        mp.force_device_scope = knobs.device_scope ? 1 : 0;
        const size_t mlds = (size_t)ConvMwGeom::LDS_FLOATS * 4;
        auto km = L.train_bf16 ? train_conv_epoch_kernel_mw<true> : train_conv_epoch_kernel_mw<false>;
        HIP_TRY(h, hipFuncSetAttribute(reinterpret_cast<const void*>(km), hipFuncAttributeMaxDynamicSharedMemorySize, (int)mlds));
        hipLaunchKernelGGL(km, dim3(CONV_MW_WGS * CONV_MW_XCDS), dim3(CONV_TRAIN_THREADS), mlds, h->stream, mp);
        HIP_TRY(h, hipGetLastError());
        unsigned status[4] = {0u, 0u, 0u, 0u};
        HIP_TRY(h, hipMemcpyAsync(status, L.d_tsync, 16, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        if (status[1] == 0u && !epoch_force_abort()) {
            if (step_losses) HIP_TRY(h, hipMemcpy(step_losses, st.d_losses, n_steps * 8, hipMemcpyDeviceToHost));
            if (prof) rc = print_conv_mw_stamps(h, st.d_stamps, status[3] != 0u);
            if (rc != SYN_OK) return rc;
            L.train_step += (long long)n_steps;
            return SYN_OK;
        }
        rc = learner_restore(h);
        if (rc != SYN_OK) return rc;
        if (prof) HIP_TRY(h, hipMemsetAsync(st.d_stamps, 0, 128, h->stream));
    }
    const size_t clds = (size_t)ConvMfmaGeom::LDS_FLOATS * 4;
    auto ke = L.train_bf16 ? train_conv_epoch_kernel<true> : train_conv_epoch_kernel<false>;
    HIP_TRY(h, hipFuncSetAttribute(reinterpret_cast<const void*>(ke), hipFuncAttributeMaxDynamicSharedMemorySize, (int)clds));
    hipLaunchKernelGGL(ke, dim3(1), dim3(CONV_TRAIN_THREADS), clds, h->stream, ep);
    HIP_TRY(h, hipGetLastError());
    if (step_losses) HIP_TRY(h, hipMemcpyAsync(step_losses, st.d_losses, n_steps * 8, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (prof && !L.train_bf16) {
        const int rc = print_conv_stamps(h, st.d_stamps);
        if (rc != SYN_OK) return rc;
    }
    L.train_step += (long long)n_steps;
    return SYN_OK;
}

// Two launches per step (three in SYN_TRAIN_BATCH_MICRO: launch_grads is then blocks + reduce), queued and never synchronised in
// between (the weights of step s feed step s + 1): batches above 32 positions, a persistent kernel that gave up, the micro-batch
// mode, and SYN_DEBUG=1 SYN_TRAIN_QUEUED=1.
static int epoch_queued(syn_engine* h, const EpochStage& st, size_t n_steps, int batch, float lr, float* step_losses) {
    auto& L = h->learner;
    for (size_t s = 0; s < n_steps; s++) {
        const size_t o = s * (size_t)batch;
        int rc = launch_grads(h, h->stream, columns_from(st.batches, o), batch, L.d_tgrad, st.d_losses + 2 * s);
        if (rc != SYN_OK) return rc;
        rc = launch_adam(h, h->stream, L.d_tgrad, lr, 1.0f);
        if (rc != SYN_OK) return rc;
    }
    if (step_losses) HIP_TRY(h, hipMemcpyAsync(step_losses, st.d_losses, n_steps * 8, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return SYN_OK;
}

// "run the staged epoch": the n_steps optimiser steps over st.batches, whoever ordered them (the caller's permutation: stage_epoch; the
// device sampler: syn_train_epochs_sampled). Returns after the epoch: the stream is idle and the scratch may be staged again.
static int run_staged_epoch(syn_engine* h, const EpochStage& st, size_t n_steps, int batch, float lr, float* step_losses) {
    int rc = SYN_OK;
    // SYN_TRAIN_BATCH_MICRO: three queued launches per step (blocks, reduce, Adam) whatever the batch, one synchronisation at the end;
    // no workgroup waits for another, so there is no snapshot and never a persistent kernel
    if (h->learner.batch_mode == SYN_TRAIN_BATCH_MICRO) return epoch_queued(h, st, n_steps, batch, lr, step_losses);
    // One persistent launch for the whole epoch when the batch fits one 32-sample chunk — the reference's batch_size. Larger batches
    // queue two launches per step, as does a Connect4Net epoch whose persistent kernel gave up.
    const int kind = h->learner.trainer_kind;
    if (!learner_knobs().queued && kind == 1 && batch <= ConvTrainGeom::CHUNK)
        return epoch_persistent_conv(h, st, n_steps, batch, lr, step_losses);
    if (!learner_knobs().queued && kind == 0 && batch <= TrainGeom::CHUNK) {
        bool done = false;
        rc = epoch_persistent_mlp(h, st, n_steps, batch, lr, step_losses, &done);
        if (rc != SYN_OK || done) return rc;
    }
    return epoch_queued(h, st, n_steps, batch, lr, step_losses);
}

int syn_train_epoch(syn_engine* h, const int32_t* perm, size_t n_steps, int batch, float lr, float* step_losses) {
    int rc = check_epoch(h, perm, n_steps, batch);
    if (rc != SYN_OK || n_steps == 0) return rc;
    rc = check_micro_batch(h, batch);
    if (rc != SYN_OK) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    EpochStage st{};
    rc = stage_epoch(h, perm, n_steps, batch, &st);
    if (rc != SYN_OK) return rc;
    return run_staged_epoch(h, st, n_steps, batch, lr, step_losses);
}

// ---- the device-side epoch sampler (sampler_kernels.cuh; include/synthesis_amd.h syn_train_epochs_sampled)
// The sort's buffers for n rows: keys and row indices, in and out, and hipcub's temporary storage.
struct SamplerBuffers {
    unsigned long long* k_in;
    unsigned long long* k_out;
    int* i_in;
    int* i_out;
    void* tmp;
    size_t tmp_bytes;
};
static int sampler_bytes(syn_engine* h, size_t n, size_t* tmp_bytes, size_t* total) {
    *tmp_bytes = 0;
    HIP_TRY(h, hipcub::DeviceRadixSort::SortPairs(nullptr, *tmp_bytes, (const unsigned long long*)nullptr, (unsigned long long*)nullptr,
                                                  (const int*)nullptr, (int*)nullptr, (int)n, 0, 64, h->stream));
    *total = 2 * align256(n * 8) + 2 * align256(n * 4) + align256(*tmp_bytes);
    return SYN_OK;
}
static SamplerBuffers sampler_buffers_at(void* base, size_t n, size_t tmp_bytes) {
    unsigned char* b = static_cast<unsigned char*>(base);
    const size_t k = align256(n * 8), i = align256(n * 4);
    return {reinterpret_cast<unsigned long long*>(b), reinterpret_cast<unsigned long long*>(b + k), reinterpret_cast<int*>(b + 2 * k),
            reinterpret_cast<int*>(b + 2 * k + i), b + 2 * k + 2 * i, tmp_bytes};
}
// epoch `epoch`'s order on the stream: B.i_out = perm_e, B.k_out = the keys in that order (bit 0 = the row's flip flag)
static int enqueue_sampler(syn_engine* h, const SamplerBuffers& B, uint64_t key, uint32_t epoch, size_t n) {
    const int ni = (int)n;
    hipLaunchKernelGGL(sampler_keys_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, sampler_epoch_key(key, epoch), ni,
                       B.k_in, B.i_in);
    HIP_TRY(h, hipGetLastError());
    size_t tmp = B.tmp_bytes;
    HIP_TRY(h, hipcub::DeviceRadixSort::SortPairs(B.tmp, tmp, B.k_in, B.k_out, B.i_in, B.i_out, ni, 0, 64, h->stream));
    return SYN_OK;
}

int syn_train_epochs_sampled(syn_engine* h, const syn_sampler_config* cfg, int n_epochs, int batch, float lr, float* step_losses,
                             size_t* n_steps_out) {
    int rc = learner_check(h);
    if (rc != SYN_OK) return rc;
    if (n_steps_out) *n_steps_out = 0;
    if (!cfg) return fail(h, SYN_ERR_INVALID_ARGUMENT, "syn_train_epochs_sampled: cfg is NULL");
    if (cfg->flip != SYN_SAMPLER_FLIP_NONE && cfg->flip != SYN_SAMPLER_FLIP_RANDOM)
        return fail(h, SYN_ERR_INVALID_ARGUMENT, "syn_train_epochs_sampled: unknown flip mode %d", cfg->flip);
    if (n_epochs < 0 || batch < 1) return fail(h, SYN_ERR_INVALID_ARGUMENT, "syn_train_epochs_sampled: n_epochs = %d, batch = %d", n_epochs, batch);
    if ((uint64_t)cfg->first_epoch + (uint64_t)n_epochs > (1ull << 32))
        return fail(h, SYN_ERR_INVALID_ARGUMENT, "syn_train_epochs_sampled: epochs %u + %d run past 2^32", cfg->first_epoch, n_epochs);
    const size_t n = h->learner.data.n;
    if (n == 0) return fail(h, SYN_ERR_INVALID_ARGUMENT, "call syn_train_set_data first");
    const size_t n_steps = n / (size_t)batch, ni = n_steps * (size_t)batch;
    if (n_epochs == 0 || n_steps == 0) return SYN_OK;
    rc = check_micro_batch(h, batch);
    if (rc != SYN_OK) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    // one scratch for the whole call: the epoch's stage, then the sort's buffers; every pointer is derived after the one ensure_scratch
    // (nothing below it grows the scratch), and epoch e + 1 is staged over epoch e's once run_staged_epoch has returned
    const EpochStageLayout lay = epoch_stage_layout(n_steps, batch);
    size_t tmp_bytes = 0, sort_bytes = 0;
    rc = sampler_bytes(h, n, &tmp_bytes, &sort_bytes);
    if (rc != SYN_OK) return rc;
    const size_t o_sort = align256(lay.bytes());
    rc = ensure_scratch(h, o_sort + sort_bytes + 256);
    if (rc != SYN_OK) return rc;
    EpochStage st = epoch_stage_at(h->d_scratch, lay, ni);
    const SamplerBuffers B = sampler_buffers_at(static_cast<unsigned char*>(h->d_scratch) + o_sort, n, tmp_bytes);
    st.d_perm = B.i_out;
    const PositionColumns data = columns_at(h->learner.data.d, n, false);
    for (int e = 0; e < n_epochs; e++) {
        rc = enqueue_sampler(h, B, cfg->key, cfg->first_epoch + (uint32_t)e, n);
        if (rc != SYN_OK) return rc;
        hipLaunchKernelGGL(sampler_gather_kernel, dim3((unsigned)((ni * 16 + 255) / 256)), dim3(256), 0, h->stream, B.k_out, B.i_out, (int)ni,
                           (int)n, cfg->flip == SYN_SAMPLER_FLIP_RANDOM ? 1 : 0, data.my, data.op, data.pi, data.v, st.batches.my,
                           st.batches.op, st.batches.pi, st.batches.v);
        HIP_TRY(h, hipGetLastError());
        rc = run_staged_epoch(h, st, n_steps, batch, lr, step_losses ? step_losses + (size_t)e * n_steps * 2 : nullptr);
        if (rc != SYN_OK) return rc;
    }
    if (n_steps_out) *n_steps_out = n_steps;
    return SYN_OK;
}

int syn_debug_sampler(syn_engine* h, const syn_sampler_config* cfg, uint32_t epoch, size_t n, int32_t* perm_out, uint8_t* flip_out) {
    if (!h) return SYN_ERR_INVALID_ARGUMENT;
    if (!cfg || n < 1 || n > 0x7FFFFFFFu) return fail(h, SYN_ERR_INVALID_ARGUMENT, "bad arguments to syn_debug_sampler");
    HIP_TRY(h, hipSetDevice(h->device));
    size_t tmp_bytes = 0, sort_bytes = 0;
    int rc = sampler_bytes(h, n, &tmp_bytes, &sort_bytes);
    if (rc != SYN_OK) return rc;
    rc = ensure_scratch(h, sort_bytes + align256(n) + 256);
    if (rc != SYN_OK) return rc;
    const SamplerBuffers B = sampler_buffers_at(h->d_scratch, n, tmp_bytes);
    unsigned char* d_flip = static_cast<unsigned char*>(h->d_scratch) + sort_bytes;
    rc = enqueue_sampler(h, B, cfg->key, epoch, n);
    if (rc != SYN_OK) return rc;
    hipLaunchKernelGGL(sampler_flags_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, sampler_epoch_key(cfg->key, epoch),
                       (int)n, d_flip);
    HIP_TRY(h, hipGetLastError());
    if (perm_out) HIP_TRY(h, hipMemcpyAsync(perm_out, B.i_out, n * 4, hipMemcpyDeviceToHost, h->stream));
    if (flip_out) HIP_TRY(h, hipMemcpyAsync(flip_out, d_flip, n, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return SYN_OK;
}

int syn_trainer_get_state(syn_engine* h, float* blob, float* m, float* v, long long* step, float* grads) {
    const int rc = learner_check(h);
    if (rc != SYN_OK) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    auto& L = h->learner;
    const size_t bytes = g_net_desc[L.trainer_kind].param_bytes();
    if (blob) HIP_TRY(h, hipMemcpyAsync(blob, L.d_tw, bytes, hipMemcpyDeviceToHost, h->stream));
    if (m) HIP_TRY(h, hipMemcpyAsync(m, L.d_tm, bytes, hipMemcpyDeviceToHost, h->stream));
    if (v) HIP_TRY(h, hipMemcpyAsync(v, L.d_tv, bytes, hipMemcpyDeviceToHost, h->stream));
    if (grads) HIP_TRY(h, hipMemcpyAsync(grads, L.d_tgrad, bytes, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (step) *step = L.train_step;
    return SYN_OK;
}

// The inverse of syn_trainer_get_state: parameters, moments and step count of an initialised trainer, and the images derived from the
// parameters as syn_trainer_init builds them. Everything is checked (and Connect4Net's images are built) before the first copy is queued.
int syn_trainer_set_state(syn_engine* h, const float* blob, const float* m, const float* v, size_t n_floats, long long step) {
    int rc = learner_check(h);
    if (rc != SYN_OK) return rc;
    auto& L = h->learner;
    const NetDesc& d = g_net_desc[L.trainer_kind];
    if (!blob || !m || !v) return fail(h, SYN_ERR_INVALID_ARGUMENT, "syn_trainer_set_state: blob/m/v is NULL");
    if (n_floats != (size_t)d.num_params)
        return fail(h, SYN_ERR_INVALID_ARGUMENT, "the trainer's %s has %d parameters, got %zu", d.name, d.num_params, n_floats);
    if (step < 0) return fail(h, SYN_ERR_INVALID_ARGUMENT, "syn_trainer_set_state: step is negative (%lld)", step);
    HIP_TRY(h, hipSetDevice(h->device));
    std::vector<float> img, timg;
    if (L.trainer_kind == 0) {
        rc = build_trainer_images(h, blob, img, timg);
        if (rc != SYN_OK) return rc;
        HIP_TRY(h, hipMemcpyAsync(L.d_twimg, img.data(), img.size() * 4, hipMemcpyHostToDevice, h->stream));
        HIP_TRY(h, hipMemcpyAsync(L.d_ttimg, timg.data(), timg.size() * 4, hipMemcpyHostToDevice, h->stream));
        // (the epoch kernel copies both into its second buffer before every launch; it is set here all the same, so that no image of
        //  the trainer describes another network)
        HIP_TRY(h, hipMemcpyAsync(L.d_timg2, img.data(), img.size() * 4, hipMemcpyHostToDevice, h->stream));
        HIP_TRY(h, hipMemcpyAsync(L.d_timg2 + MlpGeom::IMG_FLOATS, timg.data(), timg.size() * 4, hipMemcpyHostToDevice, h->stream));
    }
    HIP_TRY(h, hipMemcpyAsync(L.d_tw, blob, d.param_bytes(), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipMemcpyAsync(L.d_tm, m, d.param_bytes(), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipMemcpyAsync(L.d_tv, v, d.param_bytes(), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    L.train_step = step;
    return SYN_OK;
}

// weight hand-off learner -> self-play (the reference does it through models/model_i.ot, alpha_zero.rs:97,194)
int syn_trainer_publish_weights(syn_engine* h) {
    const int rc = learner_check(h);
    if (rc != SYN_OK) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    const int cap_rc = require_lane_cap_of_network(h, h->learner.trainer_kind);
    return cap_rc != SYN_OK ? cap_rc : install_network(h, h->learner.trainer_kind, nullptr);
}

// ------------------------------------------------------------------------------------------------ deduplicate
// The device core of ReplayBuffer::deduplicate (data.rs:196-235): n positions at device pointers -> the unique states in ascending
// (my_bb, op_bb) order, targets summed in buffer order. `work` is the caller's scratch of dedup_layout(n, tmp, mirror).total bytes with
// tmp from dedup_tmp_bytes; the outputs point into it. Stream-ordered on h->stream with ONE synchronise in the middle (the number of
// unique states sizes the reduce's grid).
struct DedupOut {
    PositionColumns rows{};
    unsigned* num = nullptr;
    int m = 0;       // unique (with mirror: canonical) states, rows [0, m)
    int total = 0;   // rows in all: m, with mirror m + the mirror images of the classes that are not self-symmetric
};
// hipcub's temporary storage for the core's sorts and scans over n positions
static int dedup_tmp_bytes(syn_engine* h, size_t n, bool mirror, size_t* tmp_bytes) {
    const int ni = (int)n;
    size_t tmp_sort = 0, tmp_scan = 0;
    HIP_TRY(h, hipcub::DeviceRadixSort::SortPairs(nullptr, tmp_sort, (const unsigned long long*)nullptr,
                                                  (unsigned long long*)nullptr, (const unsigned*)nullptr,
                                                  (unsigned*)nullptr, ni, 0, 64, h->stream));
    HIP_TRY(h, hipcub::DeviceScan::InclusiveSum(nullptr, tmp_scan, (const unsigned*)nullptr, (unsigned*)nullptr, ni,
                                                h->stream));
    *tmp_bytes = tmp_sort > tmp_scan ? tmp_sort : tmp_scan;
    if (mirror) {
        size_t tmp_excl = 0;
        HIP_TRY(h, hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_excl, (const unsigned*)nullptr, (unsigned*)nullptr, ni, h->stream));
        if (tmp_excl > *tmp_bytes) *tmp_bytes = tmp_excl;
    }
    return SYN_OK;
}
// The number of set words among n 0/1 flags whose exclusive scan is in `ranks`: the last rank and the last flag to the host, ONE
// synchronise. A further device word (`d_also`) rides along in the same synchronise.
static int read_flag_count(syn_engine* h, const unsigned* flags, const unsigned* ranks, int n, size_t* count, const unsigned* d_also = nullptr,
                           unsigned* also = nullptr) {
    unsigned last[2] = {0, 0};
    HIP_TRY(h, hipMemcpyAsync(&last[0], ranks + (n - 1), 4, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipMemcpyAsync(&last[1], flags + (n - 1), 4, hipMemcpyDeviceToHost, h->stream));
    if (d_also) HIP_TRY(h, hipMemcpyAsync(also, d_also, 4, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    *count = (size_t)last[0] + last[1];
    return SYN_OK;
}
// the scan as well: flags -> ranks with hipcub's temporary storage at `tmp`, then the count
static int count_flags(syn_engine* h, void* tmp, size_t tmp_bytes, const unsigned* flags, unsigned* ranks, int n, size_t* count) {
    HIP_TRY(h, hipcub::DeviceScan::ExclusiveSum(tmp, tmp_bytes, flags, ranks, n, h->stream));
    return read_flag_count(h, flags, ranks, n, count);
}
static int dedup_device_core(syn_engine* h, char* work, size_t tmp, const unsigned long long* d_my, const unsigned long long* d_op,
                             const float* d_pi, const float* d_v, size_t n, DedupOut* out, bool mirror = false) {
    const int ni = (int)n;
    const DedupLayout lay = dedup_layout(n, tmp, mirror);
    const size_t rows = lay.rows;
    const size_t o_k0 = lay.k0, o_k1 = lay.k1, o_i0 = lay.i0, o_i1 = lay.i1, o_head = lay.head, o_scan = lay.scan, o_start = lay.start;
    const size_t o_on = lay.out_num, o_tmp = lay.tmp, o_cmy = lay.c_my, o_cop = lay.c_op, o_flip = lay.flip, o_exp = lay.expand, o_dst = lay.dst;
    char* base = work;
    const PositionColumns O = columns_in(base, lay.out);
    auto P8 = [&](size_t o) { return reinterpret_cast<unsigned long long*>(base + o); };
    auto P4 = [&](size_t o) { return reinterpret_cast<unsigned*>(base + o); };
    const int blocks = (ni + 255) / 256;
    const unsigned long long* in_my = d_my;
    const unsigned long long* in_op = d_op;
    if (mirror) {
        // symmetric: every record in its canonical orientation first, so that the sort still runs over n keys; from here on the
        // keys are the canonical boards and the records' own boards are not read again
        hipLaunchKernelGGL(replay_canonicalise_kernel, dim3(blocks), dim3(256), 0, h->stream, in_my, in_op, ni, P8(o_cmy), P8(o_cop),
                           P4(o_flip));
        d_my = P8(o_cmy);
        d_op = P8(o_cop);
    }
    // stable LSD sort of the buffer indices by the 128-bit key: first by op_bb, then by my_bb
    hipLaunchKernelGGL(iota_kernel, dim3(blocks), dim3(256), 0, h->stream, P4(o_i0), ni);
    size_t t1 = tmp;
    HIP_TRY(h, hipcub::DeviceRadixSort::SortPairs(base + o_tmp, t1, d_op, P8(o_k0), P4(o_i0), P4(o_i1), ni, 0, 64,
                                                  h->stream));
    hipLaunchKernelGGL(gather_u64_kernel, dim3(blocks), dim3(256), 0, h->stream, d_my, P4(o_i1), ni, P8(o_k1));
    t1 = tmp;
    HIP_TRY(h, hipcub::DeviceRadixSort::SortPairs(base + o_tmp, t1, P8(o_k1), P8(o_k0), P4(o_i1), P4(o_i0), ni, 0, 64,
                                                  h->stream));
    // o_k0 = my_bb sorted, o_i0 = buffer indices in (my, op, index) order; op_bb in that order:
    hipLaunchKernelGGL(gather_u64_kernel, dim3(blocks), dim3(256), 0, h->stream, d_op, P4(o_i0), ni, P8(o_k1));
    hipLaunchKernelGGL(dedup_heads_kernel, dim3(blocks), dim3(256), 0, h->stream, P8(o_k0), P8(o_k1), ni, P4(o_head));
    t1 = tmp;
    HIP_TRY(h, hipcub::DeviceScan::InclusiveSum(base + o_tmp, t1, P4(o_head), P4(o_scan), ni, h->stream));
    hipLaunchKernelGGL(dedup_starts_kernel, dim3(blocks), dim3(256), 0, h->stream, P4(o_head), P4(o_scan), ni,
                       P4(o_start));
    unsigned m_u = 0;
    HIP_TRY(h, hipMemcpyAsync(&m_u, P4(o_scan) + (ni - 1), 4, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    const int m = (int)m_u;
    int total = m;
    if (!mirror) {
        hipLaunchKernelGGL(dedup_reduce_kernel, dim3((m * 16 + 255) / 256), dim3(256), 0, h->stream, P4(o_i0), P4(o_start),
                           m, ni, d_my, d_op, d_pi, d_v, O.my, O.op, O.pi, O.v, P4(o_on));
        HIP_TRY(h, hipGetLastError());
    } else if (m > 0) {
        const dim3 rows16((unsigned)(((size_t)m * 16 + 255) / 256));
        hipLaunchKernelGGL(dedup_reduce_mirror_kernel, rows16, dim3(256), 0, h->stream, P4(o_i0), P4(o_start), m, ni, d_my, d_op,
                           P4(o_flip), d_pi, d_v, O.my, O.op, O.pi, O.v, P4(o_on), P4(o_exp));
        HIP_TRY(h, hipGetLastError());
        // rows [m, m + M): the mirror images of the classes that are not self-symmetric, in class order
        size_t extra = 0;
        if (const int rc = count_flags(h, base + o_tmp, tmp, P4(o_exp), P4(o_dst), m, &extra)) return rc;
        if (extra > (size_t)m) return fail(h, SYN_ERR_HIP, "%zu mirror images for %d canonical states", extra, m);
        hipLaunchKernelGGL(dedup_expand_mirror_kernel, rows16, dim3(256), 0, h->stream, P4(o_exp), P4(o_dst), m, rows, O.my,
                           O.op, O.pi, O.v, P4(o_on));
        HIP_TRY(h, hipGetLastError());
        total = m + (int)extra;
    }
    out->rows = O;
    out->num = P4(o_on);
    out->m = m;
    out->total = total;
    return SYN_OK;
}

// the rows of the symmetric forms are counted in an int like the plain ones: 2n must fit
constexpr size_t DEDUP_MIRROR_MAX_N = 0x3FFFFFFFu;

// (the entry points have selected the engine's device)
static int replay_deduplicate_host(syn_engine* h, const char* who, bool mirror, const uint64_t* my_bb, const uint64_t* op_bb,
                                   const float* pis, const float* vs, size_t n, uint64_t* out_my, uint64_t* out_op, float* out_pi,
                                   float* out_v, uint32_t* out_num, size_t* out_canonical, size_t* out_count) {
    if (!h) return SYN_ERR_INVALID_ARGUMENT;
    if (!out_count) return fail(h, SYN_ERR_INVALID_ARGUMENT, "out_count is NULL");
    *out_count = 0;
    if (out_canonical) *out_canonical = 0;
    if (n == 0) return SYN_OK;
    if (!my_bb || !op_bb || !pis || !vs || !out_my || !out_op || !out_pi || !out_v || !out_num ||
        n > (mirror ? DEDUP_MIRROR_MAX_N : (size_t)0x7FFFFFFFu))
        return fail(h, SYN_ERR_INVALID_ARGUMENT, "bad arguments to %s", who);
    // device layout: inputs | the core's work area
    size_t tmp = 0;
    int rc = dedup_tmp_bytes(h, n, mirror, &tmp);
    if (rc != SYN_OK) return rc;
    Carve c;
    const ColumnOffsets staged = carve_columns(c, n);
    const size_t o_work = c.at;
    rc = ensure_scratch(h, o_work + dedup_layout(n, tmp, mirror).total + 256);
    if (rc != SYN_OK) return rc;
    char* base = static_cast<char*>(h->d_scratch);
    const PositionColumns in = columns_in(base, staged);
    rc = copy_positions(h, in, columns_of(my_bb, op_bb, nullptr, pis, vs), n, hipMemcpyHostToDevice);
    if (rc != SYN_OK) return rc;
    DedupOut o;
    rc = dedup_device_core(h, base + o_work, tmp, in.my, in.op, in.pi, in.v, n, &o, mirror);
    if (rc != SYN_OK) return rc;
    const size_t m = (size_t)o.total;
    rc = copy_positions(h, columns_of(out_my, out_op, nullptr, out_pi, out_v), o.rows, m, hipMemcpyDeviceToHost);
    if (rc != SYN_OK) return rc;
    HIP_TRY(h, hipMemcpyAsync(out_num, o.num, m * 4, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    *out_count = m;
    if (out_canonical) *out_canonical = (size_t)o.m;
    return SYN_OK;
}

int syn_replay_deduplicate(syn_engine* h, const uint64_t* my_bb, const uint64_t* op_bb, const float* pis,
                           const float* vs, size_t n, uint64_t* out_my, uint64_t* out_op, float* out_pi, float* out_v,
                           uint32_t* out_num, size_t* out_count) {
    if (!h) return SYN_ERR_INVALID_ARGUMENT;
    HIP_TRY(h, hipSetDevice(h->device));
    return replay_deduplicate_host(h, "syn_replay_deduplicate", false, my_bb, op_bb, pis, vs, n, out_my, out_op, out_pi, out_v, out_num,
                                   nullptr, out_count);
}

int syn_replay_deduplicate_symmetric(syn_engine* h, const uint64_t* my_bb, const uint64_t* op_bb, const float* pis, const float* vs,
                                     size_t n, uint64_t* out_my, uint64_t* out_op, float* out_pi, float* out_v, uint32_t* out_num,
                                     size_t* out_canonical, size_t* out_count) {
    if (!h) return SYN_ERR_INVALID_ARGUMENT;
    if (!out_canonical) return fail(h, SYN_ERR_INVALID_ARGUMENT, "out_canonical is NULL");
    HIP_TRY(h, hipSetDevice(h->device));
    return replay_deduplicate_host(h, "syn_replay_deduplicate_symmetric", true, my_bb, op_bb, pis, vs, n, out_my, out_op, out_pi, out_v,
                                   out_num, out_canonical, out_count);
}

int syn_positions_mirror(syn_engine* h, const uint64_t* my_bb, const uint64_t* op_bb, const float* pis, size_t n, uint64_t* out_my,
                         uint64_t* out_op, float* out_pi) {
    if (!h) return SYN_ERR_INVALID_ARGUMENT;
    if (n == 0) return SYN_OK;
    if (!my_bb || !op_bb || !out_my || !out_op || (pis != nullptr) != (out_pi != nullptr) || n > 0x7FFFFFFFu)
        return fail(h, SYN_ERR_INVALID_ARGUMENT, "bad arguments to syn_positions_mirror");
    HIP_TRY(h, hipSetDevice(h->device));
    // device layout: my | op | pi | mirrored my | op | pi
    Carve c;
    const ColumnOffsets o_in = carve_columns(c, n, pis != nullptr, false), o_out = carve_columns(c, n, pis != nullptr, false);
    int rc = ensure_scratch(h, c.at + 256);
    if (rc != SYN_OK) return rc;
    const PositionColumns in = columns_in(h->d_scratch, o_in), mirrored = columns_in(h->d_scratch, o_out);
    rc = copy_positions(h, in, columns_of(my_bb, op_bb, nullptr, pis, nullptr), n, hipMemcpyHostToDevice);
    if (rc != SYN_OK) return rc;
    const size_t threads = pis ? n * POS_PI_FLOATS : n;
    hipLaunchKernelGGL(replay_mirror_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, h->stream, in.my, in.op, in.pi, (int)n,
                       mirrored.my, mirrored.op, mirrored.pi);
    HIP_TRY(h, hipGetLastError());
    rc = copy_positions(h, columns_of(out_my, out_op, nullptr, out_pi, nullptr), mirrored, n, hipMemcpyDeviceToHost);
    if (rc != SYN_OK) return rc;
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return SYN_OK;
}

// ------------------------------------------------------------------------------------------------ device-resident replay buffer
// (data.rs:107-235 on the device; kernels in replay_kernels.cuh). Everything is ordered on h->stream; the host waits only where a
// count has to reach it.
// The buffer is columns_at(h->d_replay, h->replay_cap, true): my | op | gid | pi | v, 72 bytes a position.
// The last syn_selfplay_run's positions, compacted to `dst` (room for `room` positions): exclusive sum of plies, the total to the
// host (one synchronise), then one wave per game. Nothing is written when the total does not fit (SYN_ERR_CAPACITY).
static int replay_compact_last_selfplay(syn_engine* h, long long first_gid, const PositionColumns& dst, size_t room, size_t* n_out) {
    *n_out = 0;
    if (h->last_selfplay_games < 0)
        return fail(h, SYN_ERR_INVALID_ARGUMENT, "no syn_selfplay_run has completed on this engine: there are no positions to compact");
    const int ng = h->last_selfplay_games;
    if (ng == 0) return SYN_OK;
    size_t tmp = 0;
    HIP_TRY(h, hipcub::DeviceScan::ExclusiveSum(nullptr, tmp, (const int*)nullptr, (unsigned*)nullptr, ng, h->stream));
    const size_t off_bytes = align256((size_t)ng * 4);
    int rc = ensure_scratch(h, off_bytes + tmp + 256);
    if (rc != SYN_OK) return rc;
    unsigned* d_off = static_cast<unsigned*>(h->d_scratch);
    HIP_TRY(h, hipcub::DeviceScan::ExclusiveSum(static_cast<char*>(h->d_scratch) + off_bytes, tmp, h->d_plies, d_off, ng, h->stream));
    unsigned last_off = 0;
    int last_plies = 0;
    HIP_TRY(h, hipMemcpyAsync(&last_off, d_off + (ng - 1), 4, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipMemcpyAsync(&last_plies, h->d_plies + (ng - 1), 4, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    const size_t total = (size_t)last_off + (size_t)(last_plies > 0 ? last_plies : 0);
    if (total > room)
        return fail(h, SYN_ERR_CAPACITY, "the last self-play launch has %zu positions, there is room for %zu", total, room);
    if (total) {
        hipLaunchKernelGGL(replay_compact_kernel, dim3((unsigned)(((size_t)ng * 64 + 255) / 256)), dim3(256), 0, h->stream, h->d_plies,
                           d_off, ng, h->d_states, h->d_pis, h->d_vs, first_gid, (unsigned long long)room, dst.my, dst.op, dst.gid,
                           dst.pi, dst.v);
        HIP_TRY(h, hipGetLastError());
    }
    *n_out = total;
    return SYN_OK;
}

int syn_replay_reserve(syn_engine* h, size_t capacity_positions) {
    if (!h) return SYN_ERR_INVALID_ARGUMENT;
    if (capacity_positions > 0x7FFFFFFFu) return fail(h, SYN_ERR_INVALID_ARGUMENT, "a replay buffer holds at most 2^31 - 1 positions");
    if (capacity_positions <= h->replay_cap) return SYN_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    unsigned char* fresh = nullptr;
    HIP_TRY(h, hipMalloc(&fresh, capacity_positions * POS_ROW_GID_BYTES));
    if (h->replay_n) {
        int rc = copy_positions(h, columns_at(fresh, capacity_positions, true), columns_at(h->d_replay, h->replay_cap, true), h->replay_n,
                                hipMemcpyDeviceToDevice);
        if (rc != SYN_OK) {
            (void)hipFree(fresh);
            return rc;
        }
    }
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    (void)hipFree(h->d_replay);
    (void)hipFree(h->d_replay_alt);   // (the keep-window's second buffer follows the capacity: allocated again when next needed)
    h->d_replay = fresh;
    h->d_replay_alt = nullptr;
    h->replay_cap = capacity_positions;
    return SYN_OK;
}

int syn_replay_clear(syn_engine* h) {
    if (!h) return SYN_ERR_INVALID_ARGUMENT;
    HIP_TRY(h, hipSetDevice(h->device));   // (like every entry point of a handle; appends in flight are ordered before later ones by the stream)
    h->replay_n = 0;
    return SYN_OK;
}

int syn_replay_size(syn_engine* h, size_t* n_positions) {
    if (!h) return SYN_ERR_INVALID_ARGUMENT;
    if (!n_positions) return fail(h, SYN_ERR_INVALID_ARGUMENT, "n_positions is NULL");
    HIP_TRY(h, hipSetDevice(h->device));
    *n_positions = h->replay_n;
    return SYN_OK;
}

int syn_selfplay_positions_device(syn_engine* h, int64_t first_gid, uint64_t* d_my, uint64_t* d_op, int64_t* d_gid, float* d_pi,
                                  float* d_v, size_t capacity, size_t* n_positions) {
    if (!h) return SYN_ERR_INVALID_ARGUMENT;
    if (!n_positions) return fail(h, SYN_ERR_INVALID_ARGUMENT, "n_positions is NULL");
    *n_positions = 0;
    if (capacity && (!d_my || !d_op || !d_gid || !d_pi || !d_v))
        return fail(h, SYN_ERR_INVALID_ARGUMENT, "bad arguments to syn_selfplay_positions_device");
    HIP_TRY(h, hipSetDevice(h->device));
    int rc = replay_compact_last_selfplay(h, (long long)first_gid, columns_of(d_my, d_op, d_gid, d_pi, d_v), capacity, n_positions);
    if (rc != SYN_OK) return rc;
    HIP_TRY(h, hipStreamSynchronize(h->stream));   // the sections belong to the caller, who reads them on a stream of their own
    return SYN_OK;
}

int syn_replay_append_selfplay(syn_engine* h, int64_t first_gid, size_t* n_appended) {
    if (!h) return SYN_ERR_INVALID_ARGUMENT;
    if (n_appended) *n_appended = 0;
    HIP_TRY(h, hipSetDevice(h->device));
    size_t n = 0;
    int rc = replay_compact_last_selfplay(h, (long long)first_gid, columns_from(columns_at(h->d_replay, h->replay_cap, true), h->replay_n),
                                          h->replay_cap - h->replay_n, &n);
    if (rc != SYN_OK) return rc;
    h->replay_n += n;
    if (n_appended) *n_appended = n;
    return SYN_OK;
}

static int replay_append_impl(syn_engine* h, const PositionColumns& src, size_t n, hipMemcpyKind kind) {
    if (n == 0) return SYN_OK;
    if (!src.my || !src.op || !src.gid || !src.pi || !src.v) return fail(h, SYN_ERR_INVALID_ARGUMENT, "a section pointer is NULL");
    if (n > h->replay_cap - h->replay_n)
        return fail(h, SYN_ERR_CAPACITY, "%zu positions do not fit: the replay buffer holds %zu of %zu (syn_replay_reserve)", n,
                    h->replay_n, h->replay_cap);
    int rc = copy_positions(h, columns_from(columns_at(h->d_replay, h->replay_cap, true), h->replay_n), src, n, kind);
    if (rc != SYN_OK) return rc;
    if (kind == hipMemcpyHostToDevice) HIP_TRY(h, hipStreamSynchronize(h->stream));   // pageable host memory: the caller may reuse it
    h->replay_n += n;
    return SYN_OK;
}

int syn_replay_append_device(syn_engine* h, const uint64_t* d_my, const uint64_t* d_op, const int64_t* d_gid, const float* d_pi,
                             const float* d_v, size_t n) {
    if (!h) return SYN_ERR_INVALID_ARGUMENT;
    HIP_TRY(h, hipSetDevice(h->device));
    return replay_append_impl(h, columns_of(d_my, d_op, d_gid, d_pi, d_v), n, hipMemcpyDeviceToDevice);
}

int syn_replay_append(syn_engine* h, const uint64_t* my_bb, const uint64_t* op_bb, const int64_t* gid, const float* pis, const float* vs,
                      size_t n) {
    if (!h) return SYN_ERR_INVALID_ARGUMENT;
    HIP_TRY(h, hipSetDevice(h->device));
    return replay_append_impl(h, columns_of(my_bb, op_bb, gid, pis, vs), n, hipMemcpyHostToDevice);
}

int syn_replay_keep_games_from(syn_engine* h, int64_t min_gid) {
    if (!h) return SYN_ERR_INVALID_ARGUMENT;
    const size_t n = h->replay_n;
    if (n == 0) return SYN_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    const int ni = (int)n;
    size_t tmp = 0;
    HIP_TRY(h, hipcub::DeviceScan::ExclusiveSum(nullptr, tmp, (const unsigned*)nullptr, (unsigned*)nullptr, ni, h->stream));
    Carve c;   // keep flags | their ranks | cub temp
    const size_t o_keep = c.take(n * 4), o_dst = c.take(n * 4), o_tmp = c.at;
    int rc = ensure_scratch(h, o_tmp + tmp + 256);
    if (rc != SYN_OK) return rc;
    char* sc = static_cast<char*>(h->d_scratch);
    unsigned* d_keep = reinterpret_cast<unsigned*>(sc + o_keep);
    unsigned* d_dst = reinterpret_cast<unsigned*>(sc + o_dst);
    const PositionColumns cur = columns_at(h->d_replay, h->replay_cap, true);
    hipLaunchKernelGGL(replay_keep_flags_kernel, dim3((ni + 255) / 256), dim3(256), 0, h->stream, cur.gid, ni, (long long)min_gid,
                       d_keep);
    HIP_TRY(h, hipGetLastError());
    size_t kept = 0;
    rc = count_flags(h, sc + o_tmp, tmp, d_keep, d_dst, ni, &kept);
    if (rc != SYN_OK) return rc;
    if (kept == n) return SYN_OK;   // nothing to drop: the buffer stays where it is
    if (kept == 0) {
        h->replay_n = 0;
        return SYN_OK;
    }
    // stable scatter into the second buffer, which then becomes the buffer
    if (!h->d_replay_alt) HIP_TRY(h, hipMalloc(&h->d_replay_alt, h->replay_cap * POS_ROW_GID_BYTES));
    const PositionColumns alt = columns_at(h->d_replay_alt, h->replay_cap, true);
    auto U = [](const void* p) { return reinterpret_cast<const unsigned*>(p); };
    auto W = [](void* p) { return reinterpret_cast<unsigned*>(p); };
    hipLaunchKernelGGL(replay_keep_scatter_kernel, dim3((unsigned)((n * 9 + 255) / 256), 5), dim3(256), 0, h->stream, d_keep, d_dst, ni,
                       U(cur.my), U(cur.op), U(cur.gid), U(cur.pi), U(cur.v), W(alt.my), W(alt.op), W(alt.gid), W(alt.pi), W(alt.v));
    HIP_TRY(h, hipGetLastError());
    unsigned char* t = h->d_replay;
    h->d_replay = h->d_replay_alt;
    h->d_replay_alt = t;
    h->replay_n = kept;
    return SYN_OK;
}

int syn_replay_read(syn_engine* h, uint64_t* my_bb, uint64_t* op_bb, int64_t* gid, float* pis, float* vs, size_t capacity,
                    size_t* n_positions) {
    if (!h) return SYN_ERR_INVALID_ARGUMENT;
    if (n_positions) *n_positions = h->replay_n;
    if (h->replay_n > capacity)
        return fail(h, SYN_ERR_CAPACITY, "the replay buffer holds %zu positions, the caller's arrays %zu", h->replay_n, capacity);
    HIP_TRY(h, hipSetDevice(h->device));
    int rc = copy_positions(h, columns_of(my_bb, op_bb, gid, pis, vs), columns_at(h->d_replay, h->replay_cap, true), h->replay_n,
                            hipMemcpyDeviceToHost);
    if (rc != SYN_OK) return rc;
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return SYN_OK;
}

// ------------------------------------------------------------------------------------------------ reanalyse
// syn_replay_reanalyse (include/synthesis_amd.h "Reanalyse"; kernels in reanalyse_kernels.cuh): the selected rows of the buffer are
// compacted into job arrays, searched in chunks by the MODE_SEARCH kernels (as run_games drives them: roots and results stay on
// the device) and rewritten by the write-back kernel. The scratch is position_layout.hpp's reanalyse_layout.
// The selection that syn_replay_reanalyse and syn_replay_select_positions share: the flags kernel over the n stored rows (n >= 1), the
// exclusive scan of the selected flags, the sum of the skipped ones, and both counts to the host in one synchronise. The job arrays are
// not filled yet: the caller checks its capacity and launches the compaction.
struct ReanalyseSelection {
    unsigned *d_sel, *d_dst, *d_job_row, *d_moved, *d_done, *d_counts;
    unsigned long long *d_job_my, *d_job_op;
    void* d_tmp;
    DevSearchResult* d_res;
    size_t tmp_sum;        // hipcub's temporary bytes for a DeviceReduce::Sum over n words
    PositionColumns R;     // the buffer's columns (the ones syn_replay_read reads)
    dim3 grid_rows;        // one thread per stored row, blocks of 256
    size_t sel_n;
    unsigned skipped;
};
static int reanalyse_select(syn_engine* h, const char* who, uint64_t key, uint64_t threshold, int64_t before_gid, size_t chunk_rows,
                            ReanalyseSelection* S) {
    const size_t n = h->replay_n;
    const int ni = (int)n;
    size_t tmp_scan = 0, tmp_sum = 0;
    HIP_TRY(h, hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_scan, (const unsigned*)nullptr, (unsigned*)nullptr, ni, h->stream));
    HIP_TRY(h, hipcub::DeviceReduce::Sum(nullptr, tmp_sum, (const unsigned*)nullptr, (unsigned*)nullptr, ni, h->stream));
    const ReanalyseLayout L = reanalyse_layout(n, std::max(tmp_scan, tmp_sum), chunk_rows);
    if (const int rc = ensure_scratch(h, L.total)) return rc;
    unsigned char* const base = static_cast<unsigned char*>(h->d_scratch);
    const auto u32_at = [base](size_t o) { return reinterpret_cast<unsigned*>(base + o); };
    S->d_sel = u32_at(L.sel);
    unsigned* const d_skip = u32_at(L.skip);
    S->d_dst = u32_at(L.dst);
    S->d_job_my = reinterpret_cast<unsigned long long*>(base + L.job_my);
    S->d_job_op = reinterpret_cast<unsigned long long*>(base + L.job_op);
    S->d_job_row = u32_at(L.job_row);
    S->d_moved = u32_at(L.moved);
    S->d_done = u32_at(L.done);
    S->d_counts = u32_at(L.counts);
    S->d_tmp = base + L.tmp;
    S->d_res = reinterpret_cast<DevSearchResult*>(base + L.results);
    S->tmp_sum = tmp_sum;
    S->R = columns_at(h->d_replay, h->replay_cap, true);
    S->grid_rows = dim3((unsigned)((n + 255) / 256));
    hipLaunchKernelGGL(reanalyse_flags_kernel, S->grid_rows, dim3(256), 0, h->stream, S->R.gid, S->R.my, S->R.op, ni,
                       (unsigned long long)key ^ REANALYSE_TAG, (unsigned long long)threshold, (long long)before_gid, S->d_sel, d_skip);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipcub::DeviceScan::ExclusiveSum(S->d_tmp, tmp_scan, S->d_sel, S->d_dst, ni, h->stream));
    HIP_TRY(h, hipcub::DeviceReduce::Sum(S->d_tmp, tmp_sum, d_skip, S->d_counts, ni, h->stream));
    S->skipped = 0;
    if (const int rc = read_flag_count(h, S->d_sel, S->d_dst, ni, &S->sel_n, S->d_counts, &S->skipped)) return rc;
    if (S->sel_n > n) return fail(h, SYN_ERR_HIP, "%s: %zu rows selected out of %zu", who, S->sel_n, n);
    return SYN_OK;
}

int syn_replay_reanalyse(syn_engine* h, const syn_mcts_config* mcts, const syn_reanalyse_config* cfg, syn_reanalyse_stats* out,
                         int64_t* selected_rows, size_t capacity) {
    if (!h) return SYN_ERR_INVALID_ARGUMENT;
    HIP_TRY(h, hipSetDevice(h->device));   // (selecting the device changes nothing of the engine: the refusals follow)
    if (out) std::memset(out, 0, sizeof(*out));
    // ---- everything that can refuse the call, before anything of the engine or the device changes
    if (!mcts || !cfg) return fail(h, SYN_ERR_INVALID_ARGUMENT, "syn_replay_reanalyse: mcts or cfg is NULL");
    if (cfg->threshold > (1ull << 32))
        return fail(h, SYN_ERR_INVALID_ARGUMENT, "syn_replay_reanalyse: threshold %llu exceeds 2^32", (unsigned long long)cfg->threshold);
    if (!(cfg->value_mix >= 0.0f && cfg->value_mix <= 1.0f))
        return fail(h, SYN_ERR_INVALID_ARGUMENT, "syn_replay_reanalyse: value_mix must be in [0, 1], got %g", (double)cfg->value_mix);
    if (cfg->chunk_roots < 0) return fail(h, SYN_ERR_INVALID_ARGUMENT, "syn_replay_reanalyse: chunk_roots must be >= 0, got %d", cfg->chunk_roots);
    if (cfg->action_selection != SYN_ACTION_Q && cfg->action_selection != SYN_ACTION_NUM_VISITS)
        return fail(h, SYN_ERR_INVALID_ARGUMENT, "unknown action selection %d", cfg->action_selection);
    DevMctsCfg m{};
    int rc = convert_mcts(h, mcts, m);
    if (rc != SYN_OK) return rc;
    EngineParams P;
    rc = common_params(h, P, cfg->explores);
    if (rc != SYN_OK) return rc;
    P.mcts = m;
    if ((rc = check_lane_only(h, P.mcts)) != SYN_OK) return rc;
    if (!h->d_replay || h->replay_cap == 0)
        return fail(h, SYN_ERR_INVALID_ARGUMENT, "syn_replay_reanalyse: no replay buffer is reserved (syn_replay_reserve)");
    const size_t n = h->replay_n;
    if (n == 0 || cfg->threshold == 0) return SYN_OK;

    // ---- selection: flags, scan, the counts to the host
    const int ni = (int)n;
    const size_t chunk_max = cfg->chunk_roots > 0 ? (size_t)cfg->chunk_roots : std::max((size_t)65536, (size_t)h->slots);
    const size_t chunk_rows = std::min(chunk_max, n);
    ReanalyseSelection S{};
    rc = reanalyse_select(h, "syn_replay_reanalyse", cfg->key, cfg->threshold, cfg->before_gid, chunk_rows, &S);
    if (rc != SYN_OK) return rc;
    const size_t sel_n = S.sel_n;
    size_t tmp_sum = S.tmp_sum;
    unsigned* const d_job_row = S.d_job_row;
    unsigned* const d_moved = S.d_moved;
    unsigned* const d_done = S.d_done;
    unsigned* const d_counts = S.d_counts;
    void* const d_tmp = S.d_tmp;
    DevSearchResult* const d_res = S.d_res;
    const PositionColumns R = S.R;
    const dim3 block(256), grid_rows = S.grid_rows;
    int launches = 1;   // the flags kernel
    if (selected_rows && sel_n > capacity)
        return fail(h, SYN_ERR_CAPACITY, "syn_replay_reanalyse: %zu rows are selected, selected_rows has room for %zu", sel_n, capacity);
    h->last_kernel_ms = 0.0f;
    h->last_launches = launches;
    h->last_cache_hits = h->last_cache_misses = 0;
    if (out) {
        out->rows = n;
        out->skipped = S.skipped;
        out->launches = (uint32_t)launches;
    }
    if (sel_n == 0) return SYN_OK;
    hipLaunchKernelGGL(reanalyse_compact_kernel, grid_rows, block, 0, h->stream, S.d_sel, S.d_dst, ni, (unsigned)n, R.my, R.op, S.d_job_my,
                       S.d_job_op, d_job_row);
    HIP_TRY(h, hipGetLastError());
    launches++;
    HIP_TRY(h, hipMemsetAsync(d_moved, 0, sel_n * 4, h->stream));
    HIP_TRY(h, hipMemsetAsync(d_done, 0, sel_n * 4, h->stream));
    std::vector<unsigned> rows32;
    if (selected_rows) {
        rows32.resize(sel_n);
        HIP_TRY(h, hipMemcpyAsync(rows32.data(), d_job_row, sel_n * 4, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        for (size_t j = 0; j < sel_n; j++) selected_rows[j] = (int64_t)rows32[j];
    }

    // ---- per chunk: the search on job_my + c0 / job_op + c0, the write-back, the error word
    const int v_mode = cfg->value_mix == 0.0f ? REANALYSE_V_KEEP : (cfg->value_mix == 1.0f ? REANALYSE_V_STORE : REANALYSE_V_MIX);
    P.roll.num_explores = cfg->explores;
    P.action_selection = cfg->action_selection;
    P.first_game = 0;
    P.results = d_res;
    CallScope scope(h, (int)std::min(sel_n, chunk_rows));
    float kernel_ms = 0.0f;
    unsigned long long hits = 0, misses = 0;
    uint32_t chunks = 0;
    int status = SYN_OK;
    for (size_t c0 = 0; c0 < sel_n; c0 += chunk_rows) {
        const int jobs = (int)std::min(chunk_rows, sel_n - c0);
        // (a syn_cancel's word does not survive the next chunk's reset: the loop itself stops at the first chunk that ends after it)
        HIP_TRY(h, hipMemsetAsync(h->d_job_next, 0, 64, h->stream));
        if (c0 == 0) HIP_TRY(h, scope.armed());
        HIP_TRY(h, hipMemsetAsync(h->d_cache_stats, 0, 16, h->stream));
        // a root that syn_cancel kept from being searched reads as all zeros: the write-back leaves its row alone
        HIP_TRY(h, hipMemsetAsync(d_res, 0, (size_t)jobs * sizeof(DevSearchResult), h->stream));
        EngineParams Q = P;
        Q.n_jobs = jobs;
        Q.in_my = S.d_job_my + c0;
        Q.in_op = S.d_job_op + c0;
        Q.base_seed = cfg->stream_base + (unsigned long long)c0;
        HIP_TRY(h, hipEventRecord(h->ev0, h->stream));
        if (const int lrc = launch_engine(h, Q, jobs, MODE_SEARCH, false, false)) return lrc;
        HIP_TRY(h, hipEventRecord(h->ev1, h->stream));
        hipLaunchKernelGGL(reanalyse_writeback_kernel, dim3((unsigned)(((size_t)jobs * 16 + 255) / 256)), block, 0, h->stream,
                           reinterpret_cast<const unsigned*>(d_res), jobs, d_job_row + c0, (unsigned)n, v_mode, cfg->value_mix,
                           h->d_job_next + 8, R.pi, R.v, d_moved + c0, d_done + c0);
        HIP_TRY(h, hipGetLastError());
        int kerr = 0;
        unsigned long long cstats[2] = {0, 0};
        HIP_TRY(h, hipMemcpyAsync(&kerr, h->d_job_next + 8, 4, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipMemcpyAsync(cstats, h->d_cache_stats, 16, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        float ms = 0.0f;
        HIP_TRY(h, hipEventElapsedTime(&ms, h->ev0, h->ev1));
        kernel_ms += ms;
        launches += 2;   // the search and the write-back
        chunks++;
        hits += cstats[0];
        misses += cstats[1];
        h->last_kernel_ms = kernel_ms;
        h->last_launches = launches;
        h->last_cache_hits = hits;
        h->last_cache_misses = misses;
        if (const int rc = fail_search_error(h, kerr, "; the rows of this chunk and of the later ones keep their old targets")) return rc;
        if (scope.cancelled()) {
            status = SYN_ERR_CANCELLED;
            break;
        }
    }
    // ---- the counts: moved flags, and after a cancel the rows that were searched
    HIP_TRY(h, hipcub::DeviceReduce::Sum(d_tmp, tmp_sum, d_moved, d_counts + 1, (int)sel_n, h->stream));
    HIP_TRY(h, hipcub::DeviceReduce::Sum(d_tmp, tmp_sum, d_done, d_counts + 2, (int)sel_n, h->stream));
    unsigned tail[2] = {0, 0};
    HIP_TRY(h, hipMemcpyAsync(tail, d_counts + 1, 8, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (out) {
        out->selected = sel_n;
        out->moved = tail[0];
        out->chunks = chunks;
        out->launches = (uint32_t)launches;
    }
    if (status == SYN_ERR_CANCELLED && (size_t)tail[1] < sel_n)
        return fail(h, SYN_ERR_CANCELLED, "cancelled by syn_cancel: %zu of %zu selected rows were not searched and keep their old targets",
                    sel_n - (size_t)tail[1], sel_n);
    return SYN_OK;
}

// syn_replay_select_positions (include/synthesis_amd.h "Recorded games"): syn_replay_reanalyse's selection alone (reanalyse_select and
// the compaction) and a download of the selected positions, 16 bytes each. The buffer is read, never written.
int syn_replay_select_positions(syn_engine* h, uint64_t key, uint64_t threshold, int64_t before_gid, uint64_t* my_bb, uint64_t* op_bb,
                                size_t capacity, size_t* n_selected, size_t* n_skipped) {
    if (!h) return SYN_ERR_INVALID_ARGUMENT;
    HIP_TRY(h, hipSetDevice(h->device));
    if (n_selected) *n_selected = 0;
    if (n_skipped) *n_skipped = 0;
    if (!n_selected) return fail(h, SYN_ERR_INVALID_ARGUMENT, "syn_replay_select_positions: n_selected is NULL");
    if (threshold > (1ull << 32))
        return fail(h, SYN_ERR_INVALID_ARGUMENT, "syn_replay_select_positions: threshold %llu exceeds 2^32", (unsigned long long)threshold);
    if (capacity && (!my_bb || !op_bb)) return fail(h, SYN_ERR_INVALID_ARGUMENT, "syn_replay_select_positions: my_bb or op_bb is NULL");
    if (!h->d_replay || h->replay_cap == 0)
        return fail(h, SYN_ERR_INVALID_ARGUMENT, "syn_replay_select_positions: no replay buffer is reserved (syn_replay_reserve)");
    const size_t n = h->replay_n;
    if (n == 0 || threshold == 0) return SYN_OK;
    ReanalyseSelection S{};
    if (const int rc = reanalyse_select(h, "syn_replay_select_positions", key, threshold, before_gid, 0, &S)) return rc;
    const size_t sel_n = S.sel_n;
    *n_selected = sel_n;
    if (n_skipped) *n_skipped = S.skipped;
    if (sel_n > capacity)
        return fail(h, SYN_ERR_CAPACITY, "syn_replay_select_positions: %zu rows are selected, the arrays have room for %zu", sel_n, capacity);
    if (sel_n == 0) return SYN_OK;
    hipLaunchKernelGGL(reanalyse_compact_kernel, S.grid_rows, dim3(256), 0, h->stream, S.d_sel, S.d_dst, (int)n, (unsigned)n, S.R.my, S.R.op,
                       S.d_job_my, S.d_job_op, S.d_job_row);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipMemcpyAsync(my_bb, S.d_job_my, sel_n * POS_BOARD_BYTES, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipMemcpyAsync(op_bb, S.d_job_op, sel_n * POS_BOARD_BYTES, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return SYN_OK;
}

// syn_replay_deduplicate_to_trainer[_symmetric] with games held out (syn_replay_set_holdout; replay_kernels.cuh "holding games out"):
// the buffer is stably partitioned by the games' flag into a second set of sections, the de-duplication core runs on either part, the
// part that is not held out becomes the learner's data set and the held-out part, its unseen rows first, the evaluation set. Scratch:
//   [the partitioned rows: my | op | pi | v of n][flags of 2n][ranks of 2n][cub temp][the core's work area, sized for the larger part]
// (the caller has checked the trainer, n >= 1 and the symmetric form's bound)
static int replay_deduplicate_holdout(syn_engine* h, bool mirror, size_t* n_canonical, size_t* n_unique) {
    auto& E = h->evalset;
    const size_t n = h->replay_n;
    const int ni = (int)n;
    const size_t rows_max = mirror ? 2 * n : n;   // rows of a de-duplicated part
    size_t tmp_scan = 0;
    HIP_TRY(h, hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_scan, (const unsigned*)nullptr, (unsigned*)nullptr, (int)rows_max, h->stream));
    Carve c;
    const size_t o_part = c.take(n * POS_ROW_BYTES), o_flag = c.take(rows_max * 4), o_rank = c.take(rows_max * 4), o_tmp = c.take(tmp_scan);
    const size_t o_work = c.at;
    int rc = ensure_scratch(h, o_work + 4096);
    if (rc != SYN_OK) return rc;
    const PositionColumns cur = columns_at(h->d_replay, h->replay_cap, true);
    auto U = [](const void* p) { return reinterpret_cast<const unsigned*>(p); };
    auto W = [](void* p) { return reinterpret_cast<unsigned*>(p); };
    // ---- the split by game: flags and their ranks (enqueued; run again if the scratch buffer has to grow for the work area)
    auto flags_and_ranks = [&]() -> int {
        char* b = static_cast<char*>(h->d_scratch);
        hipLaunchKernelGGL(replay_holdout_flags_kernel, dim3((ni + 255) / 256), dim3(256), 0, h->stream, cur.gid, ni,
                           (unsigned long long)(E.holdout_key ^ HOLDOUT_TAG), (unsigned long long)E.holdout_threshold,
                           reinterpret_cast<unsigned*>(b + o_flag));
        HIP_TRY(h, hipGetLastError());
        size_t t = tmp_scan;
        HIP_TRY(h, hipcub::DeviceScan::ExclusiveSum(b + o_tmp, t, reinterpret_cast<unsigned*>(b + o_flag), reinterpret_cast<unsigned*>(b + o_rank), ni,
                                                    h->stream));
        return SYN_OK;
    };
    rc = flags_and_ranks();
    if (rc != SYN_OK) return rc;
    size_t n_held = 0;
    rc = read_flag_count(h, reinterpret_cast<unsigned*>(static_cast<char*>(h->d_scratch) + o_flag),
                         reinterpret_cast<unsigned*>(static_cast<char*>(h->d_scratch) + o_rank), ni, &n_held);
    if (rc != SYN_OK) return rc;
    if (n_held > n) return fail(h, SYN_ERR_HIP, "internal: %zu of %zu positions held out", n_held, n);
    const size_t n_train = n - n_held;
    if (n_train == 0)
        return fail(h, SYN_ERR_INVALID_ARGUMENT, "the holdout threshold holds out every game of the buffer: the learner would have no data set");
    size_t tmp_t = 0, tmp_h = 0;
    rc = dedup_tmp_bytes(h, n_train, mirror, &tmp_t);
    if (rc == SYN_OK && n_held > 0) rc = dedup_tmp_bytes(h, n_held, mirror, &tmp_h);
    if (rc != SYN_OK) return rc;
    const size_t work_t = dedup_layout(n_train, tmp_t, mirror).total, work_h = n_held > 0 ? dedup_layout(n_held, tmp_h, mirror).total : 0;
    const size_t need = o_work + (work_t > work_h ? work_t : work_h) + 4096;
    if (need > h->scratch_bytes) {
        rc = ensure_scratch(h, need);
        if (rc == SYN_OK) rc = flags_and_ranks();
        if (rc != SYN_OK) return rc;
    }
    char* sc = static_cast<char*>(h->d_scratch);
    unsigned* d_flag = reinterpret_cast<unsigned*>(sc + o_flag);
    unsigned* d_rank = reinterpret_cast<unsigned*>(sc + o_rank);
    const PositionColumns part = columns_at(sc + o_part, n, false);
    hipLaunchKernelGGL(replay_partition_scatter_kernel, dim3((unsigned)((n * 9 + 255) / 256), 4), dim3(256), 0, h->stream, d_flag, d_rank, ni,
                       (unsigned)n_train, U(cur.my), U(cur.op), U(cur.pi), U(cur.v), W(part.my), W(part.op), W(part.pi), W(part.v));
    HIP_TRY(h, hipGetLastError());
    // ---- the learner's data set: the part that is not held out
    DedupOut o;
    rc = dedup_device_core(h, sc + o_work, tmp_t, part.my, part.op, part.pi, part.v, n_train, &o, mirror);
    if (rc != SYN_OK) return rc;
    const size_t m = (size_t)o.total, m_canonical = (size_t)o.m;
    if (m == 0) return fail(h, SYN_ERR_HIP, "the de-duplication of %zu positions reported no unique state", n_train);
    rc = ensure_position_rows(h, h->learner.data, m, m + m / 4);
    if (rc != SYN_OK) return rc;
    const PositionColumns tr = columns_at(h->learner.data.d, m, false);
    rc = copy_positions(h, tr, o.rows, m, hipMemcpyDeviceToDevice);
    if (rc != SYN_OK) return rc;
    h->learner.data.n = m;
    if (n_unique) *n_unique = m;
    if (n_canonical) *n_canonical = m_canonical;
    // ---- the evaluation set: the held-out part, its unseen rows first
    E.rows.n = E.n_unseen = 0;
    if (n_held == 0) return SYN_OK;
    const PositionColumns held = columns_from(part, n_train);
    DedupOut e;
    rc = dedup_device_core(h, sc + o_work, tmp_h, held.my, held.op, held.pi, held.v, n_held, &e, mirror);
    if (rc != SYN_OK) return rc;
    const size_t me = (size_t)e.total;
    if (me == 0 || me > rows_max) return fail(h, SYN_ERR_HIP, "the de-duplication of %zu held-out positions reported %zu rows", n_held, me);
    rc = ensure_position_rows(h, E.rows, me, me + me / 4);
    if (rc != SYN_OK) return rc;
    // seen = the state (symmetric: its canonical form) is among the learner's rows [0, m_canonical): sorted ascending by (my, op)
    const int mei = (int)me;
    hipLaunchKernelGGL(replay_seen_flags_kernel, dim3((mei + 255) / 256), dim3(256), 0, h->stream, e.rows.my, e.rows.op, mei, tr.my, tr.op,
                       (int)m_canonical, mirror ? 1 : 0, d_flag);
    HIP_TRY(h, hipGetLastError());
    size_t n_seen = 0;
    rc = count_flags(h, sc + o_tmp, tmp_scan, d_flag, d_rank, mei, &n_seen);
    if (rc != SYN_OK) return rc;
    if (n_seen > me) return fail(h, SYN_ERR_HIP, "internal: %zu of %zu held-out rows seen", n_seen, me);
    const PositionColumns ev = columns_at(E.rows.d, me, false);
    hipLaunchKernelGGL(replay_partition_scatter_kernel, dim3((unsigned)((me * 9 + 255) / 256), 4), dim3(256), 0, h->stream, d_flag, d_rank, mei,
                       (unsigned)(me - n_seen), U(e.rows.my), U(e.rows.op), U(e.rows.pi), U(e.rows.v), W(ev.my), W(ev.op), W(ev.pi), W(ev.v));
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    E.rows.n = me;
    E.n_unseen = me - n_seen;
    return SYN_OK;
}

// (the entry points have selected the engine's device)
static int replay_deduplicate_to_trainer(syn_engine* h, bool mirror, size_t* n_canonical, size_t* n_unique) {
    if (!h) return SYN_ERR_INVALID_ARGUMENT;
    if (n_unique) *n_unique = 0;
    if (n_canonical) *n_canonical = 0;
    if (!h->learner.has_trainer) return fail(h, SYN_ERR_NO_WEIGHTS, "call syn_trainer_init first");
    const size_t n = h->replay_n;
    if (n == 0) return fail(h, SYN_ERR_INVALID_ARGUMENT, "the replay buffer is empty");
    if (mirror && n > DEDUP_MIRROR_MAX_N)
        return fail(h, SYN_ERR_INVALID_ARGUMENT, "the symmetric de-duplication takes at most %zu positions", DEDUP_MIRROR_MAX_N);
    if (h->evalset.holdout_threshold != 0) return replay_deduplicate_holdout(h, mirror, n_canonical, n_unique);
    size_t tmp = 0;
    int rc = dedup_tmp_bytes(h, n, mirror, &tmp);
    if (rc != SYN_OK) return rc;
    rc = ensure_scratch(h, dedup_layout(n, tmp, mirror).total + 256);
    if (rc != SYN_OK) return rc;
    const PositionColumns cur = columns_at(h->d_replay, h->replay_cap, true);
    DedupOut o;
    rc = dedup_device_core(h, static_cast<char*>(h->d_scratch), tmp, cur.my, cur.op, cur.pi, cur.v, n, &o, mirror);
    if (rc != SYN_OK) return rc;
    const size_t m = (size_t)o.total;   // (with mirror: the canonical rows and their mirror images, all of them the learner's)
    if (m == 0) return fail(h, SYN_ERR_HIP, "the de-duplication of %zu positions reported no unique state", n);
    // the unique set becomes the learner's data set (the state syn_train_set_data leaves): syn_train_epoch stages in d_scratch too,
    // so it moves to the learner's own buffer before this call returns
    rc = ensure_position_rows(h, h->learner.data, m, m + m / 4);   // (the unique count drifts from iteration to iteration: do not reallocate for every rise)
    if (rc != SYN_OK) return rc;
    rc = copy_positions(h, columns_at(h->learner.data.d, m, false), o.rows, m, hipMemcpyDeviceToDevice);
    if (rc != SYN_OK) return rc;
    h->learner.data.n = m;
    if (n_unique) *n_unique = m;
    if (n_canonical) *n_canonical = (size_t)o.m;
    return SYN_OK;
}

int syn_replay_set_holdout(syn_engine* h, uint64_t key, uint64_t threshold) {
    if (!h) return SYN_ERR_INVALID_ARGUMENT;
    if (threshold > (1ull << 32)) return fail(h, SYN_ERR_INVALID_ARGUMENT, "the holdout threshold is at most 2^32 (got %llu)", (unsigned long long)threshold);
    HIP_TRY(h, hipSetDevice(h->device));   // (as every entry point that belongs to a device: the next call's kernels read these two words)
    h->evalset.holdout_key = key;
    h->evalset.holdout_threshold = threshold;
    return SYN_OK;
}

int syn_replay_deduplicate_to_trainer(syn_engine* h, size_t* n_unique) {
    if (!h) return SYN_ERR_INVALID_ARGUMENT;
    HIP_TRY(h, hipSetDevice(h->device));
    return replay_deduplicate_to_trainer(h, false, nullptr, n_unique);
}

int syn_replay_deduplicate_to_trainer_symmetric(syn_engine* h, size_t* n_canonical, size_t* n_total) {
    if (!h) return SYN_ERR_INVALID_ARGUMENT;
    HIP_TRY(h, hipSetDevice(h->device));
    return replay_deduplicate_to_trainer(h, true, n_canonical, n_total);
}

int syn_train_get_data(syn_engine* h, uint64_t* my_bb, uint64_t* op_bb, float* target_pi, float* target_v, size_t capacity,
                       size_t* n) {
    const int rc = learner_check(h);
    if (rc != SYN_OK) return rc;
    const size_t m = h->learner.data.n;
    if (n) *n = m;
    if (m > capacity) return fail(h, SYN_ERR_CAPACITY, "the learner's data set has %zu states, the caller's arrays %zu", m, capacity);
    if (m == 0) return SYN_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    if (const int crc = copy_positions(h, columns_of(my_bb, op_bb, nullptr, target_pi, target_v), columns_at(h->learner.data.d, m, false), m,
                                       hipMemcpyDeviceToHost))
        return crc;
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return SYN_OK;
}

// ------------------------------------------------------------------------------------------------ held-out evaluation
// (dataset_eval.cuh; include/synthesis_amd.h "Held-out evaluation")
static_assert(sizeof(DsBlockRecord) == 32 && sizeof(DsChunkSum) == 40 && sizeof(DsTotals) == 40, "dataset_eval.cuh's records");
static_assert((size_t)ConvGeom::NUM_PARAMS <= (size_t)MlpGeom::IMG_FLOATS, "the evaluation's image buffer holds either network");

int syn_dataset_set(syn_engine* h, const uint64_t* my_bb, const uint64_t* op_bb, const float* target_pi, const float* target_v, size_t n) {
    if (!h) return SYN_ERR_INVALID_ARGUMENT;
    if (n > 0x7FFFFFFFu || (n > 0 && (!my_bb || !op_bb || !target_pi || !target_v)))
        return fail(h, SYN_ERR_INVALID_ARGUMENT, "bad arguments to syn_dataset_set");
    HIP_TRY(h, hipSetDevice(h->device));
    auto& E = h->evalset;
    if (n == 0) {
        E.rows.n = E.n_unseen = 0;
        return SYN_OK;
    }
    int rc = ensure_position_rows(h, E.rows, n, n);
    if (E.rows.n == 0) E.n_unseen = 0;   // (a buffer that had to grow dropped its rows)
    if (rc != SYN_OK) return rc;
    E.rows.n = E.n_unseen = 0;
    rc = copy_positions(h, columns_at(E.rows.d, n, false), columns_of(my_bb, op_bb, nullptr, target_pi, target_v), n, hipMemcpyHostToDevice);
    if (rc != SYN_OK) return rc;
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    E.rows.n = E.n_unseen = n;
    return SYN_OK;
}

int syn_dataset_counts(syn_engine* h, size_t* n_eval, size_t* n_unseen) {
    if (!h) return SYN_ERR_INVALID_ARGUMENT;
    HIP_TRY(h, hipSetDevice(h->device));
    if (n_eval) *n_eval = h->evalset.rows.n;
    if (n_unseen) *n_unseen = h->evalset.n_unseen;
    return SYN_OK;
}

int syn_dataset_get(syn_engine* h, uint64_t* my_bb, uint64_t* op_bb, float* target_pi, float* target_v, size_t capacity, size_t* n) {
    if (!h) return SYN_ERR_INVALID_ARGUMENT;
    const size_t m = h->evalset.rows.n;
    if (n) *n = m;
    if (m > capacity) return fail(h, SYN_ERR_CAPACITY, "the evaluation set has %zu rows, the caller's arrays %zu", m, capacity);
    if (m == 0) return SYN_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    if (const int rc = copy_positions(h, columns_of(my_bb, op_bb, nullptr, target_pi, target_v), columns_at(h->evalset.rows.d, m, false), m,
                                      hipMemcpyDeviceToHost))
        return rc;
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return SYN_OK;
}

int syn_dataset_evaluate(syn_engine* h, int which, size_t first_row, size_t n_rows, const float* blob, size_t n_floats, int max_workgroups,
                         syn_dataset_metrics* out, float* block_losses, float* row_logits, float* row_kl) {
    if (!h) return SYN_ERR_INVALID_ARGUMENT;
    HIP_TRY(h, hipSetDevice(h->device));
    return syn_dataset_evaluate_arith(h, which, first_row, n_rows, blob, n_floats, SYN_EVAL_ARITH_F32, max_workgroups, out, block_losses,
                                      row_logits, row_kl);
}

int syn_dataset_evaluate_arith(syn_engine* h, int which, size_t first_row, size_t n_rows, const float* blob, size_t n_floats, int arithmetic,
                               int max_workgroups, syn_dataset_metrics* out, float* block_losses, float* row_logits, float* row_kl) {
    if (!h) return SYN_ERR_INVALID_ARGUMENT;
    if (arithmetic != SYN_EVAL_ARITH_F32 && arithmetic != SYN_EVAL_ARITH_F16X2 && arithmetic != SYN_EVAL_ARITH_BF16)
        return fail(h, SYN_ERR_INVALID_ARGUMENT, "unknown evaluation arithmetic %d", arithmetic);
    if (which != SYN_DATASET_TRAIN && which != SYN_DATASET_EVAL) return fail(h, SYN_ERR_INVALID_ARGUMENT, "unknown data set %d", which);
    if (max_workgroups < 0) return fail(h, SYN_ERR_INVALID_ARGUMENT, "max_workgroups is negative (%d); 0 lets the library choose", max_workgroups);
    auto& L = h->learner;
    const size_t set_n = which == SYN_DATASET_TRAIN ? L.data.n : h->evalset.rows.n;
    void* set_base = which == SYN_DATASET_TRAIN ? L.data.d : h->evalset.rows.d;
    if (set_n == 0 || !set_base)
        return fail(h, SYN_ERR_INVALID_ARGUMENT, "%s", which == SYN_DATASET_TRAIN ? "the learner has no data set" : "there is no evaluation set");
    if (first_row > set_n || n_rows > set_n - first_row)
        return fail(h, SYN_ERR_INVALID_ARGUMENT, "rows [%zu, %zu + %zu) are outside the data set's %zu rows", first_row, first_row, n_rows, set_n);
    int kind;
    if (blob) {
        if (n_floats == (size_t)MlpGeom::NUM_PARAMS) kind = 0;
        else if (n_floats == (size_t)ConvGeom::NUM_PARAMS) kind = 1;
        else
            return fail(h, SYN_ERR_INVALID_ARGUMENT, "Connect4Net has %d parameters, Connect4ConvNet %d, got %zu", MlpGeom::NUM_PARAMS,
                        ConvGeom::NUM_PARAMS, n_floats);
    } else {
        if (!L.has_trainer) return fail(h, SYN_ERR_NO_WEIGHTS, "blob is NULL (the trainer's weights): call syn_trainer_init first");
        kind = L.trainer_kind;
    }
    if (arithmetic == SYN_EVAL_ARITH_BF16 && kind != 1)
        return fail(h, SYN_ERR_UNSUPPORTED, "the bf16 precision exists for Connect4ConvNet only (syn_trainer_set_precision)");
    syn_dataset_metrics m;
    std::memset(&m, 0, sizeof(m));
    h->last_kernel_ms = 0.0f;
    h->last_launches = 0;
    if (n_rows == 0) {
        if (out) *out = m;
        return SYN_OK;
    }
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t nb = (n_rows + DS_BLOCK - 1) / DS_BLOCK, nch = (nb + DS_CHUNK_BLOCKS - 1) / DS_CHUNK_BLOCKS;
    Carve c;
    const size_t o_rec = c.take(nb * sizeof(DsBlockRecord)), o_chunk = c.take(nch * sizeof(DsChunkSum)), o_tot = c.take(sizeof(DsTotals));
    const size_t o_bl = c.take(block_losses ? nb * 8 : 0), o_lg = c.take(row_logits ? n_rows * 48 : 0), o_kl = c.take(row_kl ? n_rows * 8 : 0);
    int rc = ensure_scratch(h, c.at + 256);
    if (rc != SYN_OK) return rc;
    char* sc = static_cast<char*>(h->d_scratch);
    // the parameters: the trainer's own buffers (read only), or the caller's blob built into the evaluation's own image buffer
    HostImage im;
    const float* d_w = nullptr;
    auto& E = h->evalset;
    if (arithmetic == SYN_EVAL_ARITH_F16X2) {
        // the f16x2 image is built on the host from the canonical parameters, per call, into a buffer of the call's own: the engine's
        // network, arithmetic, f16x2 image, host blob and policy cache do not enter. Parameters without a plan are refused here, before
        // anything is enqueued.
        std::vector<float> own;
        if (!blob) {
            own.resize((size_t)g_net_desc[kind].num_params);
            HIP_TRY(h, hipMemcpyAsync(own.data(), L.d_tw, g_net_desc[kind].param_bytes(), hipMemcpyDeviceToHost, h->stream));
            HIP_TRY(h, hipStreamSynchronize(h->stream));
        }
        im.f16x2 = true;
        if (!g_net_desc[kind].build_f16x2(blob ? blob : own.data(), im.words))
            return fail(h, SYN_ERR_UNSUPPORTED, "these parameters have no f16x2 plan (non-finite values, scales outside the f32-safe window or a "
                                                "bias that does not fit; syn_f16x2_plan_of_blob): nothing was evaluated");
        if (!E.d_img16) HIP_TRY(h, hipMalloc(&E.d_img16, (size_t)F16Geom::IMG_WORDS * 4));
        rc = enqueue_image_upload(h, im, E.d_img16);
        if (rc != SYN_OK) return rc;
    } else if (blob) {
        if (!E.d_img) HIP_TRY(h, hipMalloc(&E.d_img, (size_t)MlpGeom::IMG_FLOATS * 4));
        if (kind == 0) {
            rc = build_host_image(h, 0, blob, false, im);
            if (rc == SYN_OK) rc = enqueue_image_upload(h, im, E.d_img);
            if (rc != SYN_OK) return rc;
        } else {
            HIP_TRY(h, hipMemcpyAsync(E.d_img, blob, (size_t)ConvGeom::NUM_PARAMS * 4, hipMemcpyHostToDevice, h->stream));
        }
        d_w = E.d_img;
    } else {
        d_w = kind == 0 ? L.d_twimg : L.d_tw;
    }
    const PositionColumns s = columns_from(columns_at(set_base, set_n, false), first_row);
    DsArgs A;
    A.my_bb = s.my;
    A.op_bb = s.op;
    A.tpi = s.pi;
    A.tv = s.v;
    A.n = (long long)n_rows;
    A.n_blocks = (long long)nb;
    A.records = reinterpret_cast<DsBlockRecord*>(sc + o_rec);
    A.block_losses = block_losses ? reinterpret_cast<float*>(sc + o_bl) : nullptr;
    A.row_logits = row_logits ? reinterpret_cast<float*>(sc + o_lg) : nullptr;
    A.row_kl = row_kl ? reinterpret_cast<float*>(sc + o_kl) : nullptr;
    // the library's choice: two workgroups of either kernel are resident on a CU (8 waves each at 4 waves per SIMD);
    // Connect4Net gets exactly those, Connect4ConvNet twice as many, the second half taking the CUs as the first drains
    // f16x2: the image takes most of a CU's LDS (Connect4Net: one workgroup per CU; Connect4ConvNet: LDS allows two, its 131 VGPRs one
    // resident at a time, the second half taking the CUs as the first drains) and a workgroup has four blocks in flight, so the grid is
    // counted in passes of four blocks
    const bool f16 = arithmetic == SYN_EVAL_ARITH_F16X2;
    const size_t fit = f16 ? (size_t)h->num_cus * (kind == 0 ? 1 : 2) : (size_t)h->num_cus * (kind == 0 ? 2 : 4);
    const size_t cap = max_workgroups > 0 ? (size_t)max_workgroups : fit;
    const size_t want = f16 ? (nb + DS_F16_SLOTS - 1) / DS_F16_SLOTS : nb;
    const unsigned grid = (unsigned)(want < cap ? want : cap);
    HIP_TRY(h, hipEventRecord(h->ev0, h->stream));
    if (f16 && kind == 0) {
        const size_t lds = (size_t)DsF16Geom<0>::LDS_WORDS * 4;
        HIP_TRY(h, hipFuncSetAttribute(reinterpret_cast<const void*>(dataset_eval_blocks_f16x2_kernel<0>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(dataset_eval_blocks_f16x2_kernel<0>, dim3(grid), dim3(DS_F16_THREADS), lds, h->stream, E.d_img16, A);
    } else if (f16) {
        const size_t lds = (size_t)DsF16Geom<1>::LDS_WORDS * 4;
        HIP_TRY(h, hipFuncSetAttribute(reinterpret_cast<const void*>(dataset_eval_blocks_f16x2_kernel<1>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(dataset_eval_blocks_f16x2_kernel<1>, dim3(grid), dim3(DS_F16_THREADS), lds, h->stream, E.d_img16, A);
    } else if (arithmetic == SYN_EVAL_ARITH_BF16) {
        const size_t lds = (size_t)DsConvGeom::LDS_FLOATS * 4;
        HIP_TRY(h, hipFuncSetAttribute(reinterpret_cast<const void*>(dataset_eval_blocks_conv_bf16_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(dataset_eval_blocks_conv_bf16_kernel, dim3(grid), dim3(CONV_TRAIN_THREADS), lds, h->stream, d_w, A);
    } else if (kind == 0) {
        const size_t lds = (size_t)DsMlpGeom::LDS_FLOATS * 4;
        HIP_TRY(h, hipFuncSetAttribute(reinterpret_cast<const void*>(dataset_eval_blocks_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(dataset_eval_blocks_kernel, dim3(grid), dim3(DS_MLP_THREADS), lds, h->stream, d_w, A);
    } else {
        const size_t lds = (size_t)DsConvGeom::LDS_FLOATS * 4;
        HIP_TRY(h, hipFuncSetAttribute(reinterpret_cast<const void*>(dataset_eval_blocks_conv_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(dataset_eval_blocks_conv_kernel, dim3(grid), dim3(CONV_TRAIN_THREADS), lds, h->stream, d_w, A);
    }
    HIP_TRY(h, hipGetLastError());
    hipLaunchKernelGGL(dataset_eval_reduce_kernel, dim3(1), dim3(DS_REDUCE_THREADS), 0, h->stream, A.records, A.n_blocks,
                       reinterpret_cast<DsChunkSum*>(sc + o_chunk), reinterpret_cast<DsTotals*>(sc + o_tot));
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipEventRecord(h->ev1, h->stream));
    DsTotals t;
    HIP_TRY(h, hipMemcpyAsync(&t, sc + o_tot, sizeof(t), hipMemcpyDeviceToHost, h->stream));
    if (block_losses) HIP_TRY(h, hipMemcpyAsync(block_losses, sc + o_bl, nb * 8, hipMemcpyDeviceToHost, h->stream));
    if (row_logits) HIP_TRY(h, hipMemcpyAsync(row_logits, sc + o_lg, n_rows * 48, hipMemcpyDeviceToHost, h->stream));
    if (row_kl) HIP_TRY(h, hipMemcpyAsync(row_kl, sc + o_kl, n_rows * 8, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    HIP_TRY(h, hipEventElapsedTime(&h->last_kernel_ms, h->ev0, h->ev1));
    h->last_launches = 2;
    if (t.rows != (unsigned long long)n_rows) return fail(h, SYN_ERR_HIP, "internal: the block records cover %llu rows of %zu", t.rows, n_rows);
    m.rows = (uint64_t)n_rows;
    m.blocks = (uint64_t)nb;
    m.mean_pi = t.sum_pi / (double)n_rows;
    m.mean_v = t.sum_v / (double)n_rows;
    m.sum_pi = t.sum_pi;
    m.sum_v = t.sum_v;
    m.pi_hits = t.pi_hits;
    m.v_hits = t.v_hits;
    m.grid = grid;
    if (out) *out = m;
    return SYN_OK;
}

// ------------------------------------------------------------------------------------------------ state digests
// syn_state_digest (include/synthesis_amd.h "State digests"; kernels in digest_kernels.cuh). The component's arrays become the
// sections of one launch; words that live on the host (the trainer's step count) enter as their h_i sum. An observer: it reads the
// state and writes the scratch only.
int syn_state_digest(syn_engine* h, int what, int max_workgroups, uint64_t* digest, uint64_t* n_words) {
    if (!h) return SYN_ERR_INVALID_ARGUMENT;
    if (what < SYN_DIGEST_TRAINER || what > SYN_DIGEST_EVAL_DATA) return fail(h, SYN_ERR_INVALID_ARGUMENT, "unknown digest component %d", what);
    if (max_workgroups < 0) return fail(h, SYN_ERR_INVALID_ARGUMENT, "max_workgroups is negative (%d); 0 lets the library choose", max_workgroups);
    auto& L = h->learner;
    if (what == SYN_DIGEST_TRAINER && !L.has_trainer) return fail(h, SYN_ERR_NO_WEIGHTS, "call syn_trainer_init first");
    if (what == SYN_DIGEST_NETWORK) {
        const int rc = require_weights(h);
        if (rc != SYN_OK) return rc;
    }
    const uint64_t tag = DIGEST_TAG + (uint64_t)what;
    DigestArgs A{};
    A.tag = tag;
    uint64_t total = 0, host_sum = 0;
    const auto add = [&](const void* p, uint64_t words) {
        A.sec[A.n_sections++] = DigestSection{static_cast<const uint32_t*>(p), words, total};
        total += words;
    };
    if (what == SYN_DIGEST_TRAINER) {
        const uint64_t P = (uint64_t)g_net_desc[L.trainer_kind].num_params;
        add(L.d_tw, P);
        add(L.d_tm, P);
        add(L.d_tv, P);
        const uint64_t step = (uint64_t)L.train_step;
        host_sum = digest_word(tag, total, (uint32_t)step) + digest_word(tag, total + 1, (uint32_t)(step >> 32));
        total += 2;
    } else if (what == SYN_DIGEST_NETWORK) {
        // the parameters are on the host (Network::host_blob: what every image of the network was built from)
        const auto& blob = h->net.host_blob;
        for (size_t i = 0; i < blob.size(); i++) {
            uint32_t w;
            std::memcpy(&w, &blob[i], 4);
            host_sum += digest_word(tag, (uint64_t)i, w);
        }
        total = blob.size();
    } else if (what == SYN_DIGEST_REPLAY) {
        const uint64_t n = h->d_replay ? h->replay_n : 0;
        if (n) {
            const PositionColumns s = columns_at(h->d_replay, h->replay_cap, true);
            add(s.my, 2 * n);
            add(s.op, 2 * n);
            add(s.gid, 2 * n);
            add(s.pi, 9 * n);
            add(s.v, 3 * n);
        }
    } else {
        const bool train = what == SYN_DIGEST_TRAIN_DATA;
        void* base = train ? L.data.d : h->evalset.rows.d;
        const uint64_t n = base ? (train ? L.data.n : h->evalset.rows.n) : 0;
        if (n) {
            const PositionColumns s = columns_at(base, n, false);
            add(s.my, 2 * n);
            add(s.op, 2 * n);
            add(s.pi, 9 * n);
            add(s.v, 3 * n);
        }
    }
    h->last_kernel_ms = 0.0f;
    h->last_launches = 0;
    if (n_words) *n_words = total;
    if (A.n_sections == 0) {
        if (digest) *digest = digest_close(tag, host_sum, total);
        return SYN_OK;
    }
    HIP_TRY(h, hipSetDevice(h->device));
    // the library's choice: every lane takes 16-byte groups, eight resident workgroups of 256 threads per CU when the state is large
    uint64_t groups = 0;
    for (int s = 0; s < A.n_sections; s++) groups += (A.sec[s].words + 3) / 4;
    const uint64_t want = (groups + DIGEST_THREADS - 1) / DIGEST_THREADS;
    const uint64_t cap = max_workgroups > 0 ? (uint64_t)max_workgroups : (uint64_t)h->num_cus * 8;
    const unsigned grid = (unsigned)std::max<uint64_t>(1, std::min(want, cap));
    Carve c;
    const size_t o_part = c.take((size_t)grid * 8), o_out = c.take(16);
    const int rc = ensure_scratch(h, c.at + 256);
    if (rc != SYN_OK) return rc;
    char* sc = static_cast<char*>(h->d_scratch);
    unsigned long long* d_part = reinterpret_cast<unsigned long long*>(sc + o_part);
    unsigned long long* d_out = reinterpret_cast<unsigned long long*>(sc + o_out);
    HIP_TRY(h, hipEventRecord(h->ev0, h->stream));
    hipLaunchKernelGGL(digest_sections_kernel, dim3(grid), dim3(DIGEST_THREADS), 0, h->stream, A, d_part);
    HIP_TRY(h, hipGetLastError());
    hipLaunchKernelGGL(digest_finish_kernel, dim3(1), dim3(DIGEST_THREADS), 0, h->stream, d_part, (int)grid, (unsigned long long)host_sum,
                       (unsigned long long)tag, (unsigned long long)total, d_out);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipEventRecord(h->ev1, h->stream));
    unsigned long long out[2] = {0ull, 0ull};
    HIP_TRY(h, hipMemcpyAsync(out, d_out, 16, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    HIP_TRY(h, hipEventElapsedTime(&h->last_kernel_ms, h->ev0, h->ev1));
    h->last_launches = 2;
    if (out[1] != total) return fail(h, SYN_ERR_HIP, "internal: the digest kernel closed %llu words of %llu", out[1], (unsigned long long)total);
    if (digest) *digest = out[0];
    return SYN_OK;
}

int syn_last_timing(const syn_engine* h, float* kernel_ms, int* n_launches) {
    if (!h) return SYN_ERR_INVALID_ARGUMENT;
    if (kernel_ms) *kernel_ms = h->last_kernel_ms;
    if (n_launches) *n_launches = h->last_launches;
    return SYN_OK;
}

int syn_last_cache_stats(const syn_engine* h, uint64_t* hits, uint64_t* misses) {
    if (!h) return SYN_ERR_INVALID_ARGUMENT;
    if (hits) *hits = h->last_cache_hits;
    if (misses) *misses = h->last_cache_misses;
    return SYN_OK;
}

int syn_last_launch_shape(const syn_engine* h, int* shape, int* grid, int* threads) {
    if (!h) return SYN_ERR_INVALID_ARGUMENT;
    if (shape) *shape = h->last_shape;
    if (grid) *grid = h->last_grid;
    if (threads) *threads = h->last_threads;
    return SYN_OK;
}

int syn_debug_calibrate(syn_engine* h, const void* d_base, const uint32_t* d_span_off, int n_spans, int do_write) {
    if (!h) return SYN_ERR_INVALID_ARGUMENT;
    if (!d_base || !d_span_off || n_spans < 0) return fail(h, SYN_ERR_INVALID_ARGUMENT, "bad arguments");
    HIP_TRY(h, hipSetDevice(h->device));
    int rc = ensure_scratch(h, 1 << 20);
    if (rc != SYN_OK) return rc;
    HIP_TRY(h, hipEventRecord(h->ev0, h->stream));
    hipLaunchKernelGGL(calib_gather_kernel, dim3(2048), dim3(256), 0, h->stream, static_cast<const float4*>(d_base),
                       d_span_off, n_spans, static_cast<float4*>(h->d_scratch), do_write);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipEventRecord(h->ev1, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    HIP_TRY(h, hipEventElapsedTime(&h->last_kernel_ms, h->ev0, h->ev1));
    return SYN_OK;
}

int syn_debug_stdrng_u32(syn_engine* h, uint64_t seed, int n, uint32_t* out) {
    if (!h) return SYN_ERR_INVALID_ARGUMENT;
    if (n < 0 || (n > 0 && !out)) return fail(h, SYN_ERR_INVALID_ARGUMENT, "bad arguments");
    if (n == 0) return SYN_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    int rc = ensure_scratch(h, (size_t)n * 4 + 256);
    if (rc != SYN_OK) return rc;
    uint32_t* d = static_cast<uint32_t*>(h->d_scratch);
    hipLaunchKernelGGL(debug_rng_kernel, dim3((n + 255) / 256), dim3(256), 0, h->stream, (unsigned long long)seed, n, d);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipMemcpyAsync(out, d, (size_t)n * 4, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return SYN_OK;
}

int syn_activation_forward(syn_engine* h, int kind, const float* x, int batch, int n, float* y) {
    if (!h) return SYN_ERR_INVALID_ARGUMENT;
    if (kind < SYN_ACT_RELU || kind > SYN_ACT_SOFTMAX) return fail(h, SYN_ERR_INVALID_ARGUMENT, "unknown activation %d", kind);
    if (batch < 0 || n < 1 || (batch > 0 && (!x || !y))) return fail(h, SYN_ERR_INVALID_ARGUMENT, "bad arguments");
    if (batch == 0) return SYN_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t cnt = (size_t)batch * (size_t)n;
    int rc = ensure_scratch(h, cnt * 8 + 256);
    if (rc != SYN_OK) return rc;
    float* dx = static_cast<float*>(h->d_scratch);
    float* dy = dx + cnt;
    HIP_TRY(h, hipMemcpyAsync(dx, x, cnt * 4, hipMemcpyHostToDevice, h->stream));
    const size_t threads = kind == SYN_ACT_SOFTMAX ? (size_t)batch : cnt;
    HIP_TRY(h, hipEventRecord(h->ev0, h->stream));
    hipLaunchKernelGGL(activation_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, h->stream, kind, dx, batch, n, dy);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipEventRecord(h->ev1, h->stream));
    HIP_TRY(h, hipMemcpyAsync(y, dy, cnt * 4, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    HIP_TRY(h, hipEventElapsedTime(&h->last_kernel_ms, h->ev0, h->ev1));
    h->last_launches = 1;
    return SYN_OK;
}

int syn_debug_fast_div(syn_engine* h, const float* a, const float* b, int n, float* out_fast, float* out_full) {
    if (!h) return SYN_ERR_INVALID_ARGUMENT;
    if (n < 0 || (n > 0 && (!a || !b || !out_fast || !out_full))) return fail(h, SYN_ERR_INVALID_ARGUMENT, "bad arguments");
    if (n == 0) return SYN_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    size_t nb = (size_t)n;
    int rc = ensure_scratch(h, nb * 16 + 256);
    if (rc != SYN_OK) return rc;
    float* da = static_cast<float*>(h->d_scratch);
    float* db = da + nb;
    float* df = db + nb;
    float* dd = df + nb;
    HIP_TRY(h, hipMemcpyAsync(da, a, nb * 4, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipMemcpyAsync(db, b, nb * 4, hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(debug_fast_div_kernel, dim3((n + 255) / 256), dim3(256), 0, h->stream, da, db, n, df, dd);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipMemcpyAsync(out_fast, df, nb * 4, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipMemcpyAsync(out_full, dd, nb * 4, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return SYN_OK;
}

int syn_debug_small_int_math(syn_engine* h, int b_lo, int b_hi, unsigned long long* mismatches3) {
    if (!h) return SYN_ERR_INVALID_ARGUMENT;
    if (!mismatches3 || b_lo < 1 || b_hi < b_lo || b_hi > 65536) return fail(h, SYN_ERR_INVALID_ARGUMENT, "bad arguments");
    HIP_TRY(h, hipSetDevice(h->device));
    int rc = ensure_scratch(h, 256);
    if (rc != SYN_OK) return rc;
    unsigned long long* dm = static_cast<unsigned long long*>(h->d_scratch);
    HIP_TRY(h, hipMemsetAsync(dm, 0, 24, h->stream));
    hipLaunchKernelGGL(debug_small_int_math_kernel, dim3((1u << 23) / 256), dim3(256), 0, h->stream, b_lo, b_hi, dm);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipMemcpyAsync(mismatches3, dm, 24, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return SYN_OK;
}

int syn_debug_math(syn_engine* h, const float* a, const float* b, int n, float* out_exp_a, float* out_div,
                   float* out_sqrt_a) {
    if (!h) return SYN_ERR_INVALID_ARGUMENT;
    if (n < 0 || (n > 0 && (!a || !b || !out_exp_a || !out_div || !out_sqrt_a)))
        return fail(h, SYN_ERR_INVALID_ARGUMENT, "bad arguments");
    if (n == 0) return SYN_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    size_t nb = (size_t)n;
    int rc = ensure_scratch(h, nb * 20 + 256);
    if (rc != SYN_OK) return rc;
    float* da = static_cast<float*>(h->d_scratch);
    float* db = da + nb;
    float* de = db + nb;
    float* dd = de + nb;
    float* ds = dd + nb;
    HIP_TRY(h, hipMemcpyAsync(da, a, nb * 4, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipMemcpyAsync(db, b, nb * 4, hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(debug_math_kernel, dim3((n + 255) / 256), dim3(256), 0, h->stream, da, db, n, de, dd, ds);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipMemcpyAsync(out_exp_a, de, nb * 4, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipMemcpyAsync(out_div, dd, nb * 4, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipMemcpyAsync(out_sqrt_a, ds, nb * 4, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return SYN_OK;
}

}  // extern "C"
