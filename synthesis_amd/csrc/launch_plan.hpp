// synthesis_amd — which kernel plays a self-play / search call, and on what launch shape: the decision alone, as a pure function of
// plain numbers. Host-only C++17 without a HIP header, so the selection is read and tested on a CPU (tests/test_launch_plan.py).
// engine.hip builds the query, grows the buffers the plan asks for, looks the plan's kernel up in the table of shipped
// instantiations (lane_instances.h) and launches it. plan_eval, further down, is the same for a policy-evaluation call, and
// plan_micro_grads, at the end, for the learner's micro-batch gradient launch.
#pragma once
#include <climits>
#include <cstddef>

namespace syn {

// Geometry the selection depends on. engine.hip static_asserts each against the kernel header that owns it.
constexpr unsigned PLAN_LANE_MAX_CAP = 1u << 16;    // lane_kernel.cuh LANE_MAX_CAP
constexpr unsigned PLAN_PATH_ENTRIES = 2 * 4096;    // lane_kernel.cuh PATH_ENTRIES: 16-byte entries of one wave's descent log
constexpr int PLAN_PC_TREE_WAVES = 12;              // pc_kernel.cuh PcGeom
constexpr int PLAN_PC_NT = 1024;
constexpr int PLAN_PC_NV_MAX = 3;
constexpr size_t PLAN_PC_VW_BYTES = 11008;
constexpr int PLAN_POOL_M_MAX = 128;                // pool_kernel.cuh PoolGeom
constexpr size_t PLAN_POOL_WAVE_BYTES = 12288;

// Developer knobs that influence the selection (engine.hip fills them through debug_env: honoured with SYN_DEBUG=1 only).
// A numeric knob holds atoi of its variable; SYN_PC_STUB and SYN_L2_TILE are 1 when the variable exists.
constexpr int KNOB_UNSET = INT_MIN;
struct LaunchKnobs {
    int lanes = KNOB_UNSET, free_run = KNOB_UNSET, quads = KNOB_UNSET, lane_thresh = KNOB_UNSET, scan_min = KNOB_UNSET, ablate = KNOB_UNSET;
    // SYN_DEBUG_SHAPES builds only
    int pc = KNOB_UNSET, pc_prio = KNOB_UNSET, pc_stub = KNOB_UNSET, lanes2 = KNOB_UNSET, l2_tile = KNOB_UNSET;
    int pool = KNOB_UNSET, pool_nw = KNOB_UNSET, pool_fire = KNOB_UNSET, pool_scan = KNOB_UNSET;
};
inline bool knob_set(int k) { return k != KNOB_UNSET; }

struct LaunchQuery {
    int num_cus = 256;
    int slots = 0;        // the engine's concurrent games
    int jobs = 0;         // games or roots of this call
    unsigned cap = 0;     // nodes per tree slab
    int net_kind = 0;     // 0 Connect4Net, 1 Connect4ConvNet
    bool f16 = false;     // the call evaluates the network's f16x2 image
    int pool_trees = 0;   // engine's pool_trees (DEBUG_SHAPES builds)
    int mode = 0;         // 0 self-play, 1 search (engine_kernels.cuh MODE_*)
    bool count = false, prof = false;
    int fpu = 0, noise = 0;   // DevMctsCfg
    int family = 0;           // mcts.cuh cfg_family: 1 parity (= cfg_is_fast), 2 the reference's Fpu::Func configuration, 0 anything else
};

// The arithmetic of the network image ONE call evaluates. A call of the engine's own network leaves PLAN_ARITH_ENGINE: the engine's
// current arithmetic. A match side (syn_match_run_sides) whose blob was built into an image of its own says which kind that image is,
// whatever the engine is in: the kernel family follows the image, never the engine.
constexpr int PLAN_ARITH_ENGINE = 0, PLAN_ARITH_F32 = 1, PLAN_ARITH_F16X2 = 2;
inline bool plan_call_f16(bool engine_f16, int call_arith) {
    return call_arith == PLAN_ARITH_F16X2 || (call_arith != PLAN_ARITH_F32 && engine_f16);
}

// What of an engine the selection reads (engine.hip fills it from syn_engine) ...
struct LaunchEngine {
    int num_cus = 256;
    int slots = 0;
    unsigned cap = 0;
    int net_kind = 0;
    bool f16 = false;     // the engine's own network arithmetic is f16x2
    int pool_trees = 0;
};
// ... and the query of one call on it: `call_arith` = PLAN_ARITH_* of the image the call's EngineParams::wimg points at
inline LaunchQuery launch_query(const LaunchEngine& e, int call_arith, int jobs, int mode, bool count, bool prof, int fpu, int noise,
                                int family) {
    LaunchQuery q;
    q.num_cus = e.num_cus;
    q.slots = e.slots;
    q.jobs = jobs;
    q.cap = e.cap;
    q.net_kind = e.net_kind;
    q.f16 = plan_call_f16(e.f16, call_arith);
    q.pool_trees = e.pool_trees;
    q.mode = mode;
    q.count = count;
    q.prof = prof;
    q.fpu = fpu;
    q.noise = noise;
    q.family = family;
    return q;
}

struct LaunchPlan {
    bool error = false;   // cap > LANE_MAX_CAP for a configuration that only the lane-per-tree kernels play
    int shape = 0;        // as syn_last_launch_shape reports it: 1 / 2 row-per-tree (= workgroups per CU), 3 quads, 4 lanes, 5 producer/consumer,
                          // 6 two trees per lane, 7 free-running, 8 pool
    int grid = 0, threads = 0;
    // the kernel: template arguments of the instantiation
    int mode = 0;
    bool count = false;
    bool prof = false;    // as requested: where no profiled instantiation ships, the table lookup takes the plain one
    int fast = 0;         // 0 runtime-switched, 1 parity family, 2 the reference's self-play configuration
    int n = 0;            // shape 1 / 2: WPS; 3: NQ; 4, 6, 8: NW
    int policy = 0;       // 0 Connect4Net, 1 RolloutPolicy, 2 Connect4ConvNet, 3 Connect4Net f16x2, 4 Connect4ConvNet f16x2
    int tile = 0;         // shape 6: the TILE variant
    int slots = 0;        // tree slots the launch plays on, after the caps
    // EngineParams fields the choice fixes
    int lane_thresh = 0, nv = 0, debug_prio = 0, debug_stub = 0;
    bool no_cache = false;
    size_t path_entries = 0;   // 16-byte entries the per-wave descent logs need (0: the kernel keeps none)
    size_t vw_bytes = 0;       // bytes of per-(virtual-)wave state
    int pool_trees = 0;        // shape 8: trees per wave
};

// a round of the lane-per-tree kernels ends once this many lanes of a wave stand on a leaf (whole tiles)
inline int plan_lane_thresh(const LaunchKnobs& k, int dflt) {
    int t = knob_set(k.lane_thresh) ? k.lane_thresh : dflt;
    if (t < 16 || t > 64) t = dflt;
    return t & ~15;
}

inline LaunchPlan plan_launch(const LaunchQuery& q, const LaunchKnobs& k) {
    LaunchPlan p;
    p.mode = q.mode;
    p.count = q.count;
    p.prof = q.prof;
    const int cus = q.num_cus;
    // one 256-thread workgroup per 16 tree slots; the kernel needs ~17 KB of LDS and <= 256 VGPRs, so up to two
    // workgroups are resident per CU (concurrency beyond 2 x 16 x CUs queues behind resident workgroups)
    int want_slots = q.slots;
    if (q.jobs < want_slots) want_slots = ((q.jobs + 15) / 16) * 16;
    int grid = want_slots / 16;
    if (grid < 1) grid = 1;
    const bool fast = q.family == 1;  // compile-time-folded config family (mcts.cuh CfgView)
    const bool lanes_knob = knob_set(k.lanes);
    const bool conv = q.net_kind == 1;
    const bool lane_cap_ok = q.cap <= PLAN_LANE_MAX_CAP;
    // Kernel choice by trees per CU: <= 16 -> one 16-tree workgroup per CU, weights in registers (latency-optimal);
    // <= 32 -> two such workgroups per CU (hybrid register/LDS weights); more -> the quad-async kernel (NQ quads of 16
    // trees per workgroup sharing one LDS weight image). SYN_DEBUG=1 SYN_QUADS=0..4 overrides (0 = never use the quad kernel).
    // Lane-per-tree kernel (lane_kernel.cuh): one tree per lane, NW waves per workgroup, one workgroup per CU.
    // SYN_DEBUG=1 SYN_LANES=<waves per workgroup: 4, 8, 12 or 16> forces it (0 = never); by default it takes over once every CU can
    // be given 256 trees (4 waves; measured 41.9k games/s at 65,536 concurrent games against 31.8k for the queued
    // row-per-tree workgroups), 8 waves up to 512 trees per CU, 12 up to 768, 16 beyond (selection below).
    // Producer/consumer kernel (pc_kernel.cuh): 12 tree waves x NV virtual waves of 64 trees + 4 matrix waves per CU. Measured
    // slower than the symmetric lane kernel (the f32 MFMA shares the SIMD's FP32 datapath with the VALU, so
    // dedicating waves to the matrix pipe frees nothing), so it is never chosen automatically:
    // SYN_DEBUG=1 SYN_PC=<NV 1..3> selects it (parity tests, profiling).
#ifdef SYN_DEBUG_SHAPES
    {
        const int nv = knob_set(k.pc) ? k.pc : 0;
        if (nv >= 1 && nv <= PLAN_PC_NV_MAX && lane_cap_ok && q.net_kind == 0) {
            const int per_wg = 64 * PLAN_PC_TREE_WAVES * nv;
            const int pgrid = (want_slots + per_wg - 1) / per_wg;
            const size_t nvw = (size_t)pgrid * PLAN_PC_TREE_WAVES * nv;
            p.shape = 5; p.grid = pgrid; p.threads = PLAN_PC_NT;
            p.fast = fast; p.slots = want_slots;
            p.path_entries = nvw * PLAN_PATH_ENTRIES;
            p.vw_bytes = nvw * PLAN_PC_VW_BYTES;
            p.nv = nv;
            p.debug_prio = knob_set(k.pc_prio) ? k.pc_prio : 2;
            p.debug_stub = (q.prof && knob_set(k.pc_stub)) ? 1 : 0;
            p.lane_thresh = plan_lane_thresh(k, 48);
            return p;
        }
    }
#endif
    // At most 16 trees per CU in the f16x2 arithmetic: four free-running waves of four trees, each evaluating its own leaves in a tile
    // of its own (free_kernel.cuh). The draws of Fpu::Func / PolicyNoise::Dirichlet live in the lane-per-tree kernels only.
    // SYN_DEBUG=1 SYN_FREE=0 switches it off (the lane kernel at 4 waves then plays these games).
    if (q.net_kind == 0 && q.f16 && want_slots <= 16 * cus && q.fpu != 2 && q.noise != 2 && !lanes_knob && k.free_run != 0
#ifdef SYN_DEBUG_SHAPES
        && !(knob_set(k.pool) && k.pool > 64)
#endif
        ) {
        p.shape = 7; p.grid = (want_slots + 15) / 16; p.threads = 256;
        p.fast = fast; p.slots = want_slots;
        return p;
    }
#ifdef SYN_DEBUG_SHAPES
    // Two trees per lane (lane2_kernel.cuh): 8 waves per workgroup, 1,024 trees per CU. SYN_DEBUG=1 SYN_LANES2=8 forces it,
    // SYN_LANES2=0 switches it off.
    {
        int nw2 = knob_set(k.lanes2) ? k.lanes2 : 0;
        if (q.prof) nw2 = 0;
        if ((nw2 == 8 || nw2 == 12) && lane_cap_ok && !(conv && q.f16)) {
            const int per_wg = 128 * nw2;
            const int lgrid = (want_slots + per_wg - 1) / per_wg;
            p.shape = 6; p.grid = lgrid; p.threads = 64 * nw2;
            p.fast = fast; p.n = nw2; p.policy = conv ? 2 : 0; p.slots = want_slots;
            p.tile = (nw2 == 8 && !conv && q.mode == 0 && !q.count && fast && knob_set(k.l2_tile)) ? 1 : 0;
            p.path_entries = (size_t)lgrid * nw2 * 2 * PLAN_PATH_ENTRIES;
            p.lane_thresh = plan_lane_thresh(k, 48);
            return p;
        }
    }
    // The pool kernel (pool_kernel.cuh): a wave's 64 lanes work on a pool of M trees (64 < M <= 128) — a lane whose descent arrives
    // binds the next READY tree in the same iteration, a round fires on 64 leaves — for the two compile-time-folded configuration
    // families of Connect4Net (f32 and f16x2), 12 or 8 waves x M trees per CU. Measured slower than the lane kernel on every leg in
    // three same-box A/B runs (profiles/r06_pool_unbinding_ab.txt, NOTES round 6), so it is never chosen automatically and ships only
    // in DEBUG_SHAPES=1 builds: SYN_DEBUG=1 SYN_POOL=<M> selects it (parity tests, re-measurement).
    {
        int pm = knob_set(k.pool) ? k.pool : q.pool_trees;
        // 1 = as many trees per wave as the engine's slots give 12 waves on every CU (at most 128)
        if (pm == 1) {
            pm = (want_slots + cus * 12 - 1) / (cus * 12);
            if (pm > PLAN_POOL_M_MAX) pm = PLAN_POOL_M_MAX;
        }
        const bool lanes_forced = lanes_knob || knob_set(k.quads);
        if (pm > 64 && pm <= PLAN_POOL_M_MAX && (q.family == 1 || q.family == 2) && q.net_kind == 0 && lane_cap_ok && !q.prof && !lanes_forced &&
            (knob_set(k.pool) || want_slots >= cus * 768)) {
            // waves per workgroup: 12 (three per SIMD, 168 registers) or 8 (two per SIMD, 256 registers)
            const int nw = (knob_set(k.pool_nw) && k.pool_nw == 8) ? 8 : 12;
            const int per_wg = nw * pm;
            int pgrid = (want_slots + per_wg - 1) / per_wg;
            if (pgrid > cus) pgrid = cus;   // one workgroup per CU: a larger engine only holds idle slabs
            if (pgrid < 1) pgrid = 1;
            const size_t nwv = (size_t)pgrid * nw;
            p.shape = 8; p.grid = pgrid; p.threads = 64 * nw;
            p.fast = q.family; p.n = nw; p.policy = q.f16 ? 3 : 0; p.slots = want_slots;
            p.path_entries = nwv * 2 * PLAN_PATH_ENTRIES;
            p.vw_bytes = nwv * PLAN_POOL_WAVE_BYTES;
            p.nv = p.pool_trees = pm;
            p.lane_thresh = knob_set(k.pool_scan) ? k.pool_scan : 24;   // Fpu::Func: waiting lanes that trigger a scan iteration
            if (p.lane_thresh < 1 || p.lane_thresh > 64) p.lane_thresh = 24;
            p.debug_prio = knob_set(k.pool_fire) ? k.pool_fire : 64;    // leaves that fire a round
            if (p.debug_prio < 16 || p.debug_prio > 64) p.debug_prio = 64;
            return p;
        }
    }
#endif
    {
        int nw = 0;
        int lane_slots = want_slots;   // (the caps below shrink what the lane kernel plays on, not what the row kernels would)
        // 4 waves per workgroup up to 256 trees per CU, 8 up to 512, 12 up to 768, 16 (hand-pipelined network tile that fits
        // the 128-VGPR budget: mlp_tile16_pipe) beyond
        const int nw_by_size = want_slots > cus * 768 ? 16 : (want_slots > cus * 512 ? 12 : (want_slots > cus * 256 ? 8 : 4));
        if (want_slots >= cus * 256) nw = nw_by_size;
        // the random draws of Fpu::Func / PolicyNoise::Dirichlet (noise.cuh) exist in the lane-per-tree kernels only
        const bool needs_noise = q.fpu == 2 || q.noise == 2;
        if (needs_noise && nw == 0) nw = 4;
        if (lanes_knob) nw = k.lanes;
        const auto valid = [](int w) { return w == 4 || w == 8 || w == 12 || w == 16; };
        if (needs_noise && !valid(nw)) nw = 4;
        // Connect4ConvNet (convnet.cuh) is evaluated by the lane-per-tree kernels only: 4 waves per workgroup up to 256 trees
        // per CU, 8 up to 512, 16 beyond
        // Connect4Net in the f16x2 arithmetic (f16x2_tile.cuh) is evaluated by the lane-per-tree kernels only, at every size
        const bool f16x2 = !conv && q.f16;
        // ... and Connect4ConvNet in it (conv_f16x2_tile.cuh, POLICY 4)
        const bool conv16 = conv && q.f16;
        if ((needs_noise || f16x2 || conv) && !lane_cap_ok) {
            p.error = true;
            return p;
        }
        if (f16x2 && !(lanes_knob && valid(nw))) nw = nw_by_size;
        if (conv) {
            if (conv16) {
                // the f16x2 tile ships where its instantiations keep their registers (profiles/r07_conv_f16x2_resource_usage.txt): the
                // parity family at 4 and 8 waves (at most 512 trees per CU), the runtime-switched configurations at 4 (at most 256)
                const bool forced = lanes_knob && (nw == 4 || nw == 8);
                if (!forced) nw = want_slots > cus * 256 ? 8 : 4;
                if (!fast) nw = 4;
                if (lane_slots > cus * 64 * nw) lane_slots = cus * 64 * nw;
            } else
                nw = want_slots > cus * 512 ? 16 : (want_slots > cus * 256 ? 8 : 4);
        }
        // The runtime-switched (general) instantiations need 300-450 more registers than the 128 of a 16-wave workgroup and are
        // bound by their own scratch traffic there (PMC: 8.8x the algorithmic bytes; Fpu::ParentQ 29.5k games/s against 42.4k,
        // Fpu::Func 15.9k against 31.2k): they run 8 waves of 256 registers on at most 512 trees per CU, whatever the capacity.
        if (!fast && q.family != 2 && nw > 8 && !lanes_knob) {
            nw = 8;
            if (lane_slots > cus * 512) lane_slots = cus * 512;
        }
        // Tree-bound regimes — PolicyWithCache on (most leaf evaluations are table hits) or the reference's own Fpu::Func
        // configuration — run 12 waves of 168 registers (17 spilled) on at most 768 trees per CU rather than 16 x 128 (55 spilled):
        // measured 90.5k against 84.8k games/s with the cache, 61.2k against 55.8k with the trained checkpoint and the cache,
        // 51.2k against 47.7k for the reference configuration; without the cache the two shapes are equal (70.6k / 71.2k).
        // The f16x2 arithmetic makes every regime tree-bound (its network tile is a quarter of the f32 one): 102k games/s at 16 x 1,024
        // against 111k at 12 x 768 (random-init), 65.0k against 72.4k (trained checkpoint).
        // Round 5: the headline (parity family, f32, no cache) takes the same shape — it measures the same or better there (75.9k against
        // 74.6k at 1,048,576 games, 77.5k against 76.9k at a full step) and 12 x 164 registers spill nothing where 16 x 128 spills 35.
        if (!conv && nw == 16 && (fast || q.family == 2) && !lanes_knob) {
            nw = 12;
            if (lane_slots > cus * 768) lane_slots = cus * 768;
        }
        if (valid(nw) && lane_cap_ok) {
            // (slots are rounded up to whole workgroups; the pool was allocated for a multiple of 1024 slabs)
            const int lgrid = (lane_slots + 64 * nw - 1) / (64 * nw);
            p.shape = 4; p.grid = lgrid; p.slots = lane_slots;
            // a round ends once this many lanes of a wave stand on a leaf: 48 with the f32 tile; with the f16x2 tile (a quarter of the cost) waiting
            // for all 64 measures +1-2 % (same box: 107.5k -> 108.7k games/s random-init, 65.3k -> 66.7k trained; 32: 100.5k / 60.8k)
            p.lane_thresh = plan_lane_thresh(k, f16x2 ? 64 : 48);
            p.debug_stub = (q.prof && knob_set(k.ablate)) ? k.ablate : 0;
            // Fpu::Func: 0 = every level takes its draws on the spot (a scan is ~220 issue slots since round 6); 1..64 = scans are
            // deferred until that many lanes wait for one or nobody can move without one (rounds 4-5, when a scan was ~600: 64)
            p.nv = knob_set(k.scan_min) ? k.scan_min : 0;
            if (p.nv < 0 || p.nv > 64) p.nv = 0;
            if (f16x2) {
                // family 1 / 2 at every wave count, the runtime-switched configurations at 4 and 8 waves (nw was capped above; a
                // SYN_LANES of 12 or 16 keeps its grid and runs the 8-wave instantiation)
                p.policy = 3;
                p.fast = q.family;
                if (q.family == 0 && nw > 8) nw = 8;
            } else if (!conv && q.family == 2 && nw >= 8) {
                // the reference's own self-play configuration (Fpu::Func folded at compile time: mcts.cuh cfg_family) has instantiations of
                // its own at 8, 12 and 16 waves
                p.fast = 2;
            } else {
                p.policy = conv16 ? 4 : (conv ? 2 : 0);
                p.fast = fast;
            }
            p.n = nw;
            p.threads = 64 * nw;
            p.path_entries = (size_t)lgrid * nw * PLAN_PATH_ENTRIES;
            return p;
        }
    }
    int nq = 0;
    {
        const int per_cu = (grid + cus - 1) / cus;
        nq = per_cu <= 2 ? 0 : (per_cu >= 4 ? 4 : 3);
        if (knob_set(k.quads)) nq = k.quads;
        if (nq < 0 || nq == 1 || nq > 4) nq = 0;
    }
    p.fast = fast;
    p.slots = want_slots;
    if (nq >= 2) {
        p.shape = 3; p.grid = (grid + nq - 1) / nq; p.threads = 256 * nq; p.n = nq;
        return p;
    }
    p.shape = p.n = grid <= cus ? 1 : 2; p.grid = grid; p.threads = 256;
    return p;
}

// MCTS over RolloutPolicy: always the lane-per-tree kernel (8 waves per workgroup), RolloutPolicy instead of the network
inline LaunchPlan plan_rollout_search(int slots, int jobs, unsigned cap) {
    LaunchPlan p;
    if (cap > PLAN_LANE_MAX_CAP) {
        p.error = true;
        return p;
    }
    const int nw = 8;
    p.slots = slots < jobs ? slots : jobs;
    int lgrid = (p.slots + 64 * nw - 1) / (64 * nw);
    if (lgrid < 1) lgrid = 1;
    p.shape = 4; p.grid = lgrid; p.threads = 64 * nw;
    p.mode = 1; p.n = nw; p.policy = 1;
    p.lane_thresh = 64;
    p.no_cache = true;
    p.path_entries = (size_t)lgrid * nw * PLAN_PATH_ENTRIES;
    return p;
}

// ------------------------------------------------------------------------------------------------ policy evaluation
// Which kernel evaluates a batch of n positions (syn_policy_eval_batch*, the evaluation contexts), by network, arithmetic and size.
// engine.hip keeps the table from EvalKernel to the function (g_eval_kernels) and the one launch (launch_eval).
enum EvalKernel {
    EVAL_TILE = 0,        // policy_eval_tile_kernel (eval_small.cuh): the latency kernel, one workgroup per 16-position tile, no weight staging
    EVAL_MLP_512,         // policy_eval_kernel<512> / <768> (engine_kernels.cuh): Connect4Net, the f32 image staged in LDS
    EVAL_MLP_768,
    EVAL_CONV_512,        // policy_eval_conv_kernel<512> (convnet.cuh)
    EVAL_F16_512,         // policy_eval_f16x2_kernel<512> / <1024> (engine_kernels.cuh): Connect4Net, the f16x2 image
    EVAL_F16_1024,
    EVAL_CONV_F16_512,    // policy_eval_conv_f16x2_kernel<512> (conv_f16x2_tile.cuh)
    EVAL_KERNELS
};
// dynamic LDS of each: the tile kernel's two activation-exchange buffers, else the network's image (engine.hip static_asserts them)
constexpr size_t PLAN_EVAL_TILE_LDS = 14 * 64 * 16;
constexpr size_t PLAN_MLP_IMG_BYTES = 30816 * 4;        // mlp.cuh MlpGeom::IMG_FLOATS
constexpr size_t PLAN_CONV_IMG_BYTES = 16480 * 4;       // convnet.cuh ConvGeom::IMG_FLOATS
constexpr size_t PLAN_F16_IMG_BYTES = 31080 * 4;        // f16x2_tile.cuh F16Geom::IMG_WORDS
constexpr size_t PLAN_CONV_F16_IMG_BYTES = 16932 * 4;   // conv_f16x2_tile.cuh ConvF16Geom::IMG_WORDS
constexpr size_t PLAN_EVAL_TILE_MAX = 4096;             // the tile kernel is chosen up to this many positions (256 tiles: one per CU of an MI355X)

struct EvalQuery {
    int net_kind = 0;     // 0 Connect4Net, 1 Connect4ConvNet
    bool f16 = false;     // the engine is in the f16x2 arithmetic
    int n = 0;            // positions, >= 1
    int num_cus = 256;
    // an evaluation context's call (the engine's own launches leave the defaults: nothing in place, nothing polled)
    size_t poll_max = 0;        // batches up to this size signal completion through pinned memory
    size_t zero_copy_out = 0;   // results of up to this many positions are written into the pinned buffer by the kernel itself
    bool poll_broken = false;   // a completion word went missing once on this context
};

struct EvalPlan {
    int kernel = EVAL_TILE;   // EvalKernel
    int threads = 0, grid = 0;
    size_t lds = 0;
    bool f16_image = false;   // the kernel reads the f16x2 image (else the f32 one)
    bool in_place = false;    // results are written across the host link into the caller's pinned buffer
    bool polled = false;      // the kernel's last workgroup reports completion through pinned memory (tile kernel only)
};

inline EvalPlan plan_eval(const EvalQuery& q) {
    EvalPlan p;
    const int ntiles = (q.n + 15) / 16;
    const size_t nb = (size_t)q.n;
    // the positions are read across the host link in place (16 B each); small results are written in place, larger ones come back
    // with one DMA (syn_policy_eval_batch, measured)
    p.in_place = nb <= q.zero_copy_out;
    // the latency kernel: its last workgroup stores the call's number into pinned memory, syn_eval_ctx_wait polls it.
    // (A polled call uses it whatever its size: SYN_EVAL_POLL_MAX raised past PLAN_EVAL_TILE_MAX is not capped.)
    p.polled = p.in_place && q.net_kind == 0 && !q.f16 && nb <= q.poll_max && !q.poll_broken;
    if (p.polled || (q.net_kind == 0 && !q.f16 && nb <= PLAN_EVAL_TILE_MAX)) {
        // at most a tile per CU: the latency kernel (eval_small.cuh), one workgroup per tile, no weight staging
        p.kernel = EVAL_TILE; p.threads = 256; p.grid = ntiles; p.lds = PLAN_EVAL_TILE_LDS;
        return p;
    }
    // The throughput kernels: a workgroup stages the image once and its waves take tiles in turn, at most one workgroup per CU.
    // Two waves per SIMD (512 threads): one wave's LDS reads / feature math overlap the other's MFMAs. Large batches (every
    // wave gets several tiles) run three waves per SIMD, which also hides the loads and stores around the tiles.
    p.f16_image = q.f16;
    if (q.net_kind == 1 && q.f16) {
        // Connect4ConvNet in the f16x2 arithmetic (conv_f16x2_tile.cuh): the throughput kernel at every size, two waves per SIMD
        p.kernel = EVAL_CONV_F16_512; p.threads = 512; p.lds = PLAN_CONV_F16_IMG_BYTES;
    } else if (q.f16) {
        // Connect4Net in the f16x2 arithmetic: the throughput kernel at every size (its tile is 3x shorter than the f32 one's)
        const bool large = ntiles >= q.num_cus * 16 * 4;
        p.kernel = large ? EVAL_F16_1024 : EVAL_F16_512; p.threads = large ? 1024 : 512; p.lds = PLAN_F16_IMG_BYTES;
    } else if (q.net_kind == 1) {
        // (16 waves per CU measured the same 46 % of the MFMA peak as 8: the tile is issue-bound, not latency-bound)
        p.kernel = EVAL_CONV_512; p.threads = 512; p.lds = PLAN_CONV_IMG_BYTES;
    } else {
        const bool large = ntiles >= q.num_cus * 12 * 4;
        p.kernel = large ? EVAL_MLP_768 : EVAL_MLP_512; p.threads = large ? 768 : 512; p.lds = PLAN_MLP_IMG_BYTES;
    }
    const int waves = p.threads / 64;
    p.grid = (ntiles + waves - 1) / waves;
    if (p.grid > q.num_cus) p.grid = q.num_cus;
    return p;
}

// ------------------------------------------------------------------------------------------------ micro-batch learner step
// The blocks launch of a SYN_TRAIN_BATCH_MICRO gradient (train_micro.cuh): nb micro-batches of 32 positions over min(nb, cap)
// workgroups, cap = the caller's max_workgroups or, when that is 0, one workgroup per CU (the conv kernels' LDS admits no more, and a
// Connect4Net workgroup is 16 waves). A workgroup walks its micro-batches j = b, b + grid, ...; the result does not depend on the grid.
constexpr int PLAN_MICRO_BLOCK = 32;                   // train_micro.cuh MICRO_BLOCK
constexpr int PLAN_MICRO_MAX_BLOCKS = 1024;            // train_micro.cuh MICRO_MAX_BLOCKS
constexpr int PLAN_MLP_NUM_PARAMS = 30492;             // train_kernels.cuh TrainGeom::NUM_PARAMS
constexpr int PLAN_CONV_NUM_PARAMS = 12412;            // convnet.cuh ConvGeom::NUM_PARAMS
constexpr size_t PLAN_MICRO_MLP_LDS = 25792 * 4;      // train_kernels.cuh TrainGeom::WL_OFF floats
constexpr size_t PLAN_MICRO_CONV_LDS = 39392 * 4;      // train_conv_mfma.cuh ConvMfmaGeom::LDS_FLOATS floats = 157,568 B: one workgroup per CU

struct MicroQuery {
    int net_kind = 0;         // 0 Connect4Net, 1 Connect4ConvNet (f32 and bf16 alike)
    int nb = 0;               // micro-batches of the minibatch, 1 .. PLAN_MICRO_MAX_BLOCKS
    int max_workgroups = 0;   // the caller's cap; 0 = the device's CU count
    int num_cus = 256;
};

struct MicroPlan {
    int grid = 0, threads = 0;
    size_t lds = 0;
    int row_stride = 0;       // floats of a block-buffer row: [gradients][2 losses], padded to a multiple of 64
    size_t buffer_bytes = 0;  // nb rows
    int reduce_grid = 0, reduce_threads = 64;   // train_micro.cuh MICRO_REDUCE_THREADS: one thread per parameter and loss word
};

inline MicroPlan plan_micro_grads(const MicroQuery& q) {
    MicroPlan p;
    const int cap = q.max_workgroups > 0 ? q.max_workgroups : q.num_cus;
    p.grid = q.nb < cap ? q.nb : cap;
    if (p.grid < 1) p.grid = 1;
    const int params = q.net_kind == 1 ? PLAN_CONV_NUM_PARAMS : PLAN_MLP_NUM_PARAMS;
    p.threads = q.net_kind == 1 ? 512 : 1024;
    p.lds = q.net_kind == 1 ? PLAN_MICRO_CONV_LDS : PLAN_MICRO_MLP_LDS;
    p.row_stride = (params + 2 + 63) & ~63;
    p.buffer_bytes = (size_t)q.nb * (size_t)p.row_stride * 4;
    p.reduce_grid = (params + 2 + p.reduce_threads - 1) / p.reduce_threads;
    return p;
}

}  // namespace syn
