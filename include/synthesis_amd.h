/* synthesis_amd — MI355X-native batched self-play engine: C ABI (drop-in boundary).
 *
 * The reference (coreylowman/synthesis) has no FFI; its plug-in surface is Rust generics:
 *   trait Game<N>            synthesis/src/game.rs:68-88
 *   trait Policy<G,N>        synthesis/src/policies/traits.rs:4-6   fn eval(&mut self,&G)->([f32;N],[f32;3])
 *   trait NNPolicy<G,N>      synthesis/src/policies/traits.rs:8-11
 *   MCTS<G,P,N>              synthesis/src/mcts.rs:102-147 (private module, reached through alpha_zero/evaluator)
 *   run_n_games / run_game   synthesis/src/alpha_zero.rs:181-268
 * Every entry point below is the batched, plain-C form of one of those; the doc comment on each names the reference
 * interface it replaces. INTEGRATION.md shows the Rust `extern "C"` block + `impl Policy<Connect4, 9>` a maintainer
 * would add on the reference side.
 *
 * Conventions: all functions return SYN_OK (0) or a negative syn_status; syn_last_error() gives the message of the
 * last failure on that handle (or of the last failed syn_engine_create when handle == NULL). Nothing throws or unwinds
 * across this boundary. Host pointers unless a parameter is documented as a device pointer. The caller owns every
 * output buffer; the engine keeps no pointer past the call. One handle = one GPU + one stream; calls on a handle are
 * not re-entrant; different handles are independent (the reference's one-policy-per-thread rule, alpha_zero.rs:192-198).
 */
#ifndef SYNTHESIS_AMD_H
#define SYNTHESIS_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum syn_status {
    SYN_OK = 0,
    SYN_ERR_INVALID_ARGUMENT = -1,
    SYN_ERR_NO_DEVICE = -2,       /* no usable gfx950 device / HIP runtime failure at create */
    SYN_ERR_HIP = -3,             /* a HIP call failed; see syn_last_error */
    SYN_ERR_NO_WEIGHTS = -4,      /* policy/value network weights not loaded yet */
    SYN_ERR_UNSUPPORTED = -5,     /* config variant not implemented on the device */
    SYN_ERR_CAPACITY = -6,        /* node pool too small for the requested explores */
    SYN_ERR_CANCELLED = -7        /* syn_cancel was called while the call ran: results of the games that finished are valid */
} syn_status;

/* ---- plain-data mirrors of synthesis/src/config.rs ---------------------------------------------------------- */

/* config.rs:9-13 Exploration */
enum { SYN_EXPLORATION_UCT = 0, SYN_EXPLORATION_POLYNOMIAL_UCT = 1 };
/* config.rs:15-19 ActionSelection */
enum { SYN_ACTION_Q = 0, SYN_ACTION_NUM_VISITS = 1 };
/* config.rs:21-26 Fpu. Func(fn() -> f32) is a plain function pointer (config.rs:25), called once per unexpanded child per
 * select_best_child scan (mcts.rs:351-356):
 *   SYN_FPU_FUNC {fpu_fn}: that pointer as `float (*)(void)`. A host function — it is called by the HOST trees of
 *     syn_mcts_search_lockstep / syn_selfplay_run_lockstep (from their worker threads, as the reference calls it from its
 *     workers: it must be thread-safe, like the reference's thread_rng closure); the device entry points (syn_mcts_search,
 *     syn_selfplay_run, ...) refuse it with SYN_ERR_UNSUPPORTED — a kernel cannot call into the host.
 *   SYN_FPU_NORMAL {fpu_value = mean, fpu_std = std}: the closure the reference itself configures —
 *     Normal::new(mean, std).sample(&mut thread_rng()) (study-connect4/src/main.rs:43-47) — as a function the device can
 *     compute too: the draw comes from a per-tree counter-based stream instead of thread_rng (reproducible; csrc/noise.cuh),
 *     identical on the device and on the host trees. */
enum { SYN_FPU_CONST = 0, SYN_FPU_PARENT_Q = 1, SYN_FPU_NORMAL = 2, SYN_FPU_FUNC = 3 };
/* config.rs:39-44 PolicyNoise. Dirichlet{alpha, weight} (mcts.rs:241-256) samples rand_distr's Dirichlet on the device from
 * the tree's own stream (csrc/noise.cuh). */
enum { SYN_NOISE_NONE = 0, SYN_NOISE_EQUAL = 1, SYN_NOISE_DIRICHLET = 2 };
/* config.rs:1-7 ValueTarget */
enum { SYN_VALUE_Z = 0, SYN_VALUE_Q = 1, SYN_VALUE_QZ_AVERAGE = 2, SYN_VALUE_Q_TO_Z = 3 };
/* Outcome kind, index order of mcts.rs:10-18 (Into<usize>) */
enum { SYN_OUTCOME_LOSE = 0, SYN_OUTCOME_DRAW = 1, SYN_OUTCOME_WIN = 2 };

/* config.rs:28-37 MCTSConfig */
typedef struct syn_mcts_config {
    int32_t exploration;              /* SYN_EXPLORATION_* */
    float c;                          /* Uct{c} / PolynomialUct{c} */
    int32_t solve;
    int32_t correct_values_on_solve;
    int32_t select_solved_nodes;
    int32_t auto_extend;
    int32_t fpu;                      /* SYN_FPU_* */
    float fpu_value;                  /* Fpu::Const(value); mean of SYN_FPU_NORMAL */
    int32_t root_policy_noise;        /* SYN_NOISE_* */
    float noise_alpha;                /* Dirichlet{alpha,..} */
    float noise_weight;               /* Equal{weight} / Dirichlet{..,weight} */
    float fpu_std;                    /* standard deviation of SYN_FPU_NORMAL (>= 0) */
    float (*fpu_fn)(void);            /* SYN_FPU_FUNC: Fpu::Func's fn() -> f32 (config.rs:25); NULL otherwise */
} syn_mcts_config;

/* config.rs:46-56 RolloutConfig (num_workers has no meaning here: concurrency is syn_engine_config.concurrent_games) */
typedef struct syn_rollout_config {
    int32_t num_explores;
    int32_t random_actions_until;
    int32_t sample_actions_until;
    int32_t stop_games_when_solved;
    int32_t value_target;             /* SYN_VALUE_* */
    float value_target_p;             /* QZaverage{p} */
    float value_target_from;          /* QtoZ{from,..} */
    float value_target_to;            /* QtoZ{..,to} */
    int32_t action;                   /* SYN_ACTION_* */
    syn_mcts_config mcts_cfg;
} syn_rollout_config;

typedef struct syn_engine_config {
    int32_t concurrent_games;   /* trees resident on the GPU at once (BASELINE: 4096); rounded up to a multiple of 16 */
    int32_t max_explores;       /* node-pool slab per tree = 1 + 9*(max_explores+1) nodes */
    int32_t policy_cache_log2;  /* PolicyWithCache (policies/cache.rs:19-32) on the device: 0 = off, else a table of
                                 * 2^policy_cache_log2 entries of 64 bytes (10..30) shared by all games of the engine;
                                 * semantics-neutral (the network is deterministic), used by the lane-per-tree kernel */
    int32_t reserved1;
} syn_engine_config;

typedef struct syn_engine syn_engine;

/* Fills the deterministic parity configuration: policy_mcts_cfg of study-connect4/src/main.rs:58-66 inside the
 * rollout_cfg of main.rs:28-36 (explores 800 per BASELINE.json; the reference default is 1600). */
void syn_default_rollout_config(syn_rollout_config* cfg);

/* ---- lifecycle ------------------------------------------------------------------------------------------------- */

/* Replaces: VarStore::new + P::new(&vs) per worker (alpha_zero.rs:192-193). Allocates the device node pool. */
int syn_engine_create(const syn_engine_config* cfg, int device, syn_engine** out);
int syn_engine_destroy(syn_engine* h);
const char* syn_last_error(const syn_engine* h);

/* Replaces: vs.load(models/model_i.ot) (alpha_zero.rs:194). blob = l_1.weight[128x63], l_1.bias[128],
 * l_2.weight[96x128], l_2.bias[96], l_3.weight[64x96], l_3.bias[64], l_4.weight[48x64], l_4.bias[48],
 * l_5.weight[12x48], l_5.bias[12] (VarStore names, study-connect4/src/policies.rs:20-24), row-major [out][in],
 * n_floats must be 30492. Empties the policy cache (its entries belong to the previous network). */
int syn_load_weights(syn_engine* h, const float* blob, size_t n_floats);
/* The conv policy/value network BASELINE.json's north_star words — slimnn Conv2d (slimnn/src/conv.rs:45-85) over the 2x7x9
 * bitplane state + Linear policy/value heads (slimnn/src/linear.rs:17-25) — behind the same Policy::eval surface
 * (policies/traits.rs:4-6): x[2][7][9] = (mine, theirs) -> Conv2d<2, 16, 3, pad 1, stride 1> + ReLU -> Linear<1008, 12>, logits =
 * out[0..9], value = softmax(out[9..12]). The reference ships the layers but no such network, so the architecture is this
 * library's (oracle/nn.hpp Connect4ConvNet restates it). blob = conv.weight[16][2][3][3], conv.bias[16], head.weight[12][1008],
 * head.bias[12]; n_floats must be 12412. Replaces the engine's network: syn_policy_eval_batch*, syn_mcts_search and
 * syn_selfplay_run then evaluate this network (lane-per-tree kernels: max_explores <= 7280, else SYN_ERR_UNSUPPORTED), in the
 * engine's network arithmetic (an engine in SYN_NET_ARITH_F16X2 builds the network's f16x2 image first; a blob without an f16x2 plan
 * is then refused and changes nothing); syn_load_weights / syn_trainer_publish_weights switch back to Connect4Net. Empties the
 * policy cache. */
int syn_load_weights_conv(syn_engine* h, const float* blob, size_t n_floats);

/* The arithmetic the network (Connect4Net or Connect4ConvNet) is evaluated in. The reference's own is f32 (libtorch `y = x W^T + b`, study-connect4/src/policies.rs:
 * 28-44; slimnn/src/linear.rs:17-25 in its Rust-only form); both choices below compute that function and differ in rounding only.
 *   SYN_NET_ARITH_F32   (default) every product and sum in f32 on v_mfma_f32_16x16x4_f32, ascending input order, fused
 *                       multiply-add per term: bit for bit oracle/nn.hpp's ACC_FMA, within 1e-5 of slimnn's order.
 *   SYN_NET_ARITH_F16X2 every weight and activation as a pair of f16 numbers (hi + lo, 22-23 significand bits, exact power-of-two
 *                       scales chosen per checkpoint from a bound on the activations), products hi.hi + hi.lo + lo.hi on
 *                       v_mfma_f32_16x16x32_f16 with f32 accumulation: 5.3x fewer matrix-pipe cycles per evaluation. Bit for bit
 *                       oracle/nn_f16x2.hpp (which restates the instruction's accumulation, identified on MI355X); as close to
 *                       an f64 evaluation as the f32 arithmetic is (profiles/r05_f16_split.txt: 1.0e-7 against 1.0e-7 on the
 *                       random-init network, 1.8e-4 against 2.3e-4 on logits of magnitude 258 of a trained one).
 *                       Connect4ConvNet: the conv layer's weights split the same way against its exact 0 / 1 inputs (w_hi.x +
 *                       w_lo.x), the head as above on the conv tile's activations (csrc/conv_f16x2_tile.cuh states the definition;
 *                       222 instead of 567 matrix instructions per 16 positions, each half the cycles of an f32 one; measured
 *                       self-play at 800 explores: 1.65x the f32 conv network's games/s).
 * The choice holds for syn_policy_eval_batch*, syn_eval_ctx_*, syn_mcts_search and syn_selfplay_run — and for parameters loaded or
 * published later (syn_load_weights, syn_load_weights_conv, syn_trainer_publish_weights of either learner keep it) — until changed;
 * either switch empties the policy cache. F16X2 needs max_explores <= 7280 (lane-per-tree kernels) and finite parameters whose scales
 * fit the f32-safe window; a refused switch or load changes nothing. Results under the two arithmetics differ in the last bits of the logits, so searches may differ where two
 * moves are within rounding of each other — which is why the choice is the caller's and never made silently. */
enum { SYN_NET_ARITH_F32 = 0, SYN_NET_ARITH_F16X2 = 1 };
int syn_set_network_arithmetic(syn_engine* h, int arithmetic);
/* The scales of the f16x2 plan of the engine's current network (valid = 0 when there is none): layer l's inputs are multiplied
 * by 2^activation_exp[l], its weights by 2^weight_exp[l]; bound[l] = the bound on layer l's outputs the next exponent was chosen
 * from; raw outputs = accumulators * 2^out_exp. Connect4Net: layers 0..4. Connect4ConvNet: layer 0 = the conv layer (its 0 / 1
 * inputs unscaled: activation_exp[0] = 0), layer 1 = the head, entries 2..4 zero. arithmetic / plan may be NULL. */
typedef struct syn_f16x2_plan {
    int valid;
    int activation_exp[5];
    int weight_exp[5];
    int out_exp;
    double bound[5];
} syn_f16x2_plan;
int syn_get_network_arithmetic(syn_engine* h, int* arithmetic, syn_f16x2_plan* plan);
/* The same plan for a parameter blob without an engine (pure host code, no GPU needed): what syn_set_network_arithmetic would choose for
 * these parameters; n_floats selects the network (30492: Connect4Net, 12412: Connect4ConvNet, else SYN_ERR_INVALID_ARGUMENT). SYN_OK
 * with plan->valid = 0 when the blob has no plan (non-finite parameters, a layer's scales outside the f32-safe window |s + t| <= 60, or a
 * bias that is not a finite f32 at its layer's scale). */
int syn_f16x2_plan_of_blob(const float* blob, size_t n_floats, syn_f16x2_plan* plan);

/* ---- leaf evaluation ------------------------------------------------------------------------------------------- */

/* Replaces: Policy::eval (study-connect4/src/policies.rs:47-59) for n states at once. State i is the position with
 * bitboards (my_bb[i], op_bb[i]) in the layout of connect4.rs:3-13 (my_bb = side to move). Outputs: logits[n*9] raw
 * policy logits, value[n*3] = softmax over [lose, draw, win]. Up to 32,768 positions the call runs on the engine's own
 * evaluation context (below): 14 us for n <= 16, 27 us for 4,096; beyond, pageable transfers around the throughput kernel.
 * Side effects differ by size: a batch of up to 32,768 positions runs on that context's own non-blocking stream — it does NOT wait
 * for work queued on the engine stream (e.g. a preceding syn_policy_eval_batch_device(..., sync = 0)) and syn_last_timing reports 0
 * for it; larger batches run on the engine stream, drain it and are timed. Not re-entrant: the engine's context is one per engine
 * (two threads evaluating at once take one syn_eval_ctx each). */
int syn_policy_eval_batch(syn_engine* h, const uint64_t* my_bb, const uint64_t* op_bb, int n, float* logits,
                          float* value);
/* Same with all four pointers resident in device memory (no PCIe in the call); asynchronous on the engine stream
 * unless sync != 0. */
int syn_policy_eval_batch_device(syn_engine* h, const uint64_t* d_my_bb, const uint64_t* d_op_bb, int n,
                                 float* d_logits, float* d_value, int sync);

/* Replaces: one worker's policy object. gather_experience gives every worker thread its own policy (alpha_zero.rs:192-198:
 * VarStore, P::new, cache — "one policy per thread, &mut self eval"); an evaluation context is that object on the GPU: its own
 * stream, pinned staging and device scratch, reading the engine's weight image (loaded once, syn_load_weights*). Contexts of one
 * engine may be used at the same time from different host threads — one thread per context at a time; the engine handle's
 * own calls stay single-threaded as before. Loading other weights while a context has a batch in flight is the caller's race.
 *   submit: copies the n positions and launches their evaluation; returns without waiting (one batch in flight per context).
 *   wait:   blocks until the submitted batch is done and copies logits[n*9] / value[n*3] out (syn_policy_eval_batch's outputs,
 *           bit for bit).  eval = submit + wait.
 * A call is latency (n = 1 from a Rust `impl Policy`; the leaves of a few hundred trees from a self-play worker): the positions
 * are read and small results written across the host link in place, no transfer commands. Errors: the usual codes, the text in
 * syn_eval_ctx_last_error(ctx) (not in the engine's slot; a text starting with "note:" beside SYN_OK reports a completion word that
 * went missing — the answers were complete, the context has switched to waiting on its stream). Destroy every context before
 * syn_engine_destroy. */
typedef struct syn_eval_ctx syn_eval_ctx;
int syn_eval_ctx_create(syn_engine* h, syn_eval_ctx** out);
int syn_eval_ctx_submit(syn_eval_ctx* ctx, const uint64_t* my_bb, const uint64_t* op_bb, int n);
int syn_eval_ctx_wait(syn_eval_ctx* ctx, float* logits, float* value);
int syn_eval_ctx_eval(syn_eval_ctx* ctx, const uint64_t* my_bb, const uint64_t* op_bb, int n, float* logits, float* value);
const char* syn_eval_ctx_last_error(const syn_eval_ctx* ctx);
int syn_eval_ctx_destroy(syn_eval_ctx* ctx);

/* Replaces: Game::features (connect4.rs:235-258) for n states: out[n*63], index row*9 + col. */
int syn_features_batch(syn_engine* h, const uint64_t* my_bb, const uint64_t* op_bb, int n, float* out);

/* ---- slimnn layer semantics (slimnn/src/linear.rs:17-25, conv.rs:45-85, activations.rs) ------------------------- */
/* y[batch][O] = b + sum_i x[batch][i] * W[o][i], accumulated in ascending i with separate multiply and add. */
int syn_linear_forward(syn_engine* h, int I, int O, const float* W, const float* b, const float* x, int batch,
                       float* y, int relu);
/* slimnn activations as layers on x[batch][n] (slimnn/src/activations.rs:31-63): SYN_ACT_RELU = x.max(0.0); SYN_ACT_TANH =
 * x.tanh() (a deterministic tanh shared with the oracle: Rust's f32::tanh is libm, unpinned); SYN_ACT_SOFTMAX =
 * Softmax::apply_1d per row — exp of every element with NO max subtraction, summed in index order, divided by the total. */
enum { SYN_ACT_RELU = 0, SYN_ACT_TANH = 1, SYN_ACT_SOFTMAX = 2 };
int syn_activation_forward(syn_engine* h, int kind, const float* x, int batch, int n, float* y);
/* NCHW cross-correlation; W[COUT][CIN][K][K]; x[batch][CIN][H_IN][W_IN]; y[batch][COUT][H_OUT][W_OUT]; accumulation
 * order ci -> k1 -> k2. H_OUT/W_OUT must satisfy conv.rs:50-51 or SYN_ERR_INVALID_ARGUMENT is returned. */
int syn_conv2d_forward(syn_engine* h, int CIN, int COUT, int K, int ROW_PAD, int COL_PAD, int STRIDE, int H_IN,
                       int W_IN, int H_OUT, int W_OUT, const float* W, const float* b, const float* x, int batch,
                       float* y, int relu);

/* ---- search ---------------------------------------------------------------------------------------------------- */

/* Per-root result of a search; child_* arrays are indexed by ACTION (column); entries of columns that are not
 * children of the root are zero. */
typedef struct syn_search_result {
    float child_N[9];          /* Node::num_visits                     (mcts.rs:38) */
    float child_W[9][3];       /* Node::outcome_probs [lose,draw,win]  (mcts.rs:37) */
    float child_P[9];          /* Node::action_prob                    (mcts.rs:36) */
    int32_t child_sol[9][3];   /* {is_some, kind, turns} of Node::solution (mcts.rs:34) */
    float root_N;
    float root_W[3];
    int32_t root_sol[3];
    uint32_t num_nodes;        /* nodes.len() */
    int32_t best_action;       /* MCTS::best_action (mcts.rs:273-294) */
    float target_pi[9];        /* MCTS::target_policy (mcts.rs:174-211) */
    float target_q[3];         /* MCTS::target_q (mcts.rs:213-225) */
} syn_search_result;

/* Replaces: MCTS::with_capacity(explores+1, cfg, policy, root) + explore_n(explores) (mcts.rs:123-147) for n
 * independent roots, each on its own device-resident tree. */
int syn_mcts_search(syn_engine* h, const syn_mcts_config* cfg, const uint64_t* my_bb, const uint64_t* op_bb, int n,
                    int explores, int action_selection, syn_search_result* results);

/* Replaces: MCTS<G, RolloutPolicy> (the pairing of the reference's MCTS tests, mcts.rs:691-868): the same search with
 * RolloutPolicy (policies/rollout.rs:8-31) as the leaf evaluation — uniformly random playouts, zero logits, one-hot outcome. Root i
 * draws its playouts from its own StdRng::seed_from_u64(seed + i), in explore order. No network weights are needed. */
int syn_mcts_search_rollout(syn_engine* h, const syn_mcts_config* cfg, uint64_t seed, const uint64_t* my_bb,
                            const uint64_t* op_bb, int n, int explores, int action_selection, syn_search_result* results);

/* Replaces: the same reference call as syn_mcts_search — MCTS::with_capacity + explore_n for n roots (mcts.rs:123-147) — in the
 * reference's own division of labour (BASELINE.json configs[1] as worded: concurrent games, batched leaf inference): the trees
 * live on the HOST (include/synthesis_amd_lockstep.hpp: MCTS<G, P, N> restated over any Game, Policy::eval taken out of visit()),
 * and the leaves go to the GPU in batches: the roots are divided among host_threads workers (gather_experience's worker model,
 * alpha_zero.rs:132-154); a worker runs its trees in two halves that take turns — one half's leaves are being evaluated while it
 * advances the other — and the batches the workers hand in are combined into one launch on one evaluation context
 * (syn_eval_ctx_*). This is the driver a caller with a different Game impl instantiates; for Connect4 the fused syn_mcts_search
 * is the fast path and this entry point exists to hold the driver to it: results are identical, field for field. host_threads:
 * 0 = what the process may use (hardware concurrency cut to a cgroup CPU quota), at most 32. cfg: every configuration syn_mcts_search takes and SYN_FPU_FUNC (a host function pointer: this is where it can be called) — SYN_FPU_NORMAL and SYN_NOISE_DIRICHLET
 * draw what syn_mcts_search draws (root i: tree stream (i, turn 0)). stats may be NULL. */
typedef struct syn_lockstep_stats {
    uint64_t rounds;               /* evaluation launches (combined batches) */
    uint64_t positions_evaluated;  /* leaves over all launches */
    double seconds_total;
    double seconds_policy;         /* host time inside the evaluation context's calls (staging, launch, waiting for the GPU) */
} syn_lockstep_stats;
int syn_mcts_search_lockstep(syn_engine* h, const syn_mcts_config* cfg, const uint64_t* my_bb, const uint64_t* op_bb, int n,
                             int explores, int action_selection, int host_threads, syn_search_result* results,
                             syn_lockstep_stats* stats);
/* Replaces: run_n_games (alpha_zero.rs:181-209) in the same division of labour — BASELINE.json configs[1] as worded: concurrent
 * games (syn_selfplay_run's shape: n_games jobs over the engine's concurrent_games slots, a finished game's slot takes the next
 * game), every game's MCTS on the HOST (one tree per move, alpha_zero.rs:240-244), the leaves batched to the GPU as above,
 * run_game / sample_action / fill_state_info / store_rewards (alpha_zero.rs:229-338) on the host with game g's own
 * StdRng::seed_from_u64(base_seed + g) (include/synthesis_amd_lockstep.hpp::lockstep_selfplay_sharded).
 * Arguments and outputs are syn_selfplay_run's; the games are identical to that call's, move for move and float for float.
 * host_threads as above; SYN_FPU_FUNC, SYN_FPU_NORMAL (the reference's own self-play configuration) and SYN_NOISE_DIRICHLET included — the
 * host trees take the draws of syn_selfplay_run's trees; stats may be NULL. */
int syn_selfplay_run_lockstep(syn_engine* h, const syn_rollout_config* cfg, uint64_t base_seed, uint64_t first_game, int n_games,
                              int host_threads, int32_t* plies, uint64_t* states_bb, float* pis, float* vs, uint8_t* actions,
                              uint32_t* root_nodes, uint8_t* final_kind, syn_lockstep_stats* stats);

/* ---- evaluator baseline ---------------------------------------------------------------------------------------- */

/* One root of the evaluator's baseline tree after the search (evaluator.rs:233-243 Node fields of the root's children,
 * indexed by action; children of illegal actions are all-zero). */
typedef struct syn_frozen_result {
    float child_N[9];          /* Node::num_visits  */
    float child_cum[9];        /* Node::cum_value   */
    float child_P[9];          /* Node::action_prob */
    int32_t child_sol[9][3];   /* {is_some, kind (0 Lose, 1 Draw, 2 Win), turns} of Node::solution */
    float root_N;
    float root_cum;
    int32_t root_sol[3];
    uint32_t num_nodes;        /* nodes.len() */
    int32_t best_action;       /* FrozenMCTS::best_action (evaluator.rs:364-389) */
} syn_frozen_result;

/* Replaces: FrozenMCTS::exploit(explores, cfg, &mut RolloutPolicy { rng }, game, action_selection) (evaluator.rs:308-319
 * with policies/rollout.rs:8-31) — the "VanillaMCTS<explores>" baseline of eval_against_rollout_mcts / mcts_vs_mcts
 * (evaluator.rs:163-228) — for n independent roots, one device-resident tree each. Root i draws its playouts from
 * StdRng::seed_from_u64(seeds[i]) starting at 32-bit output word rng_words[i]; on return rng_words[i] is the first word the
 * search did not use, so a caller that replays a match move by move keeps ONE generator per match as the reference does
 * (pass 0 for the first move, hand the value back for the next). explores[i] is per root (mcts_vs_mcts gives each side its own).
 * The trees live in the engine's node pool, re-partitioned per call for the largest explores[i] of the batch (1 + 9 records of
 * 16 bytes per visit), so searches far deeper than the engine's max_explores run, fewer at a time (up to 233,014 explores:
 * the reference's largest baseline is VanillaMCTS204800); SYN_ERR_CAPACITY if not even one such tree fits.
 * cfg: Exploration::Uct and Fpu::Const only — the reference panics on anything else (SYN_ERR_UNSUPPORTED here); the
 * baseline ignores every other field except `solve`. No network weights are needed. */
int syn_frozen_search_rollout(syn_engine* h, const syn_mcts_config* cfg, const uint64_t* seeds, uint64_t* rng_words,
                              const uint64_t* my_bb, const uint64_t* op_bb, const int32_t* explores, int n,
                              int action_selection, syn_frozen_result* results);

/* ---- matches between two networks ------------------------------------------------------------------------------ */

/* One side of a match: MCTS::exploit's arguments (evaluator.rs:129-160). */
typedef struct syn_match_player {
    int32_t explores;          /* per-move explores, <= the engine's max_explores */
    int32_t action;            /* SYN_ACTION_* */
    syn_mcts_config mcts_cfg;
} syn_match_player;

/* Replaces: the game loop of eval_against_old (evaluator.rs:129-160) for n_games games between two networks, from given start
 * positions, without leaving the device between the first ply and the last. Game g starts at (start_my[g], start_op[g]) with
 * `first` to move there (start_my = the mover's stones), whatever the stone counts say. Ply k of every game is searched by player
 * k % 2 with that player's parameters, configuration and explores — MCTS::with_capacity + explore_n, then best_action
 * (mcts.rs:123-147, 273-294): what syn_mcts_search returns for that root — and the move played is best_action.
 *   rewards[g]   +1 / 0 / -1 for `first` (game.reward, evaluator.rs:160); a full board without four in a row is a draw
 *   plies[g]     moves played in the match (not counting the stones of the start position)
 *   moves        n_games x 63 columns, 255 from the game's end on; may be NULL
 *   final_bb     n_games x 2: the stones of `first`, then of `second`, after the last move; may be NULL
 * Both blobs are parameters of the engine's current network kind (n_floats = 30492 for Connect4Net, 12412 for Connect4ConvNet, else
 * SYN_ERR_INVALID_ARGUMENT) and are evaluated in the engine's current network arithmetic (f16x2: a blob without a plan is
 * SYN_ERR_UNSUPPORTED). They are built into two image buffers the match owns: the engine's own network, its f16x2 image and its policy
 * cache are bit for bit what they were before the call, and the match's searches neither read nor write the cache. The engine needs no
 * weights of its own.
 * Deterministic players only: SYN_FPU_NORMAL, SYN_FPU_FUNC and SYN_NOISE_DIRICHLET are SYN_ERR_UNSUPPORTED (their draws are keyed by
 * job index, which changes as games end). explores above max_explores is SYN_ERR_CAPACITY. A start position must pass
 * syn_mcts_search's check and neither side may have four in a row there (SYN_ERR_INVALID_ARGUMENT). Every refusal happens before
 * anything changes. n_games may exceed concurrent_games (the searches queue as in syn_mcts_search); n_games == 0 is SYN_OK.
 * Per ply the host launches the search, three small kernels and a scan and reads back four words (where the games of either mover
 * start in the live arrays, how many go on, and the ply's error word: the loop is syn_tournament_run's with two players); nothing is
 * uploaded after the first launch. syn_last_timing: the summed device time of all plies and the number of launches (four per ply:
 * search, advance, and the regroup's count and scatter). syn_cancel: the call returns SYN_ERR_CANCELLED after the ply in flight and the outputs are
 * unspecified; syn_progress reports the current ply's search. */
int syn_match_run(syn_engine* h, const syn_match_player* first, const syn_match_player* second, const float* blob_first,
                  const float* blob_second, size_t n_floats, const uint64_t* start_my, const uint64_t* start_op, int n_games,
                  float* rewards, int32_t* plies, uint8_t* moves, uint64_t* final_bb);

/* What plays one side of a match, and for a network side the arithmetic its parameters are evaluated in. */
enum { SYN_MATCH_SIDE_NETWORK = 0, SYN_MATCH_SIDE_BASELINE = 1 };
enum { SYN_MATCH_ARITH_ENGINE = 0, SYN_MATCH_ARITH_F32 = 1, SYN_MATCH_ARITH_F16X2 = 2 };
typedef struct syn_match_side {
    int32_t kind;          /* SYN_MATCH_SIDE_* */
    int32_t arithmetic;    /* SYN_MATCH_ARITH_*; network sides only */
    syn_match_player player;
    const float* blob;     /* network sides: parameters of the engine's network kind; baseline sides: NULL */
    size_t n_floats;
} syn_match_side;

/* syn_match_run with a description per side. A zero-initialised kind / arithmetic means "network side, the engine's arithmetic": two
 * such sides make the call behave as syn_match_run does, bit for bit (that call is this one with two such sides).
 * Network side (SYN_MATCH_SIDE_NETWORK): what syn_match_run plays — MCTS::with_capacity + explore_n + best_action, the policy cache
 *   off, deterministic configurations only, explores <= max_explores. `arithmetic` chooses the image this side's blob is built into
 *   and the kernel family its plies launch, independently of the other side and of the engine: SYN_MATCH_ARITH_F32 against
 *   SYN_MATCH_ARITH_F16X2 is one checkpoint's two arithmetics meeting, on an engine in either. SYN_MATCH_ARITH_F16X2 on a blob without
 *   an f16x2 plan is SYN_ERR_UNSUPPORTED. The engine's own network, arithmetic, f16x2 image, host blob and policy cache are bit for
 *   bit what they were before the call.
 * Baseline side (SYN_MATCH_SIDE_BASELINE): FrozenMCTS::exploit(explores, cfg, &mut RolloutPolicy{rng}, game, action)
 *   (evaluator.rs:308-319), the "VanillaMCTS<explores>" of eval_against_rollout_mcts / mcts_vs_mcts (evaluator.rs:163-228): what
 *   the baseline search above computes for that root. Game g owns ONE generator, StdRng::seed_from_u64(seeds[g]), for the whole game,
 *   from output word 0; every baseline ply of the game advances it, whichever side the ply belongs to (two baseline sides share it,
 *   evaluator.rs:207-208), and a network ply does not touch it. rng_words[g] (may be NULL) is the first unused word when the game
 *   ended (0 for every game when neither side is a baseline). seeds may be NULL only when neither side is a baseline.
 *   player.mcts_cfg must be Exploration::Uct + Fpu::Const (else SYN_ERR_UNSUPPORTED); player.explores is bounded by the node pool as
 *   in the baseline search (SYN_ERR_CAPACITY), not by max_explores; blob and n_floats are ignored and no weights are needed. The
 *   generator's state stays on the device and follows its game through the regroup; a stream position past 0xC0000000 (the
 *   baseline search's supported length) is detected on the device after the ply that reached it and ends the call with
 *   SYN_ERR_CAPACITY: it is never wrapped.
 * An unknown kind or arithmetic is SYN_ERR_INVALID_ARGUMENT. Everything else — start positions, the other outputs, refusals before
 * anything changes, n_games beyond the engine's slots, n_games == 0, four words read back per ply and nothing uploaded after the first
 * launch, the timing summed over plies, cancellation after the ply in flight — is as documented for syn_match_run. Both kinds of
 * search use the engine's node pool and alternate on one stream. */
int syn_match_run_sides(syn_engine* h, const syn_match_side* first, const syn_match_side* second, const uint64_t* start_my,
                        const uint64_t* start_op, const uint64_t* seeds, int n_games, float* rewards, int32_t* plies, uint8_t* moves,
                        uint64_t* final_bb, uint64_t* rng_words);

/* ---- tournaments between K players ----------------------------------------------------------------------------- */

#define SYN_TOURNAMENT_MAX_PLAYERS 64
/* A whole schedule of games between n_players players in ONE device-resident loop. players[p] is a side exactly as
 * syn_match_run_sides takes it (a network side with its own blob, search settings and arithmetic, or a VanillaMCTS<n> baseline side).
 * Game g starts at (start_my[g], start_op[g]) with players[first[g]] to move there and players[second[g]] moving second, on the
 * generator StdRng::seed_from_u64(seeds[g]) (seeds may be NULL only when no player is a baseline side).
 * Definition: game g's record — rewards[g] for the first mover, plies[g], its 63 move slots, final_bb[g] (the first mover's stones, the
 * second mover's) and rng_words[g] — is bit for bit what
 *     syn_match_run_sides(h, &players[first[g]], &players[second[g]], &start_my[g], &start_op[g], &seeds[g], 1, ...)
 * returns for that one game: a game's record depends on its own position and generator alone, never on its job index.
 * first[g] == second[g] (a player against itself) and a player that appears in no game are allowed. n_games == 0 is SYN_OK.
 * Every refusal of syn_match_run_sides is a refusal here, for any player of the call whether it plays or not, before anything of the
 * engine or the device changes; also n_players outside 1 .. SYN_TOURNAMENT_MAX_PLAYERS and an index outside [0, n_players)
 * (SYN_ERR_INVALID_ARGUMENT, naming the game). The engine's own network, host blob, f16x2 image and policy cache stay untouched: the
 * call owns one image buffer per network player, and its searches run with the cache off.
 * The loop: at ply t every live game is at the same parity, and the live games are kept grouped by the player that moves (game order
 * inside a group). Per ply: ONE search launch per player that has games to move in, over all of them whatever pairing each belongs
 * to; the advance kernel per group; a stable (n_players + 1)-way regroup by the next mover (two kernels and a scan); n_players + 2
 * words read back (the groups' starts and the ply's error word). Nothing is uploaded after the first launch.
 * syn_last_timing: the summed device time of all plies and the number of launches (two per non-empty group and two for the regroup,
 * per ply). syn_cancel, syn_progress, the capacity errors and the 63-ply bound behave as documented for syn_match_run. */
int syn_tournament_run(syn_engine* h, const syn_match_side* players, int n_players, const int32_t* first, const int32_t* second,
                       const uint64_t* start_my, const uint64_t* start_op, const uint64_t* seeds, int n_games, float* rewards,
                       int32_t* plies, uint8_t* moves, uint64_t* final_bb, uint64_t* rng_words);

/* ---- self-play ------------------------------------------------------------------------------------------------- */

/* Event counters summed over all games of a run (definitions: SURVEY.md §8d; used for algorithmic-bytes accounting) */
typedef struct syn_counters {
    uint64_t explores;          /* MCTS::explore calls + root visits */
    uint64_t select_levels;     /* select_best_child calls */
    uint64_t children_scanned;  /* children examined by select_best_child */
    uint64_t expansions;        /* visit() bodies that created children */
    uint64_t new_nodes;         /* nodes created */
    uint64_t policy_evals;      /* Policy::eval calls = leaf evaluations */
    uint64_t backprop_levels;   /* nodes updated by backprop */
    uint64_t solver_children;   /* child solutions read by the solver branch of backprop */
    uint64_t solved_hits;       /* explores that ended on an already solved node */
    uint64_t moves;             /* plies played */
    uint64_t games;             /* games finished */
    uint64_t max_depth;         /* longest root-to-leaf chain (levels) any backprop walked */
} syn_counters;

/* Replaces: run_n_games (alpha_zero.rs:181-209) for games [first_game, first_game + n_games). Game g uses its own
 * StdRng::seed_from_u64(base_seed + g). Output slot j = g - first_game. Any output pointer may be
 * NULL.  plies[n]; states_bb[n][63][2] = (my_bb, op_bb) of every recorded position (ReplayBuffer.games, data.rs:151-158);
 * pis[n][63][9]; vs[n][63][3] (after store_rewards, alpha_zero.rs:309-338); actions[n][63]; root_nodes[n][63] =
 * nodes.len() of each move's tree; final_kind[n] = outcome kind for the side to move in the final position.
 * counters may be NULL. */
int syn_selfplay_run(syn_engine* h, const syn_rollout_config* cfg, uint64_t base_seed, uint64_t first_game,
                     int n_games, int32_t* plies, uint64_t* states_bb, float* pis, float* vs, uint8_t* actions,
                     uint32_t* root_nodes, uint8_t* final_kind, syn_counters* counters);

/* ---- learner step and replay de-duplication (the step right after the self-play path) ---------- */

/* LearningConfig's optimiser fields (config.rs:76-94) + Adam::default() (alpha_zero.rs:33-36) */
typedef struct syn_train_config {
    float weight_decay;    /* LearningConfig::weight_decay (study-connect4/src/main.rs:20: 1e-6) */
    float policy_weight;   /* LearningConfig::policy_weight */
    float value_weight;    /* LearningConfig::value_weight */
    float beta1;           /* 0.9 */
    float beta2;           /* 0.999 */
    float eps;             /* 1e-8 */
} syn_train_config;

/* Replaces: P::new(&vs) + Adam::default().build(&vs, lr) (alpha_zero.rs:31-36): parameters (same blob order as
 * syn_load_weights) and zeroed Adam moments on the device. The first call on an engine also runs a ~1 ms self-check of the epoch
 * kernel's step barrier (eight steps on a synthetic batch through the fast and the device-scope barrier, compared bit for bit; a
 * mismatch makes this engine use the device-scope barrier) and thereby discards a data set uploaded with syn_train_set_data
 * before it: upload after initialising. */
int syn_trainer_init(syn_engine* h, const float* blob, size_t n_floats, const syn_train_config* cfg);
/* The same for Connect4ConvNet (syn_load_weights_conv's network and blob order, 12412 floats): the trainer then runs that
 * network through syn_train_step / syn_train_gradients_device + syn_train_apply_device / syn_train_set_data + syn_train_epoch
 * (minibatches of at most 32 positions, else SYN_ERR_UNSUPPORTED), syn_trainer_get_state copies 12412 floats per array, and
 * syn_trainer_publish_weights makes the trained conv network the engine's policy (in the engine's network arithmetic). f32, the arithmetic order of
 * oracle/train.hpp::ConvTrainer (checked against torch float64 goldens); an engine trains one network at a time. Like
 * syn_trainer_init, the first call on an engine runs a self-check (eight steps on a synthetic batch through the four-workgroup
 * epoch kernel and through the one-workgroup kernel, compared bit for bit) and thereby discards a data set uploaded before it. */
int syn_trainer_init_conv(syn_engine* h, const float* blob, size_t n_floats, const syn_train_config* cfg);
/* Replaces: one iteration of the minibatch loop alpha_zero.rs:76-92 (forward, log_softmax, kl_div(Sum)/batch for both
 * heads, loss, backward_step). States are given as bitboards; losses[2] = {pi_loss, v_loss} (may be NULL). */
int syn_train_step(syn_engine* h, const uint64_t* my_bb, const uint64_t* op_bb, const float* target_pi,
                   const float* target_v, int batch, float lr, float* losses);
/* Data-parallel form (BASELINE configs[4]): gradients of this rank's minibatch into a caller-owned DEVICE buffer of
 * 30,492 floats (all other pointers are device pointers too), to be all-reduced by the caller (RCCL), then applied with
 * syn_train_apply_device(grad_scale = 1/ranks). losses is a host pointer (may be NULL). */
int syn_train_gradients_device(syn_engine* h, const uint64_t* d_my_bb, const uint64_t* d_op_bb, const float* d_target_pi,
                               const float* d_target_v, int batch, float* d_grads, float* losses);
int syn_train_apply_device(syn_engine* h, const float* d_grads, float lr, float grad_scale);
/* The stream-ordered form of the same two calls (one optimiser step of alpha_zero.rs:76-92 split around the RCCL all-reduce, no host
 * in between): both enqueue on `stream` (a hipStream_t of the engine's device: the stream the batch was prepared on and the all-reduce
 * runs on; NULL is the device's null stream — PyTorch's default stream — not the engine's own) and return without synchronising. d_losses: DEVICE pointer to 2 floats {pi-loss sum, v-loss sum}
 * of this rank's minibatch (may be NULL) — typically the two words behind the 30,492 gradients, so they ride in the same message.
 * While a caller drives the trainer this way it keeps the engine's other trainer entry points (which use the engine's stream) idle. */
int syn_train_gradients_enqueue(syn_engine* h, void* stream, const uint64_t* d_my_bb, const uint64_t* d_op_bb, const float* d_target_pi,
                                const float* d_target_v, int batch, float* d_grads, float* d_losses);
int syn_train_apply_enqueue(syn_engine* h, void* stream, const float* d_grads, float lr, float grad_scale);
/* Arithmetic of the Connect4ConvNet learner's gradient step (forward, dZ, backward; BASELINE configs[4] words the on-node training
 * step "bf16 conv"): SYN_TRAIN_F32 (default after every syn_trainer_init*) = f32 matrix cores, bit-identical to the oracle;
 * SYN_TRAIN_BF16 = every matrix operand rounded to bf16 and multiplied on the bf16 matrix cores with f32 accumulation — master
 * weights, Adam moments, the softmax / KL head and Adam itself stay f32. Training only: inference never runs in bf16 (it cannot
 * hold north_star's 1e-5). SYN_ERR_UNSUPPORTED for the Connect4Net learner. No counterpart in the reference (its learner is
 * libtorch f32, alpha_zero.rs:28-37). */
enum { SYN_TRAIN_F32 = 0, SYN_TRAIN_BF16 = 1 };
int syn_trainer_set_precision(syn_engine* h, int precision);
/* How a minibatch above the reference's batch_size of 32 is evaluated (LearningConfig::batch_size is a free parameter: config.rs:86;
 * the minibatch loop: alpha_zero.rs:72-94). SYN_TRAIN_BATCH_CHAINED (default after every syn_trainer_init*) = the oracle's definition:
 * every gradient entry is ONE chain over all samples in ascending order, which one workgroup walks (Connect4Net; the Connect4ConvNet
 * learner refuses more than 32). SYN_TRAIN_BATCH_MICRO = a second, opt-in, deterministic definition that the whole GPU can work on:
 *   a minibatch of B = 32 nb positions, in the order given, is nb micro-batches of 32 (sample 32 j + i = sample i of micro-batch j);
 *   g_j[P], l_j[2] = exactly what the chained step computes for those 32 samples as a minibatch of their own (batch mean 1/32,
 *     policy_weight and value_weight applied, the oracle's chains; in the conv learner's bf16 variant: that variant's step);
 *   acc = g_0, then acc = acc + g_j for j = 1 .. nb-1: plain f32 additions in ascending j (nothing is added to g_0: for nb = 1 every
 *     bit, the sign of a zero included, is the chained step's);
 *   G = acc * inv, inv = 1.0f / (float)nb (an IEEE f32 division; one rounding, fused with nothing); the two losses alike;
 *   Adam is unchanged: the same expression on G, same weight decay, step counter and scalars.
 * G is the gradient of the mean loss over the B samples (a mean of equal-size block means) — gradient averaging over micro-batches of
 * the reference's own batch size — and does not depend on how many workgroups computed it. Every gradient path honours the mode:
 * syn_train_step, syn_train_gradients_device, syn_train_gradients_enqueue (on the caller's stream) and syn_train_epoch, which then
 * queues three launches per step (micro-batch gradients on min(nb, cap) workgroups, the reduction, Adam) with one synchronisation at
 * the end and never uses the persistent kernels; no workgroup waits for another one, so the step also runs beside a self-play launch.
 * max_workgroups caps the gradient launch (0 = one workgroup per CU): a caller who trains beside self-play can leave CUs to it.
 * In this mode batch % 32 != 0 is SYN_ERR_INVALID_ARGUMENT and batch > 32 * 1024 SYN_ERR_UNSUPPORTED, at every entry point above,
 * with the learner left as it was. An unknown mode or a negative cap is SYN_ERR_INVALID_ARGUMENT; before syn_trainer_init*,
 * SYN_ERR_NO_WEIGHTS. No learning rate is rescaled for the larger batch; what large batches do to the trained player is not measured. */
enum { SYN_TRAIN_BATCH_CHAINED = 0, SYN_TRAIN_BATCH_MICRO = 1 };
int syn_trainer_set_batch_mode(syn_engine* h, int mode, int max_workgroups);
/* Any pointer may be NULL. *last_grid = workgroups of the last micro-batch gradient launch on this engine, 0 if there has been none. */
int syn_trainer_get_batch_mode(syn_engine* h, int* mode, int* max_workgroups, int* last_grid);
/* Copies out parameters / Adam moments / last gradient (each may be NULL) and the optimiser step count. */
int syn_trainer_get_state(syn_engine* h, float* blob, float* m, float* v, long long* step, float* grads);
/* The inverse of syn_trainer_get_state (not in the reference, whose learner lives and dies with its process): an initialised trainer of
 * the same network (n_floats must be that network's) gets the parameters, both Adam moments and the optimiser step count set bit for
 * bit, and every derived device image rebuilt the way syn_trainer_init* builds it (Connect4Net: the forward and the transposed fragment
 * image and the epoch kernel's second buffer), so that the next syn_train_step, syn_train_gradients_*, syn_train_epoch (persistent,
 * queued or micro) and syn_train_epochs_sampled continue from the new state exactly as the learner the state was read from would have.
 * Kept as they are: precision, batch mode and workgroup cap, the hyper-parameters, the learner's data set and the evaluation set, the
 * last gradient, the engine's network and the policy cache. Nothing is published and no start-up self-check runs again.
 * Refused, with the trainer bit for bit as it was: before syn_trainer_init* (SYN_ERR_NO_WEIGHTS); a NULL pointer, a wrong n_floats or a
 * negative step (SYN_ERR_INVALID_ARGUMENT). Non-finite values are accepted as they are: this call restores, it does not judge. */
int syn_trainer_set_state(syn_engine* h, const float* blob, const float* m, const float* v, size_t n_floats, long long step);
/* Replaces: vs.save(model_{i+1}.ot) + the workers' vs.load (alpha_zero.rs:97,194): the trained parameters become the
 * engine's policy for syn_policy_eval_batch / syn_mcts_search / syn_selfplay_run, in the arithmetic the engine is in (both learners:
 * an engine in SYN_NET_ARITH_F16X2 gets the published network's f16x2 image). Before this library's Connect4ConvNet f16x2 support,
 * the conv learner's publish reset an f16x2 engine to SYN_NET_ARITH_F32; it no longer does. */
int syn_trainer_publish_weights(syn_engine* h);
/* Epochs without the host in the loop. syn_train_set_data uploads the de-duplicated buffer once per iteration (the
 * tensors `states / target_pis / target_vs` of alpha_zero.rs:52-58, positions as bitboards); syn_train_epoch then runs
 * n_steps optimiser steps in one call: step s trains on the states perm[s*batch .. (s+1)*batch) — the BatchRandSampler's
 * index_select (data.rs:41-62; the caller draws the permutation and applies drop_last) — and step_losses[s][0..1]
 * receives its (pi_loss, v_loss). Bit-identical to n_steps calls of syn_train_step on the gathered batches. For batch <= 32
 * (the reference's batch_size) the whole epoch is ONE persistent kernel launch (csrc/train_epoch.cuh: 16 workgroups, the
 * gradient of the LAST step is what syn_trainer_get_state reports). That kernel needs its 16 workgroups resident together; the
 * learner's state is snapshotted before the launch, and if the workgroups never become co-resident (another kernel holds the CUs:
 * it gives up after ~10 s) the snapshot is restored and the epoch runs through the queued per-step launches instead — same bits,
 * the call still returns SYN_OK. Larger batches queue two launches per step. The Connect4ConvNet learner (syn_trainer_init_conv;
 * minibatches of at most 32) runs an epoch as ONE persistent launch as well (csrc/train_conv_mfma.cuh), in f32 or — after
 * syn_trainer_set_precision(SYN_TRAIN_BF16) — on the bf16 matrix cores: four workgroups of one XCD share every step (same
 * chains, same bits as one workgroup), with the same snapshot; if they never become co-resident, or if the start-up self-check of
 * syn_trainer_init_conv found this engine's four-workgroup kernel disagreeing with the one-workgroup kernel, the epoch is one
 * launch of a single persistent workgroup instead (no co-residency requirement, 2.3x slower). */
int syn_train_set_data(syn_engine* h, const uint64_t* my_bb, const uint64_t* op_bb, const float* target_pi,
                       const float* target_v, size_t n);
int syn_train_epoch(syn_engine* h, const int32_t* perm, size_t n_steps, int batch, float lr, float* step_losses);

/* ---- Device-side epoch sampler (DESIGN.md §6.4 "Device-side epoch sampler"; not in the reference): a second, opt-in definition of
 * "an epoch's order" that the device computes from a 64-bit key, so that an iteration's epochs are ONE call and the host neither draws a
 * permutation nor uploads indices. All arithmetic is unsigned 64-bit with wrap-around:
 *   finalise(z):  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;  z = (z ^ (z >> 27)) * 0x94D049BB133111EB;  return z ^ (z >> 31)
 *   sm(seed, idx) = finalise(seed + (idx + 1) * 0x9E3779B97F4A7C15), idx a uint32 and idx + 1 computed in 32 bits (idx = 2^32 - 1
 *     gives 0) — csrc/noise.cuh noise_splitmix64, the generator behind the self-play noise
 *   SAMPLER_TAG = 0x5AD3C0DE5EED1E55
 *   key of epoch e (a uint32):            K_e = sm(key ^ SAMPLER_TAG, e)
 *   sort key of row i of an n-row set:    k_i = sm(K_e, i), 0 <= i < n <= 2^31 - 1   (the multiplier is odd and finalise a bijection:
 *                                         the k_i are pairwise distinct, so the order below is unique)
 *   perm_e = the row indices in ascending order of k_i;   flip_e[i] = k_i & 1
 * Epoch e runs n_steps = n / batch optimiser steps (drop_last); step s takes the rows perm_e[s*batch .. (s+1)*batch) in that order. With
 * flip = SYN_SAMPLER_FLIP_RANDOM a row i with flip_e[i] = 1 enters as (mirror my, mirror op, pi[8 - c], v) — the left-right mirror
 * image of "Mirror symmetry" below — otherwise, and always with SYN_SAMPLER_FLIP_NONE, as stored. The stored data set is never modified.
 *
 * syn_train_epochs_sampled runs the epochs first_epoch .. first_epoch + n_epochs - 1 over the learner's current data set
 * (syn_train_set_data / syn_replay_deduplicate_to_trainer[_symmetric]): per epoch a key kernel, a radix sort of the n (k_i, i) pairs,
 * a gather of the first n_steps*batch sorted rows with the flip folded in, and then exactly what syn_train_epoch runs on its gathered
 * batches — the same persistent kernels with their snapshot / give-up / queued fallback, the queued launches above 32 positions and
 * SYN_TRAIN_BATCH_MICRO with its rules — so epoch e leaves the bits of syn_train_epoch(perm_e[0 .. n_steps*batch)) over the data set
 * with the flagged rows mirrored. step_losses ([n_epochs][n_steps][2], may be NULL) receives every step's (pi_loss, v_loss);
 * *n_steps (may be NULL) = steps per epoch. The optimiser step count advances by n_epochs * n_steps.
 * n < batch (*n_steps = 0) and n_epochs = 0 are SYN_OK with the learner unchanged. Refused, with the learner bit for bit as it was:
 * cfg NULL, flip outside {0, 1}, n_epochs < 0, batch < 1, first_epoch + n_epochs > 2^32 (SYN_ERR_INVALID_ARGUMENT; also when there is
 * no data set), no trainer (SYN_ERR_NO_WEIGHTS), and SYN_TRAIN_BATCH_MICRO's refusals of a batch (syn_trainer_set_batch_mode).
 * Whether random flipping trains a stronger player is not measured (tools/arena.py is the instrument).
 *
 * syn_debug_sampler: perm_e and flip_e of epoch `epoch` alone for n rows (1 <= n <= 2^31 - 1) as host arrays: perm_out[n] in step
 * order, flip_out[n] indexed by ROW (either may be NULL). cfg->key is used, first_epoch and flip are ignored; needs no trainer. */
typedef struct syn_sampler_config {
    uint64_t key;
    uint32_t first_epoch;
    int32_t flip; /* SYN_SAMPLER_FLIP_* */
} syn_sampler_config;
enum { SYN_SAMPLER_FLIP_NONE = 0, SYN_SAMPLER_FLIP_RANDOM = 1 };
int syn_train_epochs_sampled(syn_engine* h, const syn_sampler_config* cfg, int n_epochs, int batch, float lr,
                             float* step_losses /* [n_epochs][n_steps][2], may be NULL */, size_t* n_steps /* per epoch, out */);
int syn_debug_sampler(syn_engine* h, const syn_sampler_config* cfg, uint32_t epoch, size_t n, int32_t* perm_out, uint8_t* flip_out);

/* Replaces: ReplayBuffer::deduplicate (data.rs:196-235): identical states are merged, their targets summed in buffer
 * order and divided by the count. Outputs are sized for n entries; *out_count = number of unique states, emitted in
 * ascending (my_bb, op_bb) order (the reference's order is HashMap iteration order, i.e. unspecified). */
int syn_replay_deduplicate(syn_engine* h, const uint64_t* my_bb, const uint64_t* op_bb, const float* pis,
                           const float* vs, size_t n, uint64_t* out_my, uint64_t* out_op, float* out_pi, float* out_v,
                           uint32_t* out_num, size_t* out_count);

/* ---- The replay buffer in device memory (the reference's ReplayBuffer, synthesis/src/data.rs:107-235, between gather_experience and
 * the epochs of alpha_zero.rs:42-100). It belongs to the engine: five structure-of-arrays sections my | op | gid | pi[9] | v[3] of
 * `capacity` positions each, 72 bytes per position, plus a second buffer of the same size once a keep-window has dropped something.
 * Positions keep buffer order through every call below (game order, then ply order; appended parts in call order) — the
 * de-duplication sums the targets of identical states in that order, so the learner's data set is bit for bit what the host path
 * (syn_selfplay_run's padded arrays -> mask by plies -> concatenate -> filter by game id -> syn_replay_deduplicate ->
 * syn_train_set_data) produces from the same games. All calls are ordered on the engine's stream and wait for the device only where
 * a count has to reach the host. Device pointers a caller passes in must be ready (their producer's stream synchronised) and must stay
 * valid until the next call on the handle that waits for the device. One handle, one calling thread at a time, as for the rest.
 *
 * syn_replay_reserve: ReplayBuffer::new(n) (data.rs:117-130) — allocates, or grows keeping the contents; never shrinks.
 * syn_replay_clear / syn_replay_size: drop everything / curr_steps() (data.rs:148-150). */
int syn_replay_reserve(syn_engine* h, size_t capacity_positions);
int syn_replay_clear(syn_engine* h);
int syn_replay_size(syn_engine* h, size_t* n_positions);
/* The positions of the LAST syn_selfplay_run on this handle (which always leaves its outputs on the device, whatever host pointers it
 * was given), compacted into caller-owned device sections: game slot g contributes its plies[g] positions in ply order, games in slot
 * order, gid = first_gid + g; games that never started (plies == 0 after syn_cancel) contribute nothing. This is run_n_games'
 * buffer (alpha_zero.rs:181-209) without the padded download — what a rank that is not the learner hands to the gather.
 * *n_positions = sum of plies. SYN_ERR_INVALID_ARGUMENT when no self-play has completed on the handle (or the last one failed);
 * SYN_ERR_CAPACITY, nothing written, when the sections (room for `capacity` positions each) are too small. Returns after the
 * sections are complete. */
int syn_selfplay_positions_device(syn_engine* h, int64_t first_gid, uint64_t* d_my, uint64_t* d_op, int64_t* d_gid, float* d_pi,
                                  float* d_v, size_t capacity, size_t* n_positions);
/* ReplayBuffer::extend (data.rs:132-146) for the last self-play launch: the same compaction straight onto the tail of the engine's
 * buffer. *n_appended (may be NULL) = positions added. */
int syn_replay_append_selfplay(syn_engine* h, int64_t first_gid, size_t* n_appended);
/* ReplayBuffer::extend for positions that came from elsewhere (other ranks' games, a caller's own): n positions from device sections /
 * from host arrays (my_bb[n], op_bb[n], gid[n], pis[n][9], vs[n][3]) onto the tail. Every append that would exceed the reserved
 * capacity returns SYN_ERR_CAPACITY and leaves the buffer exactly as it was. */
int syn_replay_append_device(syn_engine* h, const uint64_t* d_my, const uint64_t* d_op, const int64_t* d_gid, const float* d_pi,
                             const float* d_v, size_t n);
int syn_replay_append(syn_engine* h, const uint64_t* my_bb, const uint64_t* op_bb, const int64_t* gid, const float* pis, const float* vs,
                      size_t n);
/* ReplayBuffer::keep_last_n_games (data.rs:160-194) with the window given as its first game: every position with gid < min_gid is
 * dropped, the others keep their order (stable for any order of ids, not only non-decreasing ones). An empty result is legal. */
int syn_replay_keep_games_from(syn_engine* h, int64_t min_gid);
/* Copies the buffer out (tests, logs): arrays sized for `capacity` positions, any of them may be NULL; *n_positions (may be NULL) =
 * the buffer's size, also when SYN_ERR_CAPACITY says the arrays are too small (nothing is copied then). */
int syn_replay_read(syn_engine* h, uint64_t* my_bb, uint64_t* op_bb, int64_t* gid, float* pis, float* vs, size_t capacity,
                    size_t* n_positions);
/* ReplayBuffer::deduplicate (data.rs:196-235) + the tensors of alpha_zero.rs:52-58 without a host copy: de-duplicates the buffer
 * (syn_replay_deduplicate's device core: same order, same sums) and makes the unique set the learner's data set, i.e. the state
 * syn_train_set_data would have left; the buffer itself is unchanged. *n_unique (may be NULL) = its size. Needs syn_trainer_init*
 * first (SYN_ERR_NO_WEIGHTS); an empty buffer is SYN_ERR_INVALID_ARGUMENT. */
int syn_replay_deduplicate_to_trainer(syn_engine* h, size_t* n_unique);
/* The learner's current data set (syn_train_set_data / syn_replay_deduplicate_to_trainer) copied out — what alpha_zero.rs:98-100
 * writes as latest_*.npy. Arrays sized for `capacity` states, any may be NULL; *n (may be NULL) = the set's size, also on
 * SYN_ERR_CAPACITY. */
int syn_train_get_data(syn_engine* h, uint64_t* my_bb, uint64_t* op_bb, float* target_pi, float* target_v, size_t capacity,
                       size_t* n);

/* ---- Mirror symmetry of the 9x7 board (DESIGN.md "Mirror-symmetric de-duplication"; not in the reference). Bit index of a bitboard =
 * row + 7 * col; mirror moves bit [row, col] to [row, 8 - col] and leaves bit 63 alone; reverse: pi[c] -> pi[8 - c]; v is unchanged.
 * A record [my, op, pi, v] is FLIPPED when the pair [mirror my, mirror op] is strictly smaller than [my, op] as unsigned 64-bit
 * numbers, my first; its canonical form is then [mirror my, mirror op, reverse pi, v], otherwise it is the record itself.
 *
 * syn_positions_mirror: the mirroring kernel on its own, host arrays in and out: out_my[i] = mirror of my_bb[i], likewise op, and
 * out_pi[i][c] = pis[i][8 - c]. pis and out_pi may both be NULL (boards only). */
int syn_positions_mirror(syn_engine* h, const uint64_t* my_bb, const uint64_t* op_bb, const float* pis /*may be NULL*/, size_t n,
                         uint64_t* out_my, uint64_t* out_op, float* out_pi /*may be NULL*/);
/* syn_replay_deduplicate over the canonical forms, closed under mirroring: rows [0, U) are the unique canonical states in ascending
 * order with their targets summed over the class in buffer order (a flipped member contributes its reversed pi) and divided by the
 * count; rows [U, U+M) are the mirror images of those classes whose state is not its own mirror image, in the same order, with
 * the reversed averaged pi and the same v and num. Outputs are sized for 2n rows; *out_canonical = U, *out_count = U + M. The sort
 * runs over n keys. n is at most 2^30 - 1. */
int syn_replay_deduplicate_symmetric(syn_engine* h, const uint64_t* my_bb, const uint64_t* op_bb, const float* pis, const float* vs,
                                     size_t n, uint64_t* out_my, uint64_t* out_op, float* out_pi, float* out_v, uint32_t* out_num,
                                     size_t* out_canonical, size_t* out_count);
/* syn_replay_deduplicate_to_trainer in that form: the U + M rows become the learner's data set, the buffer itself is unchanged.
 * *n_canonical = U, *n_total = U + M, either may be NULL. Same error codes. */
int syn_replay_deduplicate_to_trainer_symmetric(syn_engine* h, size_t* n_canonical, size_t* n_total);

/* ---- Held-out evaluation (csrc/dataset_eval.cuh; not in the reference): the losses of a set of parameters on a data
 * set, forward only. Every other loss this library reports is the by-product of an optimiser step; this call is an OBSERVER: the
 * trainer's weights, moments, step count and data set, the engine's network, arithmetic, f16x2 image, host blob, policy cache and replay
 * buffer and the evaluation set are bit for bit what they were before it.
 *
 * The engine holds a second data set beside the learner's, the EVALUATION SET, in the same layout (my_bb[n], op_bb[n], pi[n][9],
 * v[n][3]). No trainer call reads or writes it and it needs no trainer. syn_dataset_set uploads it from host arrays (n = 0 empties it,
 * the pointers may then be NULL; n > 2^31 - 1 is SYN_ERR_INVALID_ARGUMENT); syn_dataset_get copies it out as syn_train_get_data does the
 * learner's (arrays sized for `capacity` rows, any may be NULL; *n = the set's size, also on SYN_ERR_CAPACITY).
 *
 * syn_dataset_evaluate evaluates the rows [first_row, first_row + n_rows) of `which` — SYN_DATASET_TRAIN: the learner's current data
 * set, SYN_DATASET_EVAL: the evaluation set — with the parameters
 *   blob == NULL   the trainer's current weights (n_floats is ignored), or
 *   blob != NULL   n_floats parameters on the host; n_floats selects the network (30492: Connect4Net, 12412: Connect4ConvNet). They are
 *                  built into an image buffer the call owns; this form needs no trainer and no weights loaded into the engine.
 * The definition is the f32 learner's. Row i of the range belongs to block j = i / 32; a block has rows_j = 32 rows, the last one
 * n_rows mod 32 when that is not zero. Per block:
 *   pi_loss_j, v_loss_j   bit for bit the two losses syn_train_gradients_device reports (chained mode, f32) for the block's rows as a
 *                         minibatch of rows_j: the learner's forward, log_softmax and kl_div chain for chain, then bm * (kl_0 + kl_1 +
 *                         ...) in row order with bm = 1.0f / rows_j — through the learners' parity the oracle's train_gradients /
 *                         convtrain_gradients losses. policy_weight and value_weight do not enter, as they do not enter those losses.
 *   pi_hit_j              rows whose arg-max of the nine policy logits over the LEGAL columns equals the arg-max of the target pi.
 *                         Column c is legal when its top cell (bit 6 + 7 c of my | op) is free; a row without a legal column is a miss.
 *   v_hit_j               rows whose arg-max of the three value logits equals the arg-max of the target v.
 *   In all four arg-maxes the first maximum wins: the best is the first (legal) entry, and a later entry replaces it only when it
 *   compares greater. An all-zero target row has KL 0 and arg-max 0.
 * The totals, in an order that depends on n_rows alone (never on the grid):
 *   chunk c = the blocks [256 c, 256 c + 256):  S_c = 0.0, then S_c = S_c + (double)rows_j * (double)loss_j in ascending j (the product
 *   is exact in f64);  sum = 0.0, then sum = sum + S_c in ascending c;  mean = sum / (double)n_rows. The hit counts are integer sums.
 * Outputs, each of which may be NULL: *out (below; `grid` = workgroups of the blocks launch); block_losses[n_blocks][2] = (pi_loss_j,
 * v_loss_j); row_logits[n_rows][12] = the nine policy and three value logits of every row; row_kl[n_rows][2] = every row's two KL
 * values (= the losses of the row as a minibatch of one). max_workgroups = 0 lets the library choose the grid, any other value caps it
 * (the results do not depend on it). n_rows = 0 is SYN_OK with an all-zero *out and nothing launched. syn_last_timing reports the device
 * time of the call's two launches (blocks, reduce).
 * Refused, with everything unchanged: an unknown `which`, a negative max_workgroups, no data set (`which` is empty or was never set), a
 * row range outside the set, a blob whose n_floats is neither network's (all SYN_ERR_INVALID_ARGUMENT); blob == NULL before
 * syn_trainer_init* (SYN_ERR_NO_WEIGHTS).
 *
 * syn_dataset_evaluate_arith is the same call in any arithmetic the library computes a forward pass in; syn_dataset_evaluate is this call
 * with SYN_EVAL_ARITH_F32, and everything above is its definition. Blocks, rows_j, the hit rules, the totals, the outputs, the grid
 * independence and the observer property are shared by all three arithmetics; only the arithmetic that produces the twelve RAW OUTPUTS of
 * a row (what row_logits returns) changes:
 *   SYN_EVAL_ARITH_F16X2  (both networks) the twelve raw outputs of row i are bit for bit what the engine's f16x2 inference ("Network
 *                         arithmetic" above; syn_policy_eval_batch_device's nine logits and the three numbers its value softmax reads)
 *                         computes for that position with these parameters. The f16x2 image is built per call on the host, from the
 *                         blob or (blob == NULL) from a copy of the trainer's current weights, into a buffer the call owns: the engine's
 *                         own network, arithmetic, f16x2 image, host blob and policy cache are neither read nor written, and the result
 *                         is the same on an engine in f32 and on one in f16x2. Parameters without an f16x2 plan (non-finite values,
 *                         scales outside the window, a bias that does not fit: syn_f16x2_plan_of_blob reports valid = 0) are refused
 *                         with SYN_ERR_UNSUPPORTED and nothing changes.
 *   SYN_EVAL_ARITH_BF16   (Connect4ConvNet only; Connect4Net: SYN_ERR_UNSUPPORTED, as syn_trainer_set_precision) the forward of the conv
 *                         learner in SYN_TRAIN_BF16: the same operands rounded to bf16, the same v_mfma_f32_16x16x16_bf16 chains.
 *                         pi_loss_j and v_loss_j are bit for bit the two losses syn_train_gradients_device reports in SYN_TRAIN_BF16,
 *                         chained mode, for the block's rows as a minibatch of rows_j. The trainer's own precision setting is neither
 *                         read nor changed: a trainer in SYN_TRAIN_F32 can be evaluated in bf16 and the reverse.
 * The head is the f32 learner's in every arithmetic, applied to the raw outputs x_0..x_8 (policy) and x_9..x_11 (value) with the targets
 * t_k, all in f32: mx = the first maximum; se = det_expf(x_k - mx) summed ascending from 0.0f; lse = mx + det_logf(se); kl = the
 * ascending sum from 0.0f of t_k * (det_logf(t_k) - (x_k - lse)) over the k with t_k > 0; loss_j = bm * (kl_0 + kl_1 + ...) in row order
 * with bm = 1.0f / rows_j; row_kl[i] = the row as a minibatch of one. The hits are computed from the same raw outputs.
 * Further refusals: an arithmetic other than the three is SYN_ERR_INVALID_ARGUMENT. n_rows = 0 is SYN_OK with an all-zero *out in every
 * arithmetic: no image is built and no plan is asked for. syn_last_timing reports the call's two launches; the host's image build of
 * the f16x2 arithmetic is outside that time. */
typedef struct syn_dataset_metrics {
    double mean_pi, mean_v;    /* sum_pi / rows, sum_v / rows (0 when rows = 0) */
    double sum_pi, sum_v;      /* the two f64 sums defined above */
    uint64_t rows, blocks;
    uint64_t pi_hits, v_hits;
    uint32_t grid, reserved;
} syn_dataset_metrics;
enum { SYN_DATASET_TRAIN = 0, SYN_DATASET_EVAL = 1 };
int syn_dataset_set(syn_engine* h, const uint64_t* my_bb, const uint64_t* op_bb, const float* target_pi, const float* target_v, size_t n);
int syn_dataset_get(syn_engine* h, uint64_t* my_bb, uint64_t* op_bb, float* target_pi, float* target_v, size_t capacity, size_t* n);
int syn_dataset_evaluate(syn_engine* h, int which, size_t first_row, size_t n_rows, const float* blob, size_t n_floats, int max_workgroups,
                         syn_dataset_metrics* out, float* block_losses, float* row_logits, float* row_kl);
enum { SYN_EVAL_ARITH_F32 = 0, SYN_EVAL_ARITH_F16X2 = 1, SYN_EVAL_ARITH_BF16 = 2 };
int syn_dataset_evaluate_arith(syn_engine* h, int which, size_t first_row, size_t n_rows, const float* blob, size_t n_floats, int arithmetic,
                               int max_workgroups, syn_dataset_metrics* out, float* block_losses, float* row_logits, float* row_kl);

/* ---- Holding games out (opt-in; csrc/replay_kernels.cuh). syn_replay_set_holdout sets a key and a threshold (at most 2^32, else
 * SYN_ERR_INVALID_ARGUMENT); with sm as in "Device-side epoch sampler" above and all arithmetic unsigned 64-bit, game gid (its 64-bit
 * pattern) is HELD OUT iff
 *   (sm(sm(key ^ HOLDOUT_TAG, (uint32)(gid >> 32)), (uint32)gid) >> 32) < threshold,        HOLDOUT_TAG = 0x401D0075E7C0FFEE
 * so about threshold / 2^32 of the games are, by game and never by position (the positions of one game are correlated), and a game
 * keeps its side for as long as it stays in the buffer. threshold = 0, the default, switches it off: every call then does exactly
 * what it did without this section.
 * With a threshold above 0, syn_replay_deduplicate_to_trainer[_symmetric] split the buffer into the subsequence of the positions whose
 * game is not held out and the subsequence of those whose game is (buffer order kept inside both: a flag kernel, a scan and a scatter),
 * and run the de-duplication on either: the first result becomes the learner's data set and is what the call's counts describe, the
 * second becomes the evaluation set. Both are bit for bit what syn_replay_deduplicate[_symmetric] returns for the two subsequences,
 * except for the order of the evaluation set's rows: Connect4 openings recur across games, so a held-out state can also be in the
 * learner's data set. A row is SEEN when its state — in the symmetric form: its canonical form — is among the learner's (canonical)
 * rows, and the evaluation set is stored UNSEEN ROWS FIRST: the unseen rows in the order the de-duplication returned them, then the
 * seen rows in that order (a stable partition; one binary search per row). syn_dataset_counts returns the set's size and the number of
 * unseen rows, rows [0, n_unseen) (after syn_dataset_set: both its n), so that first_row / n_rows of syn_dataset_evaluate select
 * either range. No game held out leaves an empty evaluation set. A threshold that holds out every game of the buffer is refused
 * (SYN_ERR_INVALID_ARGUMENT) with both data sets unchanged: the learner would have nothing to train on. */
int syn_replay_set_holdout(syn_engine* h, uint64_t key, uint64_t threshold);
int syn_dataset_counts(syn_engine* h, size_t* n_eval, size_t* n_unseen);

/* ---- Reanalyse (opt-in; csrc/reanalyse_kernels.cuh; not in the reference): stored positions of the replay buffer are
 * searched again with the engine's installed network and their pi / v targets overwritten, without the positions or the results leaving
 * the device. A stored target is the product of the network of the iteration that played its game; this call relabels it with the
 * newest one.
 * Selection. With sm as in "Device-side epoch sampler" above and all arithmetic unsigned 64-bit, row i of the buffer with (gid, my, op)
 * (their 64-bit patterns; hi32(x) = (uint32)(x >> 32), lo32(x) = (uint32)x) has
 *   h = key ^ REANALYSE_TAG;  h = sm(h, hi32(gid));  h = sm(h, lo32(gid));  h = sm(h, hi32(my));  h = sm(h, lo32(my));
 *   h = sm(h, hi32(op));  h = sm(h, lo32(op))                                                REANALYSE_TAG = 0x2EA7A1F5E5EA2C40
 * and is SELECTED iff gid < before_gid (signed; INT64_MAX: every game), (h >> 32) < threshold (at most 2^32: about threshold / 2^32 of
 * the eligible rows), and the position is searchable: syn_mcts_search's check of a root (disjoint boards inside the 63 cells, every
 * column filled from the bottom, a free column) and neither side has four in a row. The row index does not enter, so a row keeps its
 * fate when a keep-window shifts it. A row that passes the first two tests but is not searchable — only a caller's own
 * syn_replay_append can have put it there — counts as `skipped` and is left alone. selected_rows (may be NULL) receives the selected row
 * indices in ascending order; with `capacity` smaller than their number the call is SYN_ERR_CAPACITY, refused before anything changes.
 * Search. The j-th selected row, in buffer order, is searched exactly as root j of syn_mcts_search(h, mcts, ..., explores,
 * action_selection): the engine's installed network, its current arithmetic and its policy cache; its SYN_FPU_NORMAL / SYN_NOISE_DIRICHLET
 * draws come from stream stream_base + j (stream_base = 0: that call's own numbering). The selected rows are searched in chunks of
 * chunk_roots roots (0 = the larger of 65,536 and the engine's concurrent games); a chunk that starts at job c0 is launched on streams
 * stream_base + c0 onwards, so the results never depend on the chunking.
 * Write-back. pi[row] = the new search's target_pi. With q = its target_q and w = value_mix: w == 0 leaves v[row] untouched bit for bit,
 * w == 1 stores q, otherwise v[k] = v_old[k] * (1.0f - w) + q[k] * w — three f32 operations in that order, nothing fused. A root that a
 * syn_cancel kept from being searched (num_nodes == 0) writes nothing. `moved` = selected rows whose arg-max column of pi (the first
 * maximum wins, as in "Held-out evaluation") differs between the old and the new pi. Everything else is unchanged: my, op, gid, the
 * unselected rows, the row order, the trainer, both data sets and the engine's network.
 * Device work: a flags kernel, an exclusive sum, a compaction into job arrays and one read-back of the counts; then per chunk the search
 * launch and a write-back kernel, and the chunk's error word read back; finally a sum of the moved flags. The write-back runs per
 * completed chunk and not at all for a chunk whose search reported an error: after SYN_ERR_CANCELLED (returned when a syn_cancel left
 * selected rows unsearched) or SYN_ERR_CAPACITY from a tree, every row is wholly old or wholly new. stats (may be NULL): rows = the
 * buffer's size, chunks = search launches, launches = all kernel launches of the call. syn_last_timing reports the summed device time of
 * the search launches and the count of all launches, syn_last_cache_stats the sums over the chunks.
 * An empty buffer or threshold = 0 is SYN_OK with all-zero stats and nothing launched; a call that selects nothing is SYN_OK with
 * selected = moved = chunks = 0, launches no search and changes nothing.
 * Refused, with the buffer bit for bit as it was: mcts or cfg NULL, threshold > 2^32, value_mix outside [0, 1] or NaN, a negative
 * chunk_roots, explores / action_selection / mcts as syn_mcts_search refuses them (SYN_FPU_FUNC: SYN_ERR_UNSUPPORTED), no weights
 * (SYN_ERR_NO_WEIGHTS), no replay buffer reserved (SYN_ERR_INVALID_ARGUMENT).
 * Not measured: whether training on reanalysed targets gives a stronger player (tools/arena.py and syn_dataset_evaluate are the
 * instruments). Out of scope: a network other than the installed one, de-duplicating states before the search. */
typedef struct syn_reanalyse_config {
    uint64_t key;            /* selection key */
    uint64_t threshold;      /* 0 .. 2^32: about threshold / 2^32 of the eligible rows are selected */
    int64_t  before_gid;     /* only rows with gid < before_gid are eligible (INT64_MAX: all) */
    uint64_t stream_base;    /* noise stream of the j-th selected row = stream_base + j */
    int32_t  explores;       /* 0 .. engine max_explores */
    int32_t  action_selection;
    float    value_mix;      /* w in [0, 1] */
    int32_t  chunk_roots;    /* 0 = library's choice; results never depend on it */
} syn_reanalyse_config;
typedef struct syn_reanalyse_stats {
    uint64_t rows, selected, skipped, moved;
    uint32_t chunks, launches;
} syn_reanalyse_stats;
int syn_replay_reanalyse(syn_engine* h, const syn_mcts_config* mcts, const syn_reanalyse_config* cfg,
                         syn_reanalyse_stats* out /*may be NULL*/, int64_t* selected_rows /*may be NULL*/, size_t capacity);

/* ---- Recorded games (opt-in; csrc/record_kernels.cuh; not in the reference): training rows from games that start at
 * given positions and are played by given players. syn_selfplay_run is run_game (alpha_zero.rs:229-268) from the empty board with one
 * network on both sides; this call is run_game inside syn_tournament_run's loop, so exploring starts (positions of the replay buffer),
 * curricula (a file of positions) and league data (the current network against an older one) leave rows a learner can use.
 * Arguments and refusals are syn_tournament_run's, made before anything of the engine or the device changes. In addition:
 *   network sides only: a baseline side is SYN_ERR_UNSUPPORTED (its search record has no target_pi / target_q);
 *   deterministic search configurations only, the match's own rule (SYN_FPU_NORMAL, SYN_FPU_FUNC, SYN_NOISE_DIRICHLET:
 *   SYN_ERR_UNSUPPORTED — their streams are keyed by job index);
 *   rec NULL, an unknown value_target, a negative *_until, a record_mask bit at or above n_players, and seeds == NULL unless both *_until
 *   are 0: SYN_ERR_INVALID_ARGUMENT.
 * Definition. Game g is run_game with these substitutions. G::new() is (start_my[g], start_op[g]). At ply k (0-based from the start
 * position; k is run_game's num_turns, so random_actions_until and sample_actions_until count from the START position) the tree is the
 * mover's, players[k even ? first[g] : second[g]], with its blob, arithmetic, explores, mcts_cfg and action selection. sample_action's
 * draws come from StdRng::seed_from_u64(seeds[g]), from the game's stream position on: gen_range one word per candidate (rejections
 * included), WeightedIndex one word, exactly as syn_selfplay_run takes them; rng_words[g] is the first unused word. mcts.solution(&action),
 * stop_games_when_solved, fill_state_info and store_rewards are the reference's (alpha_zero.rs:254-338): t = (k + 1) / plies[g] with
 * plies[g] = ALL moves of the game, recorded or not, and z by parity from the game's last position. A ply whose mover has its bit clear
 * in record_mask is played but leaves no row; the rows of a game are stored densely (row r = its r-th recorded ply, rows[g] <=
 * plies[g]). With stop_games_when_solved a game may end before the board decides it: rewards[g] is then the solved outcome, final_bb[g]
 * the position after the last move played.
 * The property that pins it: one player (first = second = 0, record_mask = 1) with the engine's loaded weights as blob in the engine's
 * arithmetic, the empty board as every start, seeds[g] = base_seed + first_game + g and a rollout configuration's fields copied over
 * gives, bit for bit, syn_selfplay_run(cfg, base_seed, first_game, n)'s outputs: rows == its plies, states, pis, vs, actions, root_nodes,
 * final_kind.
 * Outputs. The tournament's per-game outputs, and `out` (may be NULL; each pointer may be NULL): the rows in syn_selfplay_run's padded
 * shapes, slot = game; slots no row reaches are zero. On success the rows also stay in the engine's self-play output buffers: THE CALL
 * REPLACES THE LAST SELF-PLAY LAUNCH'S OUTPUTS. syn_replay_append_selfplay(first_gid) and syn_selfplay_positions_device then compact
 * them as they compact a launch of n_games games (game slot j gets gid first_gid + j; a game without rows adds nothing). After any
 * error or refusal of this call they refuse, as after a failed syn_selfplay_run.
 * Untouched: the engine's network, images, arithmetic, policy cache, trainer, replay buffer and both data sets. syn_cancel,
 * syn_progress, the capacity errors and the 63-ply bound behave as documented for syn_tournament_run. syn_last_timing: two launches
 * per non-empty group and two for the regroup, per ply, and one more for the kernel that finishes the rows.
 * Not measured: whether rows from exploring starts, curricula or league games train a stronger player. Out of scope: noise or
 * Fpu::Normal in recorded games, baseline sides. */
typedef struct syn_record_config {
    int32_t random_actions_until;    /* RolloutConfig fields, alpha_zero.rs:270-293; turns count from the START position */
    int32_t sample_actions_until;
    int32_t stop_games_when_solved;
    int32_t value_target;            /* SYN_VALUE_* */
    float value_target_p, value_target_from, value_target_to;
    int32_t reserved;
    uint64_t record_mask;            /* bit p: the plies player p moves in become rows */
} syn_record_config;

typedef struct syn_record_outputs {  /* host pointers, each may be NULL; syn_selfplay_run's shapes, slot = game */
    int32_t* rows;          /* [n]      recorded rows of game g */
    uint64_t* states_bb;    /* [n][63][2] */
    float* pis;             /* [n][63][9] */
    float* vs;              /* [n][63][3] */
    uint8_t* actions;       /* [n][63]  the action played from that row's position */
    uint32_t* root_nodes;   /* [n][63] */
    uint8_t* final_kind;    /* [n] */
} syn_record_outputs;

int syn_games_run_recorded(syn_engine* h, const syn_match_side* players, int n_players, const int32_t* first, const int32_t* second,
                           const uint64_t* start_my, const uint64_t* start_op, const uint64_t* seeds, int n_games,
                           const syn_record_config* rec, float* rewards, int32_t* plies, uint8_t* moves, uint64_t* final_bb,
                           uint64_t* rng_words, const syn_record_outputs* out);

/* Start positions from the device replay buffer: "Reanalyse"'s selection alone — the same hash of (key, gid, my, op), the same gid
 * bound and searchable test, buffer order — with the selected positions downloaded, 16 bytes each, into my_bb / op_bb (room for
 * `capacity` positions). *n_selected = the number selected, also when SYN_ERR_CAPACITY says the arrays are too small (nothing is written
 * to them then); *n_skipped (may be NULL) = rows that passed the bound and the hash but are not searchable. The buffer is read, never
 * written. threshold > 2^32, n_selected NULL, or no buffer reserved: SYN_ERR_INVALID_ARGUMENT. */
int syn_replay_select_positions(syn_engine* h, uint64_t key, uint64_t threshold, int64_t before_gid, uint64_t* my_bb, uint64_t* op_bb,
                                size_t capacity, size_t* n_selected, size_t* n_skipped);

/* ---- State digests (csrc/digest_kernels.cuh; not in the reference): a 64-bit fingerprint of a piece of engine state,
 * computed where the state lives, so that "these two runs hold the same bits" is one word in a log instead of a download.
 * Definition. A component is a sequence of 32-bit words w_0 .. w_{L-1}: its arrays, concatenated in the order given below, each read as
 * it lies in memory (a 64-bit value is its low word followed by its high word). With finalise and sm as in "Device-side epoch sampler"
 * above, GOLDEN = 0x9E3779B97F4A7C15, T = 0xD16E57000000AA00 + what, and all arithmetic unsigned 64-bit with wrap-around:
 *   a_i    = finalise(T + (i + 1) * GOLDEN)                  i as a 64-bit number
 *   h_i    = sm(a_i, w_i)                                    = finalise(a_i + ((w_i + 1) mod 2^32) * GOLDEN)
 *   S      = (h_0 + h_1 + ... + h_{L-1}) mod 2^64            0 when L = 0
 *   digest = sm(sm(S ^ T, hi32(L)), lo32(L))
 * The sum is associative and commutative, so the word does not depend on how the device splits the work; the position i enters every
 * term, so moving a word changes it. Known answers for T = 0xD16E57000000AA01: no words 0x6dc4edd735556cbf, the single word 0
 * 0x831dcd5c179d866e, the words 0 .. 999 ascending 0x17b9ceedb8bf8015, the words 999 .. 0 descending 0x8c9cab522ff11f09.
 * Word sequences:
 *   SYN_DIGEST_TRAINER     w[P], m[P], v[P] as f32 words (P = 30,492 or 12,412), then the step count's low and high word. The last
 *                          gradient is not part of it (it is scratch: every step overwrites it before reading it).
 *   SYN_DIGEST_NETWORK     the P parameters the engine's installed network was built from, in blob order. The arithmetic and the policy
 *                          cache are not part of it: results never depend on the cache. Computed on the HOST from the engine's own copy
 *                          of those parameters (that is where they are; the device holds derived images only); nothing is launched.
 *   SYN_DIGEST_REPLAY      the device replay buffer's rows [0, n): my[n], op[n], gid[n], pi[n][9], v[n][3] — 18 n words.
 *   SYN_DIGEST_TRAIN_DATA  the learner's data set: my[n], op[n], pi[n][9], v[n][3] — 16 n words.
 *   SYN_DIGEST_EVAL_DATA   the evaluation set, likewise.
 * *n_words = L (either output may be NULL). An empty or never-reserved buffer or data set is SYN_OK with the digest of no words and
 * nothing launched. On the device: one grid-stride launch that leaves a partial sum per workgroup, and a one-workgroup launch that adds
 * them and closes the digest; no atomics. max_workgroups = 0 lets the library choose the first grid, any other value caps it (the word
 * does not depend on it). The call is an OBSERVER in syn_dataset_evaluate's sense: everything it reads is bit for bit what it was.
 * syn_last_timing reports the device time and the number of its launches (2, or 0 where nothing was launched).
 * Refused, with everything unchanged: an unknown `what` or a negative max_workgroups (SYN_ERR_INVALID_ARGUMENT); SYN_DIGEST_TRAINER before
 * syn_trainer_init*, SYN_DIGEST_NETWORK before any weights (SYN_ERR_NO_WEIGHTS). */
enum { SYN_DIGEST_TRAINER = 1, SYN_DIGEST_NETWORK = 2, SYN_DIGEST_REPLAY = 3, SYN_DIGEST_TRAIN_DATA = 4, SYN_DIGEST_EVAL_DATA = 5 };
int syn_state_digest(syn_engine* h, int what, int max_workgroups, uint64_t* digest, uint64_t* n_words);

/* Timing of the last syn_selfplay_run / syn_mcts_search / *_device call on this handle, measured with HIP events on
 * the engine stream: kernel_ms = device time of the dominant kernel launch(es), n_launches = how many. */
int syn_last_timing(const syn_engine* h, float* kernel_ms, int* n_launches);

/* PolicyWithCache statistics of the last syn_selfplay_run / syn_mcts_search: Policy::eval calls answered from the table and
 * calls that ran the network (both 0 when the cache is off or the row-per-tree kernels ran). */
int syn_last_cache_stats(const syn_engine* h, uint64_t* hits, uint64_t* misses);

/* Launch shape the last syn_selfplay_run / syn_mcts_search used (the engine picks it from the number of concurrent games,
 * DESIGN.md §6.1): *shape = 1 row-per-tree kernel with the weights in registers (16 trees per workgroup), 2 = the same
 * with two workgroups per CU, 3 = quad-async row kernel (several 16-tree quads per workgroup), 4 = lane-per-tree kernel
 * (one tree per lane), 5 = the evaluator baseline's lane-per-tree kernel / the producer-consumer debug shape, 6 = the lane-per-tree kernel
 * with two trees per lane, 7 = the free-running row kernel of the f16x2 arithmetic (at most 16 trees per CU: four waves of four trees, every
 * wave evaluating its own leaves); grid / threads = workgroups and threads per workgroup. Diagnostics and tests only. */
int syn_last_launch_shape(const syn_engine* h, int* shape, int* grid, int* threads);

/* A self-play launch plays its whole batch inside ONE kernel (seconds to tens of seconds). These two entry points may be called
 * from ANOTHER host thread while syn_selfplay_run / syn_mcts_search / syn_mcts_search_rollout runs on the handle (they use a stream
 * of their own and never touch the handle's error string):
 * syn_progress: *started = jobs (games / roots) handed to tree slots so far, capped at the call's job count; after a cancel, the
 *   number handed out when the cancel was applied (a lower bound of what finally ran). *finished = self-play games completed.
 * syn_cancel: no further job is handed out; the running call returns once the jobs already started have finished (at most one
 *   game's duration) — with SYN_ERR_CANCELLED if anything was left out: self-play games that never started have plies[g] = 0,
 *   roots that were not searched have all-zero results (num_nodes == 0); everything else is valid. A cancel that arrives after
 *   the last job was handed out cancels nothing and the call returns SYN_OK. A cancel that arrives while the call is still
 *   setting up is applied before the first job is handed out. Returns SYN_ERR_INVALID_ARGUMENT when no call is in flight.
 *   syn_frozen_search_rollout takes its roots in a grid-stride loop: a cancel during it is accepted and has no effect.
 * The reference has no counterpart (its workers are joined at the end of gather_experience, alpha_zero.rs:156-170). */
int syn_progress(syn_engine* h, int* started, int* finished);
int syn_cancel(syn_engine* h);

/* Device-side RNG / math primitives exposed for parity tests against the oracle (no reference counterpart):
 * out[i] = i-th u32 of StdRng::seed_from_u64(seed) as generated on the GPU. */
int syn_debug_stdrng_u32(syn_engine* h, uint64_t seed, int n, uint32_t* out);
/* y[i] = device det_expf(a[i]); q[i] = a[i] / b[i]; s[i] = sqrtf(a[i]), or det_logf(a[i]) where b[i] < 0
 * (IEEE-exactness checks) */
int syn_debug_math(syn_engine* h, const float* a, const float* b, int n, float* out_exp_a, float* out_div,
                   float* out_sqrt_a);

/* fast[i] = the packed division of the lane / producer-consumer kernels' descent (device_common.cuh div2_by_small_int) on
 * a[i] / b[i]; full[i] = the device's IEEE division. Equal bit for bit for a = 0 or 2^-60 <= a <= 2^60 and INTEGER 1 <= b <= 2^16. */
int syn_debug_fast_div(syn_engine* h, const float* a, const float* b, int n, float* out_fast, float* out_full);
/* Enumeration behind the descent's shortened sequences: every f32 significand (2^23) at three exponents against every integer
 * divisor b_lo .. b_hi, and every significand at four exponents under the square root. mismatches3[0] = quotients where
 * div2_by_small_int differs from the IEEE division, [1] = the same for div2_safe_range, [2] = square roots where sqrt_normal_range
 * differs from sqrtf. All three must be 0. */
int syn_debug_small_int_math(syn_engine* h, int b_lo, int b_hi, unsigned long long* mismatches3);
/* The tournament's stable multi-way regroup alone (count, scan, scatter) on the ids 0 .. n-1: keys[i] in [0, n_keys] (n_keys = dropped),
 * 1 <= n_keys <= SYN_TOURNAMENT_MAX_PLAYERS. perm_out[0 .. seg_out[n_keys]) = the ids grouped by ascending key, input order kept inside
 * a group (the rest of perm_out[0 .. n) is -1); seg_out[0 .. n_keys] = where each group starts, seg_out[n_keys] = the survivors. */
int syn_debug_tournament_regroup(syn_engine* h, const int32_t* keys, int n, int n_keys, int32_t* perm_out, int32_t* seg_out);

/* PMC calibration probe (tools/calibrate_pmc.py): gathers n_spans 288-byte sibling spans of 32-byte node records at
 * record offsets d_span_off[i] from d_base (device pointers), optionally rewriting 16 bytes per touched record. */
int syn_debug_calibrate(syn_engine* h, const void* d_base, const uint32_t* d_span_off, int n_spans, int do_write);

#ifdef __cplusplus
}
#endif
#endif /* SYNTHESIS_AMD_H */
