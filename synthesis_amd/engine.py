"""ctypes binding of the C ABI (include/synthesis_amd.h) + the Engine convenience class.

The library is loaded from synthesis_amd/libsynthesis_amd.so (built in-tree by `make -C synthesis_amd/csrc` or
__graft_entry__.build()). Nothing here computes: every method forwards to a HIP kernel launch inside the library.
"""
import ctypes as C
import os

import numpy as np

from .config import CEngineConfig, CMctsConfig, CRecordConfig, CRolloutConfig, MCTSConfig, RecordConfig, RolloutConfig

_HERE = os.path.dirname(os.path.abspath(__file__))
NUM_PARAMS = 30492  # Connect4Net: 63->128->96->64->48->12 (study-connect4/src/policies.rs:20-24)
CONV_NUM_PARAMS = 12412  # Connect4ConvNet: Conv2d<2,16,3,pad 1> + ReLU + Linear<1008,12> (include/synthesis_amd.h)

# every symbol include/synthesis_amd.h declares (checked by tests/test_abi.py)
ABI_SYMBOLS = [
    "syn_default_rollout_config", "syn_engine_create", "syn_engine_destroy", "syn_last_error", "syn_load_weights",
    "syn_load_weights_conv", "syn_set_network_arithmetic", "syn_get_network_arithmetic", "syn_f16x2_plan_of_blob",
    "syn_policy_eval_batch", "syn_policy_eval_batch_device", "syn_eval_ctx_create", "syn_eval_ctx_submit", "syn_eval_ctx_wait",
    "syn_eval_ctx_eval", "syn_eval_ctx_last_error", "syn_eval_ctx_destroy", "syn_features_batch", "syn_linear_forward",
    "syn_conv2d_forward", "syn_activation_forward", "syn_mcts_search", "syn_mcts_search_rollout", "syn_mcts_search_lockstep", "syn_selfplay_run_lockstep", "syn_frozen_search_rollout", "syn_selfplay_run", "syn_progress", "syn_cancel", "syn_trainer_set_precision", "syn_trainer_set_batch_mode", "syn_trainer_get_batch_mode", "syn_last_timing", "syn_last_launch_shape", "syn_last_cache_stats", "syn_debug_stdrng_u32",
    "syn_debug_math", "syn_debug_fast_div", "syn_debug_small_int_math", "syn_debug_calibrate", "syn_trainer_init", "syn_trainer_init_conv", "syn_train_step", "syn_train_gradients_device",
    "syn_train_apply_device", "syn_train_gradients_enqueue", "syn_train_apply_enqueue", "syn_trainer_get_state", "syn_trainer_publish_weights", "syn_replay_deduplicate", "syn_train_set_data", "syn_train_epoch",
    "syn_replay_reserve", "syn_replay_clear", "syn_replay_size", "syn_selfplay_positions_device", "syn_replay_append_selfplay",
    "syn_replay_append_device", "syn_replay_append", "syn_replay_keep_games_from", "syn_replay_read",
    "syn_replay_deduplicate_to_trainer", "syn_train_get_data",
    "syn_positions_mirror", "syn_replay_deduplicate_symmetric", "syn_replay_deduplicate_to_trainer_symmetric",
    "syn_match_run", "syn_match_run_sides", "syn_tournament_run", "syn_debug_tournament_regroup",
    "syn_train_epochs_sampled", "syn_debug_sampler",
    "syn_dataset_set", "syn_dataset_get", "syn_dataset_evaluate", "syn_dataset_evaluate_arith", "syn_replay_set_holdout", "syn_dataset_counts",
    "syn_replay_reanalyse",
    "syn_trainer_set_state", "syn_state_digest",
    "syn_games_run_recorded", "syn_replay_select_positions",
]
TOURNAMENT_MAX_PLAYERS = 64  # SYN_TOURNAMENT_MAX_PLAYERS


BATCH_MODES = {"chained": 0, "micro": 1}   # SYN_TRAIN_BATCH_*


class SynthesisAmdError(RuntimeError):
    def __init__(self, code, message):
        super().__init__(f"synthesis_amd error {code}: {message}")
        self.code = code


class CSearchResult(C.Structure):  # struct syn_search_result
    _fields_ = [
        ("child_N", C.c_float * 9), ("child_W", (C.c_float * 3) * 9), ("child_P", C.c_float * 9),
        ("child_sol", (C.c_int32 * 3) * 9),
        ("root_N", C.c_float), ("root_W", C.c_float * 3), ("root_sol", C.c_int32 * 3),
        ("num_nodes", C.c_uint32), ("best_action", C.c_int32),
        ("target_pi", C.c_float * 9), ("target_q", C.c_float * 3),
    ]


class CMatchPlayer(C.Structure):  # struct syn_match_player
    _fields_ = [("explores", C.c_int32), ("action", C.c_int32), ("mcts_cfg", CMctsConfig)]


class CMatchSide(C.Structure):  # struct syn_match_side
    _fields_ = [("kind", C.c_int32), ("arithmetic", C.c_int32), ("player", CMatchPlayer), ("blob", C.c_void_p), ("n_floats", C.c_size_t)]


MATCH_SIDE_KINDS = {"network": 0, "baseline": 1}             # SYN_MATCH_SIDE_*
MATCH_ARITHMETICS = {None: 0, "f32": 1, "f16x2": 2}          # SYN_MATCH_ARITH_*; None = the engine's


def decode_match_side(side):
    """(kind, arithmetic) names of a CMatchSide: a zero-filled one is ("network", None), a network side in the engine's arithmetic"""
    kinds = {v: k for k, v in MATCH_SIDE_KINDS.items()}
    ariths = {v: k for k, v in MATCH_ARITHMETICS.items()}
    return kinds[side.kind], ariths[side.arithmetic]


class CF16x2Plan(C.Structure):  # struct syn_f16x2_plan
    _fields_ = [("valid", C.c_int), ("activation_exp", C.c_int * 5), ("weight_exp", C.c_int * 5), ("out_exp", C.c_int),
                ("bound", C.c_double * 5)]


class CTrainConfig(C.Structure):  # struct syn_train_config
    _fields_ = [("weight_decay", C.c_float), ("policy_weight", C.c_float), ("value_weight", C.c_float),
                ("beta1", C.c_float), ("beta2", C.c_float), ("eps", C.c_float)]


class CSamplerConfig(C.Structure):  # struct syn_sampler_config
    _fields_ = [("key", C.c_uint64), ("first_epoch", C.c_uint32), ("flip", C.c_int32)]


class CDatasetMetrics(C.Structure):  # struct syn_dataset_metrics
    _fields_ = [("mean_pi", C.c_double), ("mean_v", C.c_double), ("sum_pi", C.c_double), ("sum_v", C.c_double),
                ("rows", C.c_uint64), ("blocks", C.c_uint64), ("pi_hits", C.c_uint64), ("v_hits", C.c_uint64),
                ("grid", C.c_uint32), ("reserved", C.c_uint32)]


DATASETS = {"train": 0, "eval": 1}   # SYN_DATASET_*
EVAL_ARITHMETICS = {"f32": 0, "f16x2": 1, "bf16": 2}   # SYN_EVAL_ARITH_*


class CReanalyseConfig(C.Structure):  # struct syn_reanalyse_config
    _fields_ = [("key", C.c_uint64), ("threshold", C.c_uint64), ("before_gid", C.c_int64), ("stream_base", C.c_uint64),
                ("explores", C.c_int32), ("action_selection", C.c_int32), ("value_mix", C.c_float), ("chunk_roots", C.c_int32)]


class CReanalyseStats(C.Structure):  # struct syn_reanalyse_stats
    _fields_ = [("rows", C.c_uint64), ("selected", C.c_uint64), ("skipped", C.c_uint64), ("moved", C.c_uint64),
                ("chunks", C.c_uint32), ("launches", C.c_uint32)]


class CRecordOutputs(C.Structure):  # struct syn_record_outputs
    _fields_ = [(n, C.c_void_p) for n in ("rows", "states_bb", "pis", "vs", "actions", "root_nodes", "final_kind")]


class CCounters(C.Structure):  # struct syn_counters
    _fields_ = [(n, C.c_uint64) for n in (
        "explores", "select_levels", "children_scanned", "expansions", "new_nodes", "policy_evals", "backprop_levels",
        "solver_children", "solved_hits", "moves", "games", "max_depth")]


def library_path():
    """The in-tree build; SYNTHESIS_AMD_LIB points developer tools at another build of the same ABI (A/B timing)."""
    return os.environ.get("SYNTHESIS_AMD_LIB") or os.path.join(_HERE, "libsynthesis_amd.so")


_lib = None


def _share_hip_runtime_with_torch():
    """A process must hold ONE HIP runtime. PyTorch-ROCm wheels bundle their own libamdhip64.so.7; if this library pulled
    in /opt/rocm's copy first, a later `import torch` (device buffers, torch.distributed/RCCL) finds no GPU. When a torch
    with a bundled runtime is installed, bind to that copy (same soname, so our DT_NEEDED resolves to it); otherwise the
    RUNPATH copy under /opt/rocm is used. torch itself is not imported here."""
    import importlib.util
    import sys

    if "torch" in sys.modules:
        return
    spec = importlib.util.find_spec("torch")
    if spec is None or not spec.submodule_search_locations:
        return
    cand = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
    if os.path.exists(cand):
        C.CDLL(cand, mode=C.RTLD_GLOBAL)


def load_library():
    """Loads libsynthesis_amd.so; raises (never falls back) if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    path = library_path()
    if not os.path.exists(path):
        raise SynthesisAmdError(-100, f"{path} not found: build it with `make -C synthesis_amd/csrc` "
                                      "(hipcc --offload-arch=gfx950); there is no CPU fallback")
    _share_hip_runtime_with_torch()
    lib = C.CDLL(path)
    lib.syn_last_error.restype = C.c_char_p
    lib.syn_last_error.argtypes = [C.c_void_p]
    lib.syn_engine_create.argtypes = [C.POINTER(CEngineConfig), C.c_int, C.POINTER(C.c_void_p)]
    lib.syn_engine_destroy.argtypes = [C.c_void_p]
    lib.syn_load_weights.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    lib.syn_load_weights_conv.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    lib.syn_set_network_arithmetic.argtypes = [C.c_void_p, C.c_int]
    lib.syn_get_network_arithmetic.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(CF16x2Plan)]
    lib.syn_f16x2_plan_of_blob.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(CF16x2Plan)]
    lib.syn_policy_eval_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    lib.syn_policy_eval_batch_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                                 C.c_int]
    lib.syn_eval_ctx_create.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
    lib.syn_eval_ctx_submit.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    lib.syn_eval_ctx_wait.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    lib.syn_eval_ctx_eval.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    lib.syn_eval_ctx_last_error.restype = C.c_char_p
    lib.syn_eval_ctx_last_error.argtypes = [C.c_void_p]
    lib.syn_eval_ctx_destroy.argtypes = [C.c_void_p]
    lib.syn_features_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    lib.syn_linear_forward.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                       C.c_void_p, C.c_int]
    lib.syn_conv2d_forward.argtypes = [C.c_void_p] + [C.c_int] * 10 + [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                                                      C.c_void_p, C.c_int]
    lib.syn_activation_forward.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    lib.syn_mcts_search.argtypes = [C.c_void_p, C.POINTER(CMctsConfig), C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                    C.c_int, C.c_void_p]
    lib.syn_mcts_search_lockstep.argtypes = [C.c_void_p, C.POINTER(CMctsConfig), C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                             C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    lib.syn_mcts_search_rollout.argtypes = [C.c_void_p, C.POINTER(CMctsConfig), C.c_uint64, C.c_void_p, C.c_void_p, C.c_int,
                                            C.c_int, C.c_int, C.c_void_p]
    lib.syn_frozen_search_rollout.argtypes = [C.c_void_p, C.POINTER(CMctsConfig), C.c_void_p, C.c_void_p, C.c_void_p,
                                              C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    lib.syn_selfplay_run.argtypes = [C.c_void_p, C.POINTER(CRolloutConfig), C.c_uint64, C.c_uint64, C.c_int] + \
                                    [C.c_void_p] * 8
    lib.syn_selfplay_run_lockstep.argtypes = [C.c_void_p, C.POINTER(CRolloutConfig), C.c_uint64, C.c_uint64, C.c_int, C.c_int] + \
                                             [C.c_void_p] * 8
    lib.syn_match_run.argtypes = [C.c_void_p, C.POINTER(CMatchPlayer), C.POINTER(CMatchPlayer), C.c_void_p, C.c_void_p, C.c_size_t,
                                  C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.syn_match_run_sides.argtypes = [C.c_void_p, C.POINTER(CMatchSide), C.POINTER(CMatchSide), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.syn_tournament_run.argtypes = [C.c_void_p, C.POINTER(CMatchSide), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.syn_debug_tournament_regroup.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    lib.syn_progress.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.syn_cancel.argtypes = [C.c_void_p]
    lib.syn_trainer_set_precision.argtypes = [C.c_void_p, C.c_int]
    lib.syn_trainer_set_batch_mode.argtypes = [C.c_void_p, C.c_int, C.c_int]
    lib.syn_trainer_get_batch_mode.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.syn_last_timing.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_int)]
    lib.syn_last_launch_shape.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.syn_last_cache_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    lib.syn_debug_stdrng_u32.argtypes = [C.c_void_p, C.c_uint64, C.c_int, C.c_void_p]
    lib.syn_debug_fast_div.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    lib.syn_debug_small_int_math.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    lib.syn_debug_math.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.syn_default_rollout_config.argtypes = [C.POINTER(CRolloutConfig)]
    lib.syn_debug_calibrate.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    lib.syn_trainer_init.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(CTrainConfig)]
    lib.syn_trainer_init_conv.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(CTrainConfig)]
    lib.syn_train_step.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_float,
                                   C.c_void_p]
    lib.syn_train_gradients_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                               C.c_void_p, C.c_void_p]
    lib.syn_train_apply_device.argtypes = [C.c_void_p, C.c_void_p, C.c_float, C.c_float]
    lib.syn_train_gradients_enqueue.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                                C.c_void_p, C.c_void_p]
    lib.syn_train_apply_enqueue.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_float]
    lib.syn_trainer_get_state.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_longlong),
                                          C.c_void_p]
    lib.syn_trainer_publish_weights.argtypes = [C.c_void_p]
    lib.syn_train_set_data.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
    lib.syn_train_epoch.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_float, C.c_void_p]
    lib.syn_train_epochs_sampled.argtypes = [C.c_void_p, C.POINTER(CSamplerConfig), C.c_int, C.c_int, C.c_float, C.c_void_p,
                                             C.POINTER(C.c_size_t)]
    lib.syn_debug_sampler.argtypes = [C.c_void_p, C.POINTER(CSamplerConfig), C.c_uint32, C.c_size_t, C.c_void_p, C.c_void_p]
    lib.syn_replay_deduplicate.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.POINTER(C.c_size_t)]
    lib.syn_replay_reserve.argtypes = [C.c_void_p, C.c_size_t]
    lib.syn_replay_clear.argtypes = [C.c_void_p]
    lib.syn_replay_size.argtypes = [C.c_void_p, C.POINTER(C.c_size_t)]
    lib.syn_selfplay_positions_device.argtypes = [C.c_void_p, C.c_int64] + [C.c_void_p] * 5 + [C.c_size_t, C.POINTER(C.c_size_t)]
    lib.syn_replay_append_selfplay.argtypes = [C.c_void_p, C.c_int64, C.POINTER(C.c_size_t)]
    lib.syn_replay_append_device.argtypes = [C.c_void_p] + [C.c_void_p] * 5 + [C.c_size_t]
    lib.syn_replay_append.argtypes = [C.c_void_p] + [C.c_void_p] * 5 + [C.c_size_t]
    lib.syn_replay_keep_games_from.argtypes = [C.c_void_p, C.c_int64]
    lib.syn_replay_read.argtypes = [C.c_void_p] + [C.c_void_p] * 5 + [C.c_size_t, C.POINTER(C.c_size_t)]
    lib.syn_replay_deduplicate_to_trainer.argtypes = [C.c_void_p, C.POINTER(C.c_size_t)]
    lib.syn_train_get_data.argtypes = [C.c_void_p] + [C.c_void_p] * 4 + [C.c_size_t, C.POINTER(C.c_size_t)]
    lib.syn_positions_mirror.argtypes = [C.c_void_p] + [C.c_void_p] * 3 + [C.c_size_t] + [C.c_void_p] * 3
    lib.syn_replay_deduplicate_symmetric.argtypes = [C.c_void_p] + [C.c_void_p] * 4 + [C.c_size_t] + [C.c_void_p] * 5 + [
        C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    lib.syn_replay_deduplicate_to_trainer_symmetric.argtypes = [C.c_void_p, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    # held-out evaluation: the in-tree library has these (a missing one raises here); an older build of the ABI that SYNTHESIS_AMD_LIB
    # names for an A/B arm may not
    for name, argtypes in (("syn_dataset_set", [C.c_void_p] + [C.c_void_p] * 4 + [C.c_size_t]),
                           ("syn_dataset_get", [C.c_void_p] + [C.c_void_p] * 4 + [C.c_size_t, C.POINTER(C.c_size_t)]),
                           ("syn_dataset_evaluate", [C.c_void_p, C.c_int, C.c_size_t, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int,
                                                     C.POINTER(CDatasetMetrics), C.c_void_p, C.c_void_p, C.c_void_p]),
                           ("syn_dataset_evaluate_arith", [C.c_void_p, C.c_int, C.c_size_t, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int, C.c_int,
                                                           C.POINTER(CDatasetMetrics), C.c_void_p, C.c_void_p, C.c_void_p]),
                           ("syn_replay_set_holdout", [C.c_void_p, C.c_uint64, C.c_uint64]),
                           ("syn_dataset_counts", [C.c_void_p, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
                           ("syn_replay_reanalyse", [C.c_void_p, C.POINTER(CMctsConfig), C.POINTER(CReanalyseConfig),
                                                     C.POINTER(CReanalyseStats), C.c_void_p, C.c_size_t]),
                           ("syn_trainer_set_state", [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_longlong]),
                           ("syn_state_digest", [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
                           ("syn_games_run_recorded", [C.c_void_p, C.POINTER(CMatchSide), C.c_int] + [C.c_void_p] * 5 + [
                               C.c_int, C.POINTER(CRecordConfig)] + [C.c_void_p] * 5 + [C.POINTER(CRecordOutputs)]),
                           ("syn_replay_select_positions", [C.c_void_p, C.c_uint64, C.c_uint64, C.c_int64, C.c_void_p, C.c_void_p, C.c_size_t,
                                                            C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)])):
        if hasattr(lib, name) or not os.environ.get("SYNTHESIS_AMD_LIB"):
            getattr(lib, name).argtypes = argtypes
    _lib = lib
    return lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _is_mirror(symmetry):
    if symmetry not in ("none", "mirror"):
        raise ValueError(f"symmetry must be 'none' or 'mirror', got {symmetry!r}")
    return symmetry == "mirror"


def _network_of(n_params):
    return "Connect4ConvNet" if n_params == CONV_NUM_PARAMS else "Connect4Net"


def _plan_dict(pl, network):
    """syn_f16x2_plan as a dict; "network" names the network it belongs to (Connect4ConvNet: layer 0 = the conv layer, 1 = the head,
    2..4 zero)."""
    return dict(network=network, activation_exp=list(pl.activation_exp), weight_exp=list(pl.weight_exp), out_exp=pl.out_exp,
                bound=list(pl.bound))


def f16x2_plan_of_blob(blob):
    """The f16x2 plan (power-of-two scales) syn_set_network_arithmetic would choose for a Connect4Net (30,492 floats) or Connect4ConvNet
    (12,412 floats) blob — host code only, no GPU. None when the blob has no plan (non-finite parameters)."""
    lib = load_library()
    blob = np.ascontiguousarray(blob, dtype=np.float32).ravel()
    pl = CF16x2Plan()
    rc = lib.syn_f16x2_plan_of_blob(_p(blob), blob.size, C.byref(pl))
    if rc != 0:
        raise SynthesisAmdError(rc, "syn_f16x2_plan_of_blob: bad arguments")
    if not pl.valid:
        return None
    return _plan_dict(pl, _network_of(blob.size))


def shard_games(n_games, rank, world_size):
    """Static partition of game indices over ranks/GPUs (games share nothing: alpha_zero.rs:181-209). Rank r plays
    games r, r + world, r + 2*world, ... expressed as (first_game, count, stride=1) blocks: we use contiguous blocks so
    a rank's games are [first, first + count)."""
    base, rem = divmod(n_games, world_size)
    count = base + (1 if rank < rem else 0)
    first = rank * base + min(rank, rem)
    return first, count


class EvalContext:
    """syn_eval_ctx: Policy::eval for a batch (policies/traits.rs:4-6) on its own stream — eval(), or submit() ... wait()."""

    def __init__(self, engine):
        self._engine = engine
        self._lib = engine._lib
        self._c = C.c_void_p()
        engine._check(self._lib.syn_eval_ctx_create(engine._h, C.byref(self._c)))
        self._n = None

    def _check(self, rc):
        if rc != 0:
            raise SynthesisAmdError(rc, (self._lib.syn_eval_ctx_last_error(self._c) or b"").decode())

    def submit(self, my_bb, op_bb):
        my = np.ascontiguousarray(my_bb, dtype=np.uint64).ravel()
        op = np.ascontiguousarray(op_bb, dtype=np.uint64).ravel()
        if my.size != op.size:
            raise ValueError("my_bb and op_bb must have the same length")
        self._check(self._lib.syn_eval_ctx_submit(self._c, _p(my), _p(op), int(my.size)))   # (a refused submit leaves a batch in flight as it was)
        self._n = int(my.size)

    def wait(self):
        """Results of the submitted batch. Raises when nothing was submitted (or the submission failed): there is nothing to wait for."""
        if self._n is None:
            raise SynthesisAmdError(-1, "EvalContext.wait(): no batch has been submitted")
        n, self._n = self._n, None
        logits = np.zeros((n, 9), np.float32)
        value = np.zeros((n, 3), np.float32)
        self._check(self._lib.syn_eval_ctx_wait(self._c, _p(logits), _p(value)))
        return logits, value

    def eval(self, my_bb, op_bb):
        self.submit(my_bb, op_bb)
        return self.wait()

    def close(self):
        if self._c is not None and self._c.value:
            self._lib.syn_eval_ctx_destroy(self._c)
            self._c = C.c_void_p()
            if self in getattr(self._engine, "_contexts", []):
                self._engine._contexts.remove(self)


class Engine:
    """One handle = one GPU + one stream (the reference's one policy per worker thread, alpha_zero.rs:192-198)."""

    def __init__(self, concurrent_games=4096, max_explores=800, device=0, policy_cache_log2=0):
        self._lib = load_library()
        self._h = C.c_void_p()
        cfg = CEngineConfig(int(concurrent_games), int(max_explores), int(policy_cache_log2), 0)
        rc = self._lib.syn_engine_create(C.byref(cfg), int(device), C.byref(self._h))
        if rc != 0:
            msg = self._lib.syn_last_error(None)
            raise SynthesisAmdError(rc, msg.decode() if msg else "syn_engine_create failed")
        self.concurrent_games = int(concurrent_games)
        self.max_explores = int(max_explores)
        self.device = int(device)
        self._net_params = None   # parameter count of the network the engine evaluates (set by the loads and the learner's publish)

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            for ctx in list(getattr(self, "_contexts", [])):
                ctx.close()
            self._lib.syn_engine_destroy(self._h)
            self._h = C.c_void_p()

    def eval_context(self):
        """One worker's policy object (alpha_zero.rs:192-198: every worker thread owns its policy): an evaluation context of this
        engine — own stream and staging, this engine's weights. Contexts may be used from different threads at the same time."""
        ctx = EvalContext(self)
        if not hasattr(self, "_contexts"):
            self._contexts = []
        self._contexts.append(ctx)
        return ctx

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _check(self, rc):
        if rc != 0:
            msg = self._lib.syn_last_error(self._h)
            raise SynthesisAmdError(rc, msg.decode() if msg else "")

    # ---- weights (vs.load, alpha_zero.rs:194)
    def load_weights(self, blob):
        blob = np.ascontiguousarray(blob, dtype=np.float32).ravel()
        self._check(self._lib.syn_load_weights(self._h, _p(blob), blob.size))
        self._net_params = NUM_PARAMS

    def load_weights_conv(self, blob):
        """Connect4ConvNet (Conv2d<2,16,3,pad 1> + ReLU + Linear<1008,12>; include/synthesis_amd.h) becomes the engine's policy."""
        blob = np.ascontiguousarray(blob, dtype=np.float32).ravel()
        self._check(self._lib.syn_load_weights_conv(self._h, _p(blob), blob.size))
        self._net_params = CONV_NUM_PARAMS

    # ---- the arithmetic the network is evaluated in (include/synthesis_amd.h: SYN_NET_ARITH_*)
    def set_network_arithmetic(self, arithmetic):
        """"f32" (default: v_mfma_f32_16x16x4_f32, the oracle's ACC_FMA) or "f16x2" (two-term f16 split on v_mfma_f32_16x16x32_f16: the
        oracle's ACC_F16X2 for Connect4Net, conv_f16x2_tile.cuh for Connect4ConvNet); holds for policy_eval, evaluation contexts,
        mcts_search and selfplay — and for weights loaded or published later — until changed."""
        code = {"f32": 0, "f16x2": 1}.get(arithmetic, arithmetic)
        self._check(self._lib.syn_set_network_arithmetic(self._h, int(code)))

    def network_arithmetic(self):
        """(name, plan): plan = None or a dict of the f16x2 scales of the engine's current network ("network" says which)."""
        a = C.c_int()
        pl = CF16x2Plan()
        self._check(self._lib.syn_get_network_arithmetic(self._h, C.byref(a), C.byref(pl)))
        plan = None
        if pl.valid:
            plan = _plan_dict(pl, _network_of(self._net_params))
        return ("f16x2" if a.value == 1 else "f32"), plan

    # ---- Policy::eval, batched (policies.rs:47-59)
    def policy_eval(self, my_bb, op_bb):
        my = np.ascontiguousarray(my_bb, dtype=np.uint64).ravel()
        op = np.ascontiguousarray(op_bb, dtype=np.uint64).ravel()
        if my.size != op.size:
            raise ValueError("my_bb and op_bb must have the same length")
        logits = np.zeros((my.size, 9), np.float32)
        value = np.zeros((my.size, 3), np.float32)
        self._check(self._lib.syn_policy_eval_batch(self._h, _p(my), _p(op), int(my.size), _p(logits), _p(value)))
        return logits, value

    def policy_eval_device(self, d_my, d_op, n, d_logits, d_value, sync=True):
        """Device-pointer form (ints = raw device addresses, e.g. torch tensor .data_ptr())."""
        self._check(self._lib.syn_policy_eval_batch_device(self._h, C.c_void_p(d_my), C.c_void_p(d_op), int(n),
                                                           C.c_void_p(d_logits), C.c_void_p(d_value), int(sync)))

    # ---- Game::features (connect4.rs:235-258)
    def features(self, my_bb, op_bb):
        my = np.ascontiguousarray(my_bb, dtype=np.uint64).ravel()
        op = np.ascontiguousarray(op_bb, dtype=np.uint64).ravel()
        out = np.zeros((my.size, 63), np.float32)
        self._check(self._lib.syn_features_batch(self._h, _p(my), _p(op), int(my.size), _p(out)))
        return out

    # ---- slimnn layers
    def linear(self, W, b, x, relu=False):
        W = np.ascontiguousarray(W, np.float32)
        b = np.ascontiguousarray(b, np.float32)
        x = np.ascontiguousarray(x, np.float32).reshape(-1, W.shape[1])
        y = np.zeros((x.shape[0], W.shape[0]), np.float32)
        self._check(self._lib.syn_linear_forward(self._h, W.shape[1], W.shape[0], _p(W), _p(b), _p(x), x.shape[0],
                                                 _p(y), int(relu)))
        return y

    def activation(self, kind, x):
        """slimnn activation layer on x[batch][n]: kind 0 ReLU, 1 Tanh, 2 Softmax::apply_1d per row (activations.rs:31-63)."""
        x = np.ascontiguousarray(x, np.float32)
        x2 = x.reshape(1, -1) if x.ndim == 1 else x.reshape(x.shape[0], -1)
        y = np.zeros_like(x2)
        self._check(self._lib.syn_activation_forward(self._h, int(kind), _p(x2), int(x2.shape[0]), int(x2.shape[1]), _p(y)))
        return y.reshape(x.shape)

    def conv2d(self, W, b, x, row_pad=0, col_pad=0, stride=1, relu=False, out_hw=None):
        W = np.ascontiguousarray(W, np.float32)
        b = np.ascontiguousarray(b, np.float32)
        x = np.ascontiguousarray(x, np.float32)
        if x.ndim == 3:
            x = x[None]
        cout, cin, k, _ = W.shape
        n, _, h_in, w_in = x.shape
        if out_hw is None:
            out_hw = ((h_in + 2 * row_pad - k) // stride + 1, (w_in + 2 * col_pad - k) // stride + 1)
        h_out, w_out = out_hw
        y = np.zeros((n, cout, max(h_out, 0), max(w_out, 0)), np.float32)
        self._check(self._lib.syn_conv2d_forward(self._h, cin, cout, k, row_pad, col_pad, stride, h_in, w_in, h_out,
                                                 w_out, _p(W), _p(b), _p(x), n, _p(y), int(relu)))
        return y

    # ---- MCTS::with_capacity + explore_n on n roots (mcts.rs:123-147)
    def mcts_search(self, cfg: MCTSConfig, my_bb, op_bb, explores, action_selection=1, rollout_seed=None):
        """rollout_seed=None: the network is the leaf policy. Otherwise MCTS over RolloutPolicy (policies/rollout.rs:8-31, the pairing of the reference's MCTS tests, mcts.rs:691-868): playout
        leaf evaluations, root i on StdRng::seed_from_u64(rollout_seed + i)."""
        my = np.ascontiguousarray(my_bb, dtype=np.uint64).ravel()
        op = np.ascontiguousarray(op_bb, dtype=np.uint64).ravel()
        n = int(my.size)
        res = (CSearchResult * max(n, 1))()
        c = cfg.to_c()
        if rollout_seed is None:
            rc = self._lib.syn_mcts_search(self._h, C.byref(c), _p(my), _p(op), n, int(explores),
                                           int(action_selection), C.cast(res, C.c_void_p))
        else:
            rc = self._lib.syn_mcts_search_rollout(self._h, C.byref(c), int(rollout_seed), _p(my), _p(op), n,
                                                   int(explores), int(action_selection), C.cast(res, C.c_void_p))
        if rc != -7:    # SYN_ERR_CANCELLED (Engine.cancel from another thread): searched roots are valid, the others all zero
            self._check(rc)
        out = self._search_records(res, n)
        if rc == -7:
            out["cancelled"] = True
        return out

    # ---- eval_against_old's game loop (evaluator.rs:129-160) for many games, resident on the device
    def match_run(self, first, second, blob_first, blob_second, start_my, start_op):
        """syn_match_run: game g starts at (start_my[g], start_op[g]) with `first` to move; ply k is searched by player k % 2 with its
        own blob. `first` / `second`: anything with .explores, .action and .mcts_cfg (a match.Player, an arena.ArenaPlayer); only
        deterministic configurations. Both blobs are of the engine's current network kind and run in its current arithmetic; the
        engine's own network and policy cache are untouched. Returns dict(rewards [n] for `first`, plies [n], moves [n, 63] (255 = no
        move), final_bb [n, 2] = (first's stones, second's stones))."""
        my, op, _ = self._match_starts(start_my, start_op)
        b1 = np.ascontiguousarray(blob_first, dtype=np.float32).ravel()
        b2 = np.ascontiguousarray(blob_second, dtype=np.float32).ravel()
        if b1.size != b2.size:
            raise ValueError("both blobs must be parameters of the same network")
        n = int(my.size)
        players = [CMatchPlayer(int(p.explores), int(p.action), p.mcts_cfg.to_c()) for p in (first, second)]
        out = self._match_outputs(n, rng_words=False)
        self._check(self._lib.syn_match_run(self._h, C.byref(players[0]), C.byref(players[1]), _p(b1), _p(b2), b1.size, _p(my), _p(op), n,
                                            _p(out["rewards"]), _p(out["plies"]), _p(out["moves"]), _p(out["final_bb"])))
        return out

    def match_run_sides(self, first, second, start_my, start_op, seeds=None):
        """syn_match_run_sides: match_run with a description per side. A side is anything with .explores, .action, .mcts_cfg, .frozen,
        .weights and an optional .arithmetic (a match.Player):
          .frozen True   the evaluator's baseline, FrozenMCTS over RolloutPolicy (match.vanilla_player). Game g's playouts come from
                         StdRng::seed_from_u64(seeds[g]), one generator per game for the whole game, shared by two baseline sides.
          .frozen False  a network side: .weights is its blob (of the engine's network kind), .arithmetic None (the engine's), "f32" or
                         "f16x2" — the two sides may differ from each other and from the engine.
        `seeds` is needed when a side is a baseline. Returns match_run's dict plus "rng_words" [n]: each game's stream position at its
        end. The engine's own network, arithmetic and policy cache are untouched."""
        sides, keep = [], []
        for p in (first, second):
            side, blob = self.match_side(p)
            sides.append(side)
            keep.append(blob)   # (the struct holds a raw pointer into it)
        return self.match_run_sides_c(sides[0], sides[1], start_my, start_op, seeds)

    @staticmethod
    def match_side(p):
        """(CMatchSide, the array its blob pointer points into or None) of a player object"""
        arithmetic = getattr(p, "arithmetic", None)
        if arithmetic not in MATCH_ARITHMETICS:
            raise ValueError(f"a side's arithmetic must be None, 'f32' or 'f16x2', got {arithmetic!r}")
        player = CMatchPlayer(int(p.explores), int(p.action), p.mcts_cfg.to_c())
        if getattr(p, "frozen", False):
            return CMatchSide(MATCH_SIDE_KINDS["baseline"], 0, player, None, 0), None
        if getattr(p, "rollout", False):
            raise ValueError("a rollout_player (the self-play MCTS tree over RolloutPolicy) is not a side of a device match: its playout "
                             "seed is keyed by ply x batch size in play_match, so it stays with the host path")
        if getattr(p, "weights", None) is None:
            raise ValueError("a network side of a device match needs its own .weights (the engine cannot hand back the blob it holds)")
        blob = np.ascontiguousarray(p.weights, dtype=np.float32).ravel()
        return CMatchSide(MATCH_SIDE_KINDS["network"], MATCH_ARITHMETICS[arithmetic], player, blob.ctypes.data, blob.size), blob

    def match_run_sides_c(self, side_first, side_second, start_my, start_op, seeds=None):
        """match_run_sides on two CMatchSide structs as they are (the blobs they point to must stay alive for the call)"""
        my, op, sd = self._match_starts(start_my, start_op, seeds)
        n = int(my.size)
        out = self._match_outputs(n)
        self._check(self._lib.syn_match_run_sides(self._h, C.byref(side_first), C.byref(side_second), _p(my), _p(op), _p(sd), n,
                                                  _p(out["rewards"]), _p(out["plies"]), _p(out["moves"]), _p(out["final_bb"]),
                                                  _p(out["rng_words"])))
        return out

    def tournament_run(self, players, first, second, start_my, start_op, seeds=None):
        """syn_tournament_run: a whole schedule of games between len(players) players in one device-resident loop. `players` are
        objects match_side accepts (what match_run_sides takes as a side); game g starts at (start_my[g], start_op[g]) with
        players[first[g]] to move and players[second[g]] moving second, on the generator of seeds[g] (needed when a player is a baseline).
        Game g's record is what match_run_sides(players[first[g]], players[second[g]], ...) returns for that one game. Returns
        match_run_sides' dict. The engine's own network, arithmetic and policy cache are untouched."""
        sides, keep = [], []
        for p in players:
            side, blob = self.match_side(p)
            sides.append(side)
            keep.append(blob)   # (the struct holds a raw pointer into it)
        return self.tournament_run_c(sides, first, second, start_my, start_op, seeds)

    def tournament_run_c(self, sides, first, second, start_my, start_op, seeds=None, n_players=None):
        """tournament_run on CMatchSide structs as they are (the blobs they point to must stay alive for the call); n_players
        overrides len(sides) (the refusal tests)"""
        fi = np.ascontiguousarray(first, dtype=np.int32).ravel()
        se = np.ascontiguousarray(second, dtype=np.int32).ravel()
        my, op, sd = self._match_starts(start_my, start_op, seeds, "first, second, start_my and start_op", (fi.size, se.size))
        n = int(my.size)
        arr = (CMatchSide * max(len(sides), 1))(*sides)
        out = self._match_outputs(n)
        self._check(self._lib.syn_tournament_run(self._h, arr, len(sides) if n_players is None else int(n_players), _p(fi), _p(se), _p(my),
                                                 _p(op), _p(sd), n, _p(out["rewards"]), _p(out["plies"]), _p(out["moves"]),
                                                 _p(out["final_bb"]), _p(out["rng_words"])))
        return out

    def games_run_recorded(self, players, first, second, start_my, start_op, seeds=None, record=None, outputs=True):
        """syn_games_run_recorded (include/synthesis_amd.h "Recorded games"): tournament_run's schedule of games, each played as
        run_game — sample_action, the stop rule and the value target of `record` (a RecordConfig; RecordConfig.from_rollout(cfg, mask)
        copies a rollout configuration's) — from (start_my[g], start_op[g]) on the generator of seeds[g], with training rows for the plies
        of the players whose bit is set in record.record_mask. Network players only, deterministic search configurations only.
        Returns tournament_run's dict (plies = all moves of a game) plus rows [n], and with outputs=True the padded rows in selfplay()'s
        shapes: states [n, 63, 2] (also under selfplay()'s name states_bb), pis, vs, actions, root_nodes, final_kind. The rows replace
        the last selfplay()'s in the engine: replay_append_selfplay(first_gid) / selfplay_positions_device compact them next."""
        sides, keep = [], []
        for p in players:
            side, blob = self.match_side(p)
            sides.append(side)
            keep.append(blob)   # (the struct holds a raw pointer into it)
        return self.games_run_recorded_c(sides, first, second, start_my, start_op, seeds, record, outputs)

    def games_run_recorded_c(self, sides, first, second, start_my, start_op, seeds=None, record=None, outputs=True, n_players=None):
        """games_run_recorded on CMatchSide structs as they are (the blobs they point to must stay alive for the call); n_players
        overrides len(sides) (the refusal tests)"""
        record = RecordConfig() if record is None else record
        if not isinstance(record, RecordConfig):
            raise ValueError(f"record must be a RecordConfig, got {type(record).__name__}")
        fi = np.ascontiguousarray(first, dtype=np.int32).ravel()
        se = np.ascontiguousarray(second, dtype=np.int32).ravel()
        my, op, sd = self._match_starts(start_my, start_op, seeds, "first, second, start_my and start_op", (fi.size, se.size))
        n = int(my.size)
        arr = (CMatchSide * max(len(sides), 1))(*sides)
        out = self._match_outputs(n)
        out["rows"] = np.zeros(n, np.int32)
        if outputs:
            out.update(states=np.zeros((n, 63, 2), np.uint64), pis=np.zeros((n, 63, 9), np.float32), vs=np.zeros((n, 63, 3), np.float32),
                       actions=np.zeros((n, 63), np.uint8), root_nodes=np.zeros((n, 63), np.uint32), final_kind=np.zeros(n, np.uint8))
        ptr = lambda k: out[k].ctypes.data if k in out else None
        ro = CRecordOutputs(ptr("rows"), ptr("states"), ptr("pis"), ptr("vs"), ptr("actions"), ptr("root_nodes"), ptr("final_kind"))
        rc = record.to_c()
        self._check(self._lib.syn_games_run_recorded(self._h, arr, len(sides) if n_players is None else int(n_players), _p(fi), _p(se), _p(my),
                                                     _p(op), _p(sd), n, C.byref(rc), _p(out["rewards"]), _p(out["plies"]), _p(out["moves"]),
                                                     _p(out["final_bb"]), _p(out["rng_words"]), C.byref(ro)))
        if outputs:
            out["states_bb"] = out["states"]
        return out

    @staticmethod
    def _match_starts(start_my, start_op, seeds=None, names="start_my and start_op", other_sizes=()):
        """(my, op, seeds or None) as the game loops take them: contiguous uint64 [n], seeds broadcast to n; ValueError when the
        lengths (other_sizes: the schedule's) differ"""
        my = np.ascontiguousarray(start_my, dtype=np.uint64).ravel()
        op = np.ascontiguousarray(start_op, dtype=np.uint64).ravel()
        if any(size != my.size for size in (op.size, *other_sizes)):
            raise ValueError(f"{names} must have the same length")
        sd = None
        if seeds is not None:
            sd = np.ascontiguousarray(np.broadcast_to(np.asarray(seeds, dtype=np.uint64), (my.size,)))
        return my, op, sd

    @staticmethod
    def _match_outputs(n, rng_words=True):
        """the per-game output arrays of the game loops, as they read for a game that was never played"""
        out = dict(rewards=np.zeros(n, np.float32), plies=np.zeros(n, np.int32), moves=np.full((n, 63), 255, np.uint8),
                   final_bb=np.zeros((n, 2), np.uint64))
        if rng_words:
            out["rng_words"] = np.zeros(n, np.uint64)
        return out

    @staticmethod
    def _search_records(res, n):
        raw = np.frombuffer(res, dtype=np.uint8).reshape(max(n, 1), C.sizeof(CSearchResult))[:n]
        dt = np.dtype([("child_N", np.float32, (9,)), ("child_W", np.float32, (9, 3)), ("child_P", np.float32, (9,)),
                       ("child_sol", np.int32, (9, 3)), ("root_N", np.float32), ("root_W", np.float32, (3,)),
                       ("root_sol", np.int32, (3,)), ("num_nodes", np.uint32), ("best_action", np.int32),
                       ("target_pi", np.float32, (9,)), ("target_q", np.float32, (3,))])
        assert dt.itemsize == C.sizeof(CSearchResult)
        rec = raw.copy().view(dt).reshape(n)
        out = {k: rec[k].copy() for k in dt.names}
        out["root_stat"] = np.concatenate([out.pop("root_N")[:, None], out.pop("root_W")], axis=1)
        return out

    def mcts_search_lockstep(self, cfg: MCTSConfig, my_bb, op_bb, explores, action_selection=1, host_threads=0):
        """The same search with the trees on the host and only Policy::eval on the GPU (include/synthesis_amd_lockstep.hpp behind
        syn_mcts_search_lockstep): all roots advance in lock step, one syn_policy_eval_batch launch per round. Returns mcts_search's
        dict plus "stats" (rounds, positions_evaluated, seconds_total, seconds_policy)."""
        my = np.ascontiguousarray(my_bb, dtype=np.uint64).ravel()
        op = np.ascontiguousarray(op_bb, dtype=np.uint64).ravel()
        n = int(my.size)
        res = (CSearchResult * max(n, 1))()

        class CStats(C.Structure):
            _fields_ = [("rounds", C.c_uint64), ("positions_evaluated", C.c_uint64), ("seconds_total", C.c_double),
                        ("seconds_policy", C.c_double)]
        st = CStats()
        c = cfg.to_c()
        rc = self._lib.syn_mcts_search_lockstep(self._h, C.byref(c), _p(my), _p(op), n, int(explores), int(action_selection),
                                                int(host_threads), C.cast(res, C.c_void_p), C.cast(C.byref(st), C.c_void_p))
        self._check(rc)
        out = self._search_records(res, n)
        out["stats"] = {"rounds": int(st.rounds), "positions_evaluated": int(st.positions_evaluated),
                        "seconds_total": float(st.seconds_total), "seconds_policy": float(st.seconds_policy)}
        return out

    def selfplay_lockstep(self, cfg: RolloutConfig, base_seed, n_games, first_game=0, host_threads=0):
        """run_n_games with every game's trees on the host and only Policy::eval on the GPU (syn_selfplay_run_lockstep; BASELINE
        configs[1] as worded). Returns selfplay()'s arrays plus "stats"; the games equal selfplay()'s."""
        n = int(n_games)
        r = dict(plies=np.zeros(n, np.int32), states_bb=np.zeros((n, 63, 2), np.uint64), pis=np.zeros((n, 63, 9), np.float32),
                 vs=np.zeros((n, 63, 3), np.float32), actions=np.zeros((n, 63), np.uint8), root_nodes=np.zeros((n, 63), np.uint32),
                 final_kind=np.zeros(n, np.uint8))

        class CStats(C.Structure):
            _fields_ = [("rounds", C.c_uint64), ("positions_evaluated", C.c_uint64), ("seconds_total", C.c_double),
                        ("seconds_policy", C.c_double)]
        st = CStats()
        c = cfg.to_c()
        rc = self._lib.syn_selfplay_run_lockstep(
            self._h, C.byref(c), int(base_seed), int(first_game), n, int(host_threads), _p(r["plies"]),
            _p(r["states_bb"]), _p(r["pis"]), _p(r["vs"]), _p(r["actions"]), _p(r["root_nodes"]), _p(r["final_kind"]),
            C.cast(C.byref(st), C.c_void_p))
        self._check(rc)
        r["stats"] = {"rounds": int(st.rounds), "positions_evaluated": int(st.positions_evaluated),
                      "seconds_total": float(st.seconds_total), "seconds_policy": float(st.seconds_policy)}
        return r

    # ---- the evaluator's baseline: FrozenMCTS::exploit over RolloutPolicy on n roots (evaluator.rs:308-319)
    FROZEN_DTYPE = np.dtype([("child_N", np.float32, (9,)), ("child_cum", np.float32, (9,)), ("child_P", np.float32, (9,)),
                             ("child_sol", np.int32, (9, 3)), ("root_N", np.float32), ("root_cum", np.float32),
                             ("root_sol", np.int32, (3,)), ("num_nodes", np.uint32), ("best_action", np.int32)])

    def frozen_search(self, cfg: MCTSConfig, seeds, rng_words, my_bb, op_bb, explores, action_selection=1):
        """Root i plays out on StdRng::seed_from_u64(seeds[i]) from output word rng_words[i] on (one generator per match,
        evaluator.rs:171-172); returns the per-root records plus "rng_words", the position to hand to the match's next search.
        `explores` is a scalar or one value per root."""
        my = np.ascontiguousarray(my_bb, dtype=np.uint64).ravel()
        op = np.ascontiguousarray(op_bb, dtype=np.uint64).ravel()
        n = int(my.size)
        sd = np.ascontiguousarray(np.broadcast_to(np.asarray(seeds, dtype=np.uint64), (n,)))
        words = np.array(np.broadcast_to(np.asarray(rng_words, dtype=np.uint64), (n,)), dtype=np.uint64)
        ex = np.ascontiguousarray(np.broadcast_to(np.asarray(explores, dtype=np.int32), (n,)))
        rec = np.zeros(max(n, 1), self.FROZEN_DTYPE)
        c = cfg.to_c()
        self._check(self._lib.syn_frozen_search_rollout(self._h, C.byref(c), _p(sd), _p(words), _p(my), _p(op), _p(ex), n,
                                                        int(action_selection), _p(rec)))
        out = {k: rec[k][:n].copy() for k in self.FROZEN_DTYPE.names}
        out["root_stat"] = np.stack([out.pop("root_N"), out.pop("root_cum")], axis=1)
        out["rng_words"] = words
        return out

    # ---- run_n_games (alpha_zero.rs:181-209)
    def selfplay(self, cfg: RolloutConfig, base_seed, n_games, first_game=0, outputs=True, counters=False):
        n = int(n_games)
        r = dict(plies=np.zeros(n, np.int32))
        if outputs:
            r.update(states_bb=np.zeros((n, 63, 2), np.uint64), pis=np.zeros((n, 63, 9), np.float32),
                     vs=np.zeros((n, 63, 3), np.float32), actions=np.zeros((n, 63), np.uint8),
                     root_nodes=np.zeros((n, 63), np.uint32), final_kind=np.zeros(n, np.uint8))
        ctr = CCounters() if counters else None
        c = cfg.to_c()
        rc = self._lib.syn_selfplay_run(
            self._h, C.byref(c), int(base_seed), int(first_game), n, _p(r["plies"]), _p(r.get("states_bb")),
            _p(r.get("pis")), _p(r.get("vs")), _p(r.get("actions")), _p(r.get("root_nodes")), _p(r.get("final_kind")),
            C.cast(C.byref(ctr), C.c_void_p) if ctr is not None else None)
        if rc == -7:    # SYN_ERR_CANCELLED (Engine.cancel from another thread): the games that finished are valid, plies == 0 otherwise
            r["cancelled"] = True
        else:
            self._check(rc)
        if ctr is not None:
            r["counters"] = {name: int(getattr(ctr, name)) for name, _ in CCounters._fields_}
        r["kernel_ms"] = self.last_kernel_ms()
        return r

    def progress(self):
        """(jobs started, games finished) of the call running on this engine — callable from another thread while it runs."""
        a, b = C.c_int(), C.c_int()
        self._check(self._lib.syn_progress(self._h, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def cancel(self):
        """No further game (or root) starts; the running selfplay() / mcts_search() returns once the started ones have finished,
        with result["cancelled"] = True if anything was left out (plies == 0 / num_nodes == 0 mark those). Raises
        SynthesisAmdError(SYN_ERR_INVALID_ARGUMENT) when no call is in flight on this engine."""
        self._check(self._lib.syn_cancel(self._h))

    def last_cache_stats(self):
        """(hits, misses) of the device PolicyWithCache during the last search / self-play call."""
        a, b = C.c_uint64(), C.c_uint64()
        self._check(self._lib.syn_last_cache_stats(self._h, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def last_launch_shape(self):
        """(shape, workgroups, threads per workgroup) of the last search / self-play launch; shape 4 = lane-per-tree."""
        s, g, t = C.c_int(), C.c_int(), C.c_int()
        self._check(self._lib.syn_last_launch_shape(self._h, C.byref(s), C.byref(g), C.byref(t)))
        return s.value, g.value, t.value

    def last_kernel_ms(self):
        ms = C.c_float()
        nl = C.c_int()
        self._check(self._lib.syn_last_timing(self._h, C.byref(ms), C.byref(nl)))
        return float(ms.value)

    def last_timing(self):
        """syn_last_timing: (device milliseconds, kernel launches) of the last call; summed over plies for a match or a tournament"""
        ms = C.c_float()
        nl = C.c_int()
        self._check(self._lib.syn_last_timing(self._h, C.byref(ms), C.byref(nl)))
        return float(ms.value), int(nl.value)

    # ---- learner step (alpha_zero.rs:31-36,72-94) and replay de-duplication (data.rs:196-235)
    def trainer_init(self, blob, weight_decay=1e-6, policy_weight=1.0, value_weight=1.0, beta1=0.9, beta2=0.999,
                     eps=1e-8):
        blob = np.ascontiguousarray(blob, dtype=np.float32).ravel()
        cfg = CTrainConfig(weight_decay, policy_weight, value_weight, beta1, beta2, eps)
        self._check(self._lib.syn_trainer_init(self._h, _p(blob), blob.size, C.byref(cfg)))
        self._trainer_params = NUM_PARAMS

    def trainer_init_conv(self, blob, weight_decay=1e-6, policy_weight=1.0, value_weight=1.0, beta1=0.9, beta2=0.999, eps=1e-8):
        """The learner for Connect4ConvNet (load_weights_conv's network and blob order): train_step / train_epoch /
        trainer_state / trainer_publish_weights then work on that network (minibatches of at most 32 positions)."""
        blob = np.ascontiguousarray(blob, dtype=np.float32).ravel()
        cfg = CTrainConfig(weight_decay, policy_weight, value_weight, beta1, beta2, eps)
        self._check(self._lib.syn_trainer_init_conv(self._h, _p(blob), blob.size, C.byref(cfg)))
        self._trainer_params = CONV_NUM_PARAMS

    def trainer_set_precision(self, precision):
        """"f32" (default; bit-identical to the oracle) | "bf16" (Connect4ConvNet learner only: bf16 matrix cores, f32 accumulation,
        f32 master weights and Adam — BASELINE configs[4]'s "bf16 conv")."""
        self._check(self._lib.syn_trainer_set_precision(self._h, {"f32": 0, "bf16": 1}[precision]))

    def trainer_set_batch_mode(self, mode="chained", max_workgroups=0):
        """"chained" (default: the oracle's one chain over the whole minibatch, one workgroup) | "micro" (SYN_TRAIN_BATCH_MICRO: a
        minibatch of 32 nb positions is nb micro-batches of 32, each the chained step of its 32 samples, summed in ascending order and
        multiplied by 1 / nb — on up to max_workgroups workgroups, 0 = one per CU; the batch must then be a multiple of 32)."""
        if mode not in BATCH_MODES:
            raise ValueError(f"batch mode must be one of {sorted(BATCH_MODES)}, got {mode!r}")
        self._check(self._lib.syn_trainer_set_batch_mode(self._h, BATCH_MODES[mode], int(max_workgroups)))

    def trainer_batch_mode(self):
        """(mode, max_workgroups, workgroups of the last micro-batch gradient launch: 0 if there has been none)."""
        m, w, g = C.c_int(), C.c_int(), C.c_int()
        self._check(self._lib.syn_trainer_get_batch_mode(self._h, C.byref(m), C.byref(w), C.byref(g)))
        return {v: k for k, v in BATCH_MODES.items()}[m.value], w.value, g.value

    def train_step(self, my_bb, op_bb, target_pi, target_v, lr):
        my = np.ascontiguousarray(my_bb, dtype=np.uint64).ravel()
        op = np.ascontiguousarray(op_bb, dtype=np.uint64).ravel()
        tpi = np.ascontiguousarray(target_pi, dtype=np.float32).reshape(my.size, 9)
        tv = np.ascontiguousarray(target_v, dtype=np.float32).reshape(my.size, 3)
        losses = np.zeros(2, np.float32)
        self._check(self._lib.syn_train_step(self._h, _p(my), _p(op), _p(tpi), _p(tv), int(my.size), float(lr),
                                             _p(losses)))
        return losses

    def train_gradients_device(self, d_my, d_op, d_tpi, d_tv, batch, d_grads):
        losses = np.zeros(2, np.float32)
        self._check(self._lib.syn_train_gradients_device(self._h, C.c_void_p(d_my), C.c_void_p(d_op),
                                                         C.c_void_p(d_tpi), C.c_void_p(d_tv), int(batch),
                                                         C.c_void_p(d_grads), _p(losses)))
        return losses

    def train_apply_device(self, d_grads, lr, grad_scale=1.0):
        self._check(self._lib.syn_train_apply_device(self._h, C.c_void_p(d_grads), float(lr), float(grad_scale)))

    def train_gradients_enqueue(self, stream, d_my, d_op, d_tpi, d_tv, batch, d_grads, d_losses=0):
        """syn_train_gradients_enqueue: the gradient kernel on `stream` (a raw hipStream_t, e.g. torch.cuda.current_stream().cuda_stream),
        loss sums to the device words at d_losses; nothing is synchronised."""
        self._check(self._lib.syn_train_gradients_enqueue(self._h, C.c_void_p(stream), C.c_void_p(d_my), C.c_void_p(d_op), C.c_void_p(d_tpi),
                                                          C.c_void_p(d_tv), int(batch), C.c_void_p(d_grads), C.c_void_p(d_losses)))

    def train_apply_enqueue(self, stream, d_grads, lr, grad_scale=1.0):
        self._check(self._lib.syn_train_apply_enqueue(self._h, C.c_void_p(stream), C.c_void_p(d_grads), float(lr), float(grad_scale)))

    def trainer_state(self):
        blob = np.zeros(getattr(self, "_trainer_params", NUM_PARAMS), np.float32)
        m = np.zeros_like(blob); v = np.zeros_like(blob); g = np.zeros_like(blob)
        step = C.c_longlong()
        self._check(self._lib.syn_trainer_get_state(self._h, _p(blob), _p(m), _p(v), C.byref(step), _p(g)))
        return dict(weights=blob, m=m, v=v, step=int(step.value), grads=g)

    def trainer_set_state(self, weights, m, v, step):
        """syn_trainer_set_state: the inverse of trainer_state — parameters, both Adam moments and the step count of an initialised
        trainer of the same network, bit for bit, with every derived device image rebuilt. Modes, hyper-parameters, data sets, the last
        gradient and the engine's network stay as they are; nothing is published."""
        arrays = [np.ascontiguousarray(a, dtype=np.float32).ravel() for a in (weights, m, v)]
        if len({a.size for a in arrays}) != 1:
            raise ValueError("weights, m and v must have the same size, got " + ", ".join(str(a.size) for a in arrays))
        self._check(self._lib.syn_trainer_set_state(self._h, _p(arrays[0]), _p(arrays[1]), _p(arrays[2]), int(arrays[0].size), int(step)))

    def state_digest(self, what, max_workgroups=0):
        """syn_state_digest: the 64-bit fingerprint (an int) of one piece of engine state, computed where it lives — `what` is
        "trainer" (w, m, v, step), "network" (the installed network's parameters), "replay" (the device replay buffer), "train_data" or
        "eval_data" (include/synthesis_amd.h "State digests"; synthesis_amd/digest.py is the same definition in numpy). The word does
        not depend on max_workgroups (0 = the library's grid)."""
        return self.state_digest_words(what, max_workgroups)[0]

    def state_digest_words(self, what, max_workgroups=0):
        """(digest, number of 32-bit words digested)"""
        from .digest import COMPONENTS
        if isinstance(what, str):   # (a number goes to the library as it is, which refuses the ones it does not know)
            if what not in COMPONENTS:
                raise ValueError(f"what must be one of {sorted(COMPONENTS)}, got {what!r}")
            what = COMPONENTS[what]
        d, n = C.c_uint64(), C.c_uint64()
        self._check(self._lib.syn_state_digest(self._h, int(what), int(max_workgroups), C.byref(d), C.byref(n)))
        return int(d.value), int(n.value)

    def train_set_data(self, my_bb, op_bb, target_pi, target_v):
        """Uploads the de-duplicated buffer once; train_epoch then indexes it on the device."""
        my = np.ascontiguousarray(my_bb, dtype=np.uint64).ravel()
        op = np.ascontiguousarray(op_bb, dtype=np.uint64).ravel()
        tpi = np.ascontiguousarray(target_pi, dtype=np.float32).reshape(my.size, 9)
        tv = np.ascontiguousarray(target_v, dtype=np.float32).reshape(my.size, 3)
        self._check(self._lib.syn_train_set_data(self._h, _p(my), _p(op), _p(tpi), _p(tv), int(my.size)))

    def train_epoch(self, perm, batch_size, lr):
        """len(perm) // batch_size optimiser steps in one call (drop_last = true); returns the per-step losses [steps][2]."""
        perm = np.ascontiguousarray(perm, dtype=np.int32).ravel()
        steps = perm.size // int(batch_size)
        losses = np.zeros((steps, 2), np.float32)
        self._check(self._lib.syn_train_epoch(self._h, _p(perm), steps, int(batch_size), float(lr), _p(losses)))
        return losses

    def train_epochs_sampled(self, key, n_epochs, batch_size, lr, first_epoch=0, flip=False):
        """syn_train_epochs_sampled: the epochs first_epoch .. first_epoch + n_epochs - 1 over the current data set in ONE call, every
        epoch's order (and, with flip=True, which rows enter mirrored) drawn on the device from `key` (include/synthesis_amd.h "Device-side
        epoch sampler"). Returns the per-step losses [n_epochs, n_steps, 2], n_steps = rows // batch_size (drop_last)."""
        n = C.c_size_t(0)
        if self._lib.syn_train_get_data(self._h, None, None, None, None, 1 << 62, C.byref(n)) != 0:
            n = C.c_size_t(0)   # (no trainer: the call below reports it)
        per = int(n.value) // int(batch_size) if int(batch_size) >= 1 else 0
        losses = np.zeros((max(int(n_epochs), 0), per, 2), np.float32)
        cfg = CSamplerConfig(int(key) & 0xFFFFFFFFFFFFFFFF, int(first_epoch), int(bool(flip)) if isinstance(flip, (bool, np.bool_)) else int(flip))
        steps = C.c_size_t()
        self._check(self._lib.syn_train_epochs_sampled(self._h, C.byref(cfg), int(n_epochs), int(batch_size), float(lr), _p(losses),
                                                       C.byref(steps)))
        return losses[:, : int(steps.value)]

    def debug_sampler(self, key, epoch, n, flip=False):
        """syn_debug_sampler: (perm [n] int32 = epoch `epoch`'s row order, flags [n] uint8 by row = which rows flip=True would mirror)
        for an n-row data set; needs no trainer. `flip` only fills the config: the flags do not depend on it."""
        perm = np.zeros(int(n), np.int32)
        flags = np.zeros(int(n), np.uint8)
        cfg = CSamplerConfig(int(key) & 0xFFFFFFFFFFFFFFFF, 0, int(bool(flip)))
        self._check(self._lib.syn_debug_sampler(self._h, C.byref(cfg), int(epoch), int(n), _p(perm), _p(flags)))
        return perm, flags

    def trainer_publish_weights(self):
        self._check(self._lib.syn_trainer_publish_weights(self._h))
        self._net_params = self._trainer_params

    def replay_deduplicate(self, my_bb, op_bb, pis, vs, symmetry="none"):
        """symmetry="mirror": the de-duplication over the canonical orientations, closed under the board's left-right mirror
        (syn_replay_deduplicate_symmetric): up to 2n rows, and the dict gains `canonical` = U, the number of leading canonical rows."""
        mirror = _is_mirror(symmetry)
        my = np.ascontiguousarray(my_bb, dtype=np.uint64).ravel()
        op = np.ascontiguousarray(op_bb, dtype=np.uint64).ravel()
        n = int(my.size)
        pis = np.ascontiguousarray(pis, dtype=np.float32).reshape(n, 9)
        vs = np.ascontiguousarray(vs, dtype=np.float32).reshape(n, 3)
        r = 2 * n if mirror else n
        o = dict(my_bb=np.zeros(r, np.uint64), op_bb=np.zeros(r, np.uint64), pis=np.zeros((r, 9), np.float32),
                 vs=np.zeros((r, 3), np.float32), num=np.zeros(r, np.uint32))
        cnt = C.c_size_t()
        if mirror:
            canonical = C.c_size_t()
            self._check(self._lib.syn_replay_deduplicate_symmetric(self._h, _p(my), _p(op), _p(pis), _p(vs), n, _p(o["my_bb"]),
                                                                   _p(o["op_bb"]), _p(o["pis"]), _p(o["vs"]), _p(o["num"]),
                                                                   C.byref(canonical), C.byref(cnt)))
            return dict({k: a[: cnt.value] for k, a in o.items()}, canonical=int(canonical.value))
        self._check(self._lib.syn_replay_deduplicate(self._h, _p(my), _p(op), _p(pis), _p(vs), n, _p(o["my_bb"]),
                                                     _p(o["op_bb"]), _p(o["pis"]), _p(o["vs"]), _p(o["num"]),
                                                     C.byref(cnt)))
        return {k: a[: cnt.value] for k, a in o.items()}

    def positions_mirror(self, my_bb, op_bb, pis=None):
        """The left-right mirror images of n positions (syn_positions_mirror): (my, op) as uint64 arrays, and with `pis` [n, 9] also
        the reversed policies: (my, op, pis)."""
        my = np.ascontiguousarray(my_bb, dtype=np.uint64).ravel()
        op = np.ascontiguousarray(op_bb, dtype=np.uint64).ravel()
        n = int(my.size)
        if op.size != n:
            raise ValueError("my_bb and op_bb must have the same length")
        omy, oop = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
        if pis is None:
            self._check(self._lib.syn_positions_mirror(self._h, _p(my), _p(op), None, n, _p(omy), _p(oop), None))
            return omy, oop
        pis = np.ascontiguousarray(pis, dtype=np.float32).reshape(n, 9)
        opi = np.zeros((n, 9), np.float32)
        self._check(self._lib.syn_positions_mirror(self._h, _p(my), _p(op), _p(pis), n, _p(omy), _p(oop), _p(opi)))
        return omy, oop, opi

    # ---- the replay buffer in device memory (data.rs:107-235; include/synthesis_amd.h syn_replay_*)
    def replay_reserve(self, capacity_positions):
        """Allocates the engine's buffer for that many positions (72 bytes each), or grows it keeping the contents."""
        self._check(self._lib.syn_replay_reserve(self._h, int(capacity_positions)))

    def replay_clear(self):
        self._check(self._lib.syn_replay_clear(self._h))

    def replay_size(self):
        n = C.c_size_t()
        self._check(self._lib.syn_replay_size(self._h, C.byref(n)))
        return int(n.value)

    def selfplay_positions_device(self, first_gid, d_my, d_op, d_gid, d_pi, d_v, capacity):
        """The last selfplay()'s positions compacted into caller-owned device sections (ints = raw device addresses, e.g. torch tensor
        .data_ptr(); room for `capacity` positions each): game order, then ply order, gid = first_gid + game slot. Returns their number."""
        n = C.c_size_t()
        self._check(self._lib.syn_selfplay_positions_device(self._h, int(first_gid), C.c_void_p(d_my), C.c_void_p(d_op), C.c_void_p(d_gid),
                                                            C.c_void_p(d_pi), C.c_void_p(d_v), int(capacity), C.byref(n)))
        return int(n.value)

    def replay_append_selfplay(self, first_gid):
        """The last selfplay()'s positions onto the tail of the buffer (no padded download: selfplay(..., outputs=False) is enough)."""
        n = C.c_size_t()
        self._check(self._lib.syn_replay_append_selfplay(self._h, int(first_gid), C.byref(n)))
        return int(n.value)

    def replay_append(self, my_bb, op_bb, gid, pis, vs):
        """Positions from host arrays (other ranks' games under a host transport, a caller's own) onto the tail."""
        my = np.ascontiguousarray(my_bb, dtype=np.uint64).ravel()
        op = np.ascontiguousarray(op_bb, dtype=np.uint64).ravel()
        g = np.ascontiguousarray(gid, dtype=np.int64).ravel()
        n = int(my.size)
        if op.size != n or g.size != n:
            raise ValueError("my_bb, op_bb and gid must have the same length")
        pis = np.ascontiguousarray(pis, dtype=np.float32).reshape(n, 9)
        vs = np.ascontiguousarray(vs, dtype=np.float32).reshape(n, 3)
        self._check(self._lib.syn_replay_append(self._h, _p(my), _p(op), _p(g), _p(pis), _p(vs), n))

    def replay_append_device(self, d_my, d_op, d_gid, d_pi, d_v, n):
        """n positions from device sections (raw addresses; their producer's stream must have been synchronised) onto the tail."""
        self._check(self._lib.syn_replay_append_device(self._h, C.c_void_p(d_my), C.c_void_p(d_op), C.c_void_p(d_gid), C.c_void_p(d_pi),
                                                       C.c_void_p(d_v), int(n)))

    def replay_keep_games_from(self, min_gid):
        """keep_last_n_games (data.rs:160-194): drops every position of a game before min_gid, keeps the order of the rest."""
        self._check(self._lib.syn_replay_keep_games_from(self._h, int(min_gid)))

    def replay_read(self):
        """The buffer as host arrays: dict(my, op, gid, pi [n, 9], v [n, 3]) in buffer order."""
        n = self.replay_size()
        o = dict(my=np.zeros(n, np.uint64), op=np.zeros(n, np.uint64), gid=np.zeros(n, np.int64), pi=np.zeros((n, 9), np.float32),
                 v=np.zeros((n, 3), np.float32))
        got = C.c_size_t()
        self._check(self._lib.syn_replay_read(self._h, _p(o["my"]), _p(o["op"]), _p(o["gid"]), _p(o["pi"]), _p(o["v"]), n, C.byref(got)))
        return o

    def replay_reanalyse(self, mcts_cfg: MCTSConfig, explores, key, fraction=None, threshold=None, before_gid=None, stream_base=0,
                         action_selection=1, value_mix=0.0, chunk_roots=0, rows=False):
        """syn_replay_reanalyse (include/synthesis_amd.h "Reanalyse"): the rows of the buffer that the hash of (key, gid, my, op) selects —
        about `fraction` (= threshold floor(fraction * 2^32), as holdout) of those with gid < before_gid (None: every game) — are searched
        again with the engine's network as roots of mcts_search(mcts_cfg, ..., explores, action_selection), the j-th on noise stream
        stream_base + j, and their pi (and, with value_mix > 0, v = v * (1 - value_mix) + target_q * value_mix) overwritten on the device.
        Returns dict(rows, selected, skipped, moved, chunks, launches); rows=True adds selected_rows (ascending row indices)."""
        if (fraction is None) == (threshold is None):
            raise ValueError("give exactly one of fraction and threshold")
        if threshold is None:
            if not 0.0 <= float(fraction) <= 1.0:
                raise ValueError(f"fraction must be in [0, 1], got {fraction!r}")
            threshold = int(np.floor(float(fraction) * 4294967296.0))
        if int(threshold) < 0 or int(stream_base) < 0:
            raise ValueError("threshold and stream_base must be >= 0")
        c = mcts_cfg.to_c() if mcts_cfg is not None else None
        r = CReanalyseConfig(int(key) & 0xFFFFFFFFFFFFFFFF, int(threshold), (1 << 63) - 1 if before_gid is None else int(before_gid),
                             int(stream_base) & 0xFFFFFFFFFFFFFFFF, int(explores), int(action_selection), float(value_mix), int(chunk_roots))
        sel = np.zeros(self.replay_size(), np.int64) if rows else None
        st = CReanalyseStats()
        self._check(self._lib.syn_replay_reanalyse(self._h, None if c is None else C.byref(c), C.byref(r), C.byref(st), _p(sel),
                                                   0 if sel is None else int(sel.size)))
        out = dict(rows=int(st.rows), selected=int(st.selected), skipped=int(st.skipped), moved=int(st.moved), chunks=int(st.chunks),
                   launches=int(st.launches))
        if rows:
            out["selected_rows"] = sel[: out["selected"]]
        return out

    def replay_select_positions(self, key, fraction=None, threshold=None, before_gid=None):
        """syn_replay_select_positions: the positions of the buffer's rows that replay_reanalyse(key, fraction / threshold, before_gid)
        would select (learner.reanalyse_flags is its host twin), in buffer order, downloaded alone; the buffer is untouched. Returns
        dict(my, op, skipped)."""
        if (fraction is None) == (threshold is None):
            raise ValueError("give exactly one of fraction and threshold")
        if threshold is None:
            if not 0.0 <= float(fraction) <= 1.0:
                raise ValueError(f"fraction must be in [0, 1], got {fraction!r}")
            threshold = int(np.floor(float(fraction) * 4294967296.0))
        if int(threshold) < 0:
            raise ValueError("threshold must be >= 0")
        args = (int(key) & 0xFFFFFFFFFFFFFFFF, int(threshold), (1 << 63) - 1 if before_gid is None else int(before_gid))
        n, skipped = C.c_size_t(), C.c_size_t()
        cap = self.replay_size()   # (host arrays for every row: the device sends the selected ones alone)
        my, op = np.zeros(cap, np.uint64), np.zeros(cap, np.uint64)
        self._check(self._lib.syn_replay_select_positions(self._h, *args, _p(my), _p(op), cap, C.byref(n), C.byref(skipped)))
        return dict(my=my[: int(n.value)].copy(), op=op[: int(n.value)].copy(), skipped=int(skipped.value))

    def replay_deduplicate_to_trainer(self, symmetry="none"):
        """De-duplicates the buffer on the device and makes the unique set the learner's data set (what replay_deduplicate +
        train_set_data leave, without the host copies). Returns the number of unique states; with symmetry="mirror"
        (syn_replay_deduplicate_to_trainer_symmetric) the pair (canonical states U, rows in the data set U + M)."""
        n = C.c_size_t()
        if _is_mirror(symmetry):
            u = C.c_size_t()
            self._check(self._lib.syn_replay_deduplicate_to_trainer_symmetric(self._h, C.byref(u), C.byref(n)))
            return int(u.value), int(n.value)
        self._check(self._lib.syn_replay_deduplicate_to_trainer(self._h, C.byref(n)))
        return int(n.value)

    def train_get_data(self):
        """The learner's current data set as host arrays: dict(my_bb, op_bb, pis [n, 9], vs [n, 3]) — replay_deduplicate's keys."""
        n = C.c_size_t()
        self._check(self._lib.syn_train_get_data(self._h, None, None, None, None, 1 << 62, C.byref(n)))
        n = int(n.value)
        o = dict(my_bb=np.zeros(n, np.uint64), op_bb=np.zeros(n, np.uint64), pis=np.zeros((n, 9), np.float32), vs=np.zeros((n, 3), np.float32))
        self._check(self._lib.syn_train_get_data(self._h, _p(o["my_bb"]), _p(o["op_bb"]), _p(o["pis"]), _p(o["vs"]), n, None))
        return o

    # ---- held-out evaluation (include/synthesis_amd.h "Held-out evaluation")
    def dataset_set(self, my_bb, op_bb, target_pi, target_v):
        """Uploads the evaluation set: a second data set beside the learner's that no trainer call touches; needs no trainer."""
        my = np.ascontiguousarray(my_bb, dtype=np.uint64).ravel()
        op = np.ascontiguousarray(op_bb, dtype=np.uint64).ravel()
        if op.size != my.size:
            raise ValueError("my_bb and op_bb must have the same length")
        tpi = np.ascontiguousarray(target_pi, dtype=np.float32).reshape(my.size, 9)
        tv = np.ascontiguousarray(target_v, dtype=np.float32).reshape(my.size, 3)
        self._check(self._lib.syn_dataset_set(self._h, _p(my), _p(op), _p(tpi), _p(tv), int(my.size)))

    def dataset_get(self):
        """The evaluation set as host arrays: dict(my_bb, op_bb, pis [n, 9], vs [n, 3]) — train_get_data's keys."""
        n = C.c_size_t()
        self._check(self._lib.syn_dataset_get(self._h, None, None, None, None, 1 << 62, C.byref(n)))
        n = int(n.value)
        o = dict(my_bb=np.zeros(n, np.uint64), op_bb=np.zeros(n, np.uint64), pis=np.zeros((n, 9), np.float32), vs=np.zeros((n, 3), np.float32))
        self._check(self._lib.syn_dataset_get(self._h, _p(o["my_bb"]), _p(o["op_bb"]), _p(o["pis"]), _p(o["vs"]), n, None))
        return o

    def replay_set_holdout(self, key, threshold):
        """syn_replay_set_holdout: with threshold > 0 (of 2^32), replay_deduplicate_to_trainer hands the games whose hash under `key` falls
        below it to the evaluation set instead of the learner (include/synthesis_amd.h "Holding games out"); 0 switches it off."""
        self._check(self._lib.syn_replay_set_holdout(self._h, int(key) & 0xFFFFFFFFFFFFFFFF, int(threshold)))

    def dataset_counts(self):
        """(rows of the evaluation set, how many of them — the leading ones — are states the learner's data set does not contain)"""
        n, u = C.c_size_t(), C.c_size_t()
        self._check(self._lib.syn_dataset_counts(self._h, C.byref(n), C.byref(u)))
        return int(n.value), int(u.value)

    def dataset_evaluate(self, which="eval", first_row=0, n_rows=None, blob=None, max_workgroups=0, blocks=False, rows=False, arith="f32"):
        """syn_dataset_evaluate_arith: the f32 learner's losses of `blob` (None: the trainer's current weights) on the rows
        [first_row, first_row + n_rows) of the learner's data set (which="train") or the evaluation set ("eval"); n_rows=None = to the
        end of the set. arith = the arithmetic that computes a row's twelve raw outputs: "f32" (the learner's), "f16x2" (the engine's
        f16x2 inference, an image built per call; both networks) or "bf16" (the conv learner's bf16 forward; Connect4ConvNet only); an
        int is passed through as it is. Forward only: nothing of the trainer or the engine changes. Returns dict(mean_pi, mean_v,
        sum_pi, sum_v (f64), rows, blocks, pi_hits, v_hits, pi_acc, v_acc, grid, arith); blocks=True adds block_losses [n_blocks, 2],
        rows=True row_logits [n_rows, 12] and row_kl [n_rows, 2]."""
        if which not in DATASETS:
            raise ValueError(f"which must be 'train' or 'eval', got {which!r}")
        if not isinstance(arith, (int, np.integer)) and arith not in EVAL_ARITHMETICS:
            raise ValueError(f"arith must be one of {sorted(EVAL_ARITHMETICS)}, got {arith!r}")
        arith_code = int(arith) if isinstance(arith, (int, np.integer)) else EVAL_ARITHMETICS[arith]
        if n_rows is None:
            size = C.c_size_t(0)
            if which == "train":
                if self._lib.syn_train_get_data(self._h, None, None, None, None, 1 << 62, C.byref(size)) != 0:
                    size = C.c_size_t(0)   # (no trainer: no data set, which the call below reports)
            else:
                self._check(self._lib.syn_dataset_get(self._h, None, None, None, None, 1 << 62, C.byref(size)))
            n_rows = max(int(size.value) - int(first_row), 0)
        n_rows = int(n_rows)
        nb = (n_rows + 31) // 32
        if blob is not None:
            blob = np.ascontiguousarray(blob, dtype=np.float32).ravel()
        bl = np.zeros((nb, 2), np.float32) if blocks else None
        lg = np.zeros((n_rows, 12), np.float32) if rows else None
        kl = np.zeros((n_rows, 2), np.float32) if rows else None
        m = CDatasetMetrics()
        self._check(self._lib.syn_dataset_evaluate_arith(self._h, DATASETS[which], int(first_row), n_rows, _p(blob),
                                                         0 if blob is None else int(blob.size), arith_code, int(max_workgroups), C.byref(m),
                                                         _p(bl), _p(lg), _p(kl)))
        out = dict(arith=arith, mean_pi=float(m.mean_pi), mean_v=float(m.mean_v), sum_pi=float(m.sum_pi), sum_v=float(m.sum_v), rows=int(m.rows),
                   blocks=int(m.blocks), pi_hits=int(m.pi_hits), v_hits=int(m.v_hits), grid=int(m.grid),
                   pi_acc=m.pi_hits / m.rows if m.rows else 0.0, v_acc=m.v_hits / m.rows if m.rows else 0.0)
        if blocks:
            out["block_losses"] = bl
        if rows:
            out["row_logits"] = lg
            out["row_kl"] = kl
        return out

    # ---- parity probes
    def debug_stdrng_u32(self, seed, n):
        out = np.zeros(int(n), np.uint32)
        self._check(self._lib.syn_debug_stdrng_u32(self._h, int(seed), int(n), _p(out)))
        return out

    def debug_tournament_regroup(self, keys, n_keys):
        """syn_debug_tournament_regroup: (perm [n] = ids 0..n-1 grouped by ascending key, input order kept inside a group, -1 past the
        survivors; seg [n_keys + 1] = where each group starts, seg[n_keys] = the survivors). keys[i] == n_keys drops job i."""
        k = np.ascontiguousarray(keys, np.int32).ravel()
        perm = np.full(k.size, -1, np.int32)
        seg = np.zeros(int(n_keys) + 1, np.int32)
        self._check(self._lib.syn_debug_tournament_regroup(self._h, _p(k), int(k.size), int(n_keys), _p(perm), _p(seg)))
        return perm, seg

    def debug_fast_div(self, a, b):
        a = np.ascontiguousarray(a, np.float32).ravel()
        b = np.ascontiguousarray(b, np.float32).ravel()
        f = np.zeros_like(a); d = np.zeros_like(a)
        self._check(self._lib.syn_debug_fast_div(self._h, _p(a), _p(b), int(a.size), _p(f), _p(d)))
        return f, d

    def debug_small_int_math(self, b_lo, b_hi):
        """(mismatches of div2_by_small_int, of div2_safe_range, of sqrt_normal_range) over every significand: see synthesis_amd.h"""
        out = np.zeros(3, np.uint64)
        self._check(self._lib.syn_debug_small_int_math(self._h, int(b_lo), int(b_hi), _p(out)))
        return tuple(int(x) for x in out)

    def debug_math(self, a, b):
        a = np.ascontiguousarray(a, np.float32).ravel()
        b = np.ascontiguousarray(b, np.float32).ravel()
        e = np.zeros_like(a); d = np.zeros_like(a); s = np.zeros_like(a)
        self._check(self._lib.syn_debug_math(self._h, _p(a), _p(b), int(a.size), _p(e), _p(d), _p(s)))
        return e, d, s
