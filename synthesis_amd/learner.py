"""The learner side of the reference's loop on N GPUs (BASELINE configs[4]):

    alpha_zero()            synthesis/src/alpha_zero.rs:16-118   iterate { gather_experience -> dedup -> Adam epochs -> save model }
    gather_experience()     alpha_zero.rs:120-179                worker threads play games_per_train games, buffers concatenated
    train step              alpha_zero.rs:72-94                  forward, kl_div losses, Adam

`LearningLoop` is that loop in the shape that scales on one node: EVERY rank plays its share of an iteration's games (sharded by
game index, no collective on the data path — games share nothing), rank 0 gathers the new positions, owns the replay buffer and
trains with the persistent epoch kernel (`syn_train_epoch`: 13 us per optimiser step at the reference's batch of 32 — a
data-parallel step at that batch size moves 122 KB over xGMI for 13 us of compute and can only be slower than one GPU), and the
new parameters (122 KB for Connect4Net, 50 KB for Connect4ConvNet) are broadcast once per iteration. One process per GPU;
torch.distributed is the transport (backend "nccl" is RCCL over xGMI; "gloo" in the CPU tests and when ranks share a GPU).
With one rank it is exactly the single-GPU loop. The games an iteration plays, the replay buffer and therefore the trained
weights do not depend on the number of ranks.

`DataParallelLearner` is the other reading of configs[4] — a gradient all-reduce per optimiser step — kept for callers who want
it. A large batch on ONE GPU no longer needs it: batch_mode="micro" (Engine.trainer_set_batch_mode; include/synthesis_amd.h
SYN_TRAIN_BATCH_MICRO) spreads a batch of 32 nb positions over up to nb workgroups as nb micro-batches of 32 and averages their
gradients in a fixed order, where the default chained definition walks any batch on one workgroup (and a rank's large shard here
does too, unless it is given the same batch_mode). Every rank computes the gradients of ITS shard of the batch (`syn_train_gradients_device`), the gradient
buffer and the two loss sums travel in ONE all-reduce, every rank applies the same Adam update with grad_scale = 1 / world
(`syn_train_apply_device`), so weights stay identical without a broadcast. Both networks. The data set and the epoch's
permutation live on the device; a step gathers its shard there and the losses stay on the device until asked for.

torch is plumbing in both: it owns the buffers torch.distributed moves. Nothing here touches oracle/.
"""
import time

import numpy as np

from .engine import CONV_NUM_PARAMS, NUM_PARAMS, shard_games


def _lr_at(schedule, i_iter):
    """alpha_zero.rs:62-69: the last (iteration, lr) entry whose iteration is <= i_iter + 1"""
    lr = schedule[0][1]
    for it, v in schedule:
        if it <= i_iter + 1:
            lr = v
    return lr


def _sampler_key(seed, i_iter):
    """sampler="device": the key of iteration i_iter's epochs (0-based, like _lr_at's) — (seed mod 2^32) * 2^32 + (i_iter mod 2^32), a
    64-bit number; epoch e of the iteration is the sampler's epoch e (include/synthesis_amd.h "Device-side epoch sampler")"""
    return ((int(seed) & 0xFFFFFFFF) << 32) | (int(i_iter) & 0xFFFFFFFF)


_M64 = (1 << 64) - 1
HOLDOUT_TAG = 0x401D0075E7C0FFEE   # include/synthesis_amd.h "Holding games out"


def _holdout_key(seed):
    """holdout > 0: the key of the run's split of games — (seed mod 2^32) * 2^32, the high half of every _sampler_key of the run (the
    two hashes carry different tags)"""
    return (int(seed) & 0xFFFFFFFF) << 32


def _sm(seed, idx):
    """csrc/noise.cuh noise_splitmix64 on numpy uint64 arrays (include/synthesis_amd.h "Device-side epoch sampler"): idx + 1 in 32 bits"""
    with np.errstate(over="ignore"):
        z = np.asarray(seed, np.uint64) + ((np.asarray(idx, np.uint64) + np.uint64(1)) & np.uint64(0xFFFFFFFF)) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def holdout_flags(key, threshold, gid):
    """Which game ids are held out under (key, threshold): the header's definition on the host (replay="host"; the device applies it in
    replay_holdout_flags_kernel)."""
    g = np.asarray(gid, np.int64).astype(np.uint64)
    h = _sm(_sm(np.uint64((int(key) & _M64) ^ HOLDOUT_TAG), g >> np.uint64(32)), g & np.uint64(0xFFFFFFFF)) >> np.uint64(32)
    return h < np.uint64(int(threshold))


REANALYSE_TAG = 0x2EA7A1F5E5EA2C40   # include/synthesis_amd.h "Reanalyse"


def _reanalyse_key(seed, i_iter):
    """reanalyse > 0: the selection key of iteration i_iter's reanalysis (0-based) — _sampler_key's number; the hashes carry different
    tags, so the two uses of it are independent"""
    return _sampler_key(seed, i_iter)


EXPLORING_TAG = 0xE8F10A1D57A27500   # exploring starts: what separates their selection key from the same iteration's reanalysis key


def _exploring_key(seed, i_iter):
    """exploring_starts > 0: the selection key of iteration i_iter's start positions (0-based) — _sampler_key's number under a tag of its
    own, so that a run with reanalysis and exploring starts draws the two sets of rows independently"""
    return _sampler_key(seed, i_iter) ^ EXPLORING_TAG


def exploring_threshold(n_games, rows_in_buffer):
    """The selection threshold that draws about n_games of rows_in_buffer rows: min(2^32 - 1, (n_games * 2^32) // rows_in_buffer), in
    integers (0 for an empty buffer: nothing to start from)"""
    n_games, rows_in_buffer = int(n_games), int(rows_in_buffer)
    if n_games < 0 or rows_in_buffer < 0:
        raise ValueError("exploring_threshold: need n_games >= 0 and rows_in_buffer >= 0")
    if rows_in_buffer == 0:
        return 0
    return min((1 << 32) - 1, (n_games << 32) // rows_in_buffer)


def searchable_positions(my, op):
    """The positions a search takes as a root: Engine.mcts_search's check (disjoint boards inside the 63 cells — bit index row + 7 * col —
    every column filled from the bottom without holes, at least one free column) and neither side with four in a row (connect4.rs:70-83:
    the four anchored line directions at bit distances 1, 7, 6 and 8)."""
    my = np.asarray(my, np.uint64)
    op = np.asarray(op, np.uint64)
    u = np.uint64
    occ = my | op
    ok = ((my & op) == u(0)) & ((occ >> u(63)) == u(0))
    any_free = np.zeros(occ.shape, bool)
    for c in range(9):
        col = (occ >> u(7 * c)) & u(0x7F)
        ok &= (col & (col + u(1))) == u(0)
        any_free |= col != u(0x7F)
    rows = lambda lo, hi: sum(1 << (r + 7 * c) for r in range(lo, hi + 1) for c in range(9))
    cols0to5 = sum(1 << (r + 7 * c) for r in range(7) for c in range(6))

    def won(bb):
        out = np.zeros(bb.shape, bool)
        for shift, mask in ((6, cols0to5 & rows(3, 6)), (8, cols0to5 & rows(0, 3)), (7, cols0to5), (1, rows(0, 3))):
            out |= (bb & (bb >> u(shift)) & (bb >> u(2 * shift)) & (bb >> u(3 * shift)) & u(mask)) != u(0)
        return out

    return ok & any_free & ~won(my) & ~won(op)


def reanalyse_flags(key, threshold, before_gid, gid, my, op):
    """Which rows (gid, my, op) a reanalysis under (key, threshold, before_gid) selects: the header's definition on the host
    (replay="host"; the device applies it in reanalyse_flags_kernel), the searchable test included."""
    g = np.asarray(gid, np.int64)
    h = np.uint64((int(key) & _M64) ^ REANALYSE_TAG)
    for word in (g.astype(np.uint64), np.asarray(my, np.uint64), np.asarray(op, np.uint64)):
        h = _sm(_sm(h, word >> np.uint64(32)), word & np.uint64(0xFFFFFFFF))
    drawn = (g < (int(before_gid) if before_gid is not None else (1 << 63) - 1)) & ((h >> np.uint64(32)) < np.uint64(int(threshold)))
    return drawn & searchable_positions(my, op)


_METRIC_KEYS = ("rows", "mean_pi", "mean_v", "pi_acc", "v_acc")
HOLDOUT_ARITHMETICS = ("f32", "f16x2", "bf16")   # LearningLoop(holdout_arith=...): Engine.dataset_evaluate's `arith` names
_SYN_ERR_UNSUPPORTED = -5


# ---- the state file of a LearningLoop (LearningLoop.save_state / restore_state): ONE .npz written by numpy alone, no pickling. Needs no GPU.
STATE_FORMAT_VERSION = 1
# what identifies a run: a loop continues a state file only when all of these agree (`replay` is deliberately not among them: the
# buffer is stored as arrays, so a run saved with replay="host" may continue with replay="device" and the reverse)
FINGERPRINT_FIELDS = ("net", "seed", "precision", "batch_mode", "sampler", "flip", "symmetry", "holdout", "reanalyse",
                      "reanalyse_explores", "reanalyse_value_mix", "lr_schedule", "hyper", "network_arithmetic", "world")
# optional fields: name -> the value a fingerprint without the field has. A field is written only when it differs from that value, so
# the files of runs that do not use it are the files they always were
FINGERPRINT_OPTIONAL = dict(exploring_starts=0.0)
_HYPER_DEFAULTS = dict(weight_decay=1e-6, policy_weight=1.0, value_weight=1.0, beta1=0.9, beta2=0.999, eps=1e-8)   # Engine.trainer_init*
# every array of the file: name -> (dtype, trailing shape); `torch_generator` is present only with sampler="torch"
_STATE_ARRAYS = dict(format_version=(np.int64, ()), fingerprint=(np.uint8, (-1,)), iterations_done=(np.int64, ()), games_played=(np.int64, ()),
                     weights=(np.float32, (-1,)), m=(np.float32, (-1,)), v=(np.float32, (-1,)), step=(np.int64, ()),
                     replay_my=(np.uint64, (-1,)), replay_op=(np.uint64, (-1,)), replay_gid=(np.int64, (-1,)),
                     replay_pi=(np.float32, (-1, 9)), replay_v=(np.float32, (-1, 3)),
                     digest_trainer=(np.uint64, ()), digest_replay=(np.uint64, ()))
_STATE_OPTIONAL = dict(torch_generator=(np.uint8, (-1,)))
_REPLAY_KEYS = ("my", "op", "gid", "pi", "v")


def _normal_fingerprint(fp):
    """`fp` as it comes back from the file: through JSON (tuples become lists, numpy scalars plain numbers), every field present"""
    import json

    missing = [k for k in FINGERPRINT_FIELDS if k not in fp]
    if missing:
        raise ValueError(f"a run's fingerprint needs the fields {list(FINGERPRINT_FIELDS)}; missing: {missing}")
    plain = lambda x: x.item() if isinstance(x, np.generic) else x
    out = {k: fp[k] for k in FINGERPRINT_FIELDS}
    out.update({k: fp[k] for k, default in FINGERPRINT_OPTIONAL.items() if k in fp and fp[k] != default})
    return json.loads(json.dumps(out, default=plain, sort_keys=True))


def pack_state(state):
    """A loop's state as the dict of arrays np.savez writes. `state` has `fingerprint` (a dict with FINGERPRINT_FIELDS),
    `iterations_done`, `games_played`, `weights`, `m`, `v`, `step`, `replay` (dict my, op, gid, pi, v), `digest_trainer`,
    `digest_replay` (ints below 2^64) and optionally `torch_generator` (the generator's state bytes)."""
    import json

    fp = json.dumps(_normal_fingerprint(state["fingerprint"]), sort_keys=True).encode("utf-8")
    R = state["replay"]
    out = dict(format_version=np.int64(STATE_FORMAT_VERSION), fingerprint=np.frombuffer(fp, np.uint8).copy(),
               iterations_done=np.int64(state["iterations_done"]), games_played=np.int64(state["games_played"]),
               weights=state["weights"], m=state["m"], v=state["v"], step=np.int64(state["step"]),
               replay_my=R["my"], replay_op=R["op"], replay_gid=R["gid"], replay_pi=R["pi"], replay_v=R["v"],
               digest_trainer=np.uint64(int(state["digest_trainer"])), digest_replay=np.uint64(int(state["digest_replay"])))
    if state.get("torch_generator") is not None:
        out["torch_generator"] = state["torch_generator"]
    spec = dict(_STATE_ARRAYS, **_STATE_OPTIONAL)
    out = {k: np.ascontiguousarray(a, dtype=spec[k][0]).reshape(spec[k][1]) for k, a in out.items()}
    sizes = {k: out[k].shape[0] for k in ("weights", "m", "v")}
    if len(set(sizes.values())) != 1:
        raise ValueError(f"weights, m and v must have the same size, got {sizes}")
    rows = {k: out["replay_" + k].shape[0] for k in _REPLAY_KEYS}
    if len(set(rows.values())) != 1:
        raise ValueError(f"the buffer's five arrays must have the same number of rows, got {rows}")
    return out


def unpack_state(arrays, where="state file"):
    """The inverse of pack_state on what np.load returned (any mapping of arrays). Raises ValueError, naming `where`, on a foreign
    format version, a missing array, or an array of the wrong type or shape."""
    import json

    if "format_version" not in arrays:
        raise ValueError(f"{where}: not a LearningLoop state file (no format_version)")
    version = int(np.asarray(arrays["format_version"]).reshape(-1)[0])
    if version != STATE_FORMAT_VERSION:
        raise ValueError(f"{where}: state file format version {version}; this library reads version {STATE_FORMAT_VERSION}")
    got = {}
    for k, (dt, shape) in list(_STATE_ARRAYS.items()) + list(_STATE_OPTIONAL.items()):
        if k not in arrays:
            if k in _STATE_OPTIONAL:
                continue
            raise ValueError(f"{where}: the array {k!r} is missing")
        a = np.asarray(arrays[k])
        if a.dtype != np.dtype(dt) or a.ndim != len(shape) or any(s >= 0 and s != d for s, d in zip(shape, a.shape)):
            raise ValueError(f"{where}: the array {k!r} is {a.dtype}{list(a.shape)}, expected {np.dtype(dt)}{list(shape)}")
        got[k] = a
    if len({got[k].shape[0] for k in ("weights", "m", "v")}) != 1 or len({got["replay_" + k].shape[0] for k in _REPLAY_KEYS}) != 1:
        raise ValueError(f"{where}: the trainer's or the buffer's arrays differ in length")
    try:
        fingerprint = _normal_fingerprint(json.loads(got["fingerprint"].tobytes().decode("utf-8")))
    except (UnicodeDecodeError, json.JSONDecodeError, TypeError) as e:
        raise ValueError(f"{where}: the run's fingerprint cannot be read ({e})") from None
    return dict(fingerprint=fingerprint, iterations_done=int(got["iterations_done"]), games_played=int(got["games_played"]),
                weights=got["weights"], m=got["m"], v=got["v"], step=int(got["step"]),
                replay={k: got["replay_" + k] for k in _REPLAY_KEYS},
                torch_generator=got.get("torch_generator"), digest_trainer=int(got["digest_trainer"]), digest_replay=int(got["digest_replay"]))


def write_state_file(path, state):
    """pack_state(state) into `path`: written under a temporary name in the same directory, then os.replace — a reader sees the old
    file or the new one, and a failure leaves no partial file behind."""
    import os
    import tempfile

    arrays = pack_state(state)
    directory = os.path.dirname(os.path.abspath(path))
    fd, tmp = tempfile.mkstemp(prefix=os.path.basename(path) + ".", suffix=".tmp", dir=directory)
    try:
        with os.fdopen(fd, "wb") as f:
            np.savez(f, **arrays)
            f.flush()
            os.fsync(f.fileno())
        os.replace(tmp, path)
    except BaseException:
        if os.path.exists(tmp):
            os.remove(tmp)
        raise


def read_state_file(path):
    """unpack_state of the file at `path`. A file that is truncated or not an .npz raises ValueError; nothing is written."""
    import zipfile

    try:
        with np.load(path, allow_pickle=False) as z:
            arrays = {k: z[k] for k in z.files}
    except (zipfile.BadZipFile, EOFError, OSError, ValueError, KeyError) as e:
        if isinstance(e, FileNotFoundError):
            raise
        raise ValueError(f"{path}: not a complete LearningLoop state file ({type(e).__name__}: {e})") from None
    return unpack_state(arrays, where=str(path))


def check_fingerprint(saved, current, where="state file"):
    """Raises ValueError naming the first field of FINGERPRINT_FIELDS, then of FINGERPRINT_OPTIONAL (a missing one reads as its default),
    in which the run that wrote the file and this loop differ."""
    saved, current = _normal_fingerprint(saved), _normal_fingerprint(current)
    for k in FINGERPRINT_FIELDS:
        if saved[k] != current[k]:
            raise ValueError(f"{where}: written by a run with {k}={saved[k]!r}, this loop has {k}={current[k]!r}")
    for k, default in FINGERPRINT_OPTIONAL.items():
        if saved.get(k, default) != current.get(k, default):
            raise ValueError(f"{where}: written by a run with {k}={saved.get(k, default)!r}, this loop has {k}={current.get(k, default)!r}")


class LearningLoop:
    """alpha_zero.rs:16-118 with self-play on every rank and the learner on rank 0 (see the module docstring).

    engine       this rank's sa.Engine (self-play; on rank 0 also the learner and the de-duplication)
    net          "mlp" (Connect4Net, study-connect4/src/policies.rs:14-59) | "conv" (Connect4ConvNet)
    blob         initial parameters — identical on every rank (P::new(&vs), alpha_zero.rs:31)
    precision    "f32" | "bf16" (Connect4ConvNet's learner only: syn_trainer_set_precision)
    batch_mode   "chained" (default: the oracle's step, one chain over the minibatch) | "micro" (SYN_TRAIN_BATCH_MICRO: iteration()'s
                 batch_size must then be a multiple of 32; it is nb micro-batches of 32 on up to nb workgroups, gradients averaged in
                 ascending order — another definition of the step, deterministic, not the chained bits above 32). No learning rate is
                 rescaled for the larger batch; what large batches do to the trained player is not measured.
    dist         torch.distributed (initialised) or None for one rank
    sampler      "numpy" (default: numpy's PCG64 permutation seeded by (seed, iteration, epoch)) | "torch": BatchRandSampler's own
                 `Tensor::randperm(n, INT64_CPU)` (data.rs:29) — libtorch's CPU randperm from ONE generator seeded with `seed` and
                 advanced epoch after epoch: the reference's algorithm and generator TYPE, not its stream — in a reference run
                 `tch::manual_seed(seed)` (alpha_zero.rs:28) is followed by `P::new(&vs)` (:31), whose parameter initialisation draws
                 from that same global generator before the first randperm, so the permutations of a Rust run differ
                 | "device": the device-side epoch sampler — an iteration's epochs are ONE Engine.train_epochs_sampled call keyed by
                 `_sampler_key(seed, iteration)`, the host draws no permutation and uploads no indices; a third definition of the
                 order (include/synthesis_amd.h "Device-side epoch sampler"), same records in both replay modes
    flip         sampler="device" only (else ValueError): every epoch mirrors a random half of the rows while it gathers them (the
                 sampler's flip flags) — both orientations at the plain data set's epoch cost, where symmetry="mirror" doubles the
                 data set. Whether it trains a stronger player is not measured (tools/arena.py).
    network_arithmetic  "f32" (default) | "f16x2": the arithmetic this rank's engine evaluates the network in during self-play
                 (include/synthesis_amd.h syn_set_network_arithmetic; both networks). The learner itself trains in `precision`.
    replay       "host" (default: the replay buffer is a dict of numpy arrays on the learner's rank; self-play downloads its padded
                 outputs) | "device": the buffer lives in the engine's device memory (Engine.replay_*; data.rs:107-235 on the GPU) —
                 self-play downloads only `plies`, the positions are compacted on the device, trimmed to the last games_to_keep games
                 and de-duplicated straight into the learner's data set. Same games, same buffer order, same bits as "host".
    symmetry     "none" (default) | "mirror": the de-duplication treats a position and its left-right mirror image as one class and
                 hands the learner a data set closed under mirroring (Engine.replay_deduplicate(symmetry="mirror") /
                 replay_deduplicate_to_trainer(symmetry="mirror"); DESIGN.md "Mirror-symmetric de-duplication"): `unique` counts the
                 canonical states and their mirror images, the record gains `unique_canonical`, latest_*.npy hold the augmented set.
                 Self-play, the buffer and the network are untouched. Both replay modes, same bits.
    holdout      0.0 (default: nothing is held out, every bit and every record as without the argument) | a fraction of GAMES in (0, 1):
                 the games whose hash under `_holdout_key(seed)` falls below floor(holdout * 2^32) (include/synthesis_amd.h "Holding games
                 out") never reach the learner; their de-duplicated positions are the engine's evaluation set, unseen states first. The
                 record gains `holdout_rows`, `holdout_unseen` and `holdout_before` / `holdout_after`: the f32 learner's losses and
                 arg-max accuracies (Engine.dataset_evaluate) of the weights before and after the iteration's epochs, each as
                 dict(all=..., unseen=...) over all held-out rows and over those whose state the learner's data set does not contain.
                 Both replay modes, same bits. An iteration whose buffer has no game left for the learner raises.
    holdout_arith  ("f32",) (default: no record and no bit changes) | the arithmetics the held-out metrics are taken in, names of
                 Engine.dataset_evaluate's `arith`: "f32" stands for the keys above; "f16x2" and "bf16" (Connect4ConvNet) each add
                 `holdout_before_<name>` / `holdout_after_<name>` of the same shape, the same weights and rows evaluated in that arithmetic
                 (include/synthesis_amd.h syn_dataset_evaluate_arith). Weights without an f16x2 plan give None for that entry and the run
                 goes on. An observer like `replay`: it trains nothing and is not part of the run's fingerprint. Both replay modes report
                 identical values. Not measured: what the extra evaluations cost an iteration.
    reanalyse    0.0 (default: every bit and every record as without the argument) | a fraction of ROWS in (0, 1]: after the keep-window
                 and before the de-duplication of every iteration the learner's rank searches that fraction of the stored positions of
                 OLDER games (gid below this iteration's first game; the hash of `_reanalyse_key(seed, iteration)`, the game id and the
                 position selects them: include/synthesis_amd.h "Reanalyse") again with the engine's current network, the iteration's
                 cfg.mcts_cfg and `reanalyse_explores or cfg.num_explores` explores, and overwrites their pi with the new target_pi and
                 their v with v * (1 - reanalyse_value_mix) + target_q * reanalyse_value_mix (0.0: v stays). replay="device":
                 Engine.replay_reanalyse, nothing leaves the device; replay="host": reanalyse_flags + one Engine.mcts_search over the
                 selected rows + assignment into the host buffer — same bits. The record gains `reanalysed`, `reanalyse_moved` (rows whose
                 arg-max column of pi changed) and a `reanalyse` phase time. Not measured: any training run with reanalysis, and more than
                 one rank (the other ranks idle during the learner's reanalysis).
    exploring_starts  0.0 (default: every bit and every record as without the argument) | a fraction F of an iteration's GAMES in (0, 1):
                 from the second iteration on, n_t = floor(F * games_per_train) of the games are replaced by games that start at stored
                 positions. The ranks share games_per_train - n_t ordinary self-play games; then the learner's rank takes ALL rows of
                 the buffer as it stood before the iteration that "Reanalyse"'s selection draws under `_exploring_key(seed, iteration)`,
                 threshold `exploring_threshold(n_t, rows in the buffer)` (about n_t rows, not exactly) and before_gid = the iteration's
                 first game id, in buffer order, and plays one recorded game from each (Engine.games_run_recorded: one player, the current
                 weights, the iteration's cfg unchanged, so a game's first move from a stored position is the configuration's random
                 move; game j on the generator of seed + its game id). Their rows are appended after the ordinary games' with the game
                 ids that follow them (the iteration's id games_per_train - n_t onwards; when more than n_t rows are drawn, the surplus
                 games carry ids of the next iteration's range — ids only order the keep-window and the holdout split). replay="host"
                 selects with reanalyse_flags and takes the padded rows; replay="device" uses Engine.replay_select_positions and
                 replay_append_selfplay — same buffer, weights and records. The record gains `exploring_games`, `exploring_rows` and an
                 `exploring` phase time. The run's fingerprint carries the field only when it is non-zero (a file without it reads as
                 0.0). cfg must be a deterministic search configuration. Not measured: whether exploring starts train a stronger player;
                 more than one rank (the other ranks idle while the learner's rank plays the exploring games).
    digests      False (default: every record as without the argument) | True: the learner's record gains `digests` = dict(trainer,
                 replay, train_data, and with a holdout eval_data) — the 64-bit fingerprints of that state (Engine.state_digest;
                 include/synthesis_amd.h "State digests") as 16-digit hex strings, taken after the iteration's epochs and before the
                 publish. They are computed where the state lives; replay="host" digests its numpy buffer with synthesis_amd.digest, the
                 same definition, so both replay modes report the same words. Two runs whose logs show the same words hold the same
                 bits — one rank against two, host replay against device replay, a resumed run against one that never stopped.
    save_state(path) / restore_state(path): the run can stop and continue. save_state writes ONE .npz (numpy alone, a temporary name then
                 os.replace; only the learner's rank writes): a format version, the run's fingerprint (FINGERPRINT_FIELDS: net, seed,
                 precision, batch_mode, sampler, flip, symmetry, holdout, reanalyse and its two parameters, lr_schedule, the hyper values,
                 network_arithmetic, world size), iterations_done and games_played, the trainer's weights, m, v and step, the buffer's five
                 arrays, the torch generator's state (sampler="torch") and the TRAINER and REPLAY digests. restore_state, on a freshly
                 constructed loop with the same arguments (`replay` may differ), refuses a file of another run by naming the field, puts
                 the trainer (Engine.trainer_set_state), the buffer, the network and the counters back, and proves it by recomputing both
                 digests; the iterations that follow are bit for bit those of a run that never stopped. Not saved: the policy cache
                 (results never depend on it), the last gradient (every step overwrites it) and the two data sets (every iteration
                 rebuilds them from the buffer). Not measured: any training run continued across sessions.
    logs_dir     None, or where the learner's rank writes what the reference writes per iteration (alpha_zero.rs:37,97-100):
                 models/model_{i}.ot (Connect4Net: a VarStore archive `vs.load` reads; Connect4ConvNet: the flat blob as .npy) and
                 latest_states.npy [n, 1, 7, 9] / latest_pis.npy [n, 9] / latest_vs.npy [n, 3] of the de-duplicated buffer
    """

    def __init__(self, engine, net, blob, dist=None, device=0, lr_schedule=((1, 1e-3),), seed=0, precision="f32", logs_dir=None, sampler="numpy",
                 network_arithmetic="f32", replay="host", symmetry="none", batch_mode="chained", flip=False, holdout=0.0,
                 reanalyse=0.0, reanalyse_explores=None, reanalyse_value_mix=0.0, digests=False, holdout_arith=("f32",), exploring_starts=0.0,
                 **hyper):
        holdout_arith = (holdout_arith,) if isinstance(holdout_arith, str) else tuple(holdout_arith)
        for a in holdout_arith:
            if a not in HOLDOUT_ARITHMETICS:
                raise ValueError(f"holdout_arith names must be among {list(HOLDOUT_ARITHMETICS)}, got {a!r}")
            if a == "bf16" and net != "conv":
                raise ValueError("holdout_arith 'bf16' exists for net='conv' only (the conv learner's bf16 precision)")
        _real = lambda x: not isinstance(x, bool) and isinstance(x, (int, float, np.floating, np.integer))
        if not _real(exploring_starts) or not 0.0 <= float(exploring_starts) < 1.0:
            raise ValueError(f"exploring_starts must be a fraction of an iteration's games in [0, 1), got {exploring_starts!r}")
        if not _real(reanalyse) or not 0.0 <= float(reanalyse) <= 1.0:
            raise ValueError(f"reanalyse must be a fraction of rows in [0, 1], got {reanalyse!r}")
        if reanalyse_explores is not None and (isinstance(reanalyse_explores, bool) or not isinstance(reanalyse_explores, (int, np.integer))
                                               or int(reanalyse_explores) < 0):
            raise ValueError(f"reanalyse_explores must be None or an integer >= 0, got {reanalyse_explores!r}")
        if not _real(reanalyse_value_mix) or not 0.0 <= float(reanalyse_value_mix) <= 1.0:
            raise ValueError(f"reanalyse_value_mix must be in [0, 1], got {reanalyse_value_mix!r}")
        if isinstance(holdout, bool) or not isinstance(holdout, (int, float, np.floating, np.integer)) or not 0.0 <= float(holdout) < 1.0:
            raise ValueError(f"holdout must be a fraction of games in [0, 1), got {holdout!r}")
        if sampler not in ("numpy", "torch", "device"):
            raise ValueError(f"sampler must be 'numpy', 'torch' or 'device', got {sampler!r}")
        if flip and sampler != "device":
            raise ValueError(f"flip=True needs sampler='device' (the flip is part of the device sampler's gather), got sampler={sampler!r}")
        if replay not in ("host", "device"):
            raise ValueError(f"replay must be 'host' or 'device', got {replay!r}")
        if symmetry not in ("none", "mirror"):
            raise ValueError(f"symmetry must be 'none' or 'mirror', got {symmetry!r}")
        import torch

        self._torch = torch
        self.engine = engine
        self.net = net
        self.dist = dist if (dist is not None and dist.is_initialized() and dist.get_world_size() > 1) else None
        self.world = self.dist.get_world_size() if self.dist else 1
        self.rank = self.dist.get_rank() if self.dist else 0
        self.lr_schedule = list(lr_schedule)
        self.seed = int(seed)
        self.n_params = CONV_NUM_PARAMS if net == "conv" else NUM_PARAMS
        blob = np.ascontiguousarray(blob, dtype=np.float32).ravel()
        assert blob.size == self.n_params
        self._load = engine.load_weights_conv if net == "conv" else engine.load_weights
        self._load(blob)
        if network_arithmetic != "f32":   # (later loads and the learner's publish keep the engine's arithmetic)
            engine.set_network_arithmetic(network_arithmetic)
        self.weights = blob.copy()
        # the buffer the broadcast moves: on the GPU for RCCL, on the host for gloo
        on_gpu = self.dist is not None and self.dist.get_backend() == "nccl"
        self._wbuf = torch.zeros(self.n_params, dtype=torch.float32, device=torch.device(f"cuda:{device}") if on_gpu else "cpu")
        if self.rank == 0:
            (engine.trainer_init_conv if net == "conv" else engine.trainer_init)(blob, **hyper)
            if precision != "f32":
                engine.trainer_set_precision(precision)   # "bf16": the conv learner's bf16 matrix-core variant (BASELINE configs[4])
            if batch_mode != "chained":
                engine.trainer_set_batch_mode(batch_mode)
        # replay buffer (rank 0): positions as bitboards + targets + the game each step came from (data.rs:107-158)
        self.R = dict(my=np.zeros(0, np.uint64), op=np.zeros(0, np.uint64), pi=np.zeros((0, 9), np.float32),
                      v=np.zeros((0, 3), np.float32), gid=np.zeros(0, np.int64))
        self.games_played = 0
        self.iterations_done = 0
        self.batch_mode = batch_mode
        self.precision = precision
        self.network_arithmetic = network_arithmetic
        self.hyper = dict(_HYPER_DEFAULTS, **hyper)
        self.digests = bool(digests)
        self.replay = replay
        self.symmetry = symmetry
        self._device = int(device)
        self._replay_reserved = 0
        self.sampler = sampler
        self.flip = bool(flip)
        self._torch_gen = torch.Generator().manual_seed(self.seed) if sampler == "torch" else None
        self.holdout_arith = tuple(a for a in HOLDOUT_ARITHMETICS if a in holdout_arith and a != "f32")   # the extra ones, in a fixed order
        self.holdout = float(holdout)
        self._holdout_threshold = int(np.floor(self.holdout * 4294967296.0))
        if self._holdout_threshold and self.rank == 0 and replay == "device":
            engine.replay_set_holdout(_holdout_key(self.seed), self._holdout_threshold)
        self.reanalyse = float(reanalyse)
        self._reanalyse_threshold = int(np.floor(self.reanalyse * 4294967296.0))
        self.reanalyse_explores = None if reanalyse_explores is None else int(reanalyse_explores)
        self.reanalyse_value_mix = float(reanalyse_value_mix)
        self.exploring_starts = float(exploring_starts)
        self.logs_dir = logs_dir if self.rank == 0 else None
        if self.logs_dir:
            self._save_model(0)

    def _save_model(self, i):
        import os

        from .weights import save_ot

        d = os.path.join(self.logs_dir, "models")
        os.makedirs(d, exist_ok=True)
        if self.net == "mlp":
            save_ot(self.weights, os.path.join(d, f"model_{i}.ot"))
        else:
            np.save(os.path.join(d, f"model_{i}.npy"), self.weights)

    # ---- stopping and continuing a run (save_state / restore_state) and the per-iteration fingerprints (digests=True)
    def fingerprint(self):
        """What identifies this run (FINGERPRINT_FIELDS): restore_state continues a file only when every field agrees"""
        fp = dict(net=self.net, seed=self.seed, precision=self.precision, batch_mode=self.batch_mode, sampler=self.sampler, flip=self.flip,
                  symmetry=self.symmetry, holdout=self.holdout, reanalyse=self.reanalyse, reanalyse_explores=self.reanalyse_explores,
                  reanalyse_value_mix=self.reanalyse_value_mix, lr_schedule=[[int(i), float(v)] for i, v in self.lr_schedule],
                  hyper={k: float(v) for k, v in sorted(self.hyper.items())}, network_arithmetic=self.network_arithmetic, world=self.world)
        if self.exploring_starts != FINGERPRINT_OPTIONAL["exploring_starts"]:   # (an optional field: present only when it is used)
            fp["exploring_starts"] = self.exploring_starts
        return fp

    def _replay_arrays(self):
        """The learner's rank: the buffer's five arrays (my, op, gid, pi, v), from the engine (replay="device") or from self.R"""
        if self.replay == "device":
            return self.engine.replay_read()
        return {k: self.R[k] for k in _REPLAY_KEYS}

    def _replay_put(self, R):
        """The learner's rank: `R` becomes the buffer — Engine.replay_reserve + replay_append (replay="device") or self.R"""
        n = int(np.asarray(R["my"]).size)
        if self.replay == "device":
            self.engine.replay_clear()
            if n > self._replay_reserved:
                self.engine.replay_reserve(n)
                self._replay_reserved = n
            if n:
                self.engine.replay_append(R["my"], R["op"], R["gid"], R["pi"], R["v"])
        else:
            self.R = dict(my=np.array(R["my"], np.uint64).reshape(-1), op=np.array(R["op"], np.uint64).reshape(-1),
                          pi=np.array(R["pi"], np.float32).reshape(-1, 9), v=np.array(R["v"], np.float32).reshape(-1, 3),
                          gid=np.array(R["gid"], np.int64).reshape(-1))

    def _replay_digest(self):
        """SYN_DIGEST_REPLAY of the buffer where it lives: on the device (replay="device"), with synthesis_amd.digest over self.R otherwise"""
        if self.replay == "device":
            return self.engine.state_digest("replay")
        from .digest import replay_digest

        return replay_digest(*(self.R[k] for k in _REPLAY_KEYS))

    def state_digests(self):
        """The learner's rank: the fingerprints of the run's device-resident state as 16-digit hex strings — trainer (w, m, v, step),
        replay (the buffer; both replay modes report the same word), train_data, and eval_data with a holdout (include/synthesis_amd.h
        "State digests")."""
        from .digest import hex16

        out = dict(trainer=hex16(self.engine.state_digest("trainer")), replay=hex16(self._replay_digest()),
                   train_data=hex16(self.engine.state_digest("train_data")))
        if self._holdout_threshold:
            out["eval_data"] = hex16(self.engine.state_digest("eval_data"))
        return out

    def save_state(self, path):
        """Writes everything the loop carries from one iteration to the next into ONE .npz at `path` (write_state_file: a temporary
        name in the same directory, then os.replace): the run's fingerprint, iterations_done and games_played, the trainer's weights,
        moments and step, the buffer's five arrays, the torch generator's state (sampler="torch") and the TRAINER and REPLAY digests at
        save time. Only the learner's rank writes; the other ranks return at once. Not saved: the policy cache, the last gradient and
        the two data sets (every iteration rebuilds them from the buffer)."""
        if self.rank != 0:
            return
        T = self.engine.trainer_state()
        state = dict(fingerprint=self.fingerprint(), iterations_done=self.iterations_done, games_played=self.games_played,
                     weights=T["weights"], m=T["m"], v=T["v"], step=T["step"], replay=self._replay_arrays(),
                     digest_trainer=self.engine.state_digest("trainer"), digest_replay=self._replay_digest(),
                     torch_generator=self._torch_gen.get_state().numpy() if self._torch_gen is not None else None)
        write_state_file(path, state)

    def _restore_learner(self, path):
        """restore_state on the learner's rank. Returns the file's state."""
        S = read_state_file(path)
        check_fingerprint(S["fingerprint"], self.fingerprint(), where=str(path))   # 1: before anything changes
        if S["weights"].size != self.n_params:
            raise ValueError(f"{path}: {S['weights'].size} parameters, net={self.net!r} has {self.n_params}")
        if (S["torch_generator"] is not None) != (self._torch_gen is not None):
            raise ValueError(f"{path}: the torch generator's state is {'missing' if self._torch_gen is not None else 'unexpected'}")
        old_T, old_R, old_w = self.engine.trainer_state(), self._replay_arrays(), self.weights
        self.engine.trainer_set_state(S["weights"], S["m"], S["v"], S["step"])               # 2
        self._replay_put(S["replay"])                                                         # 3
        if self._holdout_threshold and self.replay == "device":                               # 4
            self.engine.replay_set_holdout(_holdout_key(self.seed), self._holdout_threshold)
        self._load(S["weights"])                                                              # 5: in the engine's arithmetic
        got = dict(trainer=self.engine.state_digest("trainer"), replay=self._replay_digest())   # 7 (the counters, 6, follow a passed check)
        want = dict(trainer=S["digest_trainer"], replay=S["digest_replay"])
        bad = [k for k in got if got[k] != want[k]]
        if bad:
            self.engine.trainer_set_state(old_T["weights"], old_T["m"], old_T["v"], old_T["step"])
            self._replay_put(old_R)
            self._load(old_w)
            raise ValueError(f"{path}: the restored state does not have the file's digest: " +
                             ", ".join(f"{k} {got[k]:016x} != {want[k]:016x}" for k in bad) + " (the file was changed after it was written)")
        self.weights = np.array(S["weights"], np.float32)
        if self._torch_gen is not None:
            self._torch_gen.set_state(self._torch.from_numpy(np.array(S["torch_generator"], np.uint8)))
        return S

    def restore_state(self, path):
        """Continues the run that save_state wrote to `path`, on a freshly constructed loop (same engine rules as the constructor). In
        order: the file's fingerprint is checked against this loop's — a mismatch raises ValueError naming the field before anything
        changes (`replay` is not part of it: a run saved under "host" may continue under "device" and the reverse); the trainer is set
        (Engine.trainer_set_state); the buffer is put back; the holdout key is applied again; the weights become the engine's network in
        the engine's arithmetic; the counters and the generator are set; and the TRAINER and REPLAY digests are computed again where the
        state lives and compared with the file's — a difference raises ValueError with the engine's trainer, buffer and network as they
        were before the call. With several ranks the learner's rank restores, the weights reach the others through the loop's
        broadcast, and the others set only their counters. The iterations that follow leave the bits of a run that never stopped."""
        t = self._torch
        S, err = None, None
        if self.rank == 0:
            try:
                S = self._restore_learner(path)
            except Exception as e:   # (with several ranks the others must hear of it before anybody raises)
                if self.dist is None:
                    raise
                err = e
        if self.dist is not None:
            head = t.tensor([0 if S is None else 1, S["iterations_done"] if S else 0, S["games_played"] if S else 0], dtype=t.int64,
                            device=self._wbuf.device)
            self.dist.broadcast(head, src=0)
            ok, iterations_done, games_played = (int(x) for x in head.tolist())
            if not ok:
                raise err if err is not None else ValueError(f"{path}: the learner's rank refused the state file")
            if self.rank == 0:
                self._wbuf.copy_(t.from_numpy(self.weights))
            self.dist.broadcast(self._wbuf, src=0)
            if self.rank != 0:
                self.weights = self._wbuf.cpu().numpy().copy()
                self._load(self.weights)
        else:
            iterations_done, games_played = S["iterations_done"], S["games_played"]
        self.iterations_done, self.games_played = iterations_done, games_played

    # one replay position on the wire: my_bb, op_bb (u64), gid (i64), pi[9], v[3] (f32) = 72 bytes, no pickling. A rank's buffer is
    # five contiguous sections [my | op | gid | pi | v] of `cap` positions each (five block copies to pack, views to unpack).
    _FIELDS = (("my", np.uint64, 1), ("op", np.uint64, 1), ("gid", np.int64, 1), ("pi", np.float32, 9), ("v", np.float32, 3))
    _POS_BYTES = 72

    def _gather_positions(self, new):
        """The ranks' new positions to the learner's rank (in rank order = game order) as ONE fixed-layout tensor gather: the
        counts travel first (one all_gather of an int64 per rank), then every rank contributes a buffer sized for the largest count —
        device buffers under RCCL, host buffers under gloo. (The round-3 form pickled a dict of arrays per rank: rank 0 unpickled
        8 x 18 MB per iteration.)"""
        t = self._torch
        n = int(new["my"].size)
        on_gpu = self._wbuf.is_cuda
        dev = self._wbuf.device
        cnt = t.tensor([n], dtype=t.int64, device=dev)
        counts = [t.zeros(1, dtype=t.int64, device=dev) for _ in range(self.world)]
        t_w = time.perf_counter()
        self.dist.all_gather(counts, cnt)     # (also where a rank waits for the slowest rank's self-play to end)
        counts = [int(c.item()) for c in counts]
        self._last_gather_wait = time.perf_counter() - t_w
        # every rank sends the same, slowly changing size: the largest count rounded up to 32,768 positions, so that the pack buffer and
        # rank 0's receive buffers live across iterations (first-touch page faults of fresh 10 MB buffers were most of this phase)
        cap = (max(max(counts), 1) + 32767) // 32768 * 32768
        if getattr(self, "_gcap", 0) != cap:
            self._gcap = cap
            self._gbuf = np.zeros(cap * self._POS_BYTES, np.uint8)
            self._gdev = t.empty(cap * self._POS_BYTES, dtype=t.uint8, device=dev) if on_gpu else None
            like = self._gdev if on_gpu else t.from_numpy(self._gbuf)
            self._gparts = [t.zeros_like(like) for _ in range(self.world)] if self.rank == 0 else None
        buf = self._gbuf
        off = 0
        for name, dt, width in self._FIELDS:
            sec = buf[off: off + cap * np.dtype(dt).itemsize * width].view(dt)
            sec[: n * width] = np.ascontiguousarray(new[name], dtype=dt).reshape(-1)
            off += cap * np.dtype(dt).itemsize * width
        mine = t.from_numpy(buf)
        if on_gpu:
            self._gdev.copy_(mine)
            mine = self._gdev
        parts = self._gparts
        self.dist.gather(mine, parts, dst=0)
        if self.rank != 0:
            return new
        out = {name: [] for name, _, _ in self._FIELDS}
        for p_, c in zip(parts, counts):
            raw = p_.cpu().numpy()
            off = 0
            for name, dt, width in self._FIELDS:
                sec = raw[off: off + cap * np.dtype(dt).itemsize * width].view(dt)[: c * width]
                out[name].append(sec.reshape(c, width) if width > 1 else sec)
                off += cap * np.dtype(dt).itemsize * width
        return {k: np.concatenate(v) for k, v in out.items()}

    def _sections(self, base, cap):
        """Addresses of the five `_FIELDS` sections of a gather buffer of `cap` positions that starts at `base`"""
        out, off = [], 0
        for _, dt, width in self._FIELDS:
            out.append(base + off)
            off += cap * np.dtype(dt).itemsize * width
        return out

    def _gather_positions_device(self, n, first):
        """replay="device" with several ranks: the same wire format as `_gather_positions` (counts, then one fixed-layout buffer per rank),
        but a rank's buffer is filled on the device — Engine.selfplay_positions_device compacts the last launch into its sections — and
        the learner's rank appends the parts to the engine's buffer in rank order: straight from the gathered device tensors under RCCL,
        from the gathered host tensors (a download of the compact 72 B/position form on every rank) under gloo. The learner's own part
        never leaves its engine."""
        t = self._torch
        on_gpu = self._wbuf.is_cuda
        cnt = t.tensor([n], dtype=t.int64, device=self._wbuf.device)
        counts = [t.zeros(1, dtype=t.int64, device=self._wbuf.device) for _ in range(self.world)]
        t_w = time.perf_counter()
        self.dist.all_gather(counts, cnt)
        counts = [int(c.item()) for c in counts]
        self._last_gather_wait = time.perf_counter() - t_w
        cap = (max(max(counts), 1) + 32767) // 32768 * 32768
        if getattr(self, "_gcap", 0) != cap:
            self._gcap = cap
            self._gdev = t.empty(cap * self._POS_BYTES, dtype=t.uint8, device=t.device(f"cuda:{self._device}"))
            self._ghost = None if on_gpu else t.zeros(cap * self._POS_BYTES, dtype=t.uint8)
            like = self._gdev if on_gpu else self._ghost
            self._gparts = [t.zeros_like(like) for _ in range(self.world)] if self.rank == 0 else None
        if self.rank == 0:
            assert self.engine.replay_append_selfplay(first) == n
        else:
            got = self.engine.selfplay_positions_device(first, *self._sections(self._gdev.data_ptr(), cap), cap)
            assert got == n, (got, n)
        mine = self._gdev
        if not on_gpu:
            if self.rank != 0:
                self._ghost.copy_(self._gdev)
            mine = self._ghost
        self.dist.gather(mine, self._gparts, dst=0)
        if self.rank != 0:
            return
        if on_gpu:
            t.cuda.synchronize(self._gdev.device)   # the parts were written on torch's stream, the appends run on the engine's
        for r in range(1, self.world):
            c, part = counts[r], self._gparts[r]
            if c == 0:
                continue
            if on_gpu:
                self.engine.replay_append_device(*self._sections(part.data_ptr(), cap), c)
            else:
                raw, off, secs = part.numpy(), 0, []
                for _, dt, width in self._FIELDS:
                    secs.append(raw[off: off + cap * np.dtype(dt).itemsize * width].view(dt)[: c * width])
                    off += cap * np.dtype(dt).itemsize * width
                self.engine.replay_append(*secs)

    def _iteration_device(self, cfg, games_per_train, games_to_keep, epochs, batch_size):
        """`iteration` with the replay buffer in the engine's device memory (replay="device"): same games, same record."""
        it = self.iterations_done
        t0 = time.perf_counter()
        n_t = self._exploring_games(it, games_per_train)
        off, count = shard_games(games_per_train - n_t, self.rank, self.world)
        first = it * games_per_train + off
        starts = None
        if n_t and self.rank == 0:   # the buffer as it stood before the iteration
            starts = self.engine.replay_select_positions(_exploring_key(self.seed, it), before_gid=it * games_per_train,
                                                         threshold=exploring_threshold(n_t, self.engine.replay_size()))
        if self.rank == 0:   # (grows, keeping the contents, when an iteration's shape changes)
            want = (int(games_to_keep) + int(games_per_train) + (max(0, int(starts["my"].size) - n_t) if starts else 0)) * 63
            if want > self._replay_reserved:
                self.engine.replay_reserve(want)
                self._replay_reserved = want
        sp = self.engine.selfplay(cfg, base_seed=self.seed, n_games=count, first_game=first, outputs=False)
        t_play = time.perf_counter() - t0
        n = sp["plies"]
        t1 = time.perf_counter()
        self._last_gather_wait = 0.0
        if self.dist is not None:
            self._gather_positions_device(int(n.sum()), first)
        else:
            self.engine.replay_append_selfplay(first)
        t_gather = time.perf_counter() - t1 - self._last_gather_wait
        t_ex = time.perf_counter()
        exploring = (0, 0)
        if starts is not None and starts["my"].size:
            ex_first = it * games_per_train + (games_per_train - n_t)
            ex = self._play_exploring(cfg, starts["my"], starts["op"], ex_first, outputs=False)
            assert self.engine.replay_append_selfplay(ex_first) == int(ex["rows"].sum())
            exploring = (int(ex["rows"].size), int(ex["rows"].sum()))
        t_ex = time.perf_counter() - t_ex
        self.games_played += games_per_train
        lr = _lr_at(self.lr_schedule, it)
        rec = dict(iteration=it + 1, lr=lr, games=int(games_per_train), games_this_rank=int(count),
                   plies_per_game=float(n.mean()) if count else 0.0)
        t_dedup = t_train = 0.0
        if self.rank == 0:
            self.engine.replay_keep_games_from(self.games_played - games_to_keep)   # keep_last_n_games (data.rs:160-194)
            steps_in_buffer = self.engine.replay_size()
            if self._reanalyse_threshold:
                t_re = time.perf_counter()
                reanalysed = self._reanalyse_device(cfg, it, it * games_per_train)
                t_re = time.perf_counter() - t_re
            # ---- deduplicate into the learner's data set (data.rs:196-235 + alpha_zero.rs:52-58), all on the device
            t2 = time.perf_counter()
            if self.symmetry == "mirror":
                n_canonical, n_unique = self.engine.replay_deduplicate_to_trainer(symmetry="mirror")
            else:
                n_unique = self.engine.replay_deduplicate_to_trainer()
            t_dedup = time.perf_counter() - t2
            if self._holdout_threshold:
                held = self.engine.dataset_counts()
                before = self._holdout_metrics(*held)
                before_arith = self._holdout_metrics_arith("holdout_before", held)
            t3 = time.perf_counter()
            steps, epoch_losses = self._epochs(it, epochs, batch_size, lr, n_unique)
            t_train = time.perf_counter() - t3
            self.weights = self.engine.trainer_state()["weights"]
            rec.update(steps_in_buffer=steps_in_buffer, unique=n_unique, optimiser_steps=steps, epoch_losses=epoch_losses)
            if self._holdout_threshold:
                rec.update(holdout_rows=held[0], holdout_unseen=held[1], holdout_before=before, holdout_after=self._holdout_metrics(*held))
                rec.update(before_arith, **self._holdout_metrics_arith("holdout_after", held))
            if self.symmetry == "mirror":
                rec["unique_canonical"] = n_canonical
            if self._reanalyse_threshold:
                rec.update(reanalysed=reanalysed[0], reanalyse_moved=reanalysed[1])
            if self.exploring_starts:
                rec.update(exploring_games=exploring[0], exploring_rows=exploring[1])
            if self.digests:
                rec["digests"] = self.state_digests()
            if self.logs_dir:
                import os

                D = self.engine.train_get_data()
                self._save_model(it + 1)
                np.save(os.path.join(self.logs_dir, "latest_states.npy"),
                        np.asarray(self.engine.features(D["my_bb"], D["op_bb"]), np.float32).reshape(-1, 1, 7, 9))
                np.save(os.path.join(self.logs_dir, "latest_pis.npy"), D["pis"])
                np.save(os.path.join(self.logs_dir, "latest_vs.npy"), D["vs"])
        self._finish_iteration(rec, t0, t_play, t_gather, t_dedup, t_train)
        if self.rank == 0 and self._reanalyse_threshold:
            rec["seconds"]["reanalyse"] = round(t_re, 4)
        if self.rank == 0 and self.exploring_starts:
            rec["seconds"]["exploring"] = round(t_ex, 4)
        return rec

    def _exploring_games(self, it, games_per_train):
        """How many of iteration `it`'s games (0-based) are replaced by games from stored positions: floor(exploring_starts *
        games_per_train) from the second iteration on — every rank computes it, the ordinary self-play shares the rest"""
        if not self.exploring_starts or it == 0:
            return 0
        return int(np.floor(self.exploring_starts * int(games_per_train)))

    def _play_exploring(self, cfg, start_my, start_op, first_gid, outputs):
        """The learner's rank: one recorded game per start position (Engine.games_run_recorded), the current weights on both sides in the
        engine's arithmetic, the iteration's cfg unchanged — a game's first move from a stored position is the configuration's random
        move — and game j on the generator of seed + first_gid + j, as self-play seeds game first_gid + j. A cfg whose search draws
        random numbers (Fpu.Func, Dirichlet noise) is refused by the engine: recorded games take deterministic searches only."""
        from .config import RecordConfig
        from .match import Player

        n = int(start_my.size)
        me = Player("current", int(cfg.num_explores), cfg.mcts_cfg, action=cfg.action, weights=self.weights)
        seeds = np.array([(self.seed + int(first_gid) + j) & _M64 for j in range(n)], np.uint64)
        zeros = np.zeros(n, np.int32)
        return self.engine.games_run_recorded([me], zeros, zeros, start_my, start_op, seeds, record=RecordConfig.from_rollout(cfg, 1),
                                              outputs=outputs)

    def _holdout_metrics(self, n_eval, n_unseen, arith="f32"):
        """The trainer's current weights on the evaluation set: dict(all=..., unseen=...) of dict(rows, mean_pi, mean_v, pi_acc, v_acc)"""
        out = {}
        for name, n in (("all", n_eval), ("unseen", n_unseen)):
            m = self.engine.dataset_evaluate("eval", 0, n, arith=arith) if n_eval else dict.fromkeys(_METRIC_KEYS, 0.0)
            out[name] = {k: (int(m[k]) if k == "rows" else float(m[k])) for k in _METRIC_KEYS}
        return out

    def _holdout_metrics_arith(self, prefix, held):
        """{prefix_<arith>: _holdout_metrics in that arithmetic} for every extra name of holdout_arith; None where the current weights
        cannot be evaluated in it (no f16x2 plan: SYN_ERR_UNSUPPORTED) — the run goes on"""
        from .engine import SynthesisAmdError

        out = {}
        for a in self.holdout_arith:
            try:
                out[f"{prefix}_{a}"] = self._holdout_metrics(*held, arith=a)
            except SynthesisAmdError as e:
                if e.code != _SYN_ERR_UNSUPPORTED:
                    raise
                out[f"{prefix}_{a}"] = None
        return out

    def _holdout_split_host(self):
        """replay="host": the device path's split on the host arrays: (the learner's part of self.R, the held-out part), buffer order kept"""
        held = holdout_flags(_holdout_key(self.seed), self._holdout_threshold, self.R["gid"])
        if held.all():
            raise ValueError("the holdout threshold holds out every game of the buffer: the learner would have no data set")
        return {k: a[~held] for k, a in self.R.items()}, {k: a[held] for k, a in self.R.items()}

    def _holdout_set_host(self, H, D):
        """De-duplicates the held-out positions H and uploads them as the evaluation set, unseen rows first (seen: the state, with
        symmetry="mirror" its canonical form, is among the learner's (canonical) rows of D). Returns (rows, unseen rows)."""
        if H["my"].size == 0:
            self.engine.dataset_set(H["my"], H["op"], H["pi"], H["v"])
            return 0, 0
        E = self.engine.replay_deduplicate(H["my"], H["op"], H["pi"], H["v"], symmetry=self.symmetry)
        my, op = E["my_bb"], E["op_bb"]
        n_train = D["canonical"] if self.symmetry == "mirror" else int(D["my_bb"].size)
        if self.symmetry == "mirror":
            mmy, mop = self.engine.positions_mirror(my, op)
            flipped = (mmy < my) | ((mmy == my) & (mop < op))
            my, op = np.where(flipped, mmy, my), np.where(flipped, mop, op)
        train = set(zip(D["my_bb"][:n_train].tolist(), D["op_bb"][:n_train].tolist()))
        seen = np.fromiter((k in train for k in zip(my.tolist(), op.tolist())), bool, count=my.size)
        order = np.concatenate([np.flatnonzero(~seen), np.flatnonzero(seen)])
        self.engine.dataset_set(E["my_bb"][order], E["op_bb"][order], E["pis"][order], E["vs"][order])
        return int(order.size), int((~seen).sum())

    def _reanalyse_device(self, cfg, it, before_gid):
        """replay="device": iteration `it`'s reanalysis in the engine's buffer. Returns (rows reanalysed, rows whose arg-max moved)."""
        st = self.engine.replay_reanalyse(cfg.mcts_cfg, self.reanalyse_explores or cfg.num_explores, _reanalyse_key(self.seed, it),
                                          threshold=self._reanalyse_threshold, before_gid=before_gid, action_selection=cfg.action,
                                          value_mix=self.reanalyse_value_mix)
        return st["selected"], st["moved"]

    def _reanalyse_host(self, cfg, it, before_gid):
        """replay="host": the same on self.R — reanalyse_flags, ONE Engine.mcts_search over the selected rows (root j on stream j), the
        write-back as numpy f32 operations in the device's order."""
        R = self.R
        rows = np.flatnonzero(reanalyse_flags(_reanalyse_key(self.seed, it), self._reanalyse_threshold, before_gid, R["gid"], R["my"], R["op"]))
        if rows.size == 0:
            return 0, 0
        res = self.engine.mcts_search(cfg.mcts_cfg, R["my"][rows], R["op"][rows], self.reanalyse_explores or cfg.num_explores,
                                      action_selection=cfg.action)
        pi = np.asarray(res["target_pi"], np.float32).reshape(-1, 9)
        q = np.asarray(res["target_q"], np.float32).reshape(-1, 3)
        moved = int((R["pi"][rows].argmax(axis=1) != pi.argmax(axis=1)).sum())
        R["pi"][rows] = pi
        w = np.float32(self.reanalyse_value_mix)
        if w == np.float32(1.0):
            R["v"][rows] = q
        elif w != np.float32(0.0):
            R["v"][rows] = R["v"][rows] * (np.float32(1.0) - w) + q * w
        return int(rows.size), moved

    def _epochs(self, it, epochs, batch_size, lr, n_unique):
        """Iteration `it`'s epochs of optimiser steps over the learner's data set of n_unique rows (alpha_zero.rs:72-94), both replay
        modes: (optimiser steps, epoch_losses). The host samplers draw a permutation and make one train_epoch call per epoch;
        sampler="device" is ONE call whose order the device draws from _sampler_key(seed, it)."""
        n_steps = n_unique // batch_size   # drop_last = true (data.rs:41-62)
        if self.sampler == "device":
            per_epoch = self.engine.train_epochs_sampled(_sampler_key(self.seed, it), epochs, batch_size, lr, flip=self.flip)
        else:
            per_epoch = []
            for ep in range(epochs):
                if self.sampler == "torch":   # BatchRandSampler::new (data.rs:29)
                    perm = self._torch.randperm(n_unique, generator=self._torch_gen, dtype=self._torch.int64).numpy()
                else:
                    perm = np.random.default_rng([self.seed, it, ep]).permutation(n_unique)
                if n_steps:
                    per_epoch.append(self.engine.train_epoch(perm[: n_steps * batch_size], batch_size, lr))
        epoch_losses = [(sl.astype(np.float64).sum(axis=0) * batch_size / n_unique).tolist() for sl in per_epoch] if n_steps else []
        return epochs * n_steps, epoch_losses

    def _finish_iteration(self, rec, t0, t_play, t_gather, t_dedup, t_train):
        """model_{i+1} (alpha_zero.rs:97,194): the trained parameters become every rank's self-play network; the record's timings"""
        t4 = time.perf_counter()
        if self.dist is not None:
            if self.rank == 0:
                self._wbuf.copy_(self._torch.from_numpy(self.weights))
            self.dist.broadcast(self._wbuf, src=0)
            self.weights = self._wbuf.cpu().numpy().copy()
            self._load(self.weights)
        elif self.rank == 0:
            self.engine.trainer_publish_weights()
        t_bcast = time.perf_counter() - t4
        self.iterations_done += 1
        rec["seconds"] = dict(selfplay=round(t_play, 4), wait_for_ranks=round(self._last_gather_wait, 4), gather=round(t_gather, 4),
                              dedup=round(t_dedup, 4), train=round(t_train, 4),
                              broadcast=round(t_bcast, 4), total=round(time.perf_counter() - t0, 4))

    def iteration(self, cfg, games_per_train, games_to_keep, epochs, batch_size):
        """One pass of the loop body (alpha_zero.rs:42-100). Returns this rank's record of it (rank 0's has the learner's numbers)."""
        if self.replay == "device":
            return self._iteration_device(cfg, games_per_train, games_to_keep, epochs, batch_size)
        it = self.iterations_done
        t0 = time.perf_counter()
        # ---- gather_experience: this rank's share of the new games; global game index = seed offset, never reused
        n_t = self._exploring_games(it, games_per_train)
        off, count = shard_games(games_per_train - n_t, self.rank, self.world)
        first = it * games_per_train + off
        starts = None
        if n_t and self.rank == 0:   # the buffer as it stood before the iteration
            R = self.R
            sel = reanalyse_flags(_exploring_key(self.seed, it), exploring_threshold(n_t, R["my"].size), it * games_per_train, R["gid"],
                                  R["my"], R["op"])
            starts = dict(my=R["my"][sel].copy(), op=R["op"][sel].copy())
        sp = self.engine.selfplay(cfg, base_seed=self.seed, n_games=count, first_game=first)
        t_play = time.perf_counter() - t0
        n = sp["plies"]
        mask = np.arange(63)[None, :] < n[:, None]
        new = dict(my=sp["states_bb"][..., 0][mask], op=sp["states_bb"][..., 1][mask], pi=sp["pis"][mask], v=sp["vs"][mask],
                   gid=(first + np.arange(count))[:, None].repeat(63, 1)[mask])
        t1 = time.perf_counter()
        self._last_gather_wait = 0.0
        if self.dist is not None:
            new = self._gather_positions(new)
        t_gather = time.perf_counter() - t1 - self._last_gather_wait   # pack + gather + unpack, without the wait for the slowest rank
        t_ex = time.perf_counter()
        exploring = (0, 0)
        if starts is not None and starts["my"].size:
            ex_first = it * games_per_train + (games_per_train - n_t)
            ex = self._play_exploring(cfg, starts["my"], starts["op"], ex_first, outputs=True)
            emask = np.arange(63)[None, :] < ex["rows"][:, None]
            extra = dict(my=ex["states"][..., 0][emask], op=ex["states"][..., 1][emask], pi=ex["pis"][emask], v=ex["vs"][emask],
                         gid=(ex_first + np.arange(ex["rows"].size))[:, None].repeat(63, 1)[emask])
            new = {k: np.concatenate([new[k], extra[k]]) for k in extra}
            exploring = (int(ex["rows"].size), int(ex["rows"].sum()))
        t_ex = time.perf_counter() - t_ex
        self.games_played += games_per_train
        lr = _lr_at(self.lr_schedule, it)
        rec = dict(iteration=it + 1, lr=lr, games=int(games_per_train), games_this_rank=int(count),
                   plies_per_game=float(n.mean()) if count else 0.0)
        t_dedup = t_train = 0.0
        if self.rank == 0:
            R = {k: np.concatenate([self.R[k], new[k]]) for k in self.R}
            keep = R["gid"] >= self.games_played - games_to_keep   # keep_last_n_games (data.rs:160-194)
            self.R = {k: a[keep] for k, a in R.items()}
            if self._reanalyse_threshold:
                t_re = time.perf_counter()
                reanalysed = self._reanalyse_host(cfg, it, it * games_per_train)
                t_re = time.perf_counter() - t_re
            # ---- deduplicate on the GPU (data.rs:196-235)
            t2 = time.perf_counter()
            T, H = self._holdout_split_host() if self._holdout_threshold else (self.R, None)   # the learner's part, the held-out part
            if self.symmetry == "mirror":
                D = self.engine.replay_deduplicate(T["my"], T["op"], T["pi"], T["v"], symmetry="mirror")
            else:
                D = self.engine.replay_deduplicate(T["my"], T["op"], T["pi"], T["v"])
            if self._holdout_threshold:
                held = self._holdout_set_host(H, D)
            t_dedup = time.perf_counter() - t2
            n_unique = int(D["num"].size)
            # ---- epochs of optimiser steps (alpha_zero.rs:72-94): one upload, one persistent kernel launch per epoch
            t3 = time.perf_counter()
            self.engine.train_set_data(D["my_bb"], D["op_bb"], D["pis"], D["vs"])
            if self._holdout_threshold:
                before = self._holdout_metrics(*held)
                before_arith = self._holdout_metrics_arith("holdout_before", held)
            steps, epoch_losses = self._epochs(it, epochs, batch_size, lr, n_unique)
            t_train = time.perf_counter() - t3
            self.weights = self.engine.trainer_state()["weights"]
            rec.update(steps_in_buffer=int(self.R["my"].size), unique=n_unique, optimiser_steps=steps, epoch_losses=epoch_losses)
            if self._holdout_threshold:
                rec.update(holdout_rows=held[0], holdout_unseen=held[1], holdout_before=before, holdout_after=self._holdout_metrics(*held))
                rec.update(before_arith, **self._holdout_metrics_arith("holdout_after", held))
            if self.symmetry == "mirror":
                rec["unique_canonical"] = D["canonical"]
            if self._reanalyse_threshold:
                rec.update(reanalysed=reanalysed[0], reanalyse_moved=reanalysed[1])
            if self.exploring_starts:
                rec.update(exploring_games=exploring[0], exploring_rows=exploring[1])
            if self.digests:
                rec["digests"] = self.state_digests()
            if self.logs_dir:   # alpha_zero.rs:97-100
                import os

                self._save_model(it + 1)
                np.save(os.path.join(self.logs_dir, "latest_states.npy"),
                        np.asarray(self.engine.features(D["my_bb"], D["op_bb"]), np.float32).reshape(-1, 1, 7, 9))
                np.save(os.path.join(self.logs_dir, "latest_pis.npy"), np.asarray(D["pis"], np.float32).reshape(-1, 9))
                np.save(os.path.join(self.logs_dir, "latest_vs.npy"), np.asarray(D["vs"], np.float32).reshape(-1, 3))
        # ---- model_{i+1} (alpha_zero.rs:97,194): the trained parameters become every rank's self-play network
        t4 = time.perf_counter()
        if self.dist is not None:
            if self.rank == 0:
                self._wbuf.copy_(self._torch.from_numpy(self.weights))
            self.dist.broadcast(self._wbuf, src=0)
            self.weights = self._wbuf.cpu().numpy().copy()
            self._load(self.weights)
        elif self.rank == 0:
            self.engine.trainer_publish_weights()   # one rank: the learner's image is copied on the device
        t_bcast = time.perf_counter() - t4
        self.iterations_done += 1
        rec["seconds"] = dict(selfplay=round(t_play, 4), wait_for_ranks=round(self._last_gather_wait, 4), gather=round(t_gather, 4),
                              dedup=round(t_dedup, 4), train=round(t_train, 4),
                              broadcast=round(t_bcast, 4), total=round(time.perf_counter() - t0, 4))
        if self.rank == 0 and self._reanalyse_threshold:
            rec["seconds"]["reanalyse"] = round(t_re, 4)
        if self.rank == 0 and self.exploring_starts:
            rec["seconds"]["exploring"] = round(t_ex, 4)
        return rec


class DataParallelLearner:
    """Gradient all-reduce per optimiser step (see the module docstring). Every rank holds identical weights and Adam moments."""

    def __init__(self, engine, blob, dist=None, device=0, net="mlp", collective_at_world_1=False, network_arithmetic="f32", batch_mode="chained", **hyper):
        """batch_mode: "chained" | "micro" (Engine.trainer_set_batch_mode): with "micro" every rank's shard of a batch must be a multiple
        of 32 positions; it runs as micro-batches of 32 over the rank's whole GPU.
        collective_at_world_1: keep the all-reduce in the step when the group has one rank (bench.py's `data_parallel_world1`:
        the literal gradients -> RCCL all-reduce -> Adam path of BASELINE configs[4] on a one-GPU box).
        network_arithmetic: "f32" | "f16x2", the arithmetic the engine's self-play evaluates the published network in."""
        import torch

        self._torch = torch
        self.engine = engine
        self.net = net
        self.dist = dist if (dist is not None and dist.is_initialized() and (dist.get_world_size() > 1 or collective_at_world_1)) else None
        self.world = self.dist.get_world_size() if self.dist else 1
        self.device = torch.device(f"cuda:{device}")
        self.n_params = CONV_NUM_PARAMS if net == "conv" else NUM_PARAMS
        (engine.trainer_init_conv if net == "conv" else engine.trainer_init)(blob, **hyper)
        if batch_mode != "chained":
            engine.trainer_set_batch_mode(batch_mode)
        self.batch_mode = batch_mode
        if network_arithmetic != "f32":
            engine.set_network_arithmetic(network_arithmetic)
        # [gradients | pi-loss sum | v-loss sum]: one buffer, one all-reduce per step
        self.buf = torch.zeros(self.n_params + 2, dtype=torch.float32, device=self.device)
        self._staged = self.dist is not None and self.dist.get_backend() != "nccl"
        self._host = torch.zeros(self.n_params + 2, dtype=torch.float32).pin_memory() if self._staged else None
        self._loss_sum = torch.zeros(2, dtype=torch.float64, device=self.device)
        self._steps = 0
        self._data = None

    # ---- the data set of an iteration and an epoch's order: uploaded once, gathered on the device per step
    def set_data(self, my_bb, op_bb, target_pi, target_v):
        t = self._torch
        self._data = (t.from_numpy(np.ascontiguousarray(my_bb, dtype=np.uint64).view(np.int64)).to(self.device),
                      t.from_numpy(np.ascontiguousarray(op_bb, dtype=np.uint64).view(np.int64)).to(self.device),
                      t.from_numpy(np.ascontiguousarray(target_pi, dtype=np.float32).reshape(-1, 9)).to(self.device),
                      t.from_numpy(np.ascontiguousarray(target_v, dtype=np.float32).reshape(-1, 3)).to(self.device))

    def step_indices(self, idx, lr):
        """One optimiser step on the samples `idx` (THIS rank's shard of the global batch) of the uploaded data set."""
        t = self._torch
        ix = t.as_tensor(np.ascontiguousarray(idx, dtype=np.int64), device=self.device)
        my, op, tpi, tv = (a.index_select(0, ix).contiguous() for a in self._data)
        self._step_device(my, op, tpi, tv, lr)

    def epoch(self, order, batch, lr):
        """len(order) // batch optimiser steps over the uploaded data set in the given order (THIS rank's shard of every global batch):
        the order is uploaded once, every step gathers its minibatch on the device and runs gradients -> all-reduce -> Adam in stream
        order; the host only enqueues. Returns the number of steps."""
        t = self._torch
        od = t.as_tensor(np.ascontiguousarray(order, dtype=np.int64), device=self.device)
        n = int(od.numel()) // int(batch)
        for s in range(n):
            ix = od[s * batch:(s + 1) * batch]
            my, op, tpi, tv = (a.index_select(0, ix) for a in self._data)
            self._step_device(my, op, tpi, tv, lr)
        return n

    def step(self, my_bb, op_bb, target_pi, target_v, lr):
        """One optimiser step; the arguments are THIS rank's shard of the batch (host arrays). Returns the (pi_loss, v_loss) of
        the global batch (mean over ranks of the per-shard means) — which costs a device synchronisation; `step_indices` +
        `take_losses` keep that off the step's critical path."""
        t = self._torch
        my = t.from_numpy(np.ascontiguousarray(my_bb, dtype=np.uint64).view(np.int64)).to(self.device)
        op = t.from_numpy(np.ascontiguousarray(op_bb, dtype=np.uint64).view(np.int64)).to(self.device)
        tpi = t.from_numpy(np.ascontiguousarray(target_pi, dtype=np.float32)).to(self.device)
        tv = t.from_numpy(np.ascontiguousarray(target_v, dtype=np.float32)).to(self.device)
        self._step_device(my, op, tpi, tv, lr)
        return (self.buf[self.n_params:] / self.world).cpu().numpy()   # (the read-back waits for the step)

    def _step_device(self, my, op, tpi, tv, lr):
        """gradients -> all-reduce -> Adam in ONE stream order (torch's current stream, which is also where the batch was gathered and
        where RCCL orders its collective): the gradient kernel writes its two loss sums behind the gradients, so they ride in the
        same 122 KB message; no host wait, no host-to-device copy, no synchronisation per step (13 us of compute per step would
        otherwise sit behind four of them). Under a host-staged backend (gloo: CPU tests, dry runs) the message crosses the host."""
        t = self._torch
        st = t.cuda.current_stream(self.device).cuda_stream
        self.engine.train_gradients_enqueue(st, my.data_ptr(), op.data_ptr(), tpi.data_ptr(), tv.data_ptr(), int(my.numel()),
                                            self.buf.data_ptr(), self.buf.data_ptr() + 4 * self.n_params)
        if self.dist is not None:
            if self._staged:
                self._host.copy_(self.buf)      # (stream-ordered copy to pinned memory, then the host waits for it)
                t.cuda.current_stream(self.device).synchronize()
                self.dist.all_reduce(self._host)
                self.buf.copy_(self._host, non_blocking=True)
            else:
                self.dist.all_reduce(self.buf)  # RCCL over xGMI: one 122 KB message (latency-bound), ordered behind the kernel
        self._loss_sum += self.buf[self.n_params:].double() / self.world
        self._steps += 1
        self.engine.train_apply_enqueue(st, self.buf.data_ptr(), lr, grad_scale=1.0 / self.world)

    def take_losses(self):
        """(sum of the per-step global (pi_loss, v_loss), steps) since the last call — one read-back per epoch instead of per step."""
        out = self._loss_sum.cpu().numpy().copy(), self._steps
        self._loss_sum.zero_()
        self._steps = 0
        return out

    def publish(self):
        """The trained network becomes the engine's self-play network (model_{i+1}.ot of alpha_zero.rs:97)."""
        self._torch.cuda.current_stream(self.device).synchronize()   # the steps ran on torch's stream, the hand-off runs on the engine's
        self.engine.trainer_publish_weights()

    def state(self):
        self._torch.cuda.current_stream(self.device).synchronize()
        return self.engine.trainer_state()
