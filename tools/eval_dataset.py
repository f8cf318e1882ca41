#!/usr/bin/env python3
"""The losses and arg-max accuracies of one checkpoint on one data set (Engine.dataset_evaluate: the f32 learner's definition, forward
only; --arith f16x2 / bf16: the same head on the raw outputs of that arithmetic), overall and by stone count. One JSON line.

    python tools/eval_dataset.py --checkpoint logs/models/model_12.ot --logs-dir logs          # latest_states / pis / vs.npy of a run
    python tools/eval_dataset.py --checkpoint tests/golden/c4conv_trained_f32.npy --games 2048  # self-play by the checkpoint itself

--checkpoint: a flat f32 blob as .npy (30,492 floats: Connect4Net, 12,412: Connect4ConvNet) or a Connect4Net VarStore archive (.ot).
--logs-dir:   the de-duplicated buffer LearningLoop(logs_dir=...) writes per iteration (states as the 7 x 9 feature planes: +1 mine,
              -1 theirs). Those are the positions the run's LAST iteration trained on: a held-out number it is not.
--games N:    N self-play games by --player (default: the checkpoint) at --explores, de-duplicated; with --holdout F the games are split
              as LearningLoop(holdout=F) splits them and the held-out part is evaluated, all rows and unseen rows."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def load_checkpoint(path):
    if path.endswith(".ot"):
        from synthesis_amd.weights import load_ot

        return np.ascontiguousarray(load_ot(path), np.float32).ravel()
    return np.ascontiguousarray(np.load(path), np.float32).ravel()


def boards_of_features(states):
    """latest_states.npy [n, 1, 7, 9] -> (my, op): feature [row][col] = +1 mine / -1 theirs, bit = row + 7 col"""
    x = np.asarray(states, np.float32).reshape(-1, 7, 9)
    shift = (np.arange(7)[:, None] + 7 * np.arange(9)[None, :]).astype(np.uint64)
    my = ((x == 1.0).astype(np.uint64) << shift).sum(axis=(1, 2), dtype=np.uint64)
    op = ((x == -1.0).astype(np.uint64) << shift).sum(axis=(1, 2), dtype=np.uint64)
    return my, op


def by_stone_count(r, my, op, tpi, tv):
    """the per-row outputs grouped by the number of stones on the board: mean KL of both heads and the two accuracies"""
    my, op = np.asarray(my, np.uint64), np.asarray(op, np.uint64)
    stones = np.array([bin(int(a) | int(b)).count("1") for a, b in zip(my, op)])
    # the header's arg-max rules (np.argmax returns the first maximum): the policy's over the legal columns, top cell bit 6 + 7 c free
    legal = (((my | op)[:, None] >> (np.uint64(6) + np.uint64(7) * np.arange(9, dtype=np.uint64))[None, :]) & np.uint64(1)) == 0
    lg = r["row_logits"]
    ph = legal.any(axis=1) & (np.argmax(np.where(legal, lg[:, :9], -np.inf), axis=1) == np.argmax(tpi, axis=1))
    vh = np.argmax(lg[:, 9:], axis=1) == np.argmax(tv, axis=1)
    out = {}
    for s in np.unique(stones):
        m = stones == s
        out[int(s)] = dict(rows=int(m.sum()), mean_pi=float(r["row_kl"][m, 0].astype(np.float64).mean()),
                           mean_v=float(r["row_kl"][m, 1].astype(np.float64).mean()), pi_acc=float(ph[m].mean()), v_acc=float(vh[m].mean()))
    return out


def evaluate(eng, blob, first, n, breakdown, D, arith="f32"):
    keys = ("rows", "mean_pi", "mean_v", "pi_acc", "v_acc")
    r = eng.dataset_evaluate("eval", first, n, blob=blob, rows=breakdown, arith=arith)
    out = {k: r[k] for k in keys}
    if breakdown and n:
        sl = slice(first, first + n)
        out["by_stones"] = by_stone_count(r, D["my_bb"][sl], D["op_bb"][sl], D["pis"][sl], D["vs"][sl])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--checkpoint", required=True)
    ap.add_argument("--logs-dir", default="")
    ap.add_argument("--games", type=int, default=0)
    ap.add_argument("--explores", type=int, default=200)
    ap.add_argument("--player", default="", help="--games: the checkpoint that plays them (default: --checkpoint)")
    ap.add_argument("--holdout", type=float, default=0.0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--no-breakdown", action="store_true")
    ap.add_argument("--arith", default="f32", choices=["f32", "f16x2", "bf16"], help="the arithmetic that computes the rows' raw outputs: the f32 "
                    "learner's, the engine's f16x2 inference, or the conv learner's bf16 forward (Connect4ConvNet only)")
    args = ap.parse_args()
    if bool(args.logs_dir) == bool(args.games):
        raise SystemExit("give exactly one data set: --logs-dir DIR or --games N")
    if not 0.0 <= args.holdout < 1.0 or (args.holdout and not args.games):
        raise SystemExit("--holdout is a fraction of --games in [0, 1)")

    import torch  # noqa: F401  (before the engine: one HIP runtime per process)

    import synthesis_amd as sa
    from synthesis_amd.engine import CONV_NUM_PARAMS, NUM_PARAMS
    from synthesis_amd.learner import _holdout_key

    blob = load_checkpoint(args.checkpoint)
    if blob.size not in (NUM_PARAMS, CONV_NUM_PARAMS):
        raise SystemExit(f"{args.checkpoint} holds {blob.size} floats: neither Connect4Net ({NUM_PARAMS}) nor Connect4ConvNet ({CONV_NUM_PARAMS})")
    out = dict(tool="tools/eval_dataset.py", checkpoint=args.checkpoint, arith=args.arith, network="Connect4ConvNet" if blob.size == CONV_NUM_PARAMS else "Connect4Net")
    breakdown = not args.no_breakdown
    with sa.Engine(concurrent_games=max(16, min(args.games, 65536)), max_explores=max(args.explores, 8), device=args.device) as eng:
        if args.logs_dir:
            my, op = boards_of_features(np.load(os.path.join(args.logs_dir, "latest_states.npy")))
            pis, vs = np.load(os.path.join(args.logs_dir, "latest_pis.npy")), np.load(os.path.join(args.logs_dir, "latest_vs.npy"))
            eng.dataset_set(my, op, pis, vs)
            out["data_set"] = dict(logs_dir=args.logs_dir, rows=int(my.size))
            n, unseen = int(my.size), None
        else:
            player = load_checkpoint(args.player) if args.player else blob
            (eng.load_weights_conv if player.size == CONV_NUM_PARAMS else eng.load_weights)(player)
            eng.trainer_init(np.zeros(NUM_PARAMS, np.float32))   # (replay_deduplicate_to_trainer's owner; its weights are never used)
            eng.replay_reserve(args.games * 63)
            eng.selfplay(sa.parity_rollout_config(args.explores), base_seed=args.seed, n_games=args.games, outputs=False)
            positions = eng.replay_append_selfplay(0)
            threshold = int(np.floor(args.holdout * 4294967296.0))
            eng.replay_set_holdout(_holdout_key(args.seed), threshold)
            learner_rows = eng.replay_deduplicate_to_trainer()
            if threshold:
                n, unseen = eng.dataset_counts()
            else:   # nothing held out: the whole de-duplicated buffer is the data set
                D = eng.train_get_data()
                eng.dataset_set(D["my_bb"], D["op_bb"], D["pis"], D["vs"])
                n, unseen = learner_rows, None
            out["data_set"] = dict(games=args.games, explores=args.explores, player=args.player or args.checkpoint, seed=args.seed,
                                   positions=positions, holdout=args.holdout, learner_rows=learner_rows if threshold else 0, rows=n)
        D = eng.dataset_get()
        out["all"] = evaluate(eng, blob, 0, n, breakdown, D, args.arith)
        if unseen is not None:
            out["unseen"] = evaluate(eng, blob, 0, unseen, breakdown, D, args.arith)
        out["device_ms_last_call"] = eng.last_timing()[0]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
