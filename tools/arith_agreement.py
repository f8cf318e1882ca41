#!/usr/bin/env python3
"""What the arithmetic does to one checkpoint's outputs and held-out losses: held-out self-play positions of the checkpoint (made as
tools/eval_dataset.py --games N --holdout F makes them) evaluated in f32 and f16x2, and in bf16 for Connect4ConvNet
(Engine.dataset_evaluate(arith=...)), the losses per arithmetic and synthesis_amd.arena.dataset_agreement between the arithmetics' raw
outputs. One JSON line. A description, not a claim about strength.

    python tools/arith_agreement.py --checkpoint tests/golden/c4net_trained_f32.npy
    python tools/arith_agreement.py --checkpoint tests/golden/c4conv_trained_f32.npy --games 2048 --explores 200"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.eval_dataset import load_checkpoint  # noqa: E402

KEYS = ("rows", "mean_pi", "mean_v", "pi_acc", "v_acc")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--checkpoint", required=True)
    ap.add_argument("--games", type=int, default=2048)
    ap.add_argument("--explores", type=int, default=200)
    ap.add_argument("--holdout", type=float, default=0.25)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    if not 0.0 < args.holdout < 1.0:
        raise SystemExit("--holdout is a fraction of --games in (0, 1)")

    import torch  # noqa: F401  (before the engine: one HIP runtime per process)

    import synthesis_amd as sa
    from synthesis_amd.arena import dataset_agreement
    from synthesis_amd.engine import CONV_NUM_PARAMS, NUM_PARAMS, f16x2_plan_of_blob
    from synthesis_amd.learner import _holdout_key

    blob = load_checkpoint(args.checkpoint)
    if blob.size not in (NUM_PARAMS, CONV_NUM_PARAMS):
        raise SystemExit(f"{args.checkpoint} holds {blob.size} floats: neither Connect4Net ({NUM_PARAMS}) nor Connect4ConvNet ({CONV_NUM_PARAMS})")
    conv = blob.size == CONV_NUM_PARAMS
    ariths = ("f32", "f16x2", "bf16") if conv else ("f32", "f16x2")
    out = dict(tool="tools/arith_agreement.py", checkpoint=args.checkpoint, network="Connect4ConvNet" if conv else "Connect4Net",
               f16x2_plan=f16x2_plan_of_blob(blob))
    with sa.Engine(concurrent_games=max(16, min(args.games, 65536)), max_explores=max(args.explores, 8), device=args.device) as eng:
        (eng.load_weights_conv if conv else eng.load_weights)(blob)
        eng.trainer_init(np.zeros(NUM_PARAMS, np.float32))   # (replay_deduplicate_to_trainer's owner; its weights are never used)
        eng.replay_reserve(args.games * 63)
        eng.selfplay(sa.parity_rollout_config(args.explores), base_seed=args.seed, n_games=args.games, outputs=False)
        positions = eng.replay_append_selfplay(0)
        eng.replay_set_holdout(_holdout_key(args.seed), int(np.floor(args.holdout * 4294967296.0)))
        learner_rows = eng.replay_deduplicate_to_trainer()
        n, unseen = eng.dataset_counts()
        out["data_set"] = dict(games=args.games, explores=args.explores, seed=args.seed, positions=positions, holdout=args.holdout,
                               learner_rows=learner_rows, rows=n, unseen=unseen)
        D = eng.dataset_get()
        rows = {}
        out["losses"] = {}
        for a in ariths:
            r = eng.dataset_evaluate("eval", 0, n, blob=blob, rows=True, arith=a)
            rows[a] = r["row_logits"]
            out["losses"][a] = dict(all={k: r[k] for k in KEYS}, device_ms=eng.last_timing()[0])
            u = eng.dataset_evaluate("eval", 0, unseen, blob=blob, arith=a)
            out["losses"][a]["unseen"] = {k: u[k] for k in KEYS}
        out["agreement"] = {f"{a}_vs_f32": dataset_agreement(rows["f32"], rows[a], D["my_bb"], D["op_bb"]) for a in ariths[1:]}
        if conv:
            out["agreement"]["bf16_vs_f16x2"] = dataset_agreement(rows["f16x2"], rows["bf16"], D["my_bb"], D["op_bb"])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
