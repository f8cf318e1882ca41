#!/usr/bin/env python3
"""A/B of the learning loop's data path: LearningLoop(replay="host") against LearningLoop(replay="device") on two engines of ONE
process, interleaved (A B A B ...), same seed, same games.

    python tools/replay_loop_ab.py --shape bench     Engine(8192, 200), 8,192 games per iteration, keep 20,000: bench.py's
                                                     learner_loop shape, so the host arm can be read against the committed record
    python tools/replay_loop_ab.py --shape example   65,536 concurrent games, 65,536 games per iteration, keep 131,072 (892 MB of
                                                     replay buffer): a size examples/train_connect4.py's defaults run
    python tools/replay_loop_ab.py --out profiles/replay_device_ab.json     both shapes into one record

Two warm-up iterations per arm, then --timed (default 6) timed iterations per arm. The times are LearningLoop's own: the host clock
around its phases. Per arm: median and min/max of `total` and of every phase. The device arm's `dedup` phase ends where the unique
count reaches the host; the reduce behind it finishes inside `train`, so the arms are compared by `total`. The arms' records are
also compared (steps_in_buffer, unique, epoch_losses, final weights): an A/B of two loops that computed different things is void."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {
    "bench": dict(concurrent=8192, explores=200, games_per_train=8192, games_to_keep=20000, epochs=1, batch=32, seed=7),
    "example": dict(concurrent=65536, explores=200, games_per_train=65536, games_to_keep=131072, epochs=1, batch=32, seed=7),
}
PHASES = ("total", "selfplay", "gather", "dedup", "train", "broadcast")


def run_shape(name, warmup, timed, device):
    import synthesis_amd as sa
    from bench import make_weights
    from synthesis_amd.learner import LearningLoop

    s = SHAPES[name]
    blob = make_weights()
    cfg = sa.parity_rollout_config(s["explores"])
    arms = ("host", "device")
    engines = {a: sa.Engine(concurrent_games=s["concurrent"], max_explores=s["explores"], device=device) for a in arms}
    loops = {a: LearningLoop(engines[a], "mlp", blob, device=device, seed=s["seed"], weight_decay=1e-6, replay=a) for a in arms}
    recs = {a: [] for a in arms}
    for _ in range(warmup + timed):
        for a in arms:   # interleaved: drift of the box (clocks, other tenants) lands on both arms alike
            recs[a].append(loops[a].iteration(cfg, s["games_per_train"], s["games_to_keep"], s["epochs"], s["batch"]))
    same = all(ra[k] == rb[k] for ra, rb in zip(recs["host"], recs["device"])
               for k in ("steps_in_buffer", "unique", "optimiser_steps", "epoch_losses"))
    same = bool(same and np.array_equal(loops["host"].weights.view(np.uint32), loops["device"].weights.view(np.uint32)))
    out = dict(shape=dict(s), warmup_iterations=warmup, timed_iterations=timed, arms_computed_the_same=same,
               steps_in_buffer=[r["steps_in_buffer"] for r in recs["host"]], unique=[r["unique"] for r in recs["host"]],
               replay_buffer_bytes=(s["games_to_keep"] + s["games_per_train"]) * 63 * 72)
    for a in arms:
        t = {p: [r["seconds"][p] for r in recs[a][warmup:]] for p in PHASES}
        out[a] = {p: dict(median=round(statistics.median(v), 4), min=min(v), max=max(v)) for p, v in t.items()}
        out[a]["total_per_iteration"] = t["total"]
        engines[a].close()
    h, d = out["host"]["total"], out["device"]["total"]
    spread = max(h["max"] - h["min"], d["max"] - d["min"])
    out["median_total_host_minus_device"] = round(h["median"] - d["median"], 4)
    out["larger_min_max_range"] = round(spread, 4)
    # the rule the documents follow: "faster" only where the medians differ by more than the larger of the two arms' ranges
    out["resolved"] = bool(abs(h["median"] - d["median"]) > spread)
    # beside it, not instead of it: the arms ran pairwise on the same buffer sizes (which grow from iteration to iteration)
    paired = [a - b for a, b in zip(out["host"]["total_per_iteration"], out["device"]["total_per_iteration"])]
    out["paired_total_host_minus_device"] = dict(median=round(statistics.median(paired), 4), min=round(min(paired), 4),
                                                 max=round(max(paired), 4))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="both", choices=["bench", "example", "both"])
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--timed", type=int, default=6)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.timed < 6:
        raise SystemExit("--timed must be at least 6: fewer iterations per arm do not give a range worth comparing")

    import torch  # noqa: F401  (before the engine: one HIP runtime per process)

    import bench

    rec = dict(tool="tools/replay_loop_ab.py", kernel_source_hash=bench.kernel_source_hash(), device=torch.cuda.get_device_name(args.device),
               timing="host clock (time.perf_counter) inside LearningLoop.iteration; an iteration ends in a device synchronise",
               order="host, device, host, device, ... on two engines of one process",
               phases="the device arm's `dedup` ends where the number of unique states reaches the host: its segmented reduce and the "
                      "device-to-device copies into the learner's data set are stream-ordered and finish inside `train`; compare `total`",
               date=time.strftime("%Y-%m-%d"), shapes={})
    for name in (("bench", "example") if args.shape == "both" else (args.shape,)):
        rec["shapes"][name] = run_shape(name, args.warmup, args.timed, args.device)
        print(json.dumps({name: rec["shapes"][name]}), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
