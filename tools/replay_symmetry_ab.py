#!/usr/bin/env python3
"""A/B of the mirror-symmetric de-duplication: LearningLoop(replay="device", symmetry="none") against symmetry="mirror" on two engines
of ONE process, interleaved (A B A B ...), same seed — tools/replay_loop_ab.py's protocol and its "example" shape: bench.py's loop
(Connect4Net, 200 explores, one epoch, batch 32, weight decay 1e-6) at 65,536 games per iteration, keep 131,072.

    python tools/replay_symmetry_ab.py --out profiles/replay_symmetry_ab.json

Two records come out of it:

  loop    two warm-up iterations per arm, then --timed (default 6) timed ones. The times are LearningLoop's own (host clock around its
          phases). The arms play the same games in iteration 1 only: from then on they train different networks, so their buffers
          differ in content (not in shape). The mirror arm's `train` runs over U + M rows instead of U: about twice the optimiser
          steps. That is the feature, not a regression; `total` carries it. The plain arm's `dedup` phase ends where the unique
          count reaches the host (its reduce finishes inside `train`); the mirror arm's ends one synchronise later, behind its reduce.
  dedup   the de-duplication-to-trainer call alone, both forms on ONE buffer (the plain arm's final one), interleaved, each followed
          by a read of the trainer state so that the clock stops behind the last kernel and copy of the call.

Whether the augmented data set makes a stronger player is not measured here."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPE = dict(concurrent=65536, explores=200, games_per_train=65536, games_to_keep=131072, epochs=1, batch=32, seed=7)
PHASES = ("total", "selfplay", "gather", "dedup", "train", "broadcast")
ARMS = ("none", "mirror")


def summary(v):
    return dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4))


def run(warmup, timed, dedup_reps, device):
    import synthesis_amd as sa
    from bench import make_weights
    from synthesis_amd.learner import LearningLoop

    s = SHAPE
    blob = make_weights()
    cfg = sa.parity_rollout_config(s["explores"])
    engines = {a: sa.Engine(concurrent_games=s["concurrent"], max_explores=s["explores"], device=device) for a in ARMS}
    loops = {a: LearningLoop(engines[a], "mlp", blob, device=device, seed=s["seed"], weight_decay=1e-6, replay="device", symmetry=a)
             for a in ARMS}
    recs = {a: [] for a in ARMS}
    for _ in range(warmup + timed):
        for a in ARMS:   # interleaved: drift of the box (clocks, other tenants) lands on both arms alike
            recs[a].append(loops[a].iteration(cfg, s["games_per_train"], s["games_to_keep"], s["epochs"], s["batch"]))
    loop = dict(shape=dict(s), warmup_iterations=warmup, timed_iterations=timed)
    for a in ARMS:
        t = {p: [r["seconds"][p] for r in recs[a][warmup:]] for p in PHASES}
        loop[a] = {p: summary(v) for p, v in t.items()}
        loop[a]["total_per_iteration"] = t["total"]
        loop[a]["n"] = [r["steps_in_buffer"] for r in recs[a]]
        loop[a]["rows"] = [r["unique"] for r in recs[a]]
        loop[a]["optimiser_steps"] = [r["optimiser_steps"] for r in recs[a]]
    loop["mirror"]["U"] = [r["unique_canonical"] for r in recs["mirror"]]
    loop["mirror"]["M"] = [r["unique"] - r["unique_canonical"] for r in recs["mirror"]]
    for p in ("total", "dedup", "train"):
        a, b = loop["none"][p], loop["mirror"][p]
        spread = max(a["max"] - a["min"], b["max"] - b["min"])
        # "slower" / "faster" only where the medians differ by more than the larger of the two arms' ranges
        loop[f"{p}_mirror_minus_none"] = dict(median=round(b["median"] - a["median"], 4), larger_min_max_range=round(spread, 4),
                                              resolved=bool(abs(b["median"] - a["median"]) > spread))

    # the call alone, both forms on the plain arm's final buffer
    eng = engines["none"]
    n = eng.replay_size()
    times = {a: [] for a in ARMS}
    counts = {}
    for i in range(2 + dedup_reps):
        for a in ARMS:
            eng.trainer_state()   # (nothing of an earlier call is still running)
            t0 = time.perf_counter()
            counts[a] = eng.replay_deduplicate_to_trainer(symmetry=a)
            eng.trainer_state()
            if i >= 2:
                times[a].append(time.perf_counter() - t0)
    U, total = counts["mirror"]
    dedup = dict(n=n, unique_plain=counts["none"], U=U, M=total - U, repetitions=dedup_reps, warmup=2,
                 seconds={a: summary(times[a]) for a in ARMS})
    a, b = dedup["seconds"]["none"], dedup["seconds"]["mirror"]
    spread = max(a["max"] - a["min"], b["max"] - b["min"])
    dedup["mirror_minus_none"] = dict(median=round(b["median"] - a["median"], 4), larger_min_max_range=round(spread, 4),
                                      resolved=bool(abs(b["median"] - a["median"]) > spread))
    for e in engines.values():
        e.close()
    return loop, dedup


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--timed", type=int, default=6)
    ap.add_argument("--dedup-reps", type=int, default=10)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.timed < 6:
        raise SystemExit("--timed must be at least 6: fewer iterations per arm do not give a range worth comparing")

    import torch  # noqa: F401  (before the engine: one HIP runtime per process)

    import bench

    loop, dedup = run(args.warmup, args.timed, args.dedup_reps, args.device)
    rec = dict(tool="tools/replay_symmetry_ab.py", kernel_source_hash=bench.kernel_source_hash(),
               device=torch.cuda.get_device_name(args.device),
               timing="host clock (time.perf_counter); loop: inside LearningLoop.iteration, an iteration ends in a device synchronise; "
                      "dedup: around replay_deduplicate_to_trainer + a read of the trainer state (which waits for the stream)",
               order="none, mirror, none, mirror, ... on two engines of one process (dedup: on one engine and one buffer)",
               note="the mirror arm's epochs run over U + M rows (about twice the optimiser steps): the larger data set is the feature; "
                    "playing strength is not measured",
               date=time.strftime("%Y-%m-%d"), loop=loop, dedup_to_trainer=dedup)
    print(json.dumps(rec), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
