#!/usr/bin/env python3
"""A/B of the device-resident match (Engine.match_run = syn_match_run) against the host path of match.play_match on identical games
(arena.host_match: play_match's per-ply steps from given starts — weight upload, root upload, one mcts_search, result download, numpy
step), on ONE engine of ONE process, arms interleaved (device, host, device, host, ...).

    python tools/arena_ab.py --out profiles/arena_ab.json

Two checkpoints of Connect4Net (the trained golden blob against bench.py's random-init one), 800 explores, 4,096 and 65,536 random
openings of 8 plies. Per size: 2 warm-up and 6 timed matches per arm, host clock around the call (both arms end in a device
synchronise); median and min-max; a difference counts as resolved only when the medians differ by more than the larger of the two
ranges. The two arms' games are compared move for move once per size. The device arm also reports syn_last_timing's summed kernel time."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ARMS = ("device", "host")


def summary(v):
    return dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4))


def run_size(eng, n, plies, explores, blob_a, blob_b, warmup, timed):
    import numpy as np

    import synthesis_amd as sa
    from synthesis_amd import arena, match

    my, op = arena.random_openings(n, plies, seed=1)
    cfg = sa.parity_mcts_config()
    a = match.Player("A", explores, cfg, weights=blob_a)
    b = match.Player("B", explores, cfg, weights=blob_b)
    times = {k: [] for k in ARMS}
    kernel_ms, got = [], {}
    for i in range(warmup + timed):
        for arm in ARMS:   # interleaved: drift of the box lands on both arms alike
            t0 = time.perf_counter()
            got[arm] = eng.match_run(a, b, blob_a, blob_b, my, op) if arm == "device" else arena.host_match(eng, a, b, my, op)
            dt = time.perf_counter() - t0
            if i >= warmup:
                times[arm].append(dt)
                if arm == "device":
                    kernel_ms.append(eng.last_kernel_ms())
    same = all(np.array_equal(got["device"][k], got["host"][k]) for k in ("rewards", "plies", "moves", "final_bb"))
    rec = dict(openings=n, opening_plies=plies, explores=explores, identical_games=bool(same),
               mean_plies=round(float(got["device"]["plies"].mean()), 2), max_plies=int(got["device"]["plies"].max()),
               seconds={k: summary(times[k]) for k in ARMS}, device_kernel_ms=summary(kernel_ms))
    d, h = rec["seconds"]["device"], rec["seconds"]["host"]
    spread = max(d["max"] - d["min"], h["max"] - h["min"])
    rec["host_minus_device"] = dict(median=round(h["median"] - d["median"], 4), larger_min_max_range=round(spread, 4),
                                    resolved=bool(abs(h["median"] - d["median"]) > spread))
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[4096, 65536])
    ap.add_argument("--opening-plies", type=int, default=8)
    ap.add_argument("--explores", type=int, default=800)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--timed", type=int, default=6)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.timed < 6:
        raise SystemExit("--timed must be at least 6: fewer matches per arm do not give a range worth comparing")

    import numpy as np
    import torch  # noqa: F401  (before the engine: one HIP runtime per process)

    import bench
    import synthesis_amd as sa

    blob_a = np.load(os.path.join(ROOT, "tests", "golden", "c4net_trained_f32.npy")).astype(np.float32).ravel()
    blob_b = bench.make_weights()
    sizes = []
    for n in args.sizes:
        with sa.Engine(concurrent_games=min(n, 65536), max_explores=args.explores, device=args.device) as eng:
            sizes.append(run_size(eng, n, args.opening_plies, args.explores, blob_a, blob_b, args.warmup, args.timed))
        print(json.dumps(sizes[-1]), flush=True)
    rec = dict(tool="tools/arena_ab.py", kernel_source_hash=bench.kernel_source_hash(), device=torch.cuda.get_device_name(args.device),
               players="Connect4Net f32: tests/golden/c4net_trained_f32.npy (first) against bench.make_weights() (second), parity configuration",
               timing="host clock (time.perf_counter) around Engine.match_run / arena.host_match; both return after a device synchronise",
               order="device, host, device, host, ... on one engine of one process",
               warmup_matches=args.warmup, timed_matches=args.timed, date=time.strftime("%Y-%m-%d"), sizes=sizes)
    print(json.dumps(rec), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
