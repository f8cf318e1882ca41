#!/usr/bin/env python3
"""A/B of the device-resident match with a baseline side (match.play_match_device = Engine.match_run_sides = syn_match_run_sides)
against the host path of match.play_match on identical games, on ONE engine of ONE process, arms interleaved (host, device, host, ...).

    python tools/match_sides_ab.py --out profiles/match_sides_ab.json

Arm A: match.play_match — per ply the positions, seeds and stream positions go up, one syn_frozen_result per root (or one
syn_search_result) comes down, numpy steps the boards. Arm B: match.play_match_device — one call, four words read back per ply.
Workloads, from the empty board, game g on StdRng::seed_from_u64(g):
  vanilla     VanillaMCTS800 against VanillaMCTS200 (mcts_vs_mcts), at the size tools/vanilla_bench.py uses (16,384 games)
  checkpoint  the trained golden Connect4Net checkpoint, 800 explores, parity configuration, against VanillaMCTS800
              (eval_against_rollout_mcts), 4,096 games
Per workload: the two arms' games are asserted identical (moves, rewards, plies, stream positions) before anything is timed; then 2
warm-up and 6 timed matches per arm, host clock around the call (both arms end in a device synchronise); median and min-max; a
difference counts as resolved only when the medians differ by more than the larger of the two ranges."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ARMS = ("host", "device")


def summary(v):
    return dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4))


def run_workload(eng, name, first, second, games, warmup, timed):
    import numpy as np

    from synthesis_amd import match

    def play(arm):
        rec = {}
        fn = match.play_match if arm == "host" else match.play_match_device
        t0 = time.perf_counter()
        reward, plies = fn(eng, first, second, games, seed=0, record=rec)
        return time.perf_counter() - t0, reward, plies, rec

    _, r_h, p_h, rec_h = play("host")
    _, r_d, p_d, rec_d = play("device")
    same = (np.array_equal(r_h, r_d) and np.array_equal(p_h, p_d) and np.array_equal(rec_h["moves"], rec_d["moves"]) and
            np.array_equal(rec_h["rng_words"], rec_d["rng_words"]))
    assert same, f"{name}: the two arms played different games"
    times = {k: [] for k in ARMS}
    kernel_ms = []
    for i in range(warmup + timed):
        for arm in ARMS:   # interleaved: drift of the box lands on both arms alike
            dt = play(arm)[0]
            if i >= warmup:
                times[arm].append(dt)
                if arm == "device":
                    kernel_ms.append(eng.last_kernel_ms())
    w, d, l, s, _ = match.score(r_d)
    rec = dict(workload=name, first=first.name, second=second.name, games=games, identical_games=bool(same),
               mean_plies=round(float(p_d.mean()), 2), first_player_score=round(s, 4), wins=w, draws=d, losses=l,
               seconds={k: summary(times[k]) for k in ARMS}, device_kernel_ms=summary(kernel_ms),
               matches_per_second={k: round(games / statistics.median(times[k])) for k in ARMS})
    h, dv = rec["seconds"]["host"], rec["seconds"]["device"]
    spread = max(dv["max"] - dv["min"], h["max"] - h["min"])
    rec["host_minus_device"] = dict(median=round(h["median"] - dv["median"], 4), larger_min_max_range=round(spread, 4),
                                    resolved=bool(abs(h["median"] - dv["median"]) > spread))
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--vanilla-games", type=int, default=16384)
    ap.add_argument("--checkpoint-games", type=int, default=4096)
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
    from synthesis_amd import match

    blob = np.load(os.path.join(ROOT, "tests", "golden", "c4net_trained_f32.npy")).astype(np.float32).ravel()
    net = match.Player("c4net_trained_f32", args.explores, sa.parity_mcts_config(), weights=blob)
    workloads = []
    for name, first, second, games in (("vanilla", match.vanilla_player(800), match.vanilla_player(200), args.vanilla_games),
                                       ("checkpoint", net, match.vanilla_player(800), args.checkpoint_games)):
        with sa.Engine(concurrent_games=games, max_explores=args.explores, device=args.device) as eng:
            workloads.append(run_workload(eng, name, first, second, games, args.warmup, args.timed))
        print(json.dumps(workloads[-1]), flush=True)
    rec = dict(tool="tools/match_sides_ab.py", kernel_source_hash=bench.kernel_source_hash(), device=torch.cuda.get_device_name(args.device),
               arms="host = match.play_match (per-ply uploads, result downloads, numpy steps); device = match.play_match_device (one "
                    "Engine.match_run_sides call)",
               timing="host clock (time.perf_counter) around the call; both return after a device synchronise",
               order="host, device, host, device, ... on one engine of one process",
               warmup_matches=args.warmup, timed_matches=args.timed, date=time.strftime("%Y-%m-%d"), workloads=workloads)
    print(json.dumps(rec), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
