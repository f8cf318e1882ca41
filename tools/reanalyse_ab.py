#!/usr/bin/env python3
"""A/B of reanalysing a replay buffer: the route over the host against Engine.replay_reanalyse, on ONE engine of ONE process, interleaved
(A B A B ...), both arms starting from the same buffer.

    arm A (host)    replay_read -> learner.reanalyse_flags -> Engine.mcts_search over the selected rows -> replay_clear + replay_append
    arm B (device)  Engine.replay_reanalyse

    python tools/reanalyse_ab.py --out profiles/reanalyse_ab.json --first-results profiles/reanalyse_first_results.txt

The buffer is the positions of --games (65,536) self-played games at --explores (200); the reanalysis runs at the same explores with
another network (the trained golden checkpoint), pi and v rewritten (value_mix 1), for the fractions 1/16 and 1/2. Before every run the buffer is restored from a host copy
(not timed). Two warm-up runs per arm, then --timed (default 6) timed runs per arm; per arm the median and min/max of the wall time
(host clock around the arm's calls, which end in a device synchronise). A gap is "resolved" only when the medians differ by more than
the larger of the two arms' ranges. The two arms' buffers are compared bit for bit: an A/B of two different results is void. For the
device arm syn_last_timing gives the summed device time of its search launches; what is left of the wall time is everything else.

--first-results writes a description (no claim about strength) of what a reanalysis does to a buffer played by the random-init golden
network: moved / selected when reanalysed with the trained golden network and with the network that played it (the fixed point: 0), and
the trained network's losses (Engine.dataset_evaluate) on the targets before and after."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FRACTIONS = (("1/16", 1 / 16), ("1/2", 1 / 2))
KEY = 0x5EED


def restore(eng, R):
    eng.replay_clear()
    eng.replay_append(R["my"], R["op"], R["gid"], R["pi"], R["v"])


def same_buffer(a, b):
    return all(np.array_equal(np.ascontiguousarray(a[k]).view(np.uint8), np.ascontiguousarray(b[k]).view(np.uint8)) for k in a)


def arm_host(eng, cfg, explores, threshold):
    from synthesis_amd.learner import reanalyse_flags

    R = eng.replay_read()
    rows = np.flatnonzero(reanalyse_flags(KEY, threshold, None, R["gid"], R["my"], R["op"]))
    res = eng.mcts_search(cfg, R["my"][rows], R["op"][rows], explores)
    R["pi"][rows] = res["target_pi"]
    R["v"][rows] = res["target_q"]
    eng.replay_clear()
    eng.replay_append(R["my"], R["op"], R["gid"], R["pi"], R["v"])
    return int(rows.size), eng.last_timing()[0]


def arm_device(eng, cfg, explores, threshold):
    st = eng.replay_reanalyse(cfg, explores, KEY, threshold=threshold, value_mix=1.0)
    return st["selected"], eng.last_timing()[0]


def run_fraction(eng, cfg, explores, R0, frac, warmup, timed):
    threshold = int(np.floor(frac * 4294967296.0))
    arms = (("host", arm_host), ("device", arm_device))
    wall = {a: [] for a, _ in arms}
    search_ms = {a: [] for a, _ in arms}
    result, selected = {}, {}
    for i in range(warmup + timed):
        for name, fn in arms:   # interleaved: drift of the box lands on both arms alike
            restore(eng, R0)
            t = time.perf_counter()
            n, ms = fn(eng, cfg, explores, threshold)
            dt = time.perf_counter() - t
            if i >= warmup:
                wall[name].append(dt)
                search_ms[name].append(ms)
            if i == warmup + timed - 1:
                result[name] = eng.replay_read()
                selected[name] = n
    out = dict(fraction=frac, threshold=threshold, selected=selected["device"],
               arms_computed_the_same=bool(selected["host"] == selected["device"] and same_buffer(result["host"], result["device"])),
               targets_changed=not same_buffer(result["device"], R0))
    for name, _ in arms:
        w = wall[name]
        out[name] = dict(wall_seconds=dict(median=round(statistics.median(w), 4), min=round(min(w), 4), max=round(max(w), 4)),
                         wall_seconds_per_run=[round(x, 4) for x in w],
                         search_kernel_seconds_median=round(statistics.median(search_ms[name]) / 1e3, 4))
    h, d = out["host"]["wall_seconds"], out["device"]["wall_seconds"]
    spread = max(h["max"] - h["min"], d["max"] - d["min"])
    out["median_wall_host_minus_device"] = round(h["median"] - d["median"], 4)
    out["larger_min_max_range"] = round(spread, 4)
    out["resolved"] = bool(abs(h["median"] - d["median"]) > spread)
    not_search = [w - ms / 1e3 for w, ms in zip(wall["device"], search_ms["device"])]
    out["device_arm_not_search"] = dict(seconds_median=round(statistics.median(not_search), 4),
                                        share_of_wall_median=round(statistics.median(n / w for n, w in zip(not_search, wall["device"])), 4))
    return out


def first_results(eng, path, games, explores):
    import synthesis_amd as sa

    gold = os.path.join(ROOT, "tests", "golden")
    init, trained = np.load(os.path.join(gold, "c4net_blob_f32.npy")), np.load(os.path.join(gold, "c4net_trained_f32.npy"))
    rcfg = sa.parity_rollout_config(explores)
    eng.load_weights(init)
    eng.selfplay(rcfg, base_seed=11, n_games=games, outputs=False)
    eng.replay_clear()
    eng.replay_append_selfplay(0)
    R0 = eng.replay_read()
    full = 1 << 32
    lines = ["Reanalyse, first results (tools/reanalyse_ab.py --first-results). Descriptions of what the call does to targets;",
             "nothing here says anything about playing strength, and no training run with reanalysis has been made.",
             "",
             f"buffer: {R0['my'].size} positions of {games} games self-played by tests/golden/c4net_blob_f32.npy (random init) at {explores} explores,",
             "parity configuration (value_target = Q, no noise); every row reanalysed (threshold 2^32) at the same explores, value_mix 1", ""]

    def losses(R):
        eng.dataset_set(R["my"], R["op"], R["pi"], R["v"])
        m = eng.dataset_evaluate("eval", blob=trained)
        return f"mean_pi {m['mean_pi']:.6f}  mean_v {m['mean_v']:.6f}  pi_acc {m['pi_acc']:.4f}  v_acc {m['v_acc']:.4f}  rows {m['rows']}"

    lines.append("losses of tests/golden/c4net_trained_f32.npy on the stored targets (Engine.dataset_evaluate, all rows, not de-duplicated):")
    lines.append("  before:                                  " + losses(R0))
    st = eng.replay_reanalyse(rcfg.mcts_cfg, explores, KEY, threshold=full, action_selection=int(rcfg.action), value_mix=1.0)
    same = same_buffer(eng.replay_read(), R0)
    lines.insert(6, f"reanalysed with the network that played it:  moved {st['moved']} / selected {st['selected']}"
                    f"  (buffer bit for bit unchanged: {same}; the fixed point, must be 0 and True)")
    eng.load_weights(trained)
    restore(eng, R0)
    st = eng.replay_reanalyse(rcfg.mcts_cfg, explores, KEY, threshold=full, action_selection=int(rcfg.action), value_mix=1.0)
    lines.insert(7, f"reanalysed with c4net_trained_f32.npy:       moved {st['moved']} / selected {st['selected']}"
                    f" = {st['moved'] / max(st['selected'], 1):.4f}")
    lines.insert(8, "")
    lines.append("  after reanalysis with the trained network: " + losses(eng.replay_read()))
    lines.append("(the targets after are the trained network's own searches: a description of the relabelling, not a measure of quality)")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=65536)
    ap.add_argument("--explores", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--timed", type=int, default=6)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default="")
    ap.add_argument("--first-results", default="", help="write the first-results description to this file")
    ap.add_argument("--first-results-games", type=int, default=4096)
    args = ap.parse_args()
    if args.timed < 6:
        raise SystemExit("--timed must be at least 6: fewer runs per arm do not give a range worth comparing")

    import torch  # noqa: F401  (before the engine: one HIP runtime per process)

    import bench
    import synthesis_amd as sa

    blob = bench.make_weights()
    rcfg = sa.parity_rollout_config(args.explores)
    rec = dict(tool="tools/reanalyse_ab.py", kernel_source_hash=bench.kernel_source_hash(), device=torch.cuda.get_device_name(args.device),
               timing="host clock (time.perf_counter) around an arm's calls, which end in a device synchronise; restoring the buffer "
                      "before a run is not timed",
               order="host, device, host, device, ... on one engine of one process",
               arms=dict(host="replay_read -> reanalyse_flags -> Engine.mcts_search -> replay_clear + replay_append",
                         device="Engine.replay_reanalyse"),
               games=args.games, explores=args.explores, warmup_runs=args.warmup, timed_runs=args.timed, date=time.strftime("%Y-%m-%d"),
               not_measured=["any training run with reanalysis", "more than one rank (the other ranks idle during the learner's reanalysis)",
                             "playing strength"],
               fractions={})
    with sa.Engine(concurrent_games=min(args.games, 65536), max_explores=args.explores, device=args.device) as eng:
        eng.load_weights(blob)
        eng.selfplay(rcfg, base_seed=7, n_games=args.games, outputs=False)
        eng.replay_reserve(args.games * 63)
        eng.replay_append_selfplay(0)
        R0 = eng.replay_read()
        # the reanalysing network is another one than the one that played: with the same one every target would be its own fixed point
        eng.load_weights(np.load(os.path.join(ROOT, "tests", "golden", "c4net_trained_f32.npy")))
        rec["networks"] = dict(played_by="bench.make_weights()", reanalysed_with="tests/golden/c4net_trained_f32.npy")
        rec["buffer_positions"] = int(R0["my"].size)
        rec["buffer_bytes"] = int(R0["my"].size) * 72
        for name, frac in FRACTIONS:
            rec["fractions"][name] = run_fraction(eng, rcfg.mcts_cfg, args.explores, R0, frac, args.warmup, args.timed)
            print(json.dumps({name: rec["fractions"][name]}), flush=True)
        if args.first_results:
            first_results(eng, args.first_results, args.first_results_games, args.explores)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
