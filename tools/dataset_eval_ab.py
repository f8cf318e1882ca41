#!/usr/bin/env python3
"""A/B of the held-out evaluation (Engine.dataset_evaluate) and of the holdout split.

    python tools/dataset_eval_ab.py --parent-lib <libsynthesis_amd.so built from the parent commit> --out profiles/dataset_eval_ab.json

Leg 1, per network: the losses of one checkpoint on 1,048,576 rows (recorded self-play positions drawn with repetition, as
tools/train_batch_ab.py builds them).
    A_evaluate       this tree: Engine.dataset_evaluate("train") with the trainer's weights — forward only, nothing changes
    B_parent_epoch   the parent's only route to the same numbers: one Engine.train_epoch over the rows in order at batch 4,096 in
                     SYN_TRAIN_BATCH_MICRO with lr = 0, on a library built from the parent commit (SYNTHESIS_AMD_LIB). It runs the whole
                     backward pass and advances Adam's moments and step count: it disturbs the run it observes.
The two arms need two libraries, so every run is a process of its own (engine, trainer, upload, one warm-up call, ONE timed call); the
driver starts them interleaved, A, B, A, B, ... The timed region is the host clock around the one call, which ends in a device
synchronise; A also reports syn_last_timing's device time.
Leg 2: Engine.replay_deduplicate_to_trainer on one buffer of 65,536 self-play games (tools/replay_symmetry_ab.py's games per iteration;
played at 64 explores, the buffer's size is what the call sees) without a holdout and with 5 % of the games held out, one engine,
interleaved; the timed region ends when the device is idle (without a holdout the call returns while its reduce and copies are enqueued).
Protocol of tools/arena_ab.py: at least 6 timed runs per arm, median (min-max) per arm, and a difference counts as resolved only when the
medians differ by more than the larger of the two arms' ranges."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_POSITIONS = 1 << 20
BATCH = 4096
SPLIT_GAMES, SPLIT_EXPLORES, SPLIT_FRACTION = 65536, 64, 0.05


def summary(v):
    return dict(median=round(statistics.median(v), 6), min=round(min(v), 6), max=round(max(v), 6))


def compare(a, b, name_a, name_b):
    spread = max(a["max"] - a["min"], b["max"] - b["min"])
    d = a["median"] - b["median"]
    return dict(minuend=name_a, subtrahend=name_b, median_difference=round(d, 6), larger_min_max_range=round(spread, 6),
                resolved=bool(abs(d) > spread))


def trainer(eng, net):
    from bench import make_conv_weights, make_weights

    (eng.trainer_init if net == "mlp" else eng.trainer_init_conv)(make_weights() if net == "mlp" else make_conv_weights())


def child(args):
    """one run of one arm: prints one JSON line"""
    import torch  # (before the engine: one HIP runtime per process)

    import synthesis_amd as sa

    if args.child == "make_data":
        print("CHILD " + json.dumps(dict(recorded=data_set(sa, args.device, args.data), device=torch.cuda.get_device_name(args.device))), flush=True)
        return
    if args.child == "split":
        print("CHILD " + json.dumps(run_split(sa, args)), flush=True)
        return
    d = np.load(args.data)
    with sa.Engine(concurrent_games=64, max_explores=64, device=args.device) as eng:
        trainer(eng, args.net)
        eng.train_set_data(d["my"], d["op"], d["pi"], d["v"])
        out = dict(arm=args.child, net=args.net)
        if args.child == "A_evaluate":
            eng.dataset_evaluate("train")
            t0 = time.perf_counter()
            m = eng.dataset_evaluate("train")
            out.update(seconds=time.perf_counter() - t0, device_ms=eng.last_timing()[0], mean_pi=m["mean_pi"], mean_v=m["mean_v"], grid=m["grid"])
        else:
            eng.trainer_set_batch_mode("micro")
            perm = np.arange(N_POSITIONS, dtype=np.int32)
            eng.train_epoch(perm, BATCH, 0.0)
            t0 = time.perf_counter()
            losses = eng.train_epoch(perm, BATCH, 0.0)
            dt = time.perf_counter() - t0
            mean = losses.astype(np.float64).mean(axis=0)
            out.update(seconds=dt, mean_pi=float(mean[0]), mean_v=float(mean[1]), optimiser_step_count_after=eng.trainer_state()["step"])
    print("CHILD " + json.dumps(out), flush=True)


def data_set(sa, device, path, seed=7):
    from bench import make_weights

    eng = sa.Engine(concurrent_games=4096, max_explores=64, device=device)
    eng.load_weights(make_weights())
    r = eng.selfplay(sa.parity_rollout_config(64), base_seed=seed, n_games=4096)
    eng.close()
    keep = np.arange(63)[None, :] < r["plies"][:, None]
    my, op, pi, v = r["states_bb"][..., 0][keep], r["states_bb"][..., 1][keep], r["pis"][keep], r["vs"][keep]
    pick = np.random.default_rng(seed).integers(0, my.size, size=N_POSITIONS)
    np.savez(path, my=my[pick], op=op[pick], pi=pi[pick], v=v[pick])
    return int(my.size)


def start_child(args, arm, net, data_path):
    """a fresh process (the driver itself never opens the device); its one JSON line"""
    env = dict(os.environ)
    env.pop("SYNTHESIS_AMD_LIB", None)
    if arm == "B_parent_epoch":
        env["SYNTHESIS_AMD_LIB"] = os.path.abspath(args.parent_lib)
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", arm, "--net", net, "--data", data_path, "--device", str(args.device),
                        "--warmup", str(args.warmup), "--timed", str(args.timed)], env=env, capture_output=True, text=True, timeout=900)
    if p.returncode != 0:   # nothing more is started on the device after a failed run
        raise SystemExit(f"{arm} ({net}) ended with status {p.returncode}:\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")
    return json.loads([l for l in p.stdout.splitlines() if l.startswith("CHILD ")][-1][6:])


def run_children(args, net, data_path):
    arms = ("A_evaluate", "B_parent_epoch")
    runs = {a: [] for a in arms}
    for _ in range(args.timed):
        for arm in arms:
            runs[arm].append(start_child(args, arm, net, data_path))
    out = dict(network="Connect4Net" if net == "mlp" else "Connect4ConvNet", rows=N_POSITIONS, parent_batch=BATCH,
               seconds={a: summary([r["seconds"] for r in runs[a]]) for a in arms},
               seconds_all={a: [round(r["seconds"], 6) for r in runs[a]] for a in arms},
               A_device_ms=summary([r["device_ms"] for r in runs["A_evaluate"]]), A_grid=runs["A_evaluate"][0]["grid"],
               means=dict(A=[runs["A_evaluate"][0]["mean_pi"], runs["A_evaluate"][0]["mean_v"]],
                          B=[runs["B_parent_epoch"][0]["mean_pi"], runs["B_parent_epoch"][0]["mean_v"]]),
               B_optimiser_step_count_after_warmup_and_timed_call=runs["B_parent_epoch"][0]["optimiser_step_count_after"])
    s = out["seconds"]
    out["positions_per_second"] = {a: round(N_POSITIONS / s[a]["median"]) for a in arms}
    out["B_minus_A"] = compare(s["B_parent_epoch"], s["A_evaluate"], "B_parent_epoch", "A_evaluate")
    return out


def run_split(sa, args):
    import torch

    from bench import make_weights

    from synthesis_amd.learner import _holdout_key

    arms = ("no_holdout", "holdout_5_percent")
    threshold = int(np.floor(SPLIT_FRACTION * 4294967296.0))
    with sa.Engine(concurrent_games=SPLIT_GAMES, max_explores=SPLIT_EXPLORES, device=args.device) as eng:
        blob = make_weights()
        eng.load_weights(blob)
        eng.trainer_init(blob)
        eng.replay_reserve(SPLIT_GAMES * 63)
        eng.selfplay(sa.parity_rollout_config(SPLIT_EXPLORES), base_seed=7, n_games=SPLIT_GAMES, outputs=False)
        n = eng.replay_append_selfplay(0)
        times = {a: [] for a in arms}
        sizes = {}
        for run in range(args.warmup + args.timed):
            for arm in arms:
                eng.replay_set_holdout(_holdout_key(7), threshold if arm == arms[1] else 0)
                torch.cuda.synchronize(args.device)
                t0 = time.perf_counter()
                unique = eng.replay_deduplicate_to_trainer()
                torch.cuda.synchronize(args.device)   # (without a holdout the call returns with its second half still enqueued)
                dt = time.perf_counter() - t0
                if run >= args.warmup:
                    times[arm].append(dt)
                sizes[arm] = dict(learner_rows=unique, evaluation_rows=eng.dataset_counts()[0] if arm == arms[1] else 0,
                                  unseen_rows=eng.dataset_counts()[1] if arm == arms[1] else 0)
        eng.replay_set_holdout(0, 0)
    out = dict(buffer_positions=n, games=SPLIT_GAMES, explores=SPLIT_EXPLORES, sizes=sizes, seconds={a: summary(times[a]) for a in arms},
               seconds_all={a: [round(x, 6) for x in times[a]] for a in arms})
    out["holdout_minus_none"] = compare(out["seconds"][arms[1]], out["seconds"][arms[0]], arms[1], arms[0])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default="", help="libsynthesis_amd.so built from the parent commit (leg 1's arm B)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--timed", type=int, default=6)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default="")
    ap.add_argument("--scratch", default="", help="where the leg-1 data set is kept between the runs (default: a temporary directory)")
    ap.add_argument("--child", default="", help=argparse.SUPPRESS)
    ap.add_argument("--net", default="mlp", help=argparse.SUPPRESS)
    ap.add_argument("--data", default="", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    if args.timed < 6:
        raise SystemExit("--timed must be at least 6: fewer runs per arm do not give a range worth comparing")
    if not args.parent_lib or not os.path.exists(args.parent_lib):
        raise SystemExit("--parent-lib: build the parent commit's library first (make -C synthesis_amd/csrc in a checkout of it)")

    import tempfile

    import bench

    rec = dict(tool="tools/dataset_eval_ab.py", kernel_source_hash=bench.kernel_source_hash(),
               timing="host clock (time.perf_counter) around one call that ends in a device synchronise (leg 2: followed by one)",
               order="leg 1: one process per run, A, B, A, B, ... per network; leg 2: one engine, arms interleaved, 2 warm-up runs",
               timed_runs=args.timed, date=time.strftime("%Y-%m-%d"),
               not_measured=["any training run judged with the held-out metrics", "more than one GPU"])
    rec["holdout_split"] = start_child(args, "split", "mlp", "-")
    print(json.dumps(rec["holdout_split"]), flush=True)
    with tempfile.TemporaryDirectory(dir=args.scratch or None) as tmp:
        path = os.path.join(tmp, "rows.npz")
        made = start_child(args, "make_data", "mlp", path)
        rec["device"] = made["device"]
        rec["data_set"] = dict(positions=N_POSITIONS, recorded_positions_drawn_from=made["recorded"])
        rec["evaluation"] = []
        for net in ("mlp", "conv"):
            rec["evaluation"].append(run_children(args, net, path))
            print(json.dumps(rec["evaluation"][-1]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
