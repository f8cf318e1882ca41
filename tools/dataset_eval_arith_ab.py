#!/usr/bin/env python3
"""A/B of the held-out evaluation's arithmetics (Engine.dataset_evaluate(arith=...)), tools/reanalyse_ab.py's protocol: ONE engine per
network in ONE process, the arms interleaved (A B C D A B C D ...), two warm-up runs and --timed (default 6) timed runs per arm, per arm
the median and min/max of the wall time (host clock around the arm's calls, which end in a device synchronise).

    python tools/dataset_eval_arith_ab.py --out profiles/dataset_eval_arith_ab.json

Rows: 1,048,576 recorded self-play positions drawn with repetition (tools/dataset_eval_ab.py's data set), both networks, the trainer's
weights on the learner's data set. Arms:
    f32           dataset_evaluate("train", arith="f32")
    f16x2         dataset_evaluate("train", arith="f16x2"): the f16x2 image is built on the host per call — the difference between the host
                  clock and syn_last_timing's device time of the two launches shows it
    bf16          Connect4ConvNet only: arith="bf16"
    parent_f16x2  the route a caller had before arith= for f16x2 outputs on a data set: set_network_arithmetic("f16x2") (builds the
                  engine's image, empties the policy cache), policy_eval_device over the rows, download of logits and value
                  probabilities, a numpy head (policy: log-softmax and KL in f32; value: KL from the returned probabilities), switch back.
                  It changes what the engine's self-play runs while it observes, and it has no raw value outputs.
A gap is called resolved only when the medians differ by more than the larger of the two arms' min-max ranges. No speed is promised."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.dataset_eval_ab import N_POSITIONS, compare, data_set, summary  # noqa: E402


def numpy_head(logits, value, tpi, tv):
    """(mean policy KL, mean value KL) as a caller computes them from policy_eval's outputs"""
    with np.errstate(divide="ignore", invalid="ignore"):
        z = logits - logits.max(axis=1, keepdims=True)
        logp = z - np.log(np.exp(z).sum(axis=1, keepdims=True, dtype=np.float32))
        klp = np.where(tpi > 0, tpi * (np.log(np.where(tpi > 0, tpi, 1)) - logp), 0).sum(axis=1, dtype=np.float64)
        klv = np.where(tv > 0, tv * (np.log(np.where(tv > 0, tv, 1)) - np.log(value)), 0).sum(axis=1, dtype=np.float64)
    return float(klp.mean()), float(klv.mean())


def run_network(sa, torch, args, net, d):
    from bench import make_conv_weights, make_weights

    w = make_weights() if net == "mlp" else make_conv_weights()
    arms = ("f32", "f16x2") + (("bf16",) if net == "conv" else ()) + ("parent_f16x2",)
    dev = torch.device(f"cuda:{args.device}")
    with sa.Engine(concurrent_games=64, max_explores=64, device=args.device) as eng:
        (eng.load_weights if net == "mlp" else eng.load_weights_conv)(w)
        (eng.trainer_init if net == "mlp" else eng.trainer_init_conv)(w)
        eng.train_set_data(d["my"], d["op"], d["pi"], d["v"])
        d_my = torch.from_numpy(d["my"].astype(np.int64)).to(dev); d_op = torch.from_numpy(d["op"].astype(np.int64)).to(dev)
        d_lg = torch.zeros((N_POSITIONS, 9), dtype=torch.float32, device=dev); d_v = torch.zeros((N_POSITIONS, 3), dtype=torch.float32, device=dev)
        torch.cuda.synchronize(args.device)

        def arm_evaluate(arith):
            m = eng.dataset_evaluate("train", arith=arith)
            return dict(mean_pi=m["mean_pi"], mean_v=m["mean_v"], device_ms=eng.last_timing()[0], grid=m["grid"])

        def arm_parent():
            eng.set_network_arithmetic("f16x2")
            eng.policy_eval_device(d_my.data_ptr(), d_op.data_ptr(), N_POSITIONS, d_lg.data_ptr(), d_v.data_ptr())
            ms = eng.last_timing()[0]
            lg, v = d_lg.cpu().numpy(), d_v.cpu().numpy()
            mp, mv = numpy_head(lg, v, d["pi"], d["v"])
            eng.set_network_arithmetic("f32")
            return dict(mean_pi=mp, mean_v=mv, device_ms=ms)

        times = {a: [] for a in arms}; dev_ms = {a: [] for a in arms}; last = {}
        for run in range(args.warmup + args.timed):
            for arm in arms:
                torch.cuda.synchronize(args.device)
                t0 = time.perf_counter()
                r = arm_parent() if arm == "parent_f16x2" else arm_evaluate(arm)
                dt = time.perf_counter() - t0
                last[arm] = r
                if run >= args.warmup:
                    times[arm].append(dt); dev_ms[arm].append(r["device_ms"])
    out = dict(network="Connect4Net" if net == "mlp" else "Connect4ConvNet", rows=N_POSITIONS, arms=list(arms),
               seconds={a: summary(times[a]) for a in arms}, seconds_all={a: [round(x, 6) for x in times[a]] for a in arms},
               device_ms={a: summary(dev_ms[a]) for a in arms},
               host_minus_device_ms={a: round(1e3 * statistics.median(times[a]) - statistics.median(dev_ms[a]), 3) for a in arms},
               means={a: [last[a]["mean_pi"], last[a]["mean_v"]] for a in arms}, grid={a: last[a].get("grid") for a in arms if a != "parent_f16x2"})
    s = out["seconds"]
    out["positions_per_second"] = {a: round(N_POSITIONS / s[a]["median"]) for a in arms}
    out["comparisons"] = [compare(s[a], s["f32"], a, "f32") for a in arms if a != "f32"] + [compare(s["parent_f16x2"], s["f16x2"], "parent_f16x2", "f16x2")]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--timed", type=int, default=6)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.timed < 6:
        raise SystemExit("--timed must be at least 6: fewer runs per arm do not give a range worth comparing")

    import torch  # (before the engine: one HIP runtime per process)

    import bench
    import synthesis_amd as sa

    rec = dict(tool="tools/dataset_eval_arith_ab.py", kernel_source_hash=bench.kernel_source_hash(), device=torch.cuda.get_device_name(args.device),
               timing="host clock (time.perf_counter) around an arm's calls, which end in a device synchronise; device_ms = syn_last_timing "
                      "of the arm's launches (parent_f16x2: the policy evaluation alone)",
               order="one process, one engine per network, arms interleaved, 2 warm-up runs per arm", timed_runs=args.timed,
               date=time.strftime("%Y-%m-%d"),
               not_measured=["any training run judged in these arithmetics", "the learning loop's iteration time with extra arithmetics",
                             "more than one GPU", "a cached f16x2 image across calls"])
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "rows.npz")
        recorded = data_set(sa, args.device, path)
        d = dict(np.load(path))
    rec["data_set"] = dict(positions=N_POSITIONS, recorded_positions_drawn_from=recorded)
    rec["evaluation"] = []
    for net in ("mlp", "conv"):
        rec["evaluation"].append(run_network(sa, torch, args, net, d))
        print(json.dumps(rec["evaluation"][-1]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
