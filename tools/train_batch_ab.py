#!/usr/bin/env python3
"""A/B of the learner's epoch throughput across batch definitions: the micro-batch step (SYN_TRAIN_BATCH_MICRO) at B = 256, 1024 and
4096 in the in-tree library against the baselines of a library built at the parent commit, in ONE process, arms interleaved.

    SYNTHESIS_AMD_LIB=/path/to/parent/libsynthesis_amd.so python tools/train_batch_ab.py --out profiles/train_micro_batch_ab.json

SYNTHESIS_AMD_LIB names the baseline library here (it is taken out of the environment before the package loads, so the new arms run the
in-tree build). Baseline arms: batch 32 through the persistent epoch kernel, and for Connect4Net batch 4,096 in the chained definition
(one workgroup walks the 128 chunks). Every arm trains on the same 1,048,576 positions (recorded self-play positions, drawn with
repetition), one epoch = one syn_train_epoch call over a permutation of all of them (the same permutation for every arm of a round).
Protocol of tools/replay_loop_ab.py: two warm-up and six timed epochs per arm, median and min-max per arm, and a difference counts as
resolved only where the medians differ by more than the larger of the two arms' ranges. The time is the host clock around
Engine.train_epoch, which returns after the epoch's one synchronisation."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_POSITIONS = 1 << 20
MICRO_BATCHES = (256, 1024, 4096)


def engine_on_library(sa, lib_path, device):
    """An Engine whose calls go to another build of the library (same ABI for everything the arms use): its own ctypes handle, the
    prototypes copied from the in-tree binding for every symbol that build exports."""
    from synthesis_amd.config import CEngineConfig
    from synthesis_amd.engine import ABI_SYMBOLS, load_library

    cur = load_library()
    lib = C.CDLL(lib_path)
    for name in ABI_SYMBOLS:
        if hasattr(lib, name):
            getattr(lib, name).argtypes = getattr(cur, name).argtypes
            getattr(lib, name).restype = getattr(cur, name).restype
    eng = sa.Engine.__new__(sa.Engine)
    eng._lib, eng._h = lib, C.c_void_p()
    cfg = CEngineConfig(64, 64, 0, 0)
    rc = lib.syn_engine_create(C.byref(cfg), int(device), C.byref(eng._h))
    if rc != 0:
        raise SystemExit(f"baseline library: syn_engine_create failed ({rc})")
    eng.concurrent_games, eng.max_explores, eng.device, eng._net_params = 64, 64, int(device), None
    return eng


def data_set(sa, device, seed=7):
    """1,048,576 positions with their targets: the recorded positions of 4,096 self-play games, drawn with repetition."""
    from bench import make_weights

    eng = sa.Engine(concurrent_games=4096, max_explores=64, device=device)
    eng.load_weights(make_weights())
    r = eng.selfplay(sa.parity_rollout_config(64), base_seed=seed, n_games=4096)
    eng.close()
    keep = np.arange(63)[None, :] < r["plies"][:, None]
    my, op, pi, v = r["states_bb"][..., 0][keep], r["states_bb"][..., 1][keep], r["pis"][keep], r["vs"][keep]
    pick = np.random.default_rng(seed).integers(0, my.size, size=N_POSITIONS)
    return dict(my=my[pick], op=op[pick], pi=pi[pick], v=v[pick], recorded=int(my.size))


def run_network(sa, net, base_lib, data, warmup, timed, device):
    from bench import make_conv_weights, make_weights

    blob = make_weights() if net == "mlp" else make_conv_weights()
    arms = {}   # name -> (engine, batch, launches per step, description)

    def add(name, eng, batch, mode, launches):
        (eng.trainer_init if net == "mlp" else eng.trainer_init_conv)(blob)
        if mode == "micro":
            eng.trainer_set_batch_mode("micro")
        eng.train_set_data(data["my"], data["op"], data["pi"], data["v"])
        arms[name] = dict(engine=eng, batch=batch, mode=mode, launches=launches, seconds=[])

    add("baseline_b32_persistent", engine_on_library(sa, base_lib, device), 32, "chained", "1 per epoch (the persistent epoch kernel)")
    if net == "mlp":
        add("baseline_b4096_chained", engine_on_library(sa, base_lib, device), 4096, "chained", "2 per step (gradients on one workgroup, Adam)")
    for B in MICRO_BATCHES:
        add(f"micro_b{B}", sa.Engine(concurrent_games=64, max_explores=64, device=device), B, "micro", "3 per step (blocks, reduce, Adam)")
    rng = np.random.default_rng(11)
    for it in range(warmup + timed):
        perm = rng.permutation(N_POSITIONS).astype(np.int32)
        for a in arms.values():   # interleaved: drift of the box lands on every arm alike
            t0 = time.perf_counter()
            losses = a["engine"].train_epoch(perm, a["batch"], 1e-3)
            dt = time.perf_counter() - t0
            assert losses.shape == (N_POSITIONS // a["batch"], 2) and np.isfinite(losses).all()
            if it >= warmup:
                a["seconds"].append(dt)
    out = {}
    for name, a in arms.items():
        s = a["seconds"]
        out[name] = dict(batch=a["batch"], mode=a["mode"], steps_per_epoch=N_POSITIONS // a["batch"], launches=a["launches"],
                         epoch_seconds=dict(median=round(statistics.median(s), 5), min=round(min(s), 5), max=round(max(s), 5)),
                         positions_per_second=dict(median=round(N_POSITIONS / statistics.median(s)), min=round(N_POSITIONS / max(s)),
                                                   max=round(N_POSITIONS / min(s))),
                         epoch_seconds_all=[round(x, 5) for x in s])
        if a["mode"] == "micro":
            out[name]["blocks_grid"] = a["engine"].trainer_batch_mode()[2]
            out[name]["micro_batches_per_step"] = a["batch"] // 32
        a["engine"].close()

    def compare(fast, slow):
        f, s = out[fast]["epoch_seconds"], out[slow]["epoch_seconds"]
        spread = max(f["max"] - f["min"], s["max"] - s["min"])
        return dict(faster=fast, slower=slow, median_seconds_saved=round(s["median"] - f["median"], 5), larger_min_max_range=round(spread, 5),
                    resolved=bool(s["median"] - f["median"] > spread), ratio_of_medians=round(s["median"] / f["median"], 3))

    cmp = [compare("micro_b4096", b) for b in out if b.startswith("baseline")] + [compare("micro_b4096", "micro_b256"),
                                                                                   compare("micro_b1024", "micro_b256")]
    return dict(arms=out, comparisons=cmp,
                micro_b4096_resolved_faster_than_every_baseline=all(c["resolved"] for c in cmp if c["slower"].startswith("baseline")),
                micro_b4096_resolved_faster_than_micro_b256=cmp[-2]["resolved"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--timed", type=int, default=6)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--nets", default="mlp,conv")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.timed < 6:
        raise SystemExit("--timed must be at least 6: fewer epochs per arm do not give a range worth comparing")
    base_lib = os.environ.pop("SYNTHESIS_AMD_LIB", "")
    if not base_lib or not os.path.exists(base_lib):
        raise SystemExit("SYNTHESIS_AMD_LIB must name a libsynthesis_amd.so built at the parent commit: the baseline arms run in it")

    import torch  # noqa: F401  (before the engine: one HIP runtime per process)

    import bench
    import synthesis_amd as sa

    data = data_set(sa, args.device)
    rec = dict(tool="tools/train_batch_ab.py", kernel_source_hash=bench.kernel_source_hash(), device=torch.cuda.get_device_name(args.device),
               compute_units=torch.cuda.get_device_properties(args.device).multi_processor_count,
               timing="host clock (time.perf_counter) around Engine.train_epoch = one syn_train_epoch call, which stages the permutation, gathers "
                      "the batches and ends in its one synchronisation",
               order="every arm once per round, rounds repeated; one process; baseline arms in the library SYNTHESIS_AMD_LIB named",
               data_set=dict(positions=N_POSITIONS, recorded_positions_drawn_from=data["recorded"]),
               warmup_epochs=args.warmup, timed_epochs=args.timed, date=time.strftime("%Y-%m-%d"),
               not_measured=["the learning loop's end-to-end iteration time with --batch-mode micro", "anything on more than one GPU",
                             "what large batches do to the strength of the trained player (no learning-rate scaling is applied)"],
               networks={})
    for net in args.nets.split(","):
        rec["networks"][net] = run_network(sa, net, base_lib, data, args.warmup, args.timed, args.device)
        print(json.dumps({net: rec["networks"][net]}), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
