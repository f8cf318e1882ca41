#!/usr/bin/env python3
"""A/B of an iteration's epochs: the host sampler (numpy permutation + one Engine.train_epoch call per epoch, the permutation inside the
timed region because the loop pays it) against the device-side sampler (ONE Engine.train_epochs_sampled call), in ONE process on ONE
engine, arms interleaved.

    python tools/train_sampler_ab.py --out profiles/train_sampler_ab.json

Legs: Connect4Net at batch 32 (the persistent epoch kernel), Connect4Net and Connect4ConvNet at batch 4,096 in SYN_TRAIN_BATCH_MICRO;
every leg runs 4 epochs per call over the same 1,048,576 positions (recorded self-play positions drawn with repetition, as
tools/train_batch_ab.py builds them) in three arms: A = host sampler, B = device sampler, B_flip = device sampler with random flipping
(B_flip against B is the cost of the flip in the gather). Then one LearningLoop leg at tools/replay_loop_ab.py's `bench` shape,
replay="device": sampler="numpy" against sampler="device" on two engines (a loop owns its engine's replay buffer and learner).
Protocol of tools/arena_ab.py: 2 warm-up and 6 timed runs per arm, median (min-max) per arm, and a difference counts as resolved only
when the medians differ by more than the larger of the two arms' ranges. The arms train in different orders (and continue from each
other's weights on the one engine), so their weights differ: this is a timing comparison only — what the two orders compute is held
bit for bit by tests/test_gpu_sampler.py."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_POSITIONS = 1 << 20
EPOCHS = 4
LEGS = (("mlp", 32, "chained"), ("mlp", 4096, "micro"), ("conv", 4096, "micro"))
ARMS = ("A_host_permutation", "B_device_sampler", "B_device_sampler_flip")
LOOP_SHAPE = dict(concurrent=8192, explores=200, games_per_train=8192, games_to_keep=20000, epochs=1, batch=32, seed=7)


def summary(v):
    return dict(median=round(statistics.median(v), 5), min=round(min(v), 5), max=round(max(v), 5))


def compare(a, b, name_a, name_b):
    """a minus b of two summaries, with the rule the documents follow"""
    spread = max(a["max"] - a["min"], b["max"] - b["min"])
    d = a["median"] - b["median"]
    return dict(minuend=name_a, subtrahend=name_b, median_difference=round(d, 5), larger_min_max_range=round(spread, 5),
                resolved=bool(abs(d) > spread))


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


def run_leg(eng, net, batch, mode, data, warmup, timed):
    from bench import make_conv_weights, make_weights

    (eng.trainer_init if net == "mlp" else eng.trainer_init_conv)(make_weights() if net == "mlp" else make_conv_weights())
    eng.trainer_set_batch_mode(mode)
    eng.train_set_data(data["my"], data["op"], data["pi"], data["v"])
    n_steps = N_POSITIONS // batch
    times = {a: [] for a in ARMS}
    perm_seconds = []
    for run in range(warmup + timed):
        for arm in ARMS:   # interleaved: drift of the box lands on every arm alike
            t0 = time.perf_counter()
            if arm == "A_host_permutation":
                t_perm = 0.0
                losses = []
                for ep in range(EPOCHS):   # LearningLoop's own lines
                    tp = time.perf_counter()
                    perm = np.random.default_rng([7, run, ep]).permutation(N_POSITIONS)
                    t_perm += time.perf_counter() - tp
                    losses.append(eng.train_epoch(perm[: n_steps * batch], batch, 1e-3))
                losses = np.stack(losses)
            else:
                losses = eng.train_epochs_sampled(run, EPOCHS, batch, 1e-3, flip=arm.endswith("flip"))
            dt = time.perf_counter() - t0
            assert losses.shape == (EPOCHS, n_steps, 2) and np.isfinite(losses).all()
            if run >= warmup:
                times[arm].append(dt)
                if arm == "A_host_permutation":
                    perm_seconds.append(t_perm)
    out = dict(network="Connect4Net" if net == "mlp" else "Connect4ConvNet", batch=batch, batch_mode=mode, epochs_per_call=EPOCHS,
               steps_per_epoch=n_steps, seconds_per_call={a: summary(times[a]) for a in ARMS},
               seconds_per_call_all={a: [round(x, 5) for x in times[a]] for a in ARMS},
               host_permutation_seconds_inside_arm_A=summary(perm_seconds))
    s = out["seconds_per_call"]
    out["A_minus_B"] = compare(s[ARMS[0]], s[ARMS[1]], ARMS[0], ARMS[1])
    out["flip_minus_no_flip"] = compare(s[ARMS[2]], s[ARMS[1]], ARMS[2], ARMS[1])
    return out


def run_loop(sa, warmup, timed, device):
    from bench import make_weights
    from synthesis_amd.learner import LearningLoop

    s = LOOP_SHAPE
    blob = make_weights()
    cfg = sa.parity_rollout_config(s["explores"])
    arms = ("numpy", "device")
    engines = {a: sa.Engine(concurrent_games=s["concurrent"], max_explores=s["explores"], device=device) for a in arms}
    loops = {a: LearningLoop(engines[a], "mlp", blob, device=device, seed=s["seed"], weight_decay=1e-6, replay="device", sampler=a)
             for a in arms}
    recs = {a: [] for a in arms}
    for _ in range(warmup + timed):
        for a in arms:
            recs[a].append(loops[a].iteration(cfg, s["games_per_train"], s["games_to_keep"], s["epochs"], s["batch"]))
    out = dict(shape=dict(s), replay="device", warmup_iterations=warmup, timed_iterations=timed,
               note="the arms train in different orders: from the second iteration on they play different games, so `unique` differs")
    for a in arms:
        timed_recs = recs[a][warmup:]
        out[a] = dict(total=summary([r["seconds"]["total"] for r in timed_recs]), train=summary([r["seconds"]["train"] for r in timed_recs]),
                      unique=[r["unique"] for r in recs[a]], optimiser_steps=[r["optimiser_steps"] for r in recs[a]])
        engines[a].close()
    out["train_numpy_minus_device"] = compare(out["numpy"]["train"], out["device"]["train"], "numpy", "device")
    out["total_numpy_minus_device"] = compare(out["numpy"]["total"], out["device"]["total"], "numpy", "device")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--timed", type=int, default=6)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--skip-loop", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.timed < 6:
        raise SystemExit("--timed must be at least 6: fewer runs per arm do not give a range worth comparing")

    import torch  # noqa: F401  (before the engine: one HIP runtime per process)

    import bench
    import synthesis_amd as sa

    data = data_set(sa, args.device)
    rec = dict(tool="tools/train_sampler_ab.py", kernel_source_hash=bench.kernel_source_hash(), device=torch.cuda.get_device_name(args.device),
               timing="host clock (time.perf_counter) around one call of arm B, around the four permutation + Engine.train_epoch pairs of "
                      "arm A; every call ends in a device synchronise",
               order="A, B, B_flip, A, B, B_flip, ... on one engine of one process, leg after leg",
               data_set=dict(positions=N_POSITIONS, recorded_positions_drawn_from=data["recorded"]),
               warmup_runs=args.warmup, timed_runs=args.timed, date=time.strftime("%Y-%m-%d"),
               weights="the arms train in different orders and continue from each other's weights: their weights differ, only times are compared",
               not_measured=["whether random flipping trains a stronger player (tools/arena.py is the instrument)",
                             "anything on more than one GPU", "DataParallelLearner (it keeps its host-drawn order)"],
               legs=[])
    with sa.Engine(concurrent_games=64, max_explores=64, device=args.device) as eng:
        for net, batch, mode in LEGS:
            rec["legs"].append(run_leg(eng, net, batch, mode, data, args.warmup, args.timed))
            print(json.dumps(rec["legs"][-1]), flush=True)
    if not args.skip_loop:
        rec["learning_loop"] = run_loop(sa, args.warmup, args.timed, args.device)
        print(json.dumps(rec["learning_loop"]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
