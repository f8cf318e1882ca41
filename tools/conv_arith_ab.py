#!/usr/bin/env python3
"""Developer tool: same-box A/B of Connect4ConvNet's two arithmetics (f32: convnet.cuh; f16x2: conv_f16x2_tile.cuh) on the shape of
bench.py's `with_conv_policy` leg — an engine of 262,144 slots, bench.make_conv_weights(), the headline MCTS configuration
(parity_rollout_config, 800 explores), 1,048,576 games per launch. The arms alternate (A B A B ...), every timed launch behind a warm-up
launch of its own; per arm: median / min / max games/s, the launch shape, and — from one counted run of 32,768 games per arm, as bench.py's
conv_leg computes them — leaf evaluations per second and the matrix-pipe fraction.
    usage: tools/conv_arith_ab.py [--launches 6] [--games 1048576] [--out profiles/r07_conv_arith_ab.json]
           rocprofv3 --kernel-trace --stats -- python tools/conv_arith_ab.py --trace-launch    (one f16x2 launch of 262,144 games, nothing else)"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONV_F16X2_FLOP_PER_EVAL = 222 * 16384 // 16   # the f16x2 tile as executed: 63 x 2 + 32 x 3 v_mfma_f32_16x16x32_f16 per 16 positions


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=6)
    ap.add_argument("--games", type=int, default=1048576)
    ap.add_argument("--concurrent", type=int, default=262144)
    ap.add_argument("--explores", type=int, default=800)
    ap.add_argument("--out", default="")
    ap.add_argument("--trace-launch", action="store_true", help="one f16x2 launch of --concurrent games only (for a kernel-trace pass)")
    args = ap.parse_args()

    import torch  # noqa: F401  (before the engine: one HIP runtime per process)

    import synthesis_amd as sa
    from bench import CONV_FLOP_PER_EVAL, PEAK_F16_MFMA_TFLOPS, PEAK_F32_MFMA_TFLOPS, make_conv_weights

    cfg = sa.parity_rollout_config(args.explores)
    eng = sa.Engine(concurrent_games=args.concurrent, max_explores=args.explores, device=0)
    eng.load_weights_conv(make_conv_weights())
    if args.trace_launch:
        eng.set_network_arithmetic("f16x2")
        r = eng.selfplay(cfg, base_seed=0, n_games=args.concurrent, outputs=False)
        print("shape", eng.last_launch_shape(), "kernel_ms", r["kernel_ms"])
        eng.close()
        return
    arms = ("f32", "f16x2")
    res = {a: dict(games_per_s=[], kernel_ms=[], shape=None) for a in arms}
    first = 0
    for i in range(args.launches):
        for a in arms:
            eng.set_network_arithmetic(a)
            eng.selfplay(cfg, base_seed=0, n_games=args.concurrent, first_game=first, outputs=False)   # warm-up
            t = time.perf_counter()
            r = eng.selfplay(cfg, base_seed=0, n_games=args.games, first_game=first + args.concurrent, outputs=False)
            dt = time.perf_counter() - t
            res[a]["games_per_s"].append(args.games / dt)
            res[a]["kernel_ms"].append(r["kernel_ms"])
            res[a]["shape"] = list(eng.last_launch_shape())
            print(f"launch {i} {a}: {args.games / dt:.0f} games/s, shape {res[a]['shape']}", flush=True)
        first += args.concurrent + args.games
    out = dict(tool="tools/conv_arith_ab.py", network="Connect4ConvNet, bench.make_conv_weights()", concurrent_games=args.concurrent,
               explores=args.explores, games_per_launch=args.games, launches_per_arm=args.launches, order="A B A B ..., each behind its own warm-up")
    for a in arms:
        eng.set_network_arithmetic(a)
        c = eng.selfplay(cfg, base_seed=0, n_games=32768, first_game=first, outputs=False, counters=True)["counters"]
        g = res[a]["games_per_s"]
        med = statistics.median(g)
        evals_per_s = c["policy_evals"] / 32768.0 * med
        o = dict(games_per_s_median=med, games_per_s_min=min(g), games_per_s_max=max(g), games_per_s=g, kernel_ms=res[a]["kernel_ms"],
                 launch_shape=res[a]["shape"], leaf_evals_per_s=evals_per_s,
                 mfma_frac_f32_equivalent=evals_per_s * CONV_FLOP_PER_EVAL / 1e12 / PEAK_F32_MFMA_TFLOPS)
        if a == "f16x2":
            o["mfma_frac_f16_pipe_executed"] = evals_per_s * CONV_F16X2_FLOP_PER_EVAL / 1e12 / PEAK_F16_MFMA_TFLOPS
        out[a] = o
    out["speedup_median"] = out["f16x2"]["games_per_s_median"] / out["f32"]["games_per_s_median"]
    eng.close()
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
