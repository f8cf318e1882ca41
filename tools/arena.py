#!/usr/bin/env python3
"""Which of two checkpoints is stronger: synthesis_amd.arena.compare on random openings, as ONE JSON line.

    python tools/arena.py A.npy B.npy --openings 4096 --opening-plies 8 --explores 800 [--net conv] [--arithmetic f16x2]

A.npy / B.npy: parameter blobs of one network kind (30,492 floats Connect4Net, 12,412 Connect4ConvNet). Every opening is played twice,
once with A moving first and once with B; both sides search with the parity configuration (Fpu::Const, no noise, moves by visit
count) and the same explores, so the games are deterministic and the spread comes from the openings. The line carries W/D/L from A's
side, the score S = mean of the per-opening pair scores, its standard error over openings, and the Elo difference of S and of
S -/+ 1.96 SE (clipped at scores 0.001 / 0.999: +-1200 means "off the scale", not a measurement).

--arith-a / --arith-b give a side an arithmetic of its own, whatever the engine is in (Engine.match_run_sides): the same file twice with
--arith-a f32 --arith-b f16x2 is one checkpoint against itself in the faster arithmetic — what that arithmetic costs in playing
strength. --baseline N plays A against the evaluator's VanillaMCTS<N> (FrozenMCTS over RolloutPolicy, the reference's absolute scale)
on the same openings, both colours, opening o on StdRng::seed_from_u64(seed + o); B is then not read (pass A again). The same JSON line.
--same-games-in f16x2 plays the same match a second time on an engine in that arithmetic and reports its W/D/L and score beside the
first, with the number of pair scores and game lengths that differ."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("a")
    ap.add_argument("b")
    ap.add_argument("--openings", type=int, default=4096)
    ap.add_argument("--opening-plies", type=int, default=8)
    ap.add_argument("--explores", type=int, default=800)
    ap.add_argument("--net", choices=("mlp", "conv"), default="mlp")
    ap.add_argument("--arithmetic", choices=("f32", "f16x2"), default="f32")
    ap.add_argument("--arith-a", choices=("f32", "f16x2"), default=None, help="A's own arithmetic (default: the engine's, --arithmetic)")
    ap.add_argument("--arith-b", choices=("f32", "f16x2"), default=None, help="B's own arithmetic")
    ap.add_argument("--baseline", type=int, default=0, metavar="N", help="play A against VanillaMCTS<N> instead of B")
    ap.add_argument("--same-games-in", choices=("f32", "f16x2"), default=None,
                    help="also play the match in this arithmetic (a second engine) and count the games that differ")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--concurrent", type=int, default=0, help="engine slots (default: the number of openings, at most 65,536)")
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()

    import numpy as np

    import synthesis_amd as sa
    from synthesis_amd import arena, match

    blob_a = np.load(args.a).astype(np.float32).ravel()
    blob_b = np.load(args.b).astype(np.float32).ravel()
    openings = arena.random_openings(args.openings, args.opening_plies, args.seed)
    player_a = match.Player("net", args.explores, sa.parity_mcts_config(), arithmetic=args.arith_a)
    player_b = match.Player("net", args.explores, sa.parity_mcts_config(), arithmetic=args.arith_b)
    seeds = np.uint64(args.seed) + np.arange(args.openings, dtype=np.uint64)
    slots = args.concurrent or max(16, min(args.openings, 65536))

    def run(arithmetic):
        with sa.Engine(concurrent_games=slots, max_explores=args.explores, device=args.device) as eng:
            (eng.load_weights_conv if args.net == "conv" else eng.load_weights)(blob_a)   # selects the engine's network kind
            eng.set_network_arithmetic(arithmetic)
            t0 = time.perf_counter()
            if args.baseline:
                r = arena.compare_baseline(eng, blob_a, openings, player_a, match.vanilla_player(args.baseline), seeds)
            else:
                r = arena.compare(eng, blob_a, blob_b, openings, player_a, player_b)
            return r, time.perf_counter() - t0

    r, seconds = run(args.arithmetic)
    b_name = f"VanillaMCTS{args.baseline}" if args.baseline else os.path.basename(args.b)
    rec = dict(tool="tools/arena.py", a=os.path.basename(args.a), b=b_name, net=args.net, arithmetic=args.arithmetic,
               arith_a=args.arith_a or args.arithmetic, arith_b=None if args.baseline else (args.arith_b or args.arithmetic),
               openings=args.openings, opening_plies=args.opening_plies, opening_seed=args.seed, explores=args.explores,
               games=2 * args.openings, wins=r["wins"], draws=r["draws"], losses=r["losses"], score=round(r["score"], 5),
               se=round(r["se"], 5), score_interval=[round(r["score_lo"], 5), round(r["score_hi"], 5)], elo=round(r["elo"], 1),
               elo_interval=[round(r["elo_lo"], 1), round(r["elo_hi"], 1)],
               mean_plies=round(float(np.concatenate([r["plies_a_first"], r["plies_b_first"]]).mean()), 2), seconds=round(seconds, 3))
    if args.same_games_in and args.same_games_in != args.arithmetic:
        r2, _ = run(args.same_games_in)
        diff = int((r["plies_a_first"] != r2["plies_a_first"]).sum() + (r["plies_b_first"] != r2["plies_b_first"]).sum())
        rec["other_arithmetic"] = dict(arithmetic=args.same_games_in, wins=r2["wins"], draws=r2["draws"], losses=r2["losses"],
                                       score=round(r2["score"], 5), se=round(r2["se"], 5),
                                       games_of_other_length=diff,
                                       pair_scores_that_differ=int((r["pair_scores"] != r2["pair_scores"]).sum()))
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
