#!/usr/bin/env python3
"""Where several checkpoints sit on one scale: synthesis_amd.arena.round_robin / gauntlet (ONE Engine.tournament_run for the whole
schedule) and arena.ratings, as ONE JSON line.

    python tools/tournament.py A.npy B.npy C.npy --baseline 800 --baseline 3200 --openings 512 --opening-plies 8 --explores 800 --gauntlet

The files are parameter blobs of one network kind (30,492 floats Connect4Net, 12,412 Connect4ConvNet); every --baseline N adds the
evaluator's VanillaMCTS<N> (FrozenMCTS over RolloutPolicy). --round-robin (the default) pairs every player with every other;
--gauntlet pairs every checkpoint with every baseline only (it needs at least one). Every pair plays every opening twice, once per
colour; opening o of every pair runs on StdRng::seed_from_u64(seed + o). The network players search with the parity configuration
(Fpu::Const, no noise, moves by visit count) and --explores; --arith gives all of them an arithmetic of their own ("f32" / "f16x2"),
or one name per file.

The line carries the pair table (W/D/L, score, standard error over openings, the pair's own Elo difference) and the Bradley-Terry
ratings of all players on one scale, relative to --anchor (player index: files first, baselines after them), with bootstrap intervals
over openings. --prior-draws adds virtual drawn games per played pair (needed when a player won or lost everything). A rating is a
statement about these players on these openings with these search settings."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("checkpoints", nargs="+")
    ap.add_argument("--baseline", type=int, action="append", default=[], metavar="N", help="add VanillaMCTS<N> (repeatable)")
    ap.add_argument("--arith", nargs="+", choices=("f32", "f16x2"), default=None, help="one name for all checkpoints, or one per file")
    ap.add_argument("--openings", type=int, default=512)
    ap.add_argument("--opening-plies", type=int, default=8)
    ap.add_argument("--explores", type=int, default=800)
    mode = ap.add_mutually_exclusive_group()
    mode.add_argument("--round-robin", action="store_true")
    mode.add_argument("--gauntlet", action="store_true")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--anchor", type=int, default=0)
    ap.add_argument("--prior-draws", type=float, default=0.0)
    ap.add_argument("--bootstrap", type=int, default=400)
    ap.add_argument("--concurrent", type=int, default=0, help="engine slots (default: the number of games, at most 65,536)")
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    if args.gauntlet and not args.baseline:
        raise SystemExit("--gauntlet pairs checkpoints with baselines: give at least one --baseline N")
    ariths = args.arith or [None]
    if len(ariths) == 1:
        ariths = ariths * len(args.checkpoints)
    if len(ariths) != len(args.checkpoints):
        raise SystemExit("--arith takes one name, or one per checkpoint file")

    import numpy as np

    import synthesis_amd as sa
    from synthesis_amd import arena, match

    blobs = [np.load(f).astype(np.float32).ravel() for f in args.checkpoints]
    if len({b.size for b in blobs}) != 1:
        raise SystemExit("the checkpoints must be parameters of one network kind")
    nets = [match.Player(os.path.basename(f), args.explores, sa.parity_mcts_config(), weights=b, arithmetic=a)
            for f, b, a in zip(args.checkpoints, blobs, ariths)]
    anchors = [match.vanilla_player(n) for n in args.baseline]
    players = nets + anchors
    openings = arena.random_openings(args.openings, args.opening_plies, args.seed)
    seeds = np.uint64(args.seed) + np.arange(args.openings, dtype=np.uint64)
    pairs = arena.gauntlet_pairs(len(nets), len(anchors)) if args.gauntlet else arena.round_robin_pairs(len(players))
    n_games = 2 * len(pairs) * args.openings
    slots = args.concurrent or max(16, min(n_games, 65536))
    with sa.Engine(concurrent_games=slots, max_explores=args.explores, device=args.device) as eng:
        (eng.load_weights_conv if blobs[0].size == sa.engine.CONV_NUM_PARAMS else eng.load_weights)(blobs[0])   # selects the network kind
        t0 = time.perf_counter()
        res = arena.tournament(eng, players, pairs, openings, seeds=seeds)
        seconds = time.perf_counter() - t0
        device_ms, launches = eng.last_timing()
    fit = arena.ratings(res, anchor=args.anchor, prior_draws=args.prior_draws, bootstrap=args.bootstrap, seed=args.seed)
    names = [f"{i}:{p.name}" + (f"@{p.arithmetic}" if p.arithmetic else "") for i, p in enumerate(players)]   # (a file may play twice)
    table = []
    for (a, b), st in res["stats"].items():
        table.append(dict(a=names[a], b=names[b], wins=st["wins"], draws=st["draws"], losses=st["losses"], score=round(st["score"], 5),
                          se=round(st["se"], 5), elo=round(st["elo"], 1), elo_interval=[round(st["elo_lo"], 1), round(st["elo_hi"], 1)]))
    rec = dict(tool="tools/tournament.py", schedule="gauntlet" if args.gauntlet else "round-robin", players=names,
               arithmetic=[a or "engine (f32)" for a in ariths] + [None] * len(anchors), openings=args.openings,
               opening_plies=args.opening_plies, opening_seed=args.seed, explores=args.explores, games=n_games,
               mean_plies=round(float(res["games"]["plies"].mean()), 2), seconds=round(seconds, 3), device_ms=round(device_ms, 1),
               launches=launches, pairs=table,
               ratings=dict(anchor=names[args.anchor], prior_draws=args.prior_draws, bootstrap=args.bootstrap,
                            elo={n: round(float(e), 1) for n, e in zip(names, fit["elo"])},
                            interval={n: [round(float(lo), 1), round(float(hi), 1)] for n, lo, hi in zip(names, fit["elo_lo"], fit["elo_hi"])}))
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
