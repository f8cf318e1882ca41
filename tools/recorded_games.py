#!/usr/bin/env python3
"""Training rows from games that start at given positions: Engine.games_run_recorded from the command line.

    python tools/recorded_games.py A.npy [B.npy] --out rows.npz [--positions starts.npy | --openings 4096 --opening-plies 8]
                                   [--explores 800] [--record both|a|b] [--net conv] [--arithmetic f16x2]

A.npy / B.npy: parameter blobs of one network kind (30,492 floats Connect4Net, 12,412 Connect4ConvNet). With one checkpoint A plays
both sides (exploring starts, a curriculum); with two, every start position is played twice, A moving first and B moving first (league
data), and --record says whose plies become rows. Start positions: --positions names an .npy of shape [n, 2] (uint64: the stones of the
side to move, the other side's), else arena.random_openings(--openings, --opening-plies, --seed). Both sides search with the parity
configuration (Fpu::Const, no noise: recorded games take deterministic searches only) at --explores; moves follow the rollout
configuration's defaults counted from the start position (the first move random, sampled until turn 30), value target Q; game g plays
on StdRng::seed_from_u64(--seed + g).

--out receives one .npz: per row my, op (uint64), pi [rows, 9], v [rows, 3] and game (index into the per-game arrays; the rows of a
game are in ply order), and per game start_my, start_op, first (0 = A moved first), rows_per_game, plies, rewards (for the first
mover) and final_kind. One JSON line on stdout says what was played."""
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
    ap.add_argument("b", nargs="?", default=None)
    ap.add_argument("--out", required=True)
    ap.add_argument("--positions", default="", help=".npy of start positions, uint64 [n, 2] = (side to move, other side)")
    ap.add_argument("--openings", type=int, default=4096)
    ap.add_argument("--opening-plies", type=int, default=8)
    ap.add_argument("--explores", type=int, default=800)
    ap.add_argument("--record", choices=("both", "a", "b"), default="both")
    ap.add_argument("--net", choices=("mlp", "conv"), default="mlp")
    ap.add_argument("--arithmetic", choices=("f32", "f16x2"), default="f32")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--concurrent", type=int, default=0, help="engine slots (default: the number of games, at most 65,536)")
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()

    import numpy as np

    import synthesis_amd as sa
    from synthesis_amd import arena, match

    blobs = [np.load(p).astype(np.float32).ravel() for p in (args.a, args.b) if p]
    if args.positions:
        starts = np.load(args.positions)
        if starts.ndim != 2 or starts.shape[1] != 2:
            raise SystemExit(f"--positions: expected an array of shape [n, 2], got {list(starts.shape)}")
        my, op = starts[:, 0].astype(np.uint64), starts[:, 1].astype(np.uint64)
    else:
        my, op = arena.random_openings(args.openings, args.opening_plies, args.seed)
    n_starts = int(my.size)
    players = [match.Player(name, args.explores, sa.parity_mcts_config(), weights=b) for name, b in zip("AB", blobs)]
    if len(players) == 2:   # every start twice: A first, B first
        my, op = np.tile(my, 2), np.tile(op, 2)
        first = np.repeat(np.arange(2, dtype=np.int32), n_starts)
        second = 1 - first
        mask = dict(both=3, a=1, b=2)[args.record]
    else:
        if args.record == "b":
            raise SystemExit("--record b needs a second checkpoint")
        first = second = np.zeros(n_starts, np.int32)
        mask = 1
    n = int(my.size)
    seeds = np.uint64(args.seed) + np.arange(n, dtype=np.uint64)
    rec = sa.RecordConfig.from_rollout(sa.parity_rollout_config(args.explores), mask)
    with sa.Engine(concurrent_games=args.concurrent or max(16, min(n, 65536)), max_explores=args.explores, device=args.device) as eng:
        (eng.load_weights_conv if args.net == "conv" else eng.load_weights)(blobs[0])
        eng.set_network_arithmetic(args.arithmetic)
        t = time.perf_counter()
        got = eng.games_run_recorded(players, first, second, my, op, seeds, record=rec)
        seconds = time.perf_counter() - t
        device_ms, launches = eng.last_timing()
    keep = np.arange(63)[None, :] < got["rows"][:, None]
    np.savez(args.out, my=got["states"][..., 0][keep], op=got["states"][..., 1][keep], pi=got["pis"][keep], v=got["vs"][keep],
             game=np.arange(n)[:, None].repeat(63, 1)[keep], start_my=my, start_op=op, first=first, rows_per_game=got["rows"],
             plies=got["plies"], rewards=got["rewards"], final_kind=got["final_kind"])
    print(json.dumps(dict(tool="tools/recorded_games.py", checkpoints=[args.a] + ([args.b] if args.b else []), starts=n_starts, games=n,
                          explores=args.explores, record=args.record, arithmetic=args.arithmetic, rows=int(got["rows"].sum()),
                          plies_per_game=round(float(got["plies"].mean()), 3), rows_per_game=round(float(got["rows"].mean()), 3),
                          first_mover_score=round(float((got["rewards"].mean() + 1) / 2), 4), wall_seconds=round(seconds, 3),
                          device_seconds=round(device_ms / 1e3, 3), launches=launches, out=args.out)))


if __name__ == "__main__":
    main()
