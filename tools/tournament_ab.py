#!/usr/bin/env python3
"""A/B of the device-resident tournament (Engine.tournament_run = syn_tournament_run) against what the library could do before it: the
same schedule as ONE Engine.match_run_sides call per ordered pairing. Both arms run on ONE engine of ONE process, interleaved
(tournament, pairwise, tournament, pairwise, ...), after the two arms' games have been asserted identical, key for key.

    python tools/tournament_ab.py --out profiles/tournament_ab.json

Workloads (sizes a user would run), 512 openings of 8 plies, 800 explores unless said otherwise:
  round_robin8   eight network players, all 56 ordered pairings: 28,672 games
  gauntlet6x2    six network players against VanillaMCTS800 and VanillaMCTS3200, both colours: 24 ordered pairings, 12,288 games
  two_players    two network players, 4,096 openings, both colours: the tournament against match_run_sides itself (two calls)
  one_match      ONE ordered pairing of two network players (player 0 always first) at 512, 4,096 and 65,536 openings: the tournament
                 against one match_run_sides call — one group and one search launch per ply in both arms
  one_match_vanilla  one ordered pairing, a network player first against VanillaMCTS800, 512 openings: the same with a baseline group
The last three asked what the tournament's loop costs a match while the match had a loop of its own (profiles/tournament_ab.json,
profiles/match_fold_ab.json). The match now runs in the tournament's loop, so with the in-tree library their two arms issue the same
launches; against an older build named by SYNTHESIS_AMD_LIB they still compare the two loops.
Per workload: 2 warm-up and 6 timed runs per arm, host clock around calls that end in a device synchronise; median and min-max; a gap
counts as resolved only when the medians differ by more than the larger of the two ranges. syn_last_timing's device time and launch
count are reported beside each arm (summed over the pairwise arm's calls)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ARMS = ("tournament", "pairwise")
KEYS = ("rewards", "plies", "moves", "final_bb", "rng_words")


def summary(v):
    return dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4))


def network_players(n, explores):
    """n different network players: the trained golden checkpoint and fixed-seed random initialisations, under different c"""
    import numpy as np

    import bench
    import synthesis_amd as sa
    from synthesis_amd import match

    trained = np.load(os.path.join(ROOT, "tests", "golden", "c4net_trained_f32.npy")).astype(np.float32).ravel()
    out = []
    for i in range(n):
        blob = trained if i % 2 == 0 else bench.make_weights(seed=20211003 + i)
        out.append(match.Player(f"{'trained' if i % 2 == 0 else 'init'}{i}_c{1.0 + 0.5 * i}", explores, sa.MCTSConfig(c=1.0 + 0.5 * i), weights=blob))
    return out


def run_workload(eng, name, players, pairs, n_openings, plies, warmup, timed, one_colour=False):
    import numpy as np

    from synthesis_amd import arena

    my, op = arena.random_openings(n_openings, plies, seed=1)
    sch = arena.schedule(pairs, n_openings, len(players))
    keep = sch["a_first"] if one_colour else np.ones(sch["first"].size, bool)   # one_colour: the pairs as given, never reversed
    first, second, o = sch["first"][keep], sch["second"][keep], sch["opening"][keep]
    seeds = (np.uint64(1) + np.arange(n_openings, dtype=np.uint64))[o]
    pairings = sorted(set(zip(first.tolist(), second.tolist())))
    games_of = {pq: np.nonzero((first == pq[0]) & (second == pq[1]))[0] for pq in pairings}

    def tournament():
        out = eng.tournament_run(players, first, second, my[o], op[o], seeds=seeds)
        return out, eng.last_timing()

    def pairwise():
        out = dict(rewards=np.zeros(first.size, np.float32), plies=np.zeros(first.size, np.int32), moves=np.full((first.size, 63), 255, np.uint8),
                   final_bb=np.zeros((first.size, 2), np.uint64), rng_words=np.zeros(first.size, np.uint64))
        ms, launches = 0.0, 0
        for (a, b), g in games_of.items():
            r = eng.match_run_sides(players[a], players[b], my[o[g]], op[o[g]], seeds=seeds[g])
            for k in KEYS:
                out[k][g] = r[k]
            t = eng.last_timing()
            ms += t[0]; launches += t[1]
        return out, (ms, launches)

    arms = dict(tournament=tournament, pairwise=pairwise)
    got = {arm: arms[arm]()[0] for arm in ARMS}        # identical games first: a timing of different games compares nothing
    for k in KEYS:
        assert np.array_equal(got["tournament"][k], got["pairwise"][k]), f"{name}: {k} differs between the arms"
    times = {arm: [] for arm in ARMS}
    device_ms = {arm: [] for arm in ARMS}
    launches = {}
    for i in range(warmup + timed):
        for arm in ARMS:   # interleaved: drift of the machine lands on both arms alike
            t0 = time.perf_counter()
            _, (ms, nl) = arms[arm]()
            dt = time.perf_counter() - t0
            print(f"{name}: run {i} {arm} {dt:.4f} s", file=sys.stderr, flush=True)
            if i >= warmup:
                times[arm].append(dt)
                device_ms[arm].append(ms)
                launches[arm] = nl
    plies_played = got["tournament"]["plies"]
    rec = dict(workload=name, players=[p.name for p in players], ordered_pairings=len(pairings), openings=n_openings, opening_plies=plies,
               games=int(first.size), identical_games=True, mean_plies=round(float(plies_played.mean()), 2), max_plies=int(plies_played.max()),
               pairwise_calls=len(pairings), seconds={arm: summary(times[arm]) for arm in ARMS},
               device_ms={arm: summary(device_ms[arm]) for arm in ARMS}, launches=launches,
               games_per_second={arm: round(first.size / statistics.median(times[arm])) for arm in ARMS})
    t, p = rec["seconds"]["tournament"], rec["seconds"]["pairwise"]
    spread = max(t["max"] - t["min"], p["max"] - p["min"])
    gap = p["median"] - t["median"]
    rec["pairwise_minus_tournament"] = dict(median=round(gap, 4), larger_min_max_range=round(spread, 4), resolved=bool(abs(gap) > spread),
                                            ratio=round(p["median"] / t["median"], 3))
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", nargs="+", default=["round_robin8", "gauntlet6x2", "two_players"],
                    choices=["round_robin8", "gauntlet6x2", "two_players", "one_match", "one_match_vanilla"])
    ap.add_argument("--openings", type=int, default=512)
    ap.add_argument("--two-player-openings", type=int, default=4096)
    ap.add_argument("--one-match-openings", type=int, nargs="+", default=[512, 4096, 65536])
    ap.add_argument("--opening-plies", type=int, default=8)
    ap.add_argument("--explores", type=int, default=800)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--timed", type=int, default=6)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.timed < 6:
        raise SystemExit("--timed must be at least 6: fewer runs per arm do not give a range worth comparing")

    import torch  # noqa: F401  (before the engine: one HIP runtime per process)

    import bench
    import synthesis_amd as sa
    from synthesis_amd import arena, match

    def workload(name):
        if name.startswith("one_match_vanilla"):
            return network_players(1, args.explores) + [match.vanilla_player(800)], [(0, 1)], args.openings
        if name.startswith("one_match"):
            return network_players(2, args.explores), [(0, 1)], int(name.rsplit("_", 1)[1])
        if name == "round_robin8":
            players = network_players(8, args.explores)
            return players, arena.round_robin_pairs(8), args.openings
        if name == "gauntlet6x2":
            players = network_players(6, args.explores) + [match.vanilla_player(800), match.vanilla_player(3200)]
            return players, arena.gauntlet_pairs(6, 2), args.openings
        return network_players(2, args.explores), [(0, 1)], args.two_player_openings

    names = []
    for name in args.workloads:   # one_match: one workload per size
        names += [f"one_match_{n}" for n in args.one_match_openings] if name == "one_match" else [name]
    done = []
    for name in names:
        players, pairs, n_openings = workload(name)
        one_colour = name.startswith("one_match")
        n_games = (1 if one_colour else 2) * len(pairs) * n_openings
        with sa.Engine(concurrent_games=min(n_games, 65536), max_explores=args.explores, device=args.device) as eng:
            done.append(run_workload(eng, name, players, pairs, n_openings, args.opening_plies, args.warmup, args.timed, one_colour))
        print(json.dumps(done[-1]), flush=True)
        rec = dict(tool="tools/tournament_ab.py", kernel_source_hash=bench.kernel_source_hash(), device=torch.cuda.get_device_name(args.device),
                   arms="tournament = one Engine.tournament_run for the whole schedule; pairwise = one Engine.match_run_sides per ordered "
                        "pairing, results scattered into the same arrays",
                   timing="host clock (time.perf_counter) around each arm; every call returns after a device synchronise",
                   order="tournament, pairwise, tournament, pairwise, ... on one engine of one process, after the arms' games were asserted identical",
                   explores=args.explores, warmup_runs=args.warmup, timed_runs=args.timed, date=time.strftime("%Y-%m-%d"), workloads=done)
        if args.out:   # (rewritten after every workload: a run cut short leaves what it measured)
            with open(args.out, "w") as f:
                json.dump(rec, f, indent=1)
                f.write("\n")


if __name__ == "__main__":
    main()
