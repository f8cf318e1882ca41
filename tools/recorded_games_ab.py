#!/usr/bin/env python3
"""A/B of recorded games: the route over the host against Engine.games_run_recorded, on ONE engine of ONE process, interleaved
(A B A B ...), both arms playing the same games; their records are compared bit for bit (an A/B of two different results is void).

    arm A (host)    per ply ONE Engine.mcts_search over the live games, then numpy: sample_action's draws (a numpy StdRng), the stop
                    rule, match.step, and at the end z, t and store_rewards — arena.host_match extended by run_game's tail
    arm B (device)  Engine.games_run_recorded

    python tools/recorded_games_ab.py --out profiles/recorded_games_ab.json --first-results profiles/recorded_games_first_results.txt

One player (bench.make_weights(), the engine's network) on both sides, the default rollout configuration at --explores (800). Shapes:
4,096 and 65,536 starts from arena.random_openings(n, 8, seed), and 4,096 starts drawn from a played buffer
(Engine.replay_select_positions). Two warm-up runs per arm, then --timed (default 6) timed runs per arm; per arm the median and
min/max of the wall time (host clock around the arm's calls, which end in a device synchronise). A gap is "resolved" only when the
medians differ by more than the larger of the two arms' ranges. For the device arm syn_last_timing gives the summed device time of its
plies; the share of that arm that is no search launch is taken from a kernel trace (profiles/recorded_games_kernel_trace.txt), not
from here: this record reports wall time minus the device time of the plies (host work and transfers between plies) as
`device_arm_outside_the_plies`.

In the same record: the recorded call from the empty board against Engine.selfplay on the same games (identical records; per-ply
launches that drain against one persistent kernel — the ratio is reported, it is no target), and the learning loop's iteration time
with and without exploring_starts=0.25 at the bench's loop shape (8,192 games of 200 explores, keep 20,000, one epoch, batch 32).

--first-results writes descriptions, not claims: rows per game and game length from 8-ply starts and from buffer starts against from
the empty board, and the share of recorded rows whose state the buffer did not already hold."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

U32, U64, F32 = np.uint32, np.uint64, np.float32
KEYS = ("rewards", "plies", "moves", "final_bb", "rng_words", "rows", "states", "pis", "vs", "actions", "root_nodes", "final_kind")


# ---- StdRng::seed_from_u64(seed) in numpy, many seeds at once (rand_core 0.6 seed_from_u64 + ChaCha12, block counter = word >> 4)
def stdrng_words(seeds, n_blocks):
    """uint32 [n, 16 * n_blocks]: the first output words of every seed's generator"""
    seeds = np.asarray(seeds, U64)
    n = seeds.size
    key = np.zeros((n, 8), U32)
    with np.errstate(over="ignore"):
        state = seeds.copy()
        for i in range(8):
            state = state * U64(6364136223846793005) + U64(11634580027462260723)
            xs = (((state >> U64(18)) ^ state) >> U64(27)).astype(U32)
            rot = (state >> U64(59)).astype(U32)
            key[:, i] = (xs >> rot) | (xs << ((U32(32) - rot) & U32(31)))
        out = np.zeros((n, 16 * n_blocks), U32)
        rotl = lambda x, k: (x << U32(k)) | (x >> U32(32 - k))
        for blk in range(n_blocks):
            s = np.zeros((16, n), U32)
            s[0], s[1], s[2], s[3] = 0x61707865, 0x3320646E, 0x79622D32, 0x6B206574
            s[4:12] = key.T
            s[12] = blk
            x = s.copy()

            def qr(a, b, c, d):
                x[a] += x[b]; x[d] = rotl(x[d] ^ x[a], 16)
                x[c] += x[d]; x[b] = rotl(x[b] ^ x[c], 12)
                x[a] += x[b]; x[d] = rotl(x[d] ^ x[a], 8)
                x[c] += x[d]; x[b] = rotl(x[b] ^ x[c], 7)

            for _ in range(6):
                qr(0, 4, 8, 12); qr(1, 5, 9, 13); qr(2, 6, 10, 14); qr(3, 7, 11, 15)
                qr(0, 5, 10, 15); qr(1, 6, 11, 12); qr(2, 7, 8, 13); qr(3, 4, 9, 14)
            out[:, 16 * blk: 16 * blk + 16] = (x + s).T
    return out


# ---- arm A
def host_games_recorded(eng, cfg, start_my, start_op, seeds):
    """Engine.games_run_recorded's dict for one player (the engine's network) on both sides, record_mask = 1, computed over the host"""
    from synthesis_amd import arena, match

    n = int(start_my.size)
    W = stdrng_words(seeds, 4)   # 64 words per game: at most one draw per ply, and a rejected candidate has probability ~1e-9
    my, op = np.array(start_my, U64), np.array(start_op, U64)
    word = np.zeros(n, np.int64)
    alive = np.ones(n, bool)
    out = dict(rewards=np.zeros(n, F32), plies=np.zeros(n, np.int32), moves=np.full((n, 63), 255, np.uint8), final_bb=np.zeros((n, 2), U64),
               rng_words=np.zeros(n, U64), rows=np.zeros(n, np.int32), states=np.zeros((n, 63, 2), U64), pis=np.zeros((n, 63, 9), F32),
               vs=np.zeros((n, 63, 3), F32), actions=np.zeros((n, 63), np.uint8), root_nodes=np.zeros((n, 63), U32),
               final_kind=np.zeros(n, np.uint8))
    stop = bool(cfg.stop_games_when_solved)
    for ply in range(63):
        idx = np.flatnonzero(alive)
        if idx.size == 0:
            break
        m = idx.size
        ar = np.arange(m)
        res = eng.mcts_search(cfg.mcts_cfg, my[idx], op[idx], cfg.num_explores, action_selection=int(cfg.action))
        pi, sol, best = res["target_pi"], res["child_sol"], res["best_action"].astype(np.int64)
        if ply < cfg.random_actions_until:      # gen_range(0..n): widening multiply with a modulus zone, one word per candidate
            legal = arena._heights(my[idx] | op[idx]) < 7
            nl = legal.sum(axis=1).astype(U64)
            zone = U64(0xFFFFFFFF) - (U64(0xFFFFFFFF) - nl + U64(1)) % nl
            mm = W[idx, word[idx]].astype(U64) * nl
            word[idx] += 1
            rej = (mm & U64(0xFFFFFFFF)) > zone
            while rej.any():
                j = idx[rej]
                mm[rej] = W[j, word[j]].astype(U64) * nl[rej]
                word[j] += 1
                rej = (mm & U64(0xFFFFFFFF)) > zone
            col = ((np.cumsum(legal, axis=1) - 1 == (mm >> U64(32)).astype(np.int64)[:, None]) & legal).argmax(axis=1)
        elif ply < cfg.sample_actions_until:    # WeightedIndex: running f32 sums, one Uniform(0, total) draw
            samp = (sol[ar, best, 0] == 0) | (not stop)
            total = pi[:, 0].copy()
            cum = np.zeros((m, 8), F32)
            for c in range(1, 9):
                cum[:, c - 1] = total
                total = total + pi[:, c]
            u01 = ((W[idx, word[idx]] >> U32(9)) | U32(0x3F800000)).view(F32) - F32(1.0)
            chosen = u01 * total + F32(0.0)
            pick = np.zeros(m, np.int64)
            for c in range(8):
                pick = np.where(cum[:, c] <= chosen, c + 1, pick)
            col = np.where(samp, pick, best)
            word[idx] += samp
        else:
            col = best
        out["states"][idx, ply, 0], out["states"][idx, ply, 1] = my[idx], op[idx]
        out["pis"][idx, ply], out["vs"][idx, ply] = pi, res["target_q"]
        out["actions"][idx, ply] = out["moves"][idx, ply] = col
        out["root_nodes"][idx, ply] = res["num_nodes"]
        out["rows"][idx] += 1
        sol_some, sol_kind = sol[ar, col, 0] != 0, sol[ar, col, 1].copy()
        nmy, nop, over, won = match.step(my[idx], op[idx], col)
        sol_kind[over] = np.where(won[over], 0, 1)
        done = over | (sol_some & stop)
        my[idx], op[idx] = nmy, nop
        d = idx[done]
        first_moved = ply % 2 == 0
        mover_reward = np.where(sol_kind[done] == 1, 0.0, np.where(sol_kind[done] == 0, 1.0, -1.0)).astype(F32)
        out["rewards"][d] = mover_reward if first_moved else F32(0.0) - mover_reward   # (a draw is +0.0 for either mover)
        out["plies"][d] = ply + 1
        out["final_kind"][d] = sol_kind[done]
        out["final_bb"][d, 0] = nop[done] if first_moved else nmy[done]
        out["final_bb"][d, 1] = nmy[done] if first_moved else nop[done]
        out["rng_words"][d] = word[d]
        alive[d] = False
    # fill_state_info + store_rewards over every row
    k = np.arange(63)[None, :]
    npl = out["plies"][:, None]
    rows = k < npl
    last = np.where(out["final_kind"] == 1, 1, 2 - out["final_kind"].astype(np.int64))[:, None]
    zk = np.where(((npl - 1 - k) % 2 == 1) & (last != 1), 2 - last, last)
    z = (zk[..., None] == np.arange(3)[None, None, :]).astype(F32)
    t = ((k + 1).astype(F32) / np.maximum(npl, 1).astype(F32))[..., None]
    q = out["vs"]
    vt = int(cfg.value_target)
    if vt == 0:
        v = z
    elif vt == 1:
        v = q
    elif vt == 2:
        p = F32(cfg.value_target_p)
        v = q * p + z * (F32(1.0) - p)
    else:
        p = (F32(1.0) - t) * F32(cfg.value_target_from) + t * F32(cfg.value_target_to)
        v = q * (F32(1.0) - p) + z * p
    out["vs"] = np.where(rows[..., None], v, F32(0.0)).astype(F32)
    return out


def device_games_recorded(eng, cfg, blob, start_my, start_op, seeds):
    import synthesis_amd as sa
    from synthesis_amd import match

    n = int(start_my.size)
    zeros = np.zeros(n, np.int32)
    me = match.Player("net", cfg.num_explores, cfg.mcts_cfg, action=cfg.action, weights=blob)
    return eng.games_run_recorded([me], zeros, zeros, start_my, start_op, seeds, record=sa.RecordConfig.from_rollout(cfg, 1))


def same_records(a, b, keys=KEYS):
    return all(np.array_equal(np.ascontiguousarray(a[k]).view(np.uint8), np.ascontiguousarray(b[k]).view(np.uint8)) for k in keys)


def summarise(wall):
    return dict(median=round(statistics.median(wall), 4), min=round(min(wall), 4), max=round(max(wall), 4))


def interleaved(arms, warmup, timed):
    """arms: (name, fn) pairs, fn() -> (result, device_ms). Returns per arm the timed walls, device times and the last result"""
    wall = {a: [] for a, _ in arms}
    dev = {a: [] for a, _ in arms}
    last = {}
    for i in range(warmup + timed):
        for name, fn in arms:   # interleaved: drift of the box lands on both arms alike
            t = time.perf_counter()
            res, ms = fn()
            dt = time.perf_counter() - t
            if i >= warmup:
                wall[name].append(dt)
                dev[name].append(ms)
            last[name] = res
    return wall, dev, last


def compare(wall, a, b):
    sa_, sb = summarise(wall[a]), summarise(wall[b])
    spread = max(sa_["max"] - sa_["min"], sb["max"] - sb["min"])
    return {a: dict(wall_seconds=sa_, wall_seconds_per_run=[round(x, 4) for x in wall[a]]),
            b: dict(wall_seconds=sb, wall_seconds_per_run=[round(x, 4) for x in wall[b]]),
            f"median_wall_{a}_minus_{b}": round(sa_["median"] - sb["median"], 4), f"median_wall_{a}_over_{b}": round(sa_["median"] / sb["median"], 3),
            "larger_min_max_range": round(spread, 4), "resolved": bool(abs(sa_["median"] - sb["median"]) > spread)}


def run_shape(eng, cfg, blob, my, op, seeds, warmup, timed):
    arms = (("host", lambda: (host_games_recorded(eng, cfg, my, op, seeds), 0.0)),
            ("device", lambda: (device_games_recorded(eng, cfg, blob, my, op, seeds), eng.last_timing()[0])))
    wall, dev, last = interleaved(arms, warmup, timed)
    out = dict(games=int(my.size), arms_computed_the_same=bool(same_records(last["host"], last["device"])),
               rows=int(last["device"]["rows"].sum()), plies_per_game=round(float(last["device"]["plies"].mean()), 3))
    out.update(compare(wall, "host", "device"))
    outside = [w - ms / 1e3 for w, ms in zip(wall["device"], dev["device"])]
    out["device"]["plies_device_seconds_median"] = round(statistics.median(dev["device"]) / 1e3, 4)
    out["device_arm_outside_the_plies"] = dict(seconds_median=round(statistics.median(outside), 4),
                                               share_of_wall_median=round(statistics.median(o / w for o, w in zip(outside, wall["device"])), 4))
    return out, last["device"]


def run_empty_board(eng, cfg, blob, n, warmup, timed):
    """the recorded call from the empty board against Engine.selfplay on the same games"""
    zeros = np.zeros(n, U64)
    seeds = U64(7) + np.arange(n, dtype=U64)
    arms = (("selfplay", lambda: (eng.selfplay(cfg, base_seed=7, n_games=n), eng.last_timing()[0])),
            ("recorded", lambda: (device_games_recorded(eng, cfg, blob, zeros, zeros, seeds), eng.last_timing()[0])))
    wall, dev, last = interleaved(arms, warmup, timed)
    sp, rc = last["selfplay"], last["recorded"]
    keep = np.arange(63)[None, :] < sp["plies"][:, None]
    same = bool(np.array_equal(sp["plies"], rc["rows"]) and np.array_equal(sp["final_kind"], rc["final_kind"]) and
                all(np.array_equal(sp["states_bb" if k == "states" else k][keep].view(np.uint8), rc[k][keep].view(np.uint8))
                    for k in ("states", "pis", "vs", "actions", "root_nodes")))
    out = dict(games=n, identical_records=same, plies_per_game=round(float(sp["plies"].mean()), 3))
    out.update(compare(wall, "recorded", "selfplay"))
    for a in ("selfplay", "recorded"):
        out[a]["device_seconds_median"] = round(statistics.median(dev[a]) / 1e3, 4)
    return out, sp


def run_loop(blob, exploring, device):
    import synthesis_amd as sa
    from synthesis_amd.learner import LearningLoop

    with sa.Engine(concurrent_games=8192, max_explores=200, device=device) as eng:
        loop = LearningLoop(eng, "mlp", blob, seed=7, weight_decay=1e-6, replay="device", exploring_starts=exploring)
        cfg = sa.parity_rollout_config(200)
        recs = [loop.iteration(cfg, 8192, 20000, 1, 32) for _ in range(4)]
    return [dict(seconds=r["seconds"], exploring_games=r.get("exploring_games"), exploring_rows=r.get("exploring_rows"),
                 steps_in_buffer=r["steps_in_buffer"]) for r in recs[2:]]


def describe(got):
    return f"{got['rows'].mean():7.3f} rows per game, {got['plies'].mean():7.3f} plies per game, longest {int(got['plies'].max())}, shortest {int(got['plies'].min())}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--explores", type=int, default=800)
    ap.add_argument("--shapes", default="4096,65536")
    ap.add_argument("--buffer-starts", type=int, default=4096)
    ap.add_argument("--empty-board-games", type=int, default=65536)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--timed", type=int, default=6)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--no-loop", action="store_true")
    ap.add_argument("--out", default="")
    ap.add_argument("--first-results", default="")
    args = ap.parse_args()
    if args.timed < 6:
        raise SystemExit("--timed must be at least 6: fewer runs per arm do not give a range worth comparing")

    import torch  # noqa: F401  (before the engine: one HIP runtime per process)

    import bench
    import synthesis_amd as sa
    from synthesis_amd import arena

    blob = bench.make_weights()
    cfg = sa.parity_rollout_config(args.explores)
    shapes = [int(s) for s in args.shapes.split(",") if s]
    rec = dict(tool="tools/recorded_games_ab.py", kernel_source_hash=bench.kernel_source_hash(), device=torch.cuda.get_device_name(args.device),
               timing="host clock (time.perf_counter) around an arm's calls, which end in a device synchronise",
               order="host, device, host, device, ... on one engine of one process",
               arms=dict(host="per ply Engine.mcts_search over the live games + numpy draws, steps and store_rewards",
                         device="Engine.games_run_recorded"),
               network="bench.make_weights()", explores=args.explores, warmup_runs=args.warmup, timed_runs=args.timed, date=time.strftime("%Y-%m-%d"),
               not_measured=["whether exploring starts, curricula or league rows train a stronger player", "more than one rank",
                             "two different players in one call (the host arm would reload weights per ply)",
                             "the share of the device arm that is not a search launch is not taken here (a kernel trace gives it: "
                             "profiles/recorded_games_kernel_trace.txt); wall minus the plies' device time is reported instead"],
               openings={})
    lines = ["Recorded games, first results (tools/recorded_games_ab.py --first-results). Descriptions of the games the call plays;",
             "nothing here says anything about playing strength, and no training run has been judged.", "",
             f"network bench.make_weights() on both sides, {args.explores} explores, the default rollout configuration (first move from the start",
             "position random, moves sampled until turn 30 counted from the start position, value target Q)", ""]
    with sa.Engine(concurrent_games=65536, max_explores=args.explores, device=args.device) as eng:
        eng.load_weights(blob)
        # the numpy generator against the device's
        w = stdrng_words(np.array([0, 7, 1 << 40], U64), 4)
        assert all(np.array_equal(w[i], eng.debug_stdrng_u32(s, 64)) for i, s in enumerate((0, 7, 1 << 40))), "numpy StdRng differs from the device's"
        described = {}
        for n in shapes:
            my, op = arena.random_openings(n, 8, seed=n)
            res, got = run_shape(eng, cfg, blob, my, op, U64(1000) + np.arange(n, dtype=U64), args.warmup, args.timed)
            rec["openings"][str(n)] = res
            described[f"{n} starts after 8 random plies"] = got
            print(json.dumps({str(n): res}), flush=True)
        # starts from a played buffer
        nb = args.buffer_starts
        eng.replay_reserve(nb * 63)
        sp = eng.selfplay(cfg, base_seed=99, n_games=nb, outputs=False)
        eng.replay_append_selfplay(0)
        R = eng.replay_read()
        from synthesis_amd.learner import exploring_threshold

        starts = eng.replay_select_positions(0x5EED, threshold=exploring_threshold(nb, R["my"].size))
        res, got = run_shape(eng, cfg, blob, starts["my"], starts["op"], U64(5000) + np.arange(starts["my"].size, dtype=U64), args.warmup, args.timed)
        res["buffer"] = dict(games=nb, positions=int(R["my"].size), selected=int(starts["my"].size))
        rec["buffer_starts"] = res
        described[f"{starts['my'].size} starts drawn from a buffer of {nb} self-played games ({R['my'].size} positions)"] = got
        print(json.dumps(dict(buffer_starts=res)), flush=True)
        held = set(zip(R["my"].tolist(), R["op"].tolist()))
        keep = np.arange(63)[None, :] < got["rows"][:, None]
        states = list(zip(got["states"][..., 0][keep].tolist(), got["states"][..., 1][keep].tolist()))
        fresh = sum(1 for s in states if s not in held)
        # from the empty board, against self-play
        res, sp_games = run_empty_board(eng, cfg, blob, args.empty_board_games, args.warmup, args.timed)
        rec["empty_board_against_selfplay"] = res
        print(json.dumps(dict(empty_board_against_selfplay=res)), flush=True)
        lines.append(f"from the empty board ({args.empty_board_games} self-play games): {sp_games['plies'].mean():7.3f} rows per game = plies per game, "
                     f"longest {int(sp_games['plies'].max())}, shortest {int(sp_games['plies'].min())}")
        for what, g in described.items():
            lines.append(f"{what}: {describe(g)}")
        lines += ["", f"rows recorded from the buffer starts: {len(states)}; their state was not in the buffer before: {fresh} = {fresh / max(len(states), 1):.4f}",
                  "(a start position itself is always in the buffer; the rows after a start's random first move are where new states come from)"]
    if not args.no_loop:
        rec["learning_loop"] = dict(shape="8,192 games of 200 explores per iteration, keep 20,000 games, 1 epoch, batch 32, replay=device; iterations 3 and 4",
                                    without=run_loop(blob, 0.0, args.device), with_exploring_starts_0_25=run_loop(blob, 0.25, args.device))
        print(json.dumps(dict(learning_loop=rec["learning_loop"])), flush=True)
    if args.first_results:
        with open(args.first_results, "w") as f:
            f.write("\n".join(lines) + "\n")
    print("\n".join(lines), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
