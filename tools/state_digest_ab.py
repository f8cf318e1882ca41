#!/usr/bin/env python3
"""A/B of answering "is this replay buffer the one I expect": the download against Engine.state_digest, on ONE engine of ONE process,
interleaved (A B A B ...), both arms over the same device replay buffer of at least --positions (1,048,576) positions.

    arm A (host)    replay_read -> synthesis_amd.digest.replay_digest over the downloaded arrays (the only route before syn_state_digest;
                    the digest instead of a comparison array by array so that both arms compute the same word)
    arm B (device)  Engine.state_digest("replay")

    python tools/state_digest_ab.py --out profiles/state_digest_ab.json

The buffer is filled by self-play (--games games at --explores per round, rounds until it is large enough). Two warm-up runs per arm,
then --timed (default 6) timed runs per arm; per arm the median and min/max of the wall time (host clock around the arm's calls, which
end in a device synchronise). A gap is "resolved" only when the medians differ by more than the larger of the two arms' ranges. The two
arms' words are compared: an A/B of two different results is void. For the device arm syn_last_timing gives the device time of its two
launches; the buffer's bytes over that time is the kernel's achieved rate, set beside the HBM rate this GPU has been measured at.
In the interleaved runs every device call follows the host arm's numpy work (an idle device); ten more calls back to back give the
call's wall time without that.
Once, as a description: the time of LearningLoop.save_state and restore_state with a buffer of that size."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_MEASURED_BYTES_PER_S = 6.29e12   # MI355X: a float4 copy reaches 6.29 TB/s of the 8.0 TB/s specification
ORDER = ("my", "op", "gid", "pi", "v")


def arm_host(eng):
    from synthesis_amd.digest import replay_digest

    R = eng.replay_read()
    return replay_digest(*(R[k] for k in ORDER)), 0.0


def arm_device(eng):
    word = eng.state_digest("replay")
    return word, eng.last_timing()[0]


def summary(xs, digits=6):
    return dict(median=round(statistics.median(xs), digits), min=round(min(xs), digits), max=round(max(xs), digits))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--positions", type=int, default=1 << 20)
    ap.add_argument("--games", type=int, default=65536)
    ap.add_argument("--explores", type=int, default=40)
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
    from synthesis_amd.learner import LearningLoop

    blob = bench.make_weights()
    rcfg = sa.parity_rollout_config(args.explores)
    rec = dict(tool="tools/state_digest_ab.py", kernel_source_hash=bench.kernel_source_hash(), device=torch.cuda.get_device_name(args.device),
               timing="host clock (time.perf_counter) around an arm's calls, which end in a device synchronise",
               order="host, device, host, device, ... on one engine of one process",
               arms=dict(host="replay_read -> synthesis_amd.digest.replay_digest", device="Engine.state_digest('replay')"),
               explores=args.explores, warmup_runs=args.warmup, timed_runs=args.timed, date=time.strftime("%Y-%m-%d"),
               not_measured=["any training run continued across sessions", "buffers that do not fit the Infinity Cache (256 MB): the "
                             "repeated runs here may read the buffer from it, not from HBM"])
    with sa.Engine(concurrent_games=min(args.games, 65536), max_explores=args.explores, device=args.device) as eng:
        loop = LearningLoop(eng, "mlp", blob, replay="device", seed=7)
        eng.replay_reserve(args.positions + args.games * 63)
        rounds = 0
        while eng.replay_size() < args.positions:
            eng.selfplay(rcfg, base_seed=7, n_games=args.games, first_game=rounds * args.games, outputs=False)
            eng.replay_append_selfplay(rounds * args.games)
            rounds += 1
        n = eng.replay_size()
        rec.update(buffer_positions=n, buffer_bytes=n * 72, selfplay_rounds=rounds, games_per_round=args.games)
        arms = (("host", arm_host), ("device", arm_device))
        wall = {a: [] for a, _ in arms}
        kernel_ms, words = [], {}
        for i in range(args.warmup + args.timed):
            for name, fn in arms:   # interleaved: drift of the box lands on both arms alike
                t = time.perf_counter()
                word, ms = fn(eng)
                dt = time.perf_counter() - t
                words.setdefault(name, set()).add(word)
                if i >= args.warmup:
                    wall[name].append(dt)
                    if name == "device":
                        kernel_ms.append(ms)
        same = words["host"] == words["device"] and len(words["device"]) == 1
        assert same, f"the arms computed different words: {words}"
        rec["digest"] = f"{next(iter(words['device'])):016x}"
        rec["arms_computed_the_same"] = bool(same)
        for name, _ in arms:
            rec[name] = dict(wall_seconds=summary(wall[name]), wall_seconds_per_run=[round(x, 6) for x in wall[name]])
        h, d = rec["host"]["wall_seconds"], rec["device"]["wall_seconds"]
        spread = max(h["max"] - h["min"], d["max"] - d["min"])
        rec["median_wall_host_minus_device"] = round(h["median"] - d["median"], 6)
        rec["larger_min_max_range"] = round(spread, 6)
        rec["resolved"] = bool(abs(h["median"] - d["median"]) > spread)
        # the kernel's rate, and the same buffer under other grids (the word never depends on the grid; the time may)
        med = statistics.median(kernel_ms) / 1e3
        rate = n * 72 / med
        grids = {}
        for cap in (256, 512, 1024, 2048, 4096):
            ts = []
            for _ in range(5):
                assert eng.state_digest("replay", max_workgroups=cap) == next(iter(words["device"]))
                ts.append(eng.last_timing()[0] / 1e3)
            grids[str(cap)] = dict(kernel_seconds_median=round(statistics.median(ts), 7), bytes_per_s=round(n * 72 / statistics.median(ts), -6))
        # the device arm again, ten calls back to back: in the interleaved runs every call follows the host arm's numpy work, i.e. a
        # device that has been idle for the length of that work
        back = []
        for _ in range(10):
            t = time.perf_counter()
            eng.state_digest("replay")
            back.append(time.perf_counter() - t)
        rec["device"]["back_to_back_wall_seconds"] = summary(back)
        words_per_s = n * 18 / med
        rec["kernel"] = dict(device_seconds=summary([ms / 1e3 for ms in kernel_ms], 7), launches=2, bytes_per_s=round(rate, -6),
                             words_per_s=round(words_per_s, -6), hbm_measured_bytes_per_s=HBM_MEASURED_BYTES_PER_S,
                             share_of_hbm_rate=round(rate / HBM_MEASURED_BYTES_PER_S, 4), by_max_workgroups=grids,
                             per_word="five 64-bit multiplies (two finalise, one (w + 1) * GOLDEN) and a 64-bit add of the index term",
                             bound_by=("the integer multiplies: the kernel moves less than half of what the memory system delivers to a copy"
                                       if rate < 0.5 * HBM_MEASURED_BYTES_PER_S else "memory: the kernel moves bytes at more than half of a copy's rate"))
        # once, as a description: the state file at this size (the loop's trainer is the constructor's, the buffer the one above)
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "state.npz")
            t = time.perf_counter()
            loop.save_state(path)
            t_save = time.perf_counter() - t
            size = os.path.getsize(path)
            fresh = LearningLoop(eng, "mlp", blob, replay="device", seed=7)
            t = time.perf_counter()
            fresh.restore_state(path)
            t_restore = time.perf_counter() - t
            assert eng.state_digest("replay") == next(iter(words["device"]))
        rec["state_file"] = dict(save_state_seconds=round(t_save, 4), restore_state_seconds=round(t_restore, 4), file_bytes=size,
                                 note="one run each, a temporary directory of the local file system; a description, not a comparison")
    print(json.dumps(rec), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
