"""CPU-only tests: the C-ABI library loads and exports every symbol include/synthesis_amd.h declares (no compute calls
without a GPU), struct layouts agree between the header, the ctypes mirrors and the device structs, host-side config
mirrors carry the reference's values, and the N>1 sharding / reduce plumbing works under gloo with world_size 2."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    """a TCP port nobody listens on right now (the rendezvous of a torch.distributed.run child): a fixed number collides with a
    previous run's socket in TIME_WAIT or with another job on the host"""
    import socket

    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as sk:
        sk.bind(("127.0.0.1", 0))
        return str(sk.getsockname()[1])


def header_text():
    return open(os.path.join(ROOT, "include", "synthesis_amd.h")).read()


def test_library_exports_every_declared_symbol():
    from synthesis_amd.engine import ABI_SYMBOLS, load_library

    declared = set(re.findall(r"\b(syn_[a-z0-9_]+)\s*\(", header_text()))
    declared -= {"syn_status"}
    assert declared == set(ABI_SYMBOLS), declared ^ set(ABI_SYMBOLS)
    lib = load_library()
    for name in sorted(declared):
        assert hasattr(lib, name), name
    # exported with C linkage from the in-tree .so (what the reference-side FFI would bind)
    out = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "synthesis_amd", "libsynthesis_amd.so")]).decode()
    for name in declared:
        assert re.search(rf"\bT {name}\b", out), name


def test_struct_layouts_match_header():
    from synthesis_amd.config import CEngineConfig, CMctsConfig, CRolloutConfig
    from synthesis_amd.engine import CCounters, CSearchResult, CTrainConfig

    h = header_text()

    def fields(struct):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), h, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        # (a data member `type name[n];` or a function pointer `type (*name)(void);`)
        return [m.group(1) or m.group(2) for m in re.finditer(r"\b([a-z_A-Z0-9]+)(?:\[\d+\])*;|\(\*([a-z_A-Z0-9]+)\)\([a-z ]*\);", body)]

    assert fields("syn_mcts_config") == [f[0] for f in CMctsConfig._fields_]
    assert fields("syn_rollout_config") == [f[0] for f in CRolloutConfig._fields_]
    assert fields("syn_engine_config") == [f[0] for f in CEngineConfig._fields_]
    assert fields("syn_search_result") == [f[0] for f in CSearchResult._fields_]
    assert fields("syn_counters") == [f[0] for f in CCounters._fields_]
    assert fields("syn_train_config") == [f[0] for f in CTrainConfig._fields_] and C.sizeof(CTrainConfig) == 24
    assert C.sizeof(CMctsConfig) == 56 and C.sizeof(CRolloutConfig) == 40 + 56   # (fpu_fn is a pointer: 8-byte alignment)
    assert C.sizeof(CSearchResult) == 4 * (9 + 27 + 9 + 27 + 1 + 3 + 3 + 1 + 1 + 9 + 3)
    assert C.sizeof(CCounters) == 96


def test_default_config_is_the_reference_parity_config():
    """syn_default_rollout_config == study-connect4/src/main.rs:28-36 + policy_mcts_cfg (58-66), explores per BASELINE."""
    import synthesis_amd as sa
    from synthesis_amd.config import CRolloutConfig
    from synthesis_amd.engine import load_library

    c = CRolloutConfig()
    load_library().syn_default_rollout_config(C.byref(c))
    p = sa.parity_rollout_config().to_c()
    for name, _ in CRolloutConfig._fields_:
        if name == "mcts_cfg":
            for n2, _ in type(c.mcts_cfg)._fields_:
                if n2 == "fpu_fn":   # a function pointer: NULL on both sides (ctypes wraps each read in a fresh object)
                    assert not c.mcts_cfg.fpu_fn and not p.mcts_cfg.fpu_fn
                    continue
                assert getattr(c.mcts_cfg, n2) == getattr(p.mcts_cfg, n2), n2
        else:
            assert getattr(c, name) == getattr(p, name), name
    assert (c.num_explores, c.random_actions_until, c.sample_actions_until, c.stop_games_when_solved) == (800, 1, 30, 0)
    assert c.value_target == sa.ValueTarget.Q and c.action == sa.ActionSelection.NumVisits
    m = c.mcts_cfg
    assert (m.exploration, m.c, m.solve, m.correct_values_on_solve, m.select_solved_nodes, m.auto_extend, m.fpu,
            m.fpu_value, m.root_policy_noise) == (1, 3.0, 1, 1, 1, 1, 0, 1.0, 0)


def test_engine_create_fails_loudly_without_gpu():
    """No CPU fallback: on a box without an MI355X, creating an engine raises with SYN_ERR_NO_DEVICE."""
    import torch

    import synthesis_amd as sa

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(sa.SynthesisAmdError) as e:
        sa.Engine(concurrent_games=16, max_explores=8)
    assert e.value.code == -2


def test_weight_image_is_a_permutation_of_the_blob():
    """Host logic: the fragment-order weight image (engine.hip build_weight_image) must contain every parameter exactly
    once at the position the MFMA lane map expects. Rebuilt here in numpy from the documented formula and checked for
    consistency properties (the device result itself is covered by the GPU parity tests)."""
    dims = [63, 128, 96, 64, 48, 12]
    S4 = [4, 8, 6, 4, 3]; NOB = [8, 6, 4, 3, 1]
    total = 0
    for l in range(5):
        K, O = dims[l], dims[l + 1]
        seen = np.zeros((O, K), np.int32)
        for s4 in range(S4[l]):
            for ob in range(NOB[l]):
                for lane in range(64):
                    for r in range(4):
                        i, q = lane & 15, lane >> 4
                        unit = 16 * ob + i if l == 4 else 16 * ob + 4 * (i & 3) + (i >> 2)
                        k = 16 * s4 + 4 * r + q
                        if unit < O and k < K:
                            seen[unit, k] += 1
        assert np.all(seen == 1), l
        total += S4[l] * NOB[l] * 256
    assert total == 30464
    # unit permutation is a bijection on each 16-block: D register r of lane-quad q holds unit 16*ob + 4*r + q
    assert sorted(4 * (i & 3) + (i >> 2) for i in range(16)) == list(range(16))


def test_shard_and_step_ranges_cover_every_game_once():
    from synthesis_amd import dist_util, shard_games

    for world in (1, 2, 4, 8):
        seen = []
        for step in range(3):
            for rank in range(world):
                first, count = dist_util.step_game_range(step, rank, world, 1000)
                seen += list(range(first, first + count))
        assert sorted(seen) == list(range(3 * world * 1000))
        for n in (0, 1, 7, 4096, 4099):
            parts = [shard_games(n, r, world) for r in range(world)]
            cover = [g for f, c in parts for g in range(f, f + c)]
            assert cover == list(range(n))
            assert max(c for _, c in parts) - min(c for _, c in parts) <= 1


WORKER = r'''
import os, sys
sys.path.insert(0, sys.argv[1])
import torch
from synthesis_amd import dist_util
rank, local_rank, world = dist_util.rank_info()
dist = dist_util.init_process_group("gloo")
first, count = dist_util.step_game_range(2, rank, world, 500)
elapsed, (games, lo) = dist_util.reduce_scalars(dist, "cpu", 1.0 + rank, [count, first])
dist.barrier()
if rank == 0:
    print("RESULT", elapsed, games, lo)
dist.destroy_process_group()
'''


def test_multi_rank_reduce_under_gloo(tmp_path):
    """The N>1 path of bench.py (barrier, MAX of elapsed, SUM of counters) with world_size 2 on CPU (gloo)."""
    script = tmp_path / "worker.py"
    script.write_text(WORKER)
    port = _free_port()
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=port)
    out = subprocess.check_output(
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
         "127.0.0.1", "--master-port", port, str(script), ROOT], env=env, stderr=subprocess.STDOUT, timeout=300).decode()
    line = [l for l in out.splitlines() if l.startswith("RESULT")][0].split()
    assert float(line[1]) == 2.0          # MAX over ranks of (1.0, 2.0)
    assert int(line[2]) == 1000           # SUM of per-rank game counts
    assert int(line[3]) == (2 * 2 + 0) * 500 + (2 * 2 + 1) * 500  # SUM of the two shard offsets


LOOP_WORKER = r'''
import os, sys, json
sys.path.insert(0, sys.argv[1])
import numpy as np
import torch  # noqa
from synthesis_amd import dist_util
from synthesis_amd.engine import NUM_PARAMS
from synthesis_amd.learner import LearningLoop

class StandInEngine:
    """No GPU here: an engine-shaped object whose results are simple functions of its inputs, so that the loop's sharding,
    gather, replay bookkeeping and broadcast can be checked under gloo with two ranks (the real engine runs in the -m gpu tests)."""
    def __init__(self): self.w = None; self.tw = None; self.loaded = []
    def load_weights(self, w): self.w = np.array(w, np.float32); self.loaded.append(float(self.w[0]))
    def trainer_init(self, w, **kw): self.tw = np.array(w, np.float32); self.steps = 0
    def selfplay(self, cfg, base_seed, n_games, first_game=0, **kw):
        g = first_game + np.arange(n_games)
        plies = (7 + g % 5).astype(np.int32)
        st = np.zeros((n_games, 63, 2), np.uint64)
        st[..., 0] = (g[:, None] * 100 + np.arange(63)[None, :]).astype(np.uint64)
        # what the games look like depends on the network in use: a rank that missed a broadcast would be caught
        st[..., 1] = np.uint64(int(round(float(self.w[0]) * 1000)))
        return dict(plies=plies, states_bb=st, pis=np.full((n_games, 63, 9), 1 / 9, np.float32), vs=np.zeros((n_games, 63, 3), np.float32),
                    final_kind=np.zeros(n_games, np.uint8))
    def replay_deduplicate(self, my, op, pi, v):
        key = np.stack([my, op], 1)
        _, idx = np.unique(key, axis=0, return_index=True)
        idx = np.sort(idx)
        return dict(my_bb=my[idx], op_bb=op[idx], pis=pi[idx], vs=v[idx], num=np.ones(idx.size, np.uint32))
    def train_set_data(self, my, op, pi, v): self.data_n = my.size; self.data_sum = int(my.sum() % 1000003)
    def train_epoch(self, perm, batch, lr):
        steps = perm.size // batch
        self.tw = self.tw + np.float32(steps * lr) + np.float32(self.data_sum * 1e-9)
        self.steps += steps
        return np.ones((steps, 2), np.float32)
    def trainer_state(self): return dict(weights=self.tw.copy(), step=self.steps)
    def trainer_publish_weights(self): self.load_weights(self.tw)
    def features(self, my, op): return np.zeros((np.asarray(my).size, 63), np.float32)

rank, local_rank, world = dist_util.rank_info()
dist = dist_util.init_process_group("gloo") if world > 1 else None
eng = StandInEngine()
loop = LearningLoop(eng, "mlp", np.full(NUM_PARAMS, 0.5, np.float32), dist=dist, seed=3, lr_schedule=[(1, 1e-3), (2, 5e-4)],
                    logs_dir=sys.argv[2] if len(sys.argv) > 2 else None)
recs = [loop.iteration(None, 101, 150, 2, 32) for _ in range(3)]
out = dict(rank=rank, world=world, w0=float(loop.weights[0]), wsum=float(loop.weights.astype(np.float64).sum()), loaded=eng.loaded,
           games=[r["games_this_rank"] for r in recs], unique=[r.get("unique") for r in recs], steps=[r.get("optimiser_steps") for r in recs],
           lr=[r["lr"] for r in recs], buffer=[r.get("steps_in_buffer") for r in recs])
# one write per record (ranks share the pipe: print() issues the text and the newline separately, and records got cut into each other)
os.write(1, ("LOOP " + json.dumps(out) + "\n").encode())
if dist is not None:
    dist.barrier(); dist.destroy_process_group()
'''


def test_learning_loop_collectives_under_gloo(tmp_path):
    """synthesis_amd.learner.LearningLoop with world_size 2 on CPU (gloo) and a stand-in engine: every rank plays its shard (101
    games: 51 + 50), rank 0 gathers, keeps the last 150 games, de-duplicates and trains, the weights are broadcast and loaded on
    both ranks before the next iteration's games — and the result equals the single-rank run's (the loop does not depend on the
    number of ranks)."""
    script = tmp_path / "loop_worker.py"
    script.write_text(LOOP_WORKER)
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
    port = _free_port()
    env.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=port)
    out = subprocess.check_output(
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
         "127.0.0.1", "--master-port", port, str(script), ROOT], env=env, stderr=subprocess.STDOUT, timeout=300).decode()
    two = sorted((json.loads(m) for m in re.findall(r"LOOP (\{[^{}]*\})", out)), key=lambda d: d["rank"])
    logs = tmp_path / "logs"
    one = json.loads([l for l in subprocess.check_output([sys.executable, str(script), ROOT, str(logs)], env=env, stderr=subprocess.STDOUT,
                                                          timeout=300).decode().splitlines() if l.startswith("LOOP")][0].split(" ", 1)[1])
    assert len(two) == 2 and two[0]["world"] == 2 and one["world"] == 1
    # what the reference writes per iteration (alpha_zero.rs:37,97-100): model_0.ot .. model_3.ot and the latest de-duplicated tensors
    from synthesis_amd.weights import load_ot
    assert sorted(os.listdir(logs / "models")) == [f"model_{i}.ot" for i in range(4)]
    assert float(load_ot(str(logs / "models" / "model_0.ot"))[0]) == 0.5
    last = load_ot(str(logs / "models" / "model_3.ot"))
    assert float(last[0]) == one["w0"] and float(last.astype(np.float64).sum()) == one["wsum"]
    st, pis, vs = (np.load(logs / f"latest_{k}.npy") for k in ("states", "pis", "vs"))
    assert st.shape == (one["unique"][2], 1, 7, 9) and pis.shape == (one["unique"][2], 9) and vs.shape == (one["unique"][2], 3)
    assert two[0]["games"] == [51, 51, 51] and two[1]["games"] == [50, 50, 50] and one["games"] == [101, 101, 101]
    assert two[0]["w0"] == two[1]["w0"] == one["w0"] and two[0]["wsum"] == two[1]["wsum"] == one["wsum"]
    assert two[0]["loaded"] == two[1]["loaded"] and len(two[1]["loaded"]) == 4   # the initial network + one broadcast per iteration
    assert two[0]["unique"] == one["unique"] and two[0]["steps"] == one["steps"] and two[0]["buffer"] == one["buffer"]
    assert two[1]["unique"] == [None] * 3                                          # only rank 0 holds the replay buffer
    assert one["lr"] == [1e-3, 5e-4, 5e-4] and one["steps"][0] > 0
    # keep_last_n_games: 3 x 101 games played, the last 150 kept
    assert one["buffer"][2] < one["buffer"][1] + sum(7 + g % 5 for g in range(202, 303))


def test_learning_loop_torch_sampler_is_libtorchs_randperm_stream():
    """sampler="torch": the epochs' orders are BatchRandSampler's own `Tensor::randperm(n, INT64_CPU)` (data.rs:29) — successive
    draws of ONE libtorch CPU generator seeded once, as in a reference run after tch::manual_seed — cut to whole batches
    (drop_last = true, data.rs:41-62). The stand-in engine of the collective tests records what the learner is handed."""
    import torch

    from synthesis_amd.engine import NUM_PARAMS
    from synthesis_amd.learner import LearningLoop

    ns = {"np": np}
    exec("class StandInEngine:" + LOOP_WORKER.split("class StandInEngine:")[1].split("rank, local_rank, world")[0], ns)
    perms = []

    class Recording(ns["StandInEngine"]):
        def train_epoch(self, perm, batch, lr):
            perms.append(np.array(perm))
            return super().train_epoch(perm, batch, lr)

    loop = LearningLoop(Recording(), "mlp", np.full(NUM_PARAMS, 0.5, np.float32), seed=11, sampler="torch")
    recs = [loop.iteration(None, 101, 150, 2, 32) for _ in range(2)]
    g = torch.Generator().manual_seed(11)
    want = [torch.randperm(r["unique"], generator=g).numpy()[: r["unique"] // 32 * 32] for r in recs for _ in range(2)]
    assert len(perms) == 4 and all(np.array_equal(a, b) for a, b in zip(perms, want))
    with pytest.raises(ValueError):
        LearningLoop(Recording(), "mlp", np.full(NUM_PARAMS, 0.5, np.float32), sampler="mt19937")


def test_every_device_entry_point_selects_its_engines_device():
    """One process may hold engines on several GPUs (one handle per host thread and GPU: SURVEY §8b), so an entry point that touches the
    device must first make the handle's device current. Read off the source: every `syn_*` function defined in csrc/engine.hip either
    calls hipSetDevice(h->device) itself, or reaches the device only through a callee that does, or makes no HIP call at all."""
    src = open(os.path.join(ROOT, "synthesis_amd", "csrc", "engine.hip")).read()
    bodies = {}
    for m in re.finditer(r"^(?:static\s+)?(?:int|const char\*|void|hipError_t)\s+([a-z0-9_]+)\s*\([^)]*\)\s*\{", src, re.M):
        depth, j = 1, m.end()
        while depth:
            depth += {"{": 1, "}": -1}.get(src[j], 0)
            j += 1
        bodies[m.group(1)] = src[m.end():j]
    abi = sorted(n for n in bodies if n.startswith("syn_") and not n.startswith("syn_internal"))
    assert len(abi) >= 45
    # entry points without a hipSetDevice of their own, and why that is right
    delegated = {
        "syn_mcts_search": "mcts_search_impl", "syn_mcts_search_rollout": "mcts_search_impl",   # the shared body selects the device
        "syn_eval_ctx_eval": "syn_eval_ctx_submit",                                                # submit + wait, both select it
    }
    host_only = {"syn_default_rollout_config", "syn_last_error", "syn_get_network_arithmetic", "syn_f16x2_plan_of_blob",
                 "syn_eval_ctx_last_error", "syn_trainer_set_precision", "syn_last_timing", "syn_last_cache_stats", "syn_last_launch_shape"}
    for name in abi:
        body = bodies[name]
        if "hipSetDevice(h->device)" in body or "hipSetDevice(device)" in body or "hipSetDevice(c->h->device)" in body:
            continue
        if name in delegated:
            assert delegated[name] in body and "hipSetDevice(h->device)" in bodies[delegated[name]], name
            continue
        assert name in host_only, f"{name} makes device calls without selecting the engine's device"
        assert not re.search(r"\bhip[A-Z][A-Za-z]+\(", body), f"{name} is listed as host-only but calls HIP"
    # helpers that allocate or copy and can be reached before the entry point's own hipSetDevice
    assert "hipSetDevice(h->device)" in bodies["upload_f16x2_image"]


def test_eight_ranks_under_gloo(tmp_path):
    """The shape an 8-GPU node runs (BASELINE configs[3] / [4]) with world_size 8 on CPU (gloo): dist_util.step_game_range + the
    barrier / MAX / SUM reduction of bench.py, and LearningLoop's fixed-layout gather with UNEVEN per-rank position counts (101 games
    over 8 ranks: five ranks play 13, three play 12; plies differ per game), the replay bookkeeping on rank 0 and the weight broadcast —
    the trained weights equal the single-rank run's bit for bit."""
    script = tmp_path / "worker.py"
    script.write_text(WORKER)
    port = _free_port()
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
    env.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=port, OMP_NUM_THREADS="1")
    out = subprocess.check_output(
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "8", "--master-addr",
         "127.0.0.1", "--master-port", port, str(script), ROOT], env=env, stderr=subprocess.STDOUT, timeout=600).decode()
    line = [l for l in out.splitlines() if l.startswith("RESULT")][0].split()
    assert float(line[1]) == 8.0 and int(line[2]) == 8 * 500              # MAX of (1..8), SUM of the per-rank game counts
    assert int(line[3]) == sum((2 * 8 + r) * 500 for r in range(8))       # SUM of the eight shard offsets of step 2
    loop = tmp_path / "loop_worker.py"
    loop.write_text(LOOP_WORKER)
    port = _free_port()
    env.update(MASTER_PORT=port)
    out = subprocess.check_output(
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "8", "--master-addr",
         "127.0.0.1", "--master-port", port, str(loop), ROOT], env=env, stderr=subprocess.STDOUT, timeout=600).decode()
    # (eight ranks share one pipe: two records can land on one line, so they are cut out by pattern — a record holds no nested braces)
    eight = sorted((json.loads(m) for m in re.findall(r"LOOP (\{[^{}]*\})", out)), key=lambda d: d["rank"])
    one = json.loads([l for l in subprocess.check_output([sys.executable, str(loop), ROOT], env=env, stderr=subprocess.STDOUT,
                                                          timeout=300).decode().splitlines() if l.startswith("LOOP")][0].split(" ", 1)[1])
    assert len(eight) == 8 and all(d["world"] == 8 for d in eight)
    assert [d["games"][0] for d in eight] == [13, 13, 13, 13, 13, 12, 12, 12]
    assert all(d["w0"] == one["w0"] and d["wsum"] == one["wsum"] for d in eight)
    assert all(d["loaded"] == eight[0]["loaded"] and len(d["loaded"]) == 4 for d in eight)
    assert eight[0]["unique"] == one["unique"] and eight[0]["steps"] == one["steps"] and eight[0]["buffer"] == one["buffer"]
    assert all(d["unique"] == [None] * 3 for d in eight[1:])


def test_bench_starts_its_own_ranks():
    """`python bench.py --gpus 2` with no launcher (how the driver runs it) must start two ranks itself: the parent never
    touches the GPU, the ranks rendezvous over 127.0.0.1 and rank 0 reports world size 2 (launch plumbing only, no GPU)."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    out = subprocess.check_output([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--check-launch"],
                                  env=env, stderr=subprocess.DEVNULL, timeout=300).decode()
    line = json.loads([l for l in out.splitlines() if l.startswith("{")][-1])
    assert line == {"check_launch": True, "n_gpus": 2, "ranks_joined": 2, "local_rank_sum": 1}


def test_bench_refuses_a_world_size_that_disagrees_with_gpus():
    """--gpus N with WORLD_SIZE != N (a launcher started a different number of ranks) is an error, never a silent 1-GPU run"""
    env = dict(os.environ, WORLD_SIZE="2", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--check-launch"], env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode != 0 and b"WORLD_SIZE=2" in r.stderr


def test_bench_dump_outputs_is_float32_within_64_mb_and_seeded(tmp_path):
    """--dump-outputs: a step's plies go out whole as float32; a step too large for 64 MB goes out as the same seeded sample of
    games in every run, with the games' row numbers beside it."""
    import bench

    small = np.random.default_rng(1).integers(7, 64, 1000).astype(np.int32)
    bench.dump_outputs(str(tmp_path / "a"), {"plies": small})
    got = np.load(tmp_path / "a" / "plies.npy")
    assert got.dtype == np.float32 and np.array_equal(got, small) and not (tmp_path / "a" / "sample_rows.npy").exists()
    big = np.random.default_rng(2).integers(7, 64, 20_000_000).astype(np.int32)
    for d in ("b", "c"):
        bench.dump_outputs(str(tmp_path / d), {"plies": big})
        assert sum(f.stat().st_size for f in (tmp_path / d).iterdir()) <= 64 << 20
    rows = np.load(tmp_path / "b" / "sample_rows.npy")
    assert np.array_equal(rows, np.load(tmp_path / "c" / "sample_rows.npy"))
    assert np.array_equal(np.load(tmp_path / "b" / "plies.npy"), big[rows.astype(np.int64)])


def test_bench_multi_rank_fails_loudly_without_gpus():
    """No GPU here: every rank of `bench.py --gpus 2` must refuse to run (there is no CPU fallback) and the launcher must
    exit non-zero without printing a bench line."""
    import torch

    if torch.cuda.device_count() >= 2:
        pytest.skip("two GPUs visible: the run would succeed")
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0"],
                       env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode != 0 and b'"metric"' not in r.stdout


def test_match_host_rules_follow_the_oracle(oracle):
    """synthesis_amd.match applies the moves of a match on the host (numpy bitboards): positions, game end and winner must
    be the oracle's Connect4 (connect4.rs:77-83,195-233) on random playouts, and the score summary must add up."""
    from synthesis_amd import match

    rng = np.random.default_rng(0)
    for g in range(200):
        moves, h = [], [0] * 9
        my = np.zeros(1, np.uint64); op = np.zeros(1, np.uint64)
        for t_ in range(63):
            c = int(rng.choice([c for c in range(9) if h[c] < 7]))
            moves.append(c); h[c] += 1
            my, op, over, w = match.step(my, op, np.array([c]))
            r = oracle.c4_play(moves)
            assert (int(my[0]), int(op[0])) == (r["my_bb"], r["op_bb"])
            assert bool(over[0]) == bool(r["over"][-1]) and bool(w[0]) == (r["winner"] >= 0 if "winner" in r else bool(w[0]))
            if over[0]:
                break
    w, d, l, s, elo = match.score(np.array([1, 1, 0, -1], np.float32))
    assert (w, d, l) == (2, 1, 1) and abs(s - 0.625) < 1e-9 and elo > 0
    p = match.rollout_player(800)
    assert p.rollout and p.mcts_cfg.auto_extend is False and p.name == "RolloutMCTS800"


def test_play_match_rejects_mixed_weight_sources():
    """A network player without weights beside one with explicit weights would search with the other's network after the
    first swap: refused up front."""
    from synthesis_amd import match
    import synthesis_amd as sa

    a = match.Player("a", 10, sa.MCTSConfig(), sa.ActionSelection.NumVisits)
    b = match.Player("b", 10, sa.MCTSConfig(), sa.ActionSelection.NumVisits, weights=np.zeros(30492, np.float32))
    with pytest.raises(ValueError):
        match.play_match(None, a, b, 4)


def test_pgn_records_match_the_reference_format():
    """utils.rs:31-52: three tag lines and the result line per game"""
    from synthesis_amd import match

    assert match.pgn_records("model_3.ot", "VanillaMCTS800", [1.0, -1.0, 0.0]) == (
        '[White "model_3.ot"]\n[Black "VanillaMCTS800"]\n[Result "1-0"]\n1-0\n'
        '[White "model_3.ot"]\n[Black "VanillaMCTS800"]\n[Result "0-1"]\n0-1\n'
        '[White "model_3.ot"]\n[Black "VanillaMCTS800"]\n[Result "1/2-1/2"]\n1/2-1/2\n')
    assert match.vanilla_player(800).action == 0 and match.vanilla_player(800).name == "VanillaMCTS800"   # rollout_action: Q
