"""The replay buffer in device memory (include/synthesis_amd.h syn_replay_*; csrc/replay_kernels.cuh) against the host path on the same
engine, bit for bit: the numpy mask of LearningLoop.iteration for the compaction, the boolean filter for the keep-window,
Engine.replay_deduplicate + train_set_data for the learner's data set, and LearningLoop(replay="host") for the loop."""
import json
import os

import numpy as np
import pytest

from tests.conftest import free_port

pytestmark = pytest.mark.gpu

EXPLORES = 40


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(bits(a), bits(b))


def host_positions(sp, first_gid):
    """learner.py's row-major mask over syn_selfplay_run's padded arrays: game order, then ply order"""
    n = sp["plies"]
    mask = np.arange(63)[None, :] < n[:, None]
    return dict(my=sp["states_bb"][..., 0][mask], op=sp["states_bb"][..., 1][mask], pi=sp["pis"][mask], v=sp["vs"][mask],
                gid=(first_gid + np.arange(n.size, dtype=np.int64))[:, None].repeat(63, 1)[mask])


def assert_same_positions(got, want):
    for k in ("my", "op", "gid", "pi", "v"):
        assert same(got[k], want[k]), k


def cat(*parts):
    return {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}


@pytest.fixture(scope="module")
def blob(golden_dir):
    return np.load(os.path.join(golden_dir, "c4net_blob_f32.npy"))


@pytest.fixture(scope="module")
def cfg():
    import synthesis_amd as sa

    return sa.parity_rollout_config(EXPLORES)


@pytest.fixture
def engine(blob):
    import synthesis_amd as sa

    eng = sa.Engine(concurrent_games=512, max_explores=EXPLORES)
    eng.load_weights(blob)
    yield eng
    eng.close()


def test_compaction_equals_the_host_mask(engine, cfg):
    """replay_append_selfplay / selfplay_positions_device == the numpy mask over the padded outputs (all five arrays and their order); a
    second, smaller launch appended behind the first must not pick up the stale tail of the larger launch's output arrays."""
    import torch

    from synthesis_amd.engine import SynthesisAmdError

    sp = engine.selfplay(cfg, base_seed=3, n_games=601, outputs=True)
    want = host_positions(sp, 1000)
    total = int(sp["plies"].sum())
    assert total == want["my"].size and total > 601
    engine.replay_reserve(2 * 601 * 63)
    assert engine.replay_size() == 0
    assert engine.replay_append_selfplay(first_gid=1000) == total
    assert engine.replay_size() == total
    assert_same_positions(engine.replay_read(), want)

    # the same compaction into caller-owned (torch-allocated) device sections, with room to spare and a guard behind every section
    cap = total + 17
    dev = torch.device("cuda:0")
    secs = [torch.full((cap * w,), fill, dtype=dt, device=dev) for w, dt, fill in
            ((1, torch.int64, -1), (1, torch.int64, -1), (1, torch.int64, -1), (9, torch.float32, -7.0), (3, torch.float32, -7.0))]
    torch.cuda.synchronize()
    assert engine.selfplay_positions_device(1000, *[s.data_ptr() for s in secs], cap) == total
    got = dict(my=secs[0].cpu().numpy().view(np.uint64), op=secs[1].cpu().numpy().view(np.uint64), gid=secs[2].cpu().numpy(),
               pi=secs[3].cpu().numpy().reshape(cap, 9), v=secs[4].cpu().numpy().reshape(cap, 3))
    assert_same_positions({k: a[:total] for k, a in got.items()}, want)
    assert (got["gid"][total:] == -1).all() and (got["pi"][total:] == -7.0).all() and (got["v"][total:] == -7.0).all()
    with pytest.raises(SynthesisAmdError) as e:   # too small: SYN_ERR_CAPACITY, nothing written
        engine.selfplay_positions_device(1000, *[s.data_ptr() for s in secs], total - 1)
    assert e.value.code == -6

    # a second, smaller launch on the same engine: its positions follow, and only its own
    sp2 = engine.selfplay(cfg, base_seed=3, n_games=77, first_game=601, outputs=True)
    want2 = host_positions(sp2, 1601)
    assert engine.replay_append_selfplay(first_gid=1601) == want2["my"].size
    assert_same_positions(engine.replay_read(), cat(want, want2))
    # positions from elsewhere: host arrays and device sections onto the tail
    engine.replay_append(want2["my"], want2["op"], want2["gid"] + 100, want2["pi"], want2["v"])
    engine.replay_append_device(*[s.data_ptr() for s in secs], 5)
    last = {k: a[:5] for k, a in want.items()}
    assert_same_positions(engine.replay_read(), cat(want, want2, dict(want2, gid=want2["gid"] + 100), last))
    engine.replay_clear()
    assert engine.replay_size() == 0 and engine.replay_read()["my"].size == 0


def test_keep_window_is_the_stable_boolean_filter(engine, cfg):
    """Three appended launches with increasing first_gid; keep_games_from(g) for g inside the second launch, at its first game and
    beyond the last game == the boolean filter on the read-back copy; an empty result is legal."""
    engine.replay_reserve(3 * 200 * 63)
    firsts = (0, 200, 400)
    for g in (263, 200, 0, 1000):
        engine.replay_clear()
        for f in firsts:
            engine.selfplay(cfg, base_seed=5, n_games=200, first_game=f, outputs=False)
            engine.replay_append_selfplay(first_gid=f)
        before = engine.replay_read()
        assert before["gid"].min() == 0 and before["gid"].max() == 599
        engine.replay_keep_games_from(g)
        keep = before["gid"] >= g
        assert engine.replay_size() == int(keep.sum())
        assert_same_positions(engine.replay_read(), {k: a[keep] for k, a in before.items()})
        if g == 263:
            assert 0 < keep.sum() < keep.size
            # a second window on the moved buffer, and ids that are not in order: stability does not depend on sorted ids
            engine.replay_append(before["my"][:50], before["op"][:50], before["gid"][:50], before["pi"][:50], before["v"][:50])
            mid = engine.replay_read()
            engine.replay_keep_games_from(300)
            k2 = mid["gid"] >= 300
            assert_same_positions(engine.replay_read(), {k: a[k2] for k, a in mid.items()})
    assert engine.replay_size() == 0


def test_deduplicate_to_trainer_equals_the_host_path(engine, cfg, blob):
    """replay_deduplicate_to_trainer + train_get_data == replay_deduplicate of the read-back buffer (four arrays and the count); one
    epoch on it == a second engine fed through train_set_data with the host result (losses and the whole trainer state)."""
    import synthesis_amd as sa

    engine.selfplay(cfg, base_seed=3, n_games=601, outputs=False)
    engine.replay_reserve(601 * 63)
    n_positions = engine.replay_append_selfplay(first_gid=1000)
    R = engine.replay_read()
    D = engine.replay_deduplicate(R["my"], R["op"], R["pi"], R["v"])
    engine.trainer_init(blob)
    n_unique = engine.replay_deduplicate_to_trainer()
    assert n_unique == D["num"].size and n_unique < n_positions   # (every game contributes the empty board: the reduce is exercised)
    assert D["num"].max() > 1
    T = engine.train_get_data()
    for k in ("my_bb", "op_bb", "pis", "vs"):
        assert same(T[k], D[k]), k
    assert_same_positions(engine.replay_read(), R)   # the buffer itself is unchanged

    perm = np.random.default_rng(11).permutation(n_unique)[: n_unique // 32 * 32]
    la = engine.train_epoch(perm, 32, 1e-3)
    other = sa.Engine(concurrent_games=512, max_explores=EXPLORES)
    try:
        other.load_weights(blob)
        other.trainer_init(blob)
        other.train_set_data(D["my_bb"], D["op_bb"], D["pis"], D["vs"])
        lb = other.train_epoch(perm, 32, 1e-3)
        assert same(la, lb)
        sa_, sb_ = engine.trainer_state(), other.trainer_state()
        assert sa_["step"] == sb_["step"] == perm.size // 32
        for k in ("weights", "m", "v", "grads"):
            assert same(sa_[k], sb_[k]), k
    finally:
        other.close()


def test_capacity_and_errors(blob, cfg):
    import synthesis_amd as sa
    from synthesis_amd.engine import SynthesisAmdError

    eng = sa.Engine(concurrent_games=512, max_explores=EXPLORES)
    try:
        eng.load_weights(blob)
        with pytest.raises(SynthesisAmdError) as e:   # no self-play has run on this engine
            eng.replay_append_selfplay(0)
        assert e.value.code == -1
        eng.selfplay(cfg, base_seed=9, n_games=40, outputs=False)
        eng.replay_reserve(40 * 63)
        n40 = eng.replay_append_selfplay(0)
        old = eng.replay_read()
        assert n40 == old["my"].size > 40
        with pytest.raises(SynthesisAmdError) as e:   # SYN_ERR_NO_WEIGHTS: no trainer yet
            eng.replay_deduplicate_to_trainer()
        assert e.value.code == -4
        # a launch that yields more positions than are left: SYN_ERR_CAPACITY, the buffer exactly as it was
        sp = eng.selfplay(cfg, base_seed=9, n_games=300, first_game=40, outputs=True)
        assert int(sp["plies"].sum()) > 40 * 63 - n40
        with pytest.raises(SynthesisAmdError) as e:
            eng.replay_append_selfplay(40)
        assert e.value.code == -6
        assert eng.replay_size() == n40
        assert_same_positions(eng.replay_read(), old)
        new = host_positions(sp, 40)
        with pytest.raises(SynthesisAmdError) as e:
            eng.replay_append(new["my"], new["op"], new["gid"], new["pi"], new["v"])
        assert e.value.code == -6
        assert eng.replay_size() == n40
        assert_same_positions(eng.replay_read(), old)
        # growing keeps the contents; then the launch fits
        eng.replay_reserve(340 * 63)
        assert eng.replay_size() == n40
        assert_same_positions(eng.replay_read(), old)
        assert eng.replay_append_selfplay(40) == new["my"].size
        assert_same_positions(eng.replay_read(), cat(old, new))
        eng.replay_clear()
        eng.trainer_init(blob)
        with pytest.raises(SynthesisAmdError) as e:   # an empty buffer has no data set
            eng.replay_deduplicate_to_trainer()
        assert e.value.code == -1
    finally:
        eng.close()


@pytest.mark.parametrize("net", ["mlp", "conv"])
def test_learning_loop_device_replay_equals_host_replay(net):
    """LearningLoop for three iterations, replay="host" against replay="device", same seed, two engines: the third iteration drops part
    of the first; every iteration's record and the final weights are identical, and the device arm never asks for padded outputs."""
    import synthesis_amd as sa
    from bench import make_conv_weights, make_weights
    from synthesis_amd.learner import LearningLoop

    class Recording(sa.Engine):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            self.selfplay_outputs = []

        def selfplay(self, cfg, base_seed, n_games, first_game=0, outputs=True, counters=False):
            self.selfplay_outputs.append(bool(outputs))
            return super().selfplay(cfg, base_seed, n_games, first_game=first_game, outputs=outputs, counters=counters)

    blob = make_conv_weights(20260101) if net == "conv" else make_weights(20211003)
    cfg = sa.parity_rollout_config(EXPLORES)
    recs, weights, engines = {}, {}, {}
    try:
        for arm in ("host", "device"):
            eng = engines[arm] = Recording(concurrent_games=512, max_explores=EXPLORES)
            loop = LearningLoop(eng, net, blob, seed=7, replay=arm)
            recs[arm] = [loop.iteration(cfg, 601, 1000, 1, 32) for _ in range(3)]
            weights[arm] = loop.weights.copy()
        assert engines["host"].selfplay_outputs == [True] * 3
        assert engines["device"].selfplay_outputs == [False] * 3
        for a, b in zip(recs["host"], recs["device"]):
            for k in ("steps_in_buffer", "unique", "optimiser_steps", "epoch_losses", "plies_per_game", "games", "lr", "iteration"):
                assert a[k] == b[k], (k, a[k], b[k])
            assert set(a["seconds"]) == set(b["seconds"])
        new = [round(r["plies_per_game"] * 601) for r in recs["host"]]
        assert new[2] < recs["host"][2]["steps_in_buffer"] < sum(new)   # the window of 1000 games dropped games of earlier iterations
        assert same(weights["host"], weights["device"])
        assert not np.array_equal(weights["host"], blob)
        # the learner's data set is still readable on the device arm (what logs_dir writes)
        assert engines["device"].train_get_data()["my_bb"].size == recs["device"][2]["unique"]
    finally:
        for eng in engines.values():
            eng.close()


def test_training_example_two_ranks_device_replay(tmp_path):
    """examples/train_connect4.py --replay device with two ranks (gloo, both on GPU 0): both ranks end with the same weights, and they
    are the one-rank --replay host run's, bit for bit."""
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
    port = free_port()
    env.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    common = ["--iterations", "2", "--games-per-train", "601", "--explores", "40", "--epochs", "1", "--concurrent", "512",
              "--dist-backend", "gloo", "--net", "mlp"]
    prefix = str(tmp_path / "w")
    out = subprocess.run(
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
         "--master-port", str(port), os.path.join(root, "examples", "train_connect4.py")] + common +
        ["--replay", "device", "--dump-weights", prefix], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900)
    assert out.returncode == 0, out.stdout.decode()[-3000:]
    w0, w1 = np.load(prefix + ".rank0.npy"), np.load(prefix + ".rank1.npy")
    assert same(w0, w1)
    lines = [json.loads(l) for l in out.stdout.decode().splitlines() if l.startswith("{")]
    assert len(lines) == 2 and lines[0]["games"] == 601 and lines[1]["optimiser_steps"] > 0
    single = str(tmp_path / "s")
    one = subprocess.run([sys.executable, os.path.join(root, "examples", "train_connect4.py")] + common +
                         ["--replay", "host", "--dump-weights", single], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                         timeout=900)
    assert one.returncode == 0, one.stdout.decode()[-3000:]
    ws = np.load(single + ".rank0.npy")
    assert same(ws, w0), "two ranks on the device replay buffer and one rank on the host replay buffer train the same network"
    l1 = [json.loads(l) for l in one.stdout.decode().splitlines() if l.startswith("{")]
    for a, b in zip(l1, lines):
        for k in ("steps_in_buffer", "unique", "optimiser_steps", "epoch_losses"):
            assert a[k] == b[k], k
