"""LearningLoop.save_state / restore_state: a run that stops after two iterations and continues in a new engine and a new loop leaves
the bits of the run that never stopped — final trainer, buffer, and the records of iterations 3 and 4 with their four digests.
The shape is tests/test_gpu_reanalyse.py's: 601 games of 40 explores per iteration and a window of 1,000 games, which drops games
from the second iteration on, so a restored buffer goes through the keep-window."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.conftest import free_port

pytestmark = pytest.mark.gpu

SHAPE = (601, 1000, 1, 32)   # games per iteration, games to keep, epochs, batch
CASES = {
    "mlp_host_numpy": ("mlp", dict(replay="host"), None),
    "mlp_device_flip": ("mlp", dict(replay="device", sampler="device", flip=True), None),
    "conv_bf16_device": ("conv", dict(replay="device", precision="bf16"), None),
    "combined": ("mlp", dict(replay="device", symmetry="mirror", holdout=0.25, reanalyse=0.5, sampler="torch"), None),
    "host_then_device": ("mlp", dict(replay="host"), "device"),
}


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def blob_of(net):
    from bench import make_conv_weights, make_weights

    return make_conv_weights(20260101) if net == "conv" else make_weights(20211003)


def new_loop(net, kw, seed=7):
    import synthesis_amd as sa
    from synthesis_amd.learner import LearningLoop

    eng = sa.Engine(concurrent_games=512, max_explores=40)
    return eng, LearningLoop(eng, net, blob_of(net), seed=seed, digests=True, **kw)


def end_of(eng, loop, recs):
    S = eng.trainer_state()
    R = eng.replay_read() if loop.replay == "device" else loop.R
    recs = [{k: v for k, v in r.items() if k != "seconds"} for r in recs]
    return dict(trainer=(S["weights"], S["m"], S["v"], S["step"]), buffer={k: R[k].copy() for k in ("my", "op", "gid", "pi", "v")},
                recs=recs, weights=loop.weights.copy(), counters=(loop.iterations_done, loop.games_played))


_straight = {}


def straight(net, kw):
    """four iterations without a stop; one run per configuration, shared by the cases that compare against it"""
    import synthesis_amd as sa

    key = (net, json.dumps(kw, sort_keys=True))
    if key not in _straight:
        eng, loop = new_loop(net, kw)
        with eng:
            cfg = sa.parity_rollout_config(40)
            _straight[key] = end_of(eng, loop, [loop.iteration(cfg, *SHAPE) for _ in range(4)])
    return _straight[key]


def first_half(net, kw, path):
    import synthesis_amd as sa

    eng, loop = new_loop(net, kw)
    with eng:
        cfg = sa.parity_rollout_config(40)
        for _ in range(2):
            loop.iteration(cfg, *SHAPE)
        loop.save_state(path)


@pytest.fixture(scope="module")
def saved_mlp_host(tmp_path_factory):
    """the state file of the plain Connect4Net run after two iterations (the corruption and mismatch cases read it)"""
    path = str(tmp_path_factory.mktemp("state") / "mlp_host.npz")
    first_half("mlp", dict(replay="host"), path)
    return path


@pytest.mark.parametrize("case", list(CASES))
def test_a_resumed_run_equals_the_run_that_never_stopped(case, tmp_path, saved_mlp_host):
    import synthesis_amd as sa

    net, kw, replay_after = CASES[case]
    want = straight(net, kw)
    if kw == dict(replay="host"):
        path = saved_mlp_host
    else:
        path = str(tmp_path / "run.npz")
        first_half(net, kw, path)
    assert sorted(os.listdir(os.path.dirname(path))) == [os.path.basename(path)]
    eng, loop = new_loop(net, dict(kw, replay=replay_after) if replay_after else kw)
    with eng:
        loop.restore_state(path)
        assert (loop.iterations_done, loop.games_played) == (2, 2 * SHAPE[0])
        cfg = sa.parity_rollout_config(40)
        got = end_of(eng, loop, [loop.iteration(cfg, *SHAPE) for _ in range(2)])
    for i, name in enumerate(("weights", "m", "v")):
        assert same(got["trainer"][i], want["trainer"][i]), name
    assert got["trainer"][3] == want["trainer"][3] and got["counters"] == want["counters"]
    assert same(got["weights"], want["weights"])
    for k in want["buffer"]:
        assert same(got["buffer"][k], want["buffer"][k]), k
    assert len(want["buffer"]["my"]) < 4 * 601 * 20     # the window dropped games
    for a, b in zip(got["recs"], want["recs"][2:]):
        assert set(a) == set(b)
        for k in b:
            assert a[k] == b[k], (k, a[k], b[k])
        assert set(b["digests"]) == {"trainer", "replay", "train_data"} | ({"eval_data"} if kw.get("holdout") else set())
        assert all(len(w) == 16 and int(w, 16) >= 0 for w in b["digests"].values())
        for k in ("epoch_losses", "unique", "steps_in_buffer"):
            assert k in b
    words = [r["digests"]["trainer"] for r in want["recs"]]
    assert len(set(words)) == 4


def test_both_replay_modes_report_the_same_words():
    """digests=True: replay="host" digests its numpy buffer with synthesis_amd.digest, replay="device" on the device"""
    host, device = straight("mlp", dict(replay="host")), None
    import synthesis_amd as sa

    eng, loop = new_loop("mlp", dict(replay="device"))
    with eng:
        cfg = sa.parity_rollout_config(40)
        device = [loop.iteration(cfg, *SHAPE)["digests"] for _ in range(2)]
    assert device == [r["digests"] for r in host["recs"][:2]]


def constructed(eng, loop, net):
    """the trainer and the buffer as the constructor leaves them"""
    S = eng.trainer_state()
    blob = blob_of(net)
    zero = np.zeros_like(blob)
    n = eng.replay_size() if loop.replay == "device" else loop.R["my"].size
    return (same(S["weights"], blob) and same(S["m"], zero) and same(S["v"], zero) and S["step"] == 0 and n == 0 and same(loop.weights, blob)
            and (loop.iterations_done, loop.games_played) == (0, 0))


@pytest.mark.parametrize("replay", ("host", "device"))
def test_a_changed_file_is_refused_by_the_digests(saved_mlp_host, tmp_path, replay):
    from tests import state_digest_model as model

    with np.load(saved_mlp_host) as z:
        arrays = {k: z[k] for k in z.files}
    arrays["weights"] = arrays["weights"].copy()
    arrays["weights"].view(np.uint32)[12345] ^= np.uint32(1)
    weight_path = str(tmp_path / "weight.npz")
    np.savez(weight_path, **arrays)
    with np.load(saved_mlp_host) as z:
        arrays = {k: z[k] for k in z.files}
    arrays["replay_pi"] = arrays["replay_pi"].copy()
    arrays["replay_pi"].view(np.uint32)[-1, 8] ^= np.uint32(1 << 31)
    row_path = str(tmp_path / "row.npz")
    np.savez(row_path, **arrays)
    eng, loop = new_loop("mlp", dict(replay=replay))
    with eng:
        network = eng.state_digest("network")
        assert constructed(eng, loop, "mlp") and network == model.network(blob_of("mlp"))
        for path, part in ((weight_path, "trainer"), (row_path, "replay")):
            with pytest.raises(ValueError, match=rf"digest: {part} [0-9a-f]{{16}} != [0-9a-f]{{16}}"):
                loop.restore_state(path)
            assert constructed(eng, loop, "mlp") and eng.state_digest("network") == network
        loop.restore_state(saved_mlp_host)     # the loop is still good for the unchanged file
        assert loop.iterations_done == 2 and not constructed(eng, loop, "mlp")


def test_a_file_of_another_run_is_refused_by_name(saved_mlp_host):
    eng, loop = new_loop("mlp", dict(replay="host"), seed=8)
    with eng:
        with pytest.raises(ValueError, match=r"\bseed=7\b.*\bseed=8\b"):
            loop.restore_state(saved_mlp_host)
        assert constructed(eng, loop, "mlp")
    eng, loop = new_loop("conv", dict(replay="device"))
    with eng:
        with pytest.raises(ValueError, match=r"\bnet='mlp'.*\bnet='conv'"):
            loop.restore_state(saved_mlp_host)
        assert constructed(eng, loop, "conv")


def test_training_example_two_ranks_resume(tmp_path):
    """examples/train_connect4.py with two ranks (gloo, both on GPU 0): two iterations and --state, then two new ranks with --resume
    and two more iterations; both ranks end with the weights of ONE rank's four iterations without a stop, and the learner's records of
    iterations 3 and 4 carry that run's digests."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
    common = ["--games-per-train", "601", "--games-to-keep", "1000", "--explores", "40", "--epochs", "1", "--concurrent", "512",
              "--dist-backend", "gloo", "--net", "mlp", "--replay", "device", "--digests"]
    state = str(tmp_path / "run.npz")

    def launch(ranks, extra):
        port = free_port()
        env.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        head = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                "--master-port", str(port)] if ranks == 2 else [sys.executable]
        out = subprocess.run(head + [os.path.join(root, "examples", "train_connect4.py")] + common + extra, env=env,
                             stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900)
        assert out.returncode == 0, out.stdout.decode()[-3000:]
        return [json.loads(l) for l in out.stdout.decode().splitlines() if l.startswith("{")]

    launch(2, ["--iterations", "2", "--state", state])
    assert os.listdir(tmp_path) == ["run.npz"]
    resumed = launch(2, ["--iterations", "4", "--resume", state, "--dump-weights", str(tmp_path / "w")])
    single = launch(1, ["--iterations", "4", "--dump-weights", str(tmp_path / "s")])
    w0, w1, ws = (np.load(str(tmp_path / name)) for name in ("w.rank0.npy", "w.rank1.npy", "s.rank0.npy"))
    assert same(w0, w1) and same(w0, ws)
    assert [r["iteration"] for r in resumed] == [3, 4] and len(single) == 4
    for a, b in zip(resumed, single[2:]):
        for k in ("digests", "epoch_losses", "unique", "steps_in_buffer", "optimiser_steps"):
            assert a[k] == b[k], (k, a[k], b[k])
