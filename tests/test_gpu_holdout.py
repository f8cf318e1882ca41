"""Holding games out (syn_replay_set_holdout, syn_dataset_counts; csrc/replay_kernels.cuh) and LearningLoop(holdout=...):
  split   the learner's data set and the evaluation set after replay_deduplicate_to_trainer equal, bit for bit, the restatement of
          tests/dataset_eval_model.py: the hash, the two subsequences of the buffer, the existing replay_deduplicate per part, the seen
          partition — plain and with symmetry="mirror"; threshold 0 is the call as it always was; a threshold that holds out every game
          is refused with both sets unchanged
  loop    three iterations at the replay-loop tests' shapes: holdout=0.25 host against device replay, holdout=0.0 against a loop built
          without the argument, and the "after" metrics against dataset_evaluate by hand on the published weights
"""
import numpy as np
import pytest

from tests import dataset_eval_model as dm
from tests.test_gpu_replay_device import EXPLORES, host_positions, same

pytestmark = pytest.mark.gpu

KEY = 0x1234_5678_9ABC_DEF0
N_GAMES = 40
KEYS4 = ("my_bb", "op_bb", "pis", "vs")


@pytest.fixture(scope="module")
def setup(golden_dir):
    """an engine with a trainer and about 40 tiny self-play games in its replay buffer; the same positions on the host"""
    import os

    import synthesis_amd as sa

    blob = np.load(os.path.join(golden_dir, "c4net_blob_f32.npy"))
    eng = sa.Engine(concurrent_games=64, max_explores=8)
    eng.load_weights(blob)
    eng.trainer_init(blob)
    sp = eng.selfplay(sa.parity_rollout_config(8), base_seed=11, n_games=N_GAMES, outputs=True)
    R = host_positions(sp, 500)
    eng.replay_reserve(N_GAMES * 63)
    assert eng.replay_append_selfplay(first_gid=500) == R["my"].size
    yield eng, R
    eng.close()


def restatement(eng, R, threshold, symmetry):
    """(learner's set, evaluation set, n_unseen) from the buffer R by the header's definition"""
    held = dm.holdout_flags(KEY, R["gid"], threshold)
    T = {k: a[~held] for k, a in R.items()}
    H = {k: a[held] for k, a in R.items()}
    D = eng.replay_deduplicate(T["my"], T["op"], T["pi"], T["v"], symmetry=symmetry)
    if not held.any():
        return D, None, 0
    E = eng.replay_deduplicate(H["my"], H["op"], H["pi"], H["v"], symmetry=symmetry)
    my, op = E["my_bb"], E["op_bb"]
    n_train = D["my_bb"].size
    if symmetry == "mirror":
        n_train = D["canonical"]
        mmy, mop = eng.positions_mirror(my, op)
        flipped = (mmy < my) | ((mmy == my) & (mop < op))
        my, op = np.where(flipped, mmy, my), np.where(flipped, mop, op)
    seen = dm.is_seen(my, op, D["my_bb"][:n_train], D["op_bb"][:n_train])
    E, n_unseen = dm.unseen_first(E, seen)
    return D, E, n_unseen


def choose_threshold(R):
    """the smallest of a few thresholds at which — checked here on the CPU — both parts are non-empty and seen and unseen rows exist"""
    for frac in (0.2, 0.3, 0.4, 0.5):
        t = dm.holdout_threshold(frac)
        held = dm.holdout_flags(KEY, R["gid"], t)
        if not held.any() or held.all():
            continue
        train = set(zip(R["my"][~held].tolist(), R["op"][~held].tolist()))
        ev = set(zip(R["my"][held].tolist(), R["op"][held].tolist()))
        if 0 < len(ev - train) < len(ev):
            return t
    raise AssertionError("no threshold splits the buffer as the test needs")


@pytest.mark.parametrize("symmetry", ["none", "mirror"])
def test_split_equals_the_restatement(setup, symmetry):
    from synthesis_amd.engine import SynthesisAmdError

    eng, R = setup
    assert len(set(zip(R["my"].tolist(), R["op"].tolist()))) < R["my"].size   # duplicated openings
    t = choose_threshold(R)
    D, E, n_unseen = restatement(eng, R, t, symmetry)
    assert E is not None and 0 < n_unseen < E["my_bb"].size
    eng.replay_set_holdout(KEY, t)
    try:
        got_n = eng.replay_deduplicate_to_trainer(symmetry=symmetry)
        assert got_n == ((D["canonical"], D["my_bb"].size) if symmetry == "mirror" else D["my_bb"].size)
        tr, ev = eng.train_get_data(), eng.dataset_get()
        for k in KEYS4:
            assert same(tr[k], D[k]), ("train", k)
            assert same(ev[k], E[k]), ("eval", k)
        assert eng.dataset_counts() == (E["my_bb"].size, n_unseen)
        # no unseen row's state is in the learner's set; with the plain form every seen row's is
        train_keys = set(zip(tr["my_bb"].tolist(), tr["op_bb"].tolist()))
        ev_keys = list(zip(ev["my_bb"].tolist(), ev["op_bb"].tolist()))
        assert not any(k in train_keys for k in ev_keys[:n_unseen])
        if symmetry == "none":
            assert all(k in train_keys for k in ev_keys[n_unseen:])
        # either range evaluates; together they are the whole set
        a = eng.dataset_evaluate("eval", 0, n_unseen)
        b = eng.dataset_evaluate("eval", n_unseen, ev["my_bb"].size - n_unseen)
        c = eng.dataset_evaluate("eval")
        assert a["rows"] + b["rows"] == c["rows"] and a["pi_hits"] + b["pi_hits"] == c["pi_hits"] and a["v_hits"] + b["v_hits"] == c["v_hits"]
        # a threshold that holds out every game: refused, both sets as they were
        eng.replay_set_holdout(KEY, 1 << 32)
        assert dm.holdout_flags(KEY, R["gid"], 1 << 32).all()
        with pytest.raises(SynthesisAmdError) as ei:
            eng.replay_deduplicate_to_trainer(symmetry=symmetry)
        assert ei.value.code == -1
        with pytest.raises(SynthesisAmdError):
            eng.replay_set_holdout(KEY, (1 << 32) + 1)
        tr2, ev2 = eng.train_get_data(), eng.dataset_get()
        assert all(same(tr2[k], tr[k]) and same(ev2[k], ev[k]) for k in KEYS4) and eng.dataset_counts() == (E["my_bb"].size, n_unseen)
        # threshold 0: today's data set; the evaluation set is not touched by the call
        eng.replay_set_holdout(KEY, 0)
        eng.replay_deduplicate_to_trainer(symmetry=symmetry)
        W = eng.replay_deduplicate(R["my"], R["op"], R["pi"], R["v"], symmetry=symmetry)
        tr0 = eng.train_get_data()
        assert all(same(tr0[k], W[k]) for k in KEYS4)
        # a threshold under which no game of this buffer is held out: today's data set and an empty evaluation set
        eng.replay_set_holdout(KEY, 1)
        assert not dm.holdout_flags(KEY, R["gid"], 1).any()
        eng.replay_deduplicate_to_trainer(symmetry=symmetry)
        tr1 = eng.train_get_data()
        assert all(same(tr1[k], W[k]) for k in KEYS4) and eng.dataset_counts() == (0, 0) and eng.dataset_get()["my_bb"].size == 0
    finally:
        eng.replay_set_holdout(KEY, 0)


METRIC_KEYS = ("rows", "mean_pi", "mean_v", "pi_acc", "v_acc")


@pytest.mark.parametrize("net", ["mlp", "conv"])
def test_loop_holdout_host_equals_device(net):
    import synthesis_amd as sa
    from bench import make_conv_weights, make_weights
    from synthesis_amd.learner import LearningLoop

    blob = make_conv_weights(20260101) if net == "conv" else make_weights(20211003)
    cfg = sa.parity_rollout_config(EXPLORES)
    recs, weights, engines = {}, {}, {}
    try:
        for arm, kw in (("host", dict(replay="host", holdout=0.25)), ("device", dict(replay="device", holdout=0.25)),
                        ("zero", dict(replay="device", holdout=0.0)), ("plain", dict(replay="device"))):
            eng = engines[arm] = sa.Engine(concurrent_games=512, max_explores=EXPLORES)
            loop = LearningLoop(eng, net, blob, seed=7, **kw)
            recs[arm] = []
            for _ in range(3):
                rec = loop.iteration(cfg, 601, 1000, 1, 32)
                recs[arm].append(rec)
                if "holdout_after" in rec:   # by hand, on the published weights
                    n, u = rec["holdout_rows"], rec["holdout_unseen"]
                    assert 0 < u < n
                    # (replay="host" uploads the set through dataset_set, which knows nothing of the learner's set: it counts every row)
                    assert eng.dataset_counts() == ((n, u) if arm == "device" else (n, n))
                    for name, rows in (("all", n), ("unseen", u)):
                        m = eng.dataset_evaluate("eval", 0, rows, blob=loop.weights)
                        assert rec["holdout_after"][name] == {k: m[k] for k in METRIC_KEYS}, (arm, name)
            weights[arm] = loop.weights.copy()
        for a, b in zip(recs["host"], recs["device"]):
            assert set(a) == set(b)
            for k in a:
                if k != "seconds":
                    assert a[k] == b[k], (k, a[k], b[k])
            assert a["holdout_before"] != a["holdout_after"] and a["unique"] + a["holdout_unseen"] <= a["steps_in_buffer"]
        assert same(weights["host"], weights["device"])
        for a, b in zip(recs["zero"], recs["plain"]):
            assert set(a) == set(b) and not any(k.startswith("holdout") for k in a)
            assert all(a[k] == b[k] for k in a if k != "seconds")
        assert same(weights["zero"], weights["plain"]) and not same(weights["zero"], weights["device"])
        # iteration k's "before" is iteration k - 1's published network on another set; on the SAME held-out games it would be its "after":
        # the split is stable while a game stays in the window, so the evaluation set only grows until the window drops games
        assert recs["device"][1]["holdout_rows"] > recs["device"][0]["holdout_rows"]
    finally:
        for eng in engines.values():
            eng.close()
