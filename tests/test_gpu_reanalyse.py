"""Device-resident reanalyse (include/synthesis_amd.h "Reanalyse"; csrc/reanalyse_kernels.cuh) against what it is defined by, bit for bit:
learner.reanalyse_flags for the selection, Engine.mcts_search on the same engine (and the CPU oracle) for the new targets, numpy f32
arithmetic for the value mix, and LearningLoop(replay="host") for the loop."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PLAYED = 24      # explores of the self-play that fills the buffer
EXPLORES = 48    # explores of the reanalysis (= the engine's max_explores)
FULL = 1 << 32
FIRST_GID = 100
N_GAMES = 40


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(bits(a), bits(b))


def assert_same_buffer(got, want, but_rows=None):
    """Every array of two replay_read() results, optionally leaving the targets of `but_rows` out"""
    keep = np.ones(want["my"].size, bool)
    if but_rows is not None:
        keep[but_rows] = False
    for k in ("my", "op", "gid"):
        assert same(got[k], want[k]), k
    for k in ("pi", "v"):
        assert same(got[k][keep], want[k][keep]), k


@pytest.fixture(scope="module")
def blob(golden_dir):
    return np.load(os.path.join(golden_dir, "c4net_blob_f32.npy"))


@pytest.fixture(scope="module")
def trained(golden_dir):
    return np.load(os.path.join(golden_dir, "c4net_trained_f32.npy"))


@pytest.fixture(scope="module")
def engine():
    import synthesis_amd as sa

    eng = sa.Engine(concurrent_games=64, max_explores=EXPLORES)
    eng.replay_reserve(N_GAMES * 63 + 16)
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def played(engine, blob):
    """The buffer every case starts from: 40 self-play games of the random-init network at 24 explores (value_target = Q, no noise), read
    back once and never modified."""
    import synthesis_amd as sa

    engine.load_weights(blob)
    engine.selfplay(sa.parity_rollout_config(PLAYED), base_seed=3, n_games=N_GAMES, outputs=False)
    engine.replay_clear()
    n = engine.replay_append_selfplay(first_gid=FIRST_GID)
    R = engine.replay_read()
    assert n == R["my"].size > 600
    for a in R.values():
        a.setflags(write=False)
    return R


def refill(eng, R, weights):
    """The engine back in f32 with `weights` and exactly the rows of R in its buffer"""
    eng.set_network_arithmetic("f32")
    eng.load_weights(weights)
    eng.replay_clear()
    eng.replay_append(R["my"], R["op"], R["gid"], R["pi"], R["v"])


def searched(eng, cfg, R, rows, explores=EXPLORES, action_selection=1):
    res = eng.mcts_search(cfg, R["my"][rows], R["op"][rows], explores, action_selection=action_selection)
    return res["target_pi"], res["target_q"]


def n_moved(old_pi, new_pi):
    return int((old_pi.argmax(axis=1) != new_pi.argmax(axis=1)).sum())


def test_against_the_search_call(engine, played, trained):
    """fraction 0.37, 48 explores, value_mix 1: the selected rows are reanalyse_flags', their targets Engine.mcts_search's, the rest of the
    buffer is untouched and `moved` is the numpy count."""
    import synthesis_amd as sa
    from synthesis_amd.learner import reanalyse_flags

    cfg = sa.parity_mcts_config()
    refill(engine, played, trained)
    st = engine.replay_reanalyse(cfg, EXPLORES, key=0xABCDEF, fraction=0.37, value_mix=1.0, rows=True)
    rows = np.flatnonzero(reanalyse_flags(0xABCDEF, int(np.floor(0.37 * 4294967296.0)), None, played["gid"], played["my"], played["op"]))
    assert 0.25 * played["my"].size < rows.size < 0.5 * played["my"].size
    assert st["selected_rows"].dtype == np.int64 and np.array_equal(st["selected_rows"], rows)
    assert st["selected"] == rows.size and st["rows"] == played["my"].size and st["skipped"] == 0 and st["chunks"] == 1
    ms, launches = engine.last_timing()
    assert st["launches"] == launches == 4 and ms > 0.0   # flags, compaction, one search, one write-back
    got = engine.replay_read()
    pi, q = searched(engine, cfg, played, rows)
    assert same(got["pi"][rows], pi) and same(got["v"][rows], q)
    assert_same_buffer(got, played, but_rows=rows)
    assert st["moved"] == n_moved(played["pi"][rows], pi) and 0 < st["moved"] < rows.size


def test_fixed_point(engine, played, blob):
    """The network, configuration and explores that played the buffer, every row, value_mix 1: a reanalysed target is what self-play
    stored, so nothing changes."""
    import synthesis_amd as sa

    refill(engine, played, blob)
    cfg = sa.parity_rollout_config(PLAYED)
    st = engine.replay_reanalyse(cfg.mcts_cfg, PLAYED, key=1, threshold=FULL, action_selection=int(cfg.action), value_mix=1.0)
    assert st["selected"] == played["my"].size and st["moved"] == 0 and st["skipped"] == 0
    assert_same_buffer(engine.replay_read(), played)


def test_against_the_oracle(engine, played, trained, oracle):
    from tests.oracle_lib import parity_mcts_config as oracle_mcts_config

    import synthesis_amd as sa

    refill(engine, played, trained)
    st = engine.replay_reanalyse(sa.parity_mcts_config(), EXPLORES, key=5, fraction=0.2, value_mix=1.0, rows=True)
    rows = st["selected_rows"]
    assert rows.size > 60
    ref = oracle.c4_mcts_search(oracle_mcts_config(), trained, played["my"][rows], played["op"][rows], EXPLORES, nn_mode=oracle.ACC_FMA)
    got = engine.replay_read()
    assert same(got["pi"][rows], ref["target_pi"]) and same(got["v"][rows], ref["target_q"])
    assert not same(got["pi"][rows], played["pi"][rows])
    assert_same_buffer(got, played, but_rows=rows)


def test_more_selected_rows_than_concurrent_games(played, trained):
    import synthesis_amd as sa

    cfg = sa.parity_mcts_config()
    with sa.Engine(concurrent_games=16, max_explores=EXPLORES) as small:
        small.replay_reserve(played["my"].size)
        refill(small, played, trained)
        st = small.replay_reanalyse(cfg, EXPLORES, key=9, fraction=0.4, value_mix=1.0, rows=True)
        rows = st["selected_rows"]
        assert rows.size >= 200 and st["chunks"] == 1
        got = small.replay_read()
        pi, q = searched(small, cfg, played, rows)
        assert same(got["pi"][rows], pi) and same(got["v"][rows], q)
        assert_same_buffer(got, played, but_rows=rows)


def test_few_selected_rows_and_none(engine, played, trained):
    """m < 64 and no multiple of 16; m = 0 through before_gid, through the threshold and on an empty buffer"""
    import synthesis_amd as sa
    from synthesis_amd.learner import reanalyse_flags

    cfg = sa.parity_mcts_config()
    thr = FULL // 25
    key = next(k for k in range(100) if 16 < reanalyse_flags(k, thr, None, played["gid"], played["my"], played["op"]).sum() < 64
               and reanalyse_flags(k, thr, None, played["gid"], played["my"], played["op"]).sum() % 16 != 0)
    refill(engine, played, trained)
    st = engine.replay_reanalyse(cfg, EXPLORES, key=key, threshold=thr, value_mix=1.0, rows=True)
    rows = np.flatnonzero(reanalyse_flags(key, thr, None, played["gid"], played["my"], played["op"]))
    assert np.array_equal(st["selected_rows"], rows) and rows.size % 16 != 0 and rows.size < 64
    got = engine.replay_read()
    pi, q = searched(engine, cfg, played, rows)
    assert same(got["pi"][rows], pi) and same(got["v"][rows], q)
    assert_same_buffer(got, played, but_rows=rows)

    refill(engine, played, trained)
    zero = dict(rows=0, selected=0, skipped=0, moved=0, chunks=0, launches=0)
    st = engine.replay_reanalyse(cfg, EXPLORES, key=key, threshold=FULL, before_gid=FIRST_GID, value_mix=1.0, rows=True)
    assert st["selected"] == 0 and st["moved"] == 0 and st["chunks"] == 0 and st["selected_rows"].size == 0
    st = engine.replay_reanalyse(cfg, EXPLORES, key=key, threshold=0, value_mix=1.0)
    assert st == zero
    assert_same_buffer(engine.replay_read(), played)
    engine.replay_clear()
    assert engine.replay_reanalyse(cfg, EXPLORES, key=key, threshold=FULL, value_mix=1.0) == zero


@pytest.mark.parametrize("noisy", [False, True])
def test_chunking_does_not_show(engine, played, trained, noisy):
    """chunk_roots = 7 against the library's choice: identical buffers — also when every root draws Dirichlet noise and Fpu::Normal
    values from its own stream, which a chunk starting at job c0 must number from stream_base + c0."""
    import synthesis_amd as sa

    cfg = sa.parity_mcts_config()
    if noisy:
        cfg = sa.parity_mcts_config(fpu=sa.Fpu.Func, fpu_value=1.0, fpu_std=0.1, root_policy_noise=sa.PolicyNoise.Dirichlet, noise_alpha=0.3,
                                    noise_weight=0.25)
    out = []
    for chunk in (0, 7):
        refill(engine, played, trained)
        st = engine.replay_reanalyse(cfg, EXPLORES, key=21, fraction=0.15, value_mix=0.5, chunk_roots=chunk, rows=True)
        out.append((st, engine.replay_read()))
    (s0, b0), (s7, b7) = out
    assert s0["chunks"] == 1 and s7["chunks"] == (s7["selected"] + 6) // 7 > 5 and s7["launches"] == 2 + 2 * s7["chunks"]
    assert np.array_equal(s0["selected_rows"], s7["selected_rows"]) and s0["moved"] == s7["moved"]
    assert_same_buffer(b7, b0)
    rows = s0["selected_rows"]
    assert not same(b0["pi"][rows], played["pi"][rows])
    if noisy:   # the streams are the search call's: root j on stream j
        pi, q = searched(engine, cfg, played, rows)
        assert same(b0["pi"][rows], pi)
        assert same(b0["v"][rows], played["v"][rows] * np.float32(0.5) + q * np.float32(0.5))
        plain, _ = searched(engine, sa.parity_mcts_config(), played, rows)
        assert not same(pi, plain)


def test_stream_base(engine, played, trained):
    """stream_base = 5: the j-th selected row draws from stream 5 + j — what mcts_search gives entry 5 + j of five filler positions
    followed by the selected rows."""
    import synthesis_amd as sa

    cfg = sa.parity_mcts_config(fpu=sa.Fpu.Func, fpu_value=1.0, fpu_std=0.1, root_policy_noise=sa.PolicyNoise.Dirichlet, noise_alpha=0.3,
                                noise_weight=0.25)
    refill(engine, played, trained)
    st = engine.replay_reanalyse(cfg, EXPLORES, key=33, fraction=0.1, stream_base=5, value_mix=1.0, chunk_roots=16, rows=True)
    rows = st["selected_rows"]
    assert rows.size > 32
    got = engine.replay_read()
    filler = np.zeros(5, np.uint64)
    res = engine.mcts_search(cfg, np.concatenate([filler, played["my"][rows]]), np.concatenate([filler, played["op"][rows]]), EXPLORES)
    assert same(got["pi"][rows], res["target_pi"][5:]) and same(got["v"][rows], res["target_q"][5:])
    base0, _ = searched(engine, cfg, played, rows)
    assert not same(base0, res["target_pi"][5:])   # the streams matter under this configuration


def test_value_mix(engine, played, trained):
    import synthesis_amd as sa

    cfg = sa.parity_mcts_config()
    refill(engine, played, trained)
    st = engine.replay_reanalyse(cfg, EXPLORES, key=2, fraction=0.3, value_mix=0.0, rows=True)
    rows = st["selected_rows"]
    got = engine.replay_read()
    pi, q = searched(engine, cfg, played, rows)
    assert same(got["v"], played["v"])
    assert same(got["pi"][rows], pi) and not same(pi, played["pi"][rows])
    assert_same_buffer(got, played, but_rows=rows)

    refill(engine, played, trained)
    engine.replay_reanalyse(cfg, EXPLORES, key=2, fraction=0.3, value_mix=0.25)
    got = engine.replay_read()
    want = played["v"][rows] * np.float32(0.75) + q * np.float32(0.25)
    assert want.dtype == np.float32 and same(got["v"][rows], want)
    assert not same(want, q) and not same(want, played["v"][rows])
    assert same(got["pi"][rows], pi)
    assert_same_buffer(got, played, but_rows=rows)


def test_after_a_keep_window(engine, played, trained):
    """A keep-window that drops games moves the buffer into its second allocation: the call rewrites the rows replay_read returns, and
    before_gid leaves the newest games alone."""
    import synthesis_amd as sa

    cfg = sa.parity_mcts_config()
    refill(engine, played, trained)
    engine.replay_keep_games_from(FIRST_GID + 7)
    before = engine.replay_read()
    keep = played["gid"] >= FIRST_GID + 7
    assert 0 < before["my"].size < played["my"].size and same(before["pi"], played["pi"][keep])
    cut = FIRST_GID + 30
    st = engine.replay_reanalyse(cfg, EXPLORES, key=4, threshold=FULL, before_gid=cut, value_mix=1.0, rows=True)
    rows = np.flatnonzero(before["gid"] < cut)
    assert np.array_equal(st["selected_rows"], rows) and 0 < rows.size < before["my"].size
    got = engine.replay_read()
    pi, q = searched(engine, cfg, before, rows)
    assert same(got["pi"][rows], pi) and same(got["v"][rows], q)
    assert_same_buffer(got, before, but_rows=rows)
    assert not same(got["pi"][rows], before["pi"][rows])


def test_skipped_rows(engine, played, trained, oracle):
    """A finished position and a full board, appended by the caller: drawn by the hash, counted in `skipped`, never searched, untouched"""
    import synthesis_amd as sa
    from synthesis_amd.learner import searchable_positions

    cell = lambda r, c: 1 << (r + 7 * c)
    won_op = sum(cell(r, 0) for r in range(4))                  # four in column 0 for the side that just moved
    won_my = cell(0, 1) | cell(0, 2) | cell(0, 3)
    full = [0, 0]
    for c in range(9):
        for r in range(7):
            full[((r // 2) + c) % 2] |= cell(r, c)
    assert oracle.c4_won(won_op) and not oracle.c4_won(won_my)
    assert full[0] | full[1] == (1 << 63) - 1 and not oracle.c4_won(full[0]) and not oracle.c4_won(full[1])
    extra_my, extra_op = np.array([won_my, full[0]], np.uint64), np.array([won_op, full[1]], np.uint64)
    assert not searchable_positions(extra_my, extra_op).any()
    head = {k: a[:50] for k, a in played.items()}
    R = dict(my=np.concatenate([head["my"][:20], extra_my, head["my"][20:]]), op=np.concatenate([head["op"][:20], extra_op, head["op"][20:]]),
             gid=np.concatenate([head["gid"][:20], [500, 501], head["gid"][20:]]).astype(np.int64),
             pi=np.concatenate([head["pi"][:20], np.full((2, 9), 1 / 9, np.float32), head["pi"][20:]]),
             v=np.concatenate([head["v"][:20], np.full((2, 3), 1 / 3, np.float32), head["v"][20:]]))
    refill(engine, R, trained)
    cfg = sa.parity_mcts_config()
    st = engine.replay_reanalyse(cfg, EXPLORES, key=8, threshold=FULL, value_mix=1.0, rows=True)
    rows = np.delete(np.arange(52), [20, 21])
    assert st["skipped"] == 2 and st["selected"] == 50 and st["rows"] == 52 and np.array_equal(st["selected_rows"], rows)
    got = engine.replay_read()
    pi, q = searched(engine, cfg, R, rows)
    assert same(got["pi"][rows], pi) and same(got["v"][rows], q)
    assert_same_buffer(got, R, but_rows=rows)
    # the gid bound comes first: a row that is not eligible is not counted as skipped either
    refill(engine, R, trained)
    st = engine.replay_reanalyse(cfg, EXPLORES, key=8, threshold=FULL, before_gid=500, value_mix=1.0)
    assert st["skipped"] == 0 and st["selected"] == 50


def test_f16x2_engine(engine, played, trained):
    import synthesis_amd as sa

    cfg = sa.parity_mcts_config()
    refill(engine, played, trained)
    try:
        engine.set_network_arithmetic("f16x2")
        st = engine.replay_reanalyse(cfg, EXPLORES, key=12, fraction=0.25, value_mix=1.0, rows=True)
        rows = st["selected_rows"]
        got = engine.replay_read()
        pi, q = searched(engine, cfg, played, rows)
        assert rows.size > 100 and same(got["pi"][rows], pi) and same(got["v"][rows], q)
        assert_same_buffer(got, played, but_rows=rows)
    finally:
        engine.set_network_arithmetic("f32")


def test_conv_network(engine, played, trained, golden_dir):
    import synthesis_amd as sa

    cfg = sa.parity_mcts_config()
    refill(engine, played, trained)
    try:
        engine.load_weights_conv(np.load(os.path.join(golden_dir, "c4conv_trained_f32.npy")))
        st = engine.replay_reanalyse(cfg, EXPLORES, key=13, fraction=0.25, value_mix=1.0, rows=True)
        rows = st["selected_rows"]
        got = engine.replay_read()
        pi, q = searched(engine, cfg, played, rows)
        assert rows.size > 100 and same(got["pi"][rows], pi) and same(got["v"][rows], q)
        assert_same_buffer(got, played, but_rows=rows)
        engine.load_weights(trained)
        mlp_pi, _ = searched(engine, cfg, played, rows)
        assert not same(pi, mlp_pi)   # the conv network really searched
    finally:
        engine.load_weights(trained)


def test_everything_else_is_only_observed(engine, played, blob, trained):
    """The trainer's state, the learner's data set, the evaluation set and the engine's network are what they were before the call"""
    import synthesis_amd as sa

    refill(engine, played, trained)
    engine.trainer_init(blob)
    engine.train_set_data(played["my"][:200], played["op"][:200], played["pi"][:200], played["v"][:200])
    engine.train_epoch(np.arange(192), 32, 1e-3)
    engine.dataset_set(played["my"][200:300], played["op"][200:300], played["pi"][200:300], played["v"][200:300])

    def observe():
        s = engine.trainer_state()
        return ([s[k] for k in ("weights", "m", "v", "grads")] + [np.array([s["step"]])] + list(engine.train_get_data().values()) +
                list(engine.dataset_get().values()) + list(engine.policy_eval(played["my"][:64], played["op"][:64])))

    before = observe()
    st = engine.replay_reanalyse(sa.parity_mcts_config(), EXPLORES, key=3, fraction=0.5, value_mix=0.5)
    assert st["selected"] > 200 and st["moved"] > 0
    for a, b in zip(before, observe()):
        assert same(a, b)


def test_refusals(engine, played, trained):
    """Every refusal of the header, with the buffer byte-identical afterwards"""
    import synthesis_amd as sa
    from synthesis_amd.engine import CReanalyseConfig, SynthesisAmdError

    cfg = sa.parity_mcts_config()
    refill(engine, played, trained)
    ok = dict(mcts_cfg=cfg, explores=EXPLORES, key=1, threshold=FULL, value_mix=1.0)
    INVALID, UNSUPPORTED, NO_WEIGHTS, CAPACITY = -1, -5, -4, -6
    cases = [(dict(mcts_cfg=None), INVALID), (dict(threshold=FULL + 1), INVALID), (dict(value_mix=1.5), INVALID),
             (dict(value_mix=-0.01), INVALID), (dict(value_mix=float("nan")), INVALID), (dict(explores=-1), INVALID),
             (dict(explores=EXPLORES + 1), CAPACITY), (dict(action_selection=2), INVALID), (dict(chunk_roots=-1), INVALID),
             (dict(mcts_cfg=sa.parity_mcts_config(fpu=sa.Fpu.FuncPtr)), UNSUPPORTED),
             (dict(mcts_cfg=sa.parity_mcts_config(exploration=7)), INVALID)]
    for kw, code in cases:
        with pytest.raises(SynthesisAmdError) as e:
            engine.replay_reanalyse(**dict(ok, **kw))
        assert e.value.code == code, (kw, e.value)
        assert_same_buffer(engine.replay_read(), played)
    # cfg NULL, and selected_rows too small (SYN_ERR_CAPACITY before anything changes): the C entry point itself
    c = cfg.to_c()
    lib, h = engine._lib, engine._h
    assert lib.syn_replay_reanalyse(h, C.byref(c), None, None, None, 0) == INVALID
    r = CReanalyseConfig(1, FULL, (1 << 63) - 1, 0, EXPLORES, 1, 1.0, 0)
    few = np.zeros(10, np.int64)
    assert lib.syn_replay_reanalyse(h, C.byref(c), C.byref(r), None, few.ctypes.data_as(C.c_void_p), few.size) == CAPACITY
    assert not few.any()
    assert_same_buffer(engine.replay_read(), played)
    with sa.Engine(concurrent_games=64, max_explores=EXPLORES) as other:
        with pytest.raises(SynthesisAmdError) as e:   # weights, but no buffer reserved
            other.load_weights(trained)
            other.replay_reanalyse(**ok)
        assert e.value.code == INVALID
    with sa.Engine(concurrent_games=64, max_explores=EXPLORES) as other:
        other.replay_reserve(played["my"].size)
        other.replay_append(played["my"], played["op"], played["gid"], played["pi"], played["v"])
        with pytest.raises(SynthesisAmdError) as e:   # a buffer, but no weights
            other.replay_reanalyse(**ok)
        assert e.value.code == NO_WEIGHTS
        assert_same_buffer(other.replay_read(), played)


def test_learning_loop_reanalyses_the_same_rows_in_both_replay_modes():
    """LearningLoop(reanalyse=0.5) for three iterations, replay="host" against replay="device": identical records and final weights;
    reanalyse=0.0 trains the weights of a loop built without the argument."""
    import synthesis_amd as sa
    from bench import make_weights
    from synthesis_amd.learner import LearningLoop

    blob = make_weights(20211003)
    cfg = sa.parity_rollout_config(40)
    recs, weights = {}, {}
    for arm, kw in (("host", dict(replay="host", reanalyse=0.5)), ("device", dict(replay="device", reanalyse=0.5)),
                    ("off", dict(replay="device", reanalyse=0.0)), ("plain", dict(replay="device"))):
        with sa.Engine(concurrent_games=512, max_explores=40) as eng:
            loop = LearningLoop(eng, "mlp", blob, seed=7, **kw)
            recs[arm] = [loop.iteration(cfg, 601, 1000, 1, 32) for _ in range(3)]
            weights[arm] = loop.weights.copy()
    for a, b in zip(recs["host"], recs["device"]):
        for k in ("reanalysed", "reanalyse_moved", "steps_in_buffer", "unique", "optimiser_steps", "epoch_losses"):
            assert a[k] == b[k], (k, a[k], b[k])
        assert set(a["seconds"]) == set(b["seconds"]) and "reanalyse" in a["seconds"]
    done = [r["reanalysed"] for r in recs["device"]]
    # iteration 1 keeps 399 of iteration 0's 601 games (the window of 1000 games) and reanalyses about half of their rows
    older = recs["device"][1]["steps_in_buffer"] - round(recs["device"][1]["plies_per_game"] * 601)
    assert done[0] == 0 and 0.4 * older < done[1] < 0.6 * older and done[2] > 0
    assert 0 < recs["device"][1]["reanalyse_moved"] <= done[1]
    assert same(weights["host"], weights["device"])
    assert same(weights["off"], weights["plain"]) and not same(weights["off"], weights["device"])
    for a, b in zip(recs["off"], recs["plain"]):
        assert set(a) == set(b) and set(a["seconds"]) == set(b["seconds"]) and "reanalysed" not in a
        assert a["epoch_losses"] == b["epoch_losses"]
