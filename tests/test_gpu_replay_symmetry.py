"""The mirror-symmetric replay de-duplication on the device (syn_positions_mirror, syn_replay_deduplicate_symmetric,
syn_replay_deduplicate_to_trainer_symmetric; csrc/replay_kernels.cuh) against the specification, bit for bit.

The expected result is never the code under test: it is tests/symmetry_py.py's numpy canonicalisation, fed through the plain
Engine.replay_deduplicate (oracle-checked in tests/test_gpu_training.py), followed by the numpy expansion."""
import os

import numpy as np
import pytest

from tests import symmetry_py as sym

pytestmark = pytest.mark.gpu

EXPLORES = 40
KEYS = ("my_bb", "op_bb", "pis", "vs", "num")


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(bits(a), bits(b))


def expected(engine, my, op, pi, v):
    return sym.symmetric_deduplicate(engine.replay_deduplicate, my, op, pi, v)


def assert_same_set(got, want, keys=KEYS):
    assert got["canonical"] == want["canonical"], (got["canonical"], want["canonical"])
    for k in keys:
        assert same(got[k], want[k]), k


@pytest.fixture(scope="module")
def blob(golden_dir):
    return np.load(os.path.join(golden_dir, "c4net_blob_f32.npy"))


@pytest.fixture(scope="module")
def engine(blob):
    import synthesis_amd as sa

    eng = sa.Engine(concurrent_games=512, max_explores=EXPLORES)
    eng.load_weights(blob)
    eng.trainer_init(blob)
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def buffer(engine):
    """601 games of self-play in the engine's device buffer (the sizes of tests/test_gpu_replay_device.py): a few thousand positions,
    read back once; with the reference result of its symmetric de-duplication, computed once."""
    import synthesis_amd as sa

    engine.selfplay(sa.parity_rollout_config(EXPLORES), base_seed=3, n_games=601, outputs=False)
    engine.replay_clear()
    engine.replay_reserve(601 * 63)
    n = engine.replay_append_selfplay(first_gid=1000)
    R = engine.replay_read()
    assert n == R["my"].size > 2000
    want = expected(engine, R["my"], R["op"], R["pi"], R["v"])
    for a in list(R.values()) + [want[k] for k in KEYS]:
        a.setflags(write=False)
    return R, want


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 1000])
def test_positions_mirror_against_numpy(engine, n):
    rng = np.random.default_rng(100 + n)
    my = rng.integers(0, 1 << 63, size=n, dtype=np.uint64)
    op = rng.integers(0, 1 << 63, size=n, dtype=np.uint64)
    pi = rng.random((n, 9), dtype=np.float32)
    my[0], op[0] = (1 << 63) - 1, 0x7F << 28   # every board bit; the middle column alone
    m_my, m_op, m_pi = engine.positions_mirror(my, op, pi)
    assert same(m_my, sym.mirror(my)) and same(m_op, sym.mirror(op)) and same(m_pi, sym.reverse(pi))
    assert m_my[0] == my[0] and m_op[0] == op[0]
    b_my, b_op = engine.positions_mirror(my, op)   # boards only
    assert same(b_my, m_my) and same(b_op, m_op)
    i_my, i_op, i_pi = engine.positions_mirror(m_my, m_op, m_pi)   # an involution on the device
    assert same(i_my, my) and same(i_op, op) and same(i_pi, pi)


def run_case(engine, my, op, pi, v):
    my, op = np.asarray(my, np.uint64), np.asarray(op, np.uint64)
    got = engine.replay_deduplicate(my, op, pi, v, symmetry="mirror")
    assert_same_set(got, expected(engine, my, op, pi, v))
    return got


def test_hand_built_single_positions(engine):
    rng = np.random.default_rng(1)
    pi, v = rng.random((1, 9), dtype=np.float32), rng.random((1, 3), dtype=np.float32)
    got = run_case(engine, [0], [0], pi, v)   # the empty board is its own mirror image
    assert got["canonical"] == 1 and got["num"].size == 1 and same(got["pis"], pi)
    a, ma = 1 << 0, 1 << 56   # one stone in column 0 / in column 8: the smaller pair is the canonical one
    got = run_case(engine, [a], [0], pi, v)
    assert got["canonical"] == 1 and got["my_bb"].tolist() == [a, ma] and same(got["pis"], np.concatenate([pi, pi[:, ::-1]]))
    flipped_in = run_case(engine, [ma], [0], pi[:, ::-1], v)   # the same record, arriving in the other orientation
    assert_same_set(flipped_in, got)
    # the tie on my is broken by op
    got = run_case(engine, [1 << 28], [ma], pi, v)
    assert got["op_bb"].tolist() == [a, ma] and same(got["pis"][0], pi[0, ::-1])


def test_hand_built_one_class_of_five_in_both_orientations(engine):
    """Five records of one position, orientations mixed, random f32 targets: the sum runs in buffer order over the canonical forms.
    The case only proves that if the order matters — asserted here: the numpy sum in reversed order differs in at least one bit."""
    rng = np.random.default_rng(2)
    a_my, a_op = np.uint64(1 | 1 << 8), np.uint64(1 << 7 | 1 << 49)
    flip = np.array([False, True, True, False, True])
    my = np.where(flip, sym.mirror(np.full(5, a_my)), a_my)
    op = np.where(flip, sym.mirror(np.full(5, a_op)), a_op)
    pi, v = rng.random((5, 9), dtype=np.float32), rng.random((5, 3), dtype=np.float32)
    assert np.array_equal(sym.flipped(my, op), flip)
    c = np.concatenate([sym.canonicalise(my, op, pi)[2], v], axis=1)
    fwd, bwd = np.zeros(12, np.float32), np.zeros(12, np.float32)
    for i in range(5):
        fwd, bwd = fwd + c[i], bwd + c[4 - i]
    assert fwd.dtype == np.float32 and not np.array_equal(fwd.view(np.uint32), bwd.view(np.uint32))
    got = run_case(engine, my, op, pi, v)
    assert got["canonical"] == 1 and got["num"].tolist() == [5, 5]
    assert same(np.concatenate([got["pis"][0], got["vs"][0]]), fwd / np.float32(5))
    assert same(got["pis"][1], got["pis"][0, ::-1]) and same(got["vs"][1], got["vs"][0])
    # the unflipped sum would be another number
    assert not same(got["pis"][0], engine.replay_deduplicate(np.full(5, a_my), np.full(5, a_op), pi, v)["pis"][0])


def test_hand_built_buffers_without_mirror_images_and_of_one_class(engine):
    rng = np.random.default_rng(3)
    s_my = np.array([0, 1 << 28, 1 | 1 << 56, 1 << 30, 3 << 28, 1 << 7 | 1 << 49, 1 << 28], np.uint64)
    s_op = np.array([0, 1 << 29, 1 << 31, 0, 1 << 14 | 1 << 42, 1 << 28 | 1 << 21 | 1 << 35, 0], np.uint64)
    assert sym.self_symmetric(s_my, s_op).all()
    pick = rng.integers(0, s_my.size, size=300)
    got = run_case(engine, s_my[pick], s_op[pick], rng.random((300, 9), dtype=np.float32), rng.random((300, 3), dtype=np.float32))
    assert got["canonical"] == got["num"].size == s_my.size   # M == 0
    assert same(got["my_bb"], engine.replay_deduplicate(s_my[pick], s_op[pick], np.zeros((300, 9)), np.zeros((300, 3)))["my_bb"])
    # one class: 300 records of one asymmetric position in both orientations
    flip = rng.random(300) < 0.5
    a_my, a_op = np.full(300, 1 << 6 | 1 << 14, np.uint64), np.full(300, 1 << 62 | 1 << 15, np.uint64)
    my, op = np.where(flip, sym.mirror(a_my), a_my), np.where(flip, sym.mirror(a_op), a_op)
    got = run_case(engine, my, op, rng.random((300, 9), dtype=np.float32), rng.random((300, 3), dtype=np.float32))
    assert got["canonical"] == 1 and got["num"].tolist() == [300, 300]


def test_selfplay_buffer_host_pointer_and_to_trainer_paths(engine, buffer):
    R, want = buffer
    n, U, total = R["my"].size, want["canonical"], want["num"].size
    M = total - U
    assert 0 < M < U < n   # self-symmetric states and classes with more than one member are both present
    assert sym.flipped(R["my"], R["op"]).any() and (want["num"][:U][~sym.self_symmetric(want["my_bb"][:U], want["op_bb"][:U])] > 1).any()
    got = engine.replay_deduplicate(R["my"], R["op"], R["pi"], R["v"], symmetry="mirror")
    assert_same_set(got, want)
    assert engine.replay_deduplicate_to_trainer(symmetry="mirror") == (U, total)
    T = engine.train_get_data()
    for k in ("my_bb", "op_bb", "pis", "vs"):
        assert same(T[k], want[k]), k
    after = engine.replay_read()   # the buffer itself is unchanged
    for k in ("my", "op", "gid", "pi", "v"):
        assert same(after[k], R[k]), k
    # the properties the definitions promise, on the result itself
    states = set(zip(T["my_bb"].tolist(), T["op_bb"].tolist()))
    assert len(states) == total and states == set(zip(sym.mirror(T["my_bb"]).tolist(), sym.mirror(T["op_bb"]).tolist()))
    e = np.flatnonzero(~sym.self_symmetric(T["my_bb"][:U], T["op_bb"][:U]))
    assert e.size == M
    assert same(T["pis"][U:], T["pis"][e][:, ::-1]) and same(T["vs"][U:], T["vs"][e])
    assert same(T["my_bb"][U:], sym.mirror(T["my_bb"][e])) and same(T["op_bb"][U:], sym.mirror(T["op_bb"][e]))
    assert int(got["num"][:U].sum()) == n and same(got["num"][U:], got["num"][e])


def test_mirrored_buffer_gives_the_same_set(engine, buffer):
    """Every record mirrored by positions_mirror: the classes, their order, counts, v and every pi of a class with a mirror image are
    identical bit for bit (each member's canonical form is unchanged, so is the buffer order). A self-symmetric state is the one
    exception the definitions make: its record is its own canonical form in BOTH orientations, so the mirrored buffer contributes
    reverse(pi) where the original contributed pi, and the class's averaged pi arrives exactly reversed (a permutation: bit-exact).
    On the records of the states that are not self-symmetric alone, the two results are identical in every array."""
    R, want = buffer
    m_my, m_op, m_pi = engine.positions_mirror(R["my"], R["op"], R["pi"])
    got = engine.replay_deduplicate(m_my, m_op, m_pi, R["v"], symmetry="mirror")
    assert_same_set(got, want, keys=("my_bb", "op_bb", "vs", "num"))
    ss = sym.self_symmetric(want["my_bb"], want["op_bb"])
    assert ss.any() and not ss.all()
    assert same(got["pis"][~ss], want["pis"][~ss])
    assert same(got["pis"][ss], want["pis"][ss][:, ::-1])
    assert not same(got["pis"][ss], want["pis"][ss])   # (self-play's pi of the empty board is not a palindrome)
    keep = ~sym.self_symmetric(R["my"], R["op"])
    a = engine.replay_deduplicate(R["my"][keep], R["op"][keep], R["pi"][keep], R["v"][keep], symmetry="mirror")
    b = engine.replay_deduplicate(m_my[keep], m_op[keep], m_pi[keep], R["v"][keep], symmetry="mirror")
    assert a["num"].size == 2 * a["canonical"] > 0
    assert_same_set(b, a)


def test_symmetry_none_is_the_plain_call(engine, buffer):
    R, _ = buffer
    plain = engine.replay_deduplicate(R["my"], R["op"], R["pi"], R["v"])
    none = engine.replay_deduplicate(R["my"], R["op"], R["pi"], R["v"], symmetry="none")
    assert set(none) == set(plain) == set(KEYS)
    for k in KEYS:
        assert same(none[k], plain[k]), k
    n_plain = engine.replay_deduplicate_to_trainer()
    T_plain = engine.train_get_data()
    n_none = engine.replay_deduplicate_to_trainer(symmetry="none")
    T_none = engine.train_get_data()
    assert type(n_none) is int and n_none == n_plain == plain["num"].size
    for k in ("my_bb", "op_bb", "pis", "vs"):
        assert same(T_none[k], T_plain[k]) and same(T_none[k], plain[k]), k


@pytest.mark.parametrize("net", ["mlp", "conv"])
def test_learning_loop_with_mirror_symmetry(net):
    """LearningLoop(symmetry="mirror") for two iterations: replay="host" and replay="device" end with identical weights and records
    (timings apart), and those weights are not the ones a symmetry="none" run trains."""
    import synthesis_amd as sa
    from bench import make_conv_weights, make_weights
    from synthesis_amd.learner import LearningLoop

    blob = make_conv_weights(20260101) if net == "conv" else make_weights(20211003)
    cfg = sa.parity_rollout_config(EXPLORES)
    recs, weights, engines = {}, {}, {}
    try:
        for arm, replay, symmetry in (("host", "host", "mirror"), ("device", "device", "mirror"), ("none", "device", "none")):
            eng = engines[arm] = sa.Engine(concurrent_games=512, max_explores=EXPLORES)
            loop = LearningLoop(eng, net, blob, seed=7, replay=replay, symmetry=symmetry)
            recs[arm] = [loop.iteration(cfg, 601, 1000, 1, 32) for _ in range(2)]
            weights[arm] = loop.weights.copy()
        for a, b in zip(recs["host"], recs["device"]):
            assert set(a) == set(b) and set(a["seconds"]) == set(b["seconds"])
            for k in set(a) - {"seconds"}:
                assert a[k] == b[k], (k, a[k], b[k])
            assert a["steps_in_buffer"] > a["unique_canonical"] and a["unique_canonical"] < a["unique"] < 2 * a["unique_canonical"]
            assert a["optimiser_steps"] == a["unique"] // 32
        assert same(weights["host"], weights["device"])
        assert not np.array_equal(weights["host"], weights["none"]) and not np.array_equal(weights["none"], blob)
        for a, c in zip(recs["host"], recs["none"]):
            assert "unique_canonical" not in c and set(a) - set(c) == {"unique_canonical"}
        assert recs["host"][0]["steps_in_buffer"] == recs["none"][0]["steps_in_buffer"]   # the first iteration plays the same games
        assert engines["device"].train_get_data()["my_bb"].size == recs["device"][1]["unique"]
    finally:
        for eng in engines.values():
            eng.close()


def test_learning_loop_logs_hold_the_augmented_set(tmp_path, blob):
    import synthesis_amd as sa
    from synthesis_amd.learner import LearningLoop

    eng = sa.Engine(concurrent_games=512, max_explores=EXPLORES)
    try:
        loop = LearningLoop(eng, "mlp", blob, seed=7, replay="device", symmetry="mirror", logs_dir=str(tmp_path))
        rec = loop.iteration(sa.parity_rollout_config(EXPLORES), 200, 1000, 1, 32)
        states, pis = np.load(tmp_path / "latest_states.npy"), np.load(tmp_path / "latest_pis.npy")
        U, total = rec["unique_canonical"], rec["unique"]
        assert states.shape == (total, 1, 7, 9) and pis.shape == (total, 9) and np.load(tmp_path / "latest_vs.npy").shape == (total, 3)
        D = eng.train_get_data()
        e = np.flatnonzero(~sym.self_symmetric(D["my_bb"][:U], D["op_bb"][:U]))
        assert same(states[U:], states[e][..., ::-1]) and same(pis[U:], pis[e][:, ::-1])   # the planes flipped left to right
    finally:
        eng.close()


def test_errors(blob):
    import synthesis_amd as sa
    from synthesis_amd.engine import SynthesisAmdError

    eng = sa.Engine(concurrent_games=512, max_explores=EXPLORES)
    try:
        eng.load_weights(blob)
        eng.replay_reserve(64)
        eng.replay_append([1], [2], [0], np.zeros((1, 9), np.float32), np.zeros((1, 3), np.float32))
        with pytest.raises(SynthesisAmdError) as e:   # SYN_ERR_NO_WEIGHTS: no trainer yet
            eng.replay_deduplicate_to_trainer(symmetry="mirror")
        assert e.value.code == -4
        eng.trainer_init(blob)
        assert eng.replay_deduplicate_to_trainer(symmetry="mirror") == (1, 2)
        eng.replay_clear()
        with pytest.raises(SynthesisAmdError) as e:   # SYN_ERR_INVALID_ARGUMENT: an empty buffer has no data set
            eng.replay_deduplicate_to_trainer(symmetry="mirror")
        assert e.value.code == -1
        got = eng.replay_deduplicate(np.zeros(0, np.uint64), np.zeros(0, np.uint64), np.zeros((0, 9)), np.zeros((0, 3)), symmetry="mirror")
        assert got["canonical"] == 0 and all(got[k].shape[0] == 0 for k in KEYS)
        assert [a.size for a in eng.positions_mirror([], [])] == [0, 0]
        with pytest.raises(ValueError, match="symmetry"):
            eng.replay_deduplicate([1], [2], np.zeros((1, 9)), np.zeros((1, 3)), symmetry="rotate")
    finally:
        eng.close()
