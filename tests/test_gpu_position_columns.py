"""The replay buffer's and the data sets' columns at the edges a shared layout can get wrong: a buffer whose capacity (300) is not its
row count, so that the column stride differs from n, at n = 1 and around one 256-thread block. Hand-built legal positions with duplicate
and mirrored states and two game ids go in from the host; every path that reads the columns is held, bit for bit, to a restatement that
shares no code with the engine: numpy for the reads and the keep-window, the CPU oracle's de-duplication (through tests/symmetry_py.py
for the symmetric form) for the learner's data set, tests/dataset_eval_model.py's hash and partition for the holdout split."""
import os

import numpy as np
import pytest

from tests import dataset_eval_model as dm
from tests import symmetry_py as sym
from tests.test_gpu_replay_device import same

pytestmark = pytest.mark.gpu

CAPACITY = 300
G0, G1 = 41, 42          # the two game ids; the keep-window keeps G1
KEY = 0x0123_4567_89AB_CDEF
KEYS4 = ("my_bb", "op_bb", "pis", "vs")


@pytest.fixture(scope="module")
def engine(golden_dir):
    import synthesis_amd as sa

    blob = np.load(os.path.join(golden_dir, "c4net_blob_f32.npy"))
    eng = sa.Engine(concurrent_games=64, max_explores=8)
    eng.load_weights(blob)
    eng.trainer_init(blob)
    eng.replay_reserve(CAPACITY)
    yield eng
    eng.close()


def legal_positions(rng, n):
    """n positions reached by random legal play on the 9 x 7 board (bit 7 * column + row), `my` the side to move"""
    my, op = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
    for i in range(n):
        height, side = [0] * 9, [0, 0]
        for ply in range(int(rng.integers(0, 24))):
            col = int(rng.choice([c for c in range(9) if height[c] < 7]))
            side[ply & 1] |= 1 << (7 * col + height[col])
            height[col] += 1
        plies = sum(height)
        my[i], op[i] = side[plies & 1], side[1 - (plies & 1)]
    return my, op


def rows(n):
    """n hand-built rows: random legal positions, every fifth a repeat of an earlier state and every seventh the mirror image of one,
    random f32 targets, the game ids in runs of three (n == 1: the one row belongs to the game that the holdout below keeps)"""
    rng = np.random.default_rng(1000 + n)
    my, op = legal_positions(rng, n)
    for i in range(1, n):
        j = int(rng.integers(0, i))
        if i % 5 == 0:
            my[i], op[i] = my[j], op[j]
        elif i % 7 == 0:
            my[i], op[i] = sym.mirror(my[j : j + 1])[0], sym.mirror(op[j : j + 1])[0]
    gid = np.where((np.arange(n) // 3) % 2 == 0, G0, G1).astype(np.int64)
    if n == 1:
        gid[0] = kept_game()
    R = dict(my=my, op=op, gid=gid, pi=rng.random((n, 9), dtype=np.float32), v=rng.random((n, 3), dtype=np.float32))
    for a in R.values():
        a.setflags(write=False)
    return R


def holdout_threshold():
    """holds out exactly one of the two games under KEY: the one with the smaller hash"""
    h = dm.holdout_hash(KEY, np.array([G0, G1], np.int64))
    assert h[0] != h[1]
    return int(h.max())


def kept_game():
    h = dm.holdout_hash(KEY, np.array([G0, G1], np.int64))
    return G0 if h[0] > h[1] else G1


def deduplicate(oracle, my, op, pi, v, symmetry):
    if symmetry == "mirror":
        return sym.symmetric_deduplicate(oracle.dedup, my, op, pi, v)
    return oracle.dedup(my, op, pi, v)


def split(oracle, R, threshold, symmetry):
    """(learner's set, evaluation set or None, n_unseen) by the definition of the holdout (tests/test_gpu_holdout.py's restatement, with
    the oracle's de-duplication and numpy's mirror in the engine's place)"""
    held = dm.holdout_flags(KEY, R["gid"], threshold)
    D = deduplicate(oracle, R["my"][~held], R["op"][~held], R["pi"][~held], R["v"][~held], symmetry)
    if not held.any():
        return D, None, 0
    E = deduplicate(oracle, R["my"][held], R["op"][held], R["pi"][held], R["v"][held], symmetry)
    my, op, n_train = E["my_bb"], E["op_bb"], D["my_bb"].size
    if symmetry == "mirror":
        n_train = D["canonical"]
        flipped = sym.flipped(my, op)
        my, op = np.where(flipped, sym.mirror(my), my), np.where(flipped, sym.mirror(op), op)
    E, n_unseen = dm.unseen_first(E, dm.is_seen(my, op, D["my_bb"][:n_train], D["op_bb"][:n_train]))
    return D, E, n_unseen


def assert_buffer(eng, R):
    got = eng.replay_read()
    assert got["my"].size == R["my"].size
    for k in ("my", "op", "gid", "pi", "v"):
        assert same(got[k], R[k]), k


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_columns_of_a_partly_filled_buffer(engine, oracle, n):
    import synthesis_amd as sa

    eng, R = engine, rows(n)
    eng.replay_set_holdout(KEY, 0)
    eng.replay_clear()
    eng.replay_append(R["my"], R["op"], R["gid"], R["pi"], R["v"])
    assert eng.replay_size() == n < CAPACITY
    assert_buffer(eng, R)

    # ---- the learner's data set, plain and symmetric
    for symmetry in ("none", "mirror"):
        D = deduplicate(oracle, R["my"], R["op"], R["pi"], R["v"], symmetry)
        got_n = eng.replay_deduplicate_to_trainer(symmetry=symmetry)
        assert got_n == ((D["canonical"], D["my_bb"].size) if symmetry == "mirror" else D["my_bb"].size)
        if n > 1:
            assert D["my_bb"].size < (2 * n if symmetry == "mirror" else n)   # the duplicates are there
        T = eng.train_get_data()
        for k in KEYS4:
            assert same(T[k], D[k]), (symmetry, k)

    # ---- the same with one of the two games held out
    t = holdout_threshold()
    held = dm.holdout_flags(KEY, R["gid"], t)
    assert not held.all() and (n == 1 or held.any())
    eng.replay_set_holdout(KEY, t)
    try:
        for symmetry in ("none", "mirror"):
            D, E, n_unseen = split(oracle, R, t, symmetry)
            got_n = eng.replay_deduplicate_to_trainer(symmetry=symmetry)
            assert got_n == ((D["canonical"], D["my_bb"].size) if symmetry == "mirror" else D["my_bb"].size)
            tr, ev = eng.train_get_data(), eng.dataset_get()
            for k in KEYS4:
                assert same(tr[k], D[k]), (symmetry, "train", k)
            if E is None:
                assert eng.dataset_counts() == (0, 0) and ev["my_bb"].size == 0
            else:
                for k in KEYS4:
                    assert same(ev[k], E[k]), (symmetry, "eval", k)
                assert eng.dataset_counts() == (E["my_bb"].size, n_unseen)
    finally:
        eng.replay_set_holdout(KEY, 0)
    assert_buffer(eng, R)   # every call so far only read the buffer

    # ---- the selection alone and the selection of a reanalyse: the same rows for the same key and threshold
    sel = eng.replay_select_positions(key=77, fraction=0.5)
    st = eng.replay_reanalyse(sa.parity_mcts_config(), 8, key=77, fraction=0.5, rows=True)
    picked = st["selected_rows"]
    assert st["rows"] == n and st["selected"] == picked.size == sel["my"].size and st["skipped"] == sel["skipped"]
    assert np.all(np.diff(picked) > 0) and (picked.size == 0 or (0 <= picked[0] and picked[-1] < n))
    assert same(sel["my"], R["my"][picked]) and same(sel["op"], R["op"][picked])
    if n > 1:
        assert 0 < picked.size < n
    after = eng.replay_read()   # the searches rewrote pi of the selected rows and nothing else
    untouched = np.ones(n, bool)
    untouched[picked] = False
    for k in ("my", "op", "gid", "v"):
        assert same(after[k], R[k]), k
    assert same(after["pi"][untouched], R["pi"][untouched])

    # ---- the keep-window: the numpy boolean filter
    eng.replay_keep_games_from(G1)
    keep = R["gid"] >= G1
    assert_buffer(eng, {k: np.ascontiguousarray(a[keep]) for k, a in after.items()})
