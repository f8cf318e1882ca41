"""syn_state_digest (include/synthesis_amd.h "State digests"; csrc/digest_kernels.cuh) against the numpy model of the header's text
(tests/state_digest_model.py), word for word, on state that is uploaded and read back through the existing entry points."""
import os

import numpy as np
import pytest

from tests import state_digest_model as model

pytestmark = pytest.mark.gpu

INVALID, NO_WEIGHTS = -1, -4
REPLAY_ORDER = ("my", "op", "gid", "pi", "v")
DATA_ORDER = ("my", "op", "pi", "v")
SIZES = (0, 1, 31, 33, 1000)


@pytest.fixture(scope="module")
def blobs(golden_dir):
    from bench import make_conv_weights

    return dict(mlp=np.load(os.path.join(golden_dir, "c4net_blob_f32.npy")), conv=make_conv_weights())


@pytest.fixture(scope="module")
def engine(blobs):
    import synthesis_amd as sa

    eng = sa.Engine(concurrent_games=512, max_explores=40)
    eng.trainer_init(blobs["mlp"])
    eng.replay_reserve(1100)
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def rows():
    """The uploaded sets, made once: anything at all in every word (NaN payloads, negative zeros, ids above 2^32)"""
    return {n: model.random_rows(np.random.default_rng(77 + n), n) for n in SIZES}


def put_replay(eng, R):
    eng.replay_clear()
    if R["my"].size:
        eng.replay_append(*(R[k] for k in REPLAY_ORDER))


def put(eng, what, R):
    if what == "replay":
        put_replay(eng, R)
    elif what == "train_data":
        eng.train_set_data(*(R[k] for k in DATA_ORDER))
    else:
        eng.dataset_set(*(R[k] for k in DATA_ORDER))


def want(what, R):
    if what == "replay":
        return model.replay(*(R[k] for k in REPLAY_ORDER))
    return model.dataset(model.TRAIN_DATA if what == "train_data" else model.EVAL_DATA, *(R[k] for k in DATA_ORDER))


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("what", ("replay", "train_data", "eval_data"))
def test_buffer_and_data_sets_equal_the_model(engine, rows, what, n):
    import synthesis_amd as sa

    R = rows[n]
    if what == "train_data" and n == 0:   # a learner's data set cannot be emptied: the empty one is a new trainer's
        with sa.Engine(concurrent_games=512, max_explores=40) as fresh:
            fresh.trainer_init(np.zeros(30492, np.float32))
            assert fresh.state_digest_words(what) == (want(what, R), 0)
            assert fresh.last_timing()[1] == 0
        return
    put(engine, what, R)
    per_row = 18 if what == "replay" else 16
    assert engine.state_digest_words(what) == (want(what, R), per_row * n)
    assert engine.last_timing()[1] == (2 if n else 0)
    if what == "replay":   # what was uploaded is what is there
        back = engine.replay_read()
        assert all(back[k].tobytes() == R[k].tobytes() for k in REPLAY_ORDER)


def test_never_reserved_buffer_and_sets_are_no_words():
    import synthesis_amd as sa

    with sa.Engine(concurrent_games=512, max_explores=40) as fresh:
        for what, code in (("replay", model.REPLAY), ("train_data", model.TRAIN_DATA), ("eval_data", model.EVAL_DATA)):
            assert fresh.state_digest_words(what) == (model.digest_of_words(code, np.zeros(0, np.uint32)), 0)


def a_batch(seed, n=32):
    rng = np.random.default_rng(seed)
    my = rng.integers(0, 1 << 63, n, dtype=np.uint64)
    op = rng.integers(0, 1 << 63, n, dtype=np.uint64) & ~my
    pi = rng.random((n, 9), dtype=np.float32)
    v = rng.random((n, 3), dtype=np.float32)
    return my, op, pi / pi.sum(1, keepdims=True), v / v.sum(1, keepdims=True)


@pytest.mark.parametrize("net", ("mlp", "conv"))
def test_trainer_and_network_equal_the_model(blobs, net):
    import synthesis_amd as sa

    blob = blobs[net]
    with sa.Engine(concurrent_games=512, max_explores=40) as eng:
        (eng.load_weights_conv if net == "conv" else eng.load_weights)(blob)
        (eng.trainer_init_conv if net == "conv" else eng.trainer_init)(blob)
        zero = np.zeros_like(blob)
        assert eng.state_digest_words("trainer") == (model.trainer(blob, zero, zero, 0), 3 * blob.size + 2)
        assert eng.state_digest_words("network") == (model.network(blob), blob.size)
        for s in range(3):
            eng.train_step(*a_batch(s), 1e-3)
        S = eng.trainer_state()
        assert S["step"] == 3 and not np.array_equal(S["weights"], blob)
        assert eng.state_digest("trainer") == model.trainer(S["weights"], S["m"], S["v"], 3)
        assert eng.state_digest("network") == model.network(blob)          # nothing was published
        eng.trainer_publish_weights()
        assert eng.state_digest("network") == model.network(S["weights"])
        eng.set_network_arithmetic("f16x2")                                # the arithmetic is not part of it
        assert eng.state_digest("network") == model.network(S["weights"])


def test_grid_does_not_show(engine, rows):
    R = rows[1000]
    put_replay(engine, R)
    words = {cap: engine.state_digest("replay", max_workgroups=cap) for cap in (1, 3, 0, 7, 4096)}
    assert set(words.values()) == {want("replay", R)}, words


def test_after_a_keep_window_moved_the_buffer(engine, rows):
    R = {k: a.copy() for k, a in rows[1000].items()}
    R["gid"] = np.arange(1000, dtype=np.int64) // 10 + (1 << 32)
    put_replay(engine, R)
    engine.replay_keep_games_from((1 << 32) + 37)     # drops 370 rows: the kept ones are scattered into the second allocation
    kept = {k: a[370:] for k, a in R.items()}
    assert engine.replay_size() == 630
    assert engine.state_digest_words("replay") == (want("replay", kept), 18 * 630)
    engine.replay_keep_games_from((1 << 32) + 95)     # and back into the first
    assert engine.state_digest("replay") == want("replay", {k: a[950:] for k, a in R.items()})


def test_sensitivity(engine, rows):
    """One bit, two rows swapped, and a word moved across a section boundary (same multiset of words) each change the word, to the
    model's"""
    base = rows[33]
    seen = {want("replay", base)}

    def check(R):
        put_replay(engine, R)
        got = engine.state_digest("replay")
        assert got == want("replay", R) and got not in seen
        seen.add(got)

    for key, at, bit in (("my", 0, 0), ("gid", 32, 63), ("pi", (5, 8), 31), ("v", (32, 2), 0)):
        R = {k: a.copy() for k, a in base.items()}
        w = R[key].view(np.uint64 if R[key].dtype.itemsize == 8 else np.uint32)
        w[at] ^= w.dtype.type(1 << bit)
        check(R)
    R = {k: a.copy() for k, a in base.items()}
    for a in R.values():
        a[[3, 17]] = a[[17, 3]]
    check(R)
    # the last word of one section and the first of the next change places: my | op, and pi | v
    R = {k: a.copy() for k, a in base.items()}
    my, op = R["my"].view(np.uint32), R["op"].view(np.uint32)
    my[-1], op[0] = op[0], my[-1]
    check(R)
    R = {k: a.copy() for k, a in base.items()}
    pi, v = R["pi"].view(np.uint32), R["v"].view(np.uint32)
    pi[-1, -1], v[0, 0] = v[0, 0], pi[-1, -1]
    assert pi[-1, -1] != v[0, 0]
    check(R)


def snapshot(eng, my, op):
    S = eng.trainer_state()
    return [S[k].tobytes() for k in ("weights", "m", "v", "grads")] + [S["step"]] + \
           [a.tobytes() for a in eng.replay_read().values()] + [a.tobytes() for a in eng.train_get_data().values()] + \
           [a.tobytes() for a in eng.dataset_get().values()] + [a.tobytes() for a in eng.policy_eval(my, op)] + \
           [eng.network_arithmetic(), eng.trainer_batch_mode()[:2], eng.dataset_counts()]


def test_observer(engine, rows, blobs):
    engine.load_weights(blobs["mlp"])
    put_replay(engine, rows[1000])
    put(engine, "train_data", rows[33])
    put(engine, "eval_data", rows[31])
    my, op = a_batch(9)[:2]
    before = snapshot(engine, my, op)
    words = [engine.state_digest(w) for w in ("trainer", "network", "replay", "train_data", "eval_data")]
    assert snapshot(engine, my, op) == before
    assert words == [engine.state_digest(w) for w in ("trainer", "network", "replay", "train_data", "eval_data")]
    assert len(set(words)) == 5


def test_refusals(engine, rows):
    import synthesis_amd as sa

    put_replay(engine, rows[33])
    word = engine.state_digest("replay")
    for what in (0, 6, -1, 1 << 20):
        with pytest.raises(sa.SynthesisAmdError) as e:
            engine.state_digest(what)
        assert e.value.code == INVALID
        assert engine.state_digest("replay") == word
    with pytest.raises(sa.SynthesisAmdError) as e:
        engine.state_digest("replay", max_workgroups=-1)
    assert e.value.code == INVALID
    assert engine.state_digest("replay") == word
    with pytest.raises(ValueError):
        engine.state_digest("buffer")
    with sa.Engine(concurrent_games=512, max_explores=40) as fresh:
        fresh.replay_reserve(64)
        put_replay(fresh, rows[33])
        for what in ("trainer", "network"):
            with pytest.raises(sa.SynthesisAmdError) as e:
                fresh.state_digest(what)
            assert e.value.code == NO_WEIGHTS
            assert fresh.state_digest("replay") == word
