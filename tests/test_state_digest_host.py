"""State digests and the state file without a GPU: the header's known answers on the numpy model (tests/state_digest_model.py), the
product's host twin (synthesis_amd/digest.py) against that model, and the pack / unpack / write / read functions of
synthesis_amd/learner.py."""
import os

import numpy as np
import pytest

from tests import state_digest_model as model

KNOWN = (("none", np.zeros(0, np.uint32), 0x6DC4EDD735556CBF),
         ("zero", np.zeros(1, np.uint32), 0x831DCD5C179D866E),
         ("ascending", np.arange(1000, dtype=np.uint32), 0x17B9CEEDB8BF8015),
         ("descending", np.arange(999, -1, -1, dtype=np.uint32), 0x8C9CAB522FF11F09))


@pytest.mark.parametrize("name,w,want", KNOWN, ids=[k[0] for k in KNOWN])
def test_known_answers(name, w, want):
    from synthesis_amd.digest import digest_words

    assert model.digest_of_words(model.TRAINER, w) == want
    assert digest_words(model.TRAINER, w) == want
    assert digest_words("trainer", w) == want


def test_a_64_bit_value_is_its_low_word_then_its_high_word():
    from synthesis_amd.digest import digest_words

    x = np.array([0x1122334455667788, 0xFFFFFFFF00000001], np.uint64)
    as_words = np.array([0x55667788, 0x11223344, 0x00000001, 0xFFFFFFFF], np.uint32)
    for f in (model.digest, digest_words):
        assert f(3, x) == f(3, as_words) == f(3, x.view(np.int64))


@pytest.mark.parametrize("what", (1, 2, 3, 4, 5))
@pytest.mark.parametrize("n", (0, 1, 33, 1000))
def test_host_twin_equals_the_model(what, n):
    from synthesis_amd import digest as D

    rng = np.random.default_rng(1000 * what + n)
    R = model.random_rows(rng, n)
    name = {v: k for k, v in D.COMPONENTS.items()}[what]
    if what == model.REPLAY:
        order = ("my", "op", "gid", "pi", "v")
        assert D.replay_digest(*(R[k] for k in order)) == model.replay(*(R[k] for k in order))
    elif what in (model.TRAIN_DATA, model.EVAL_DATA):
        order = ("my", "op", "pi", "v")
        assert D.dataset_digest(name, *(R[k] for k in order)) == model.dataset(what, *(R[k] for k in order))
    elif what == model.TRAINER:
        w, m, v = (rng.integers(0, 1 << 32, 12412, dtype=np.uint32).view(np.float32) for _ in range(3))
        for step in (0, 3, (5 << 32) + 7):
            assert D.trainer_digest(w, m, v, step) == model.trainer(w, m, v, step)
        return
    arrays = [R[k] for k in order] if what != model.NETWORK else [rng.integers(0, 1 << 32, 30492, dtype=np.uint32).view(np.float32)]
    assert D.digest_words(name, *arrays) == D.digest_words(what, *arrays) == model.digest(what, *arrays)
    if n == 1000:   # the tag separates the components
        assert D.digest_words(what, *arrays) != D.digest_words(what % 5 + 1, *arrays)


def test_host_twin_in_chunks(monkeypatch):
    """digest.py walks long arrays in chunks: the word does not depend on the chunk size"""
    from synthesis_amd import digest as D

    w = np.random.default_rng(5).integers(0, 1 << 32, 5000, dtype=np.uint32)
    want = model.digest_of_words(3, w)
    for chunk in (1, 7, 4096, 5000, 1 << 20):
        monkeypatch.setattr(D, "_CHUNK", chunk)
        assert D.digest_words(3, w[:1234], w[1234:]) == want


def test_host_twin_refuses_what_it_cannot_digest():
    from synthesis_amd.digest import digest_words

    with pytest.raises(ValueError, match="what must be one of"):
        digest_words("buffer", np.zeros(3, np.uint32))
    with pytest.raises(ValueError, match="32-bit words"):
        digest_words("replay", np.zeros(3, np.uint8))


# ------------------------------------------------------------------------------------------------ the state file
def fingerprint(**changes):
    fp = dict(net="mlp", seed=7, precision="f32", batch_mode="chained", sampler="torch", flip=False, symmetry="mirror", holdout=0.25,
              reanalyse=0.5, reanalyse_explores=None, reanalyse_value_mix=0.125, lr_schedule=[[1, 1e-3], [20, 3e-4]],
              hyper=dict(weight_decay=1e-6, policy_weight=1.0, value_weight=1.0, beta1=0.9, beta2=0.999, eps=1e-8), network_arithmetic="f32",
              world=1)
    fp.update(changes)
    return fp


def a_state(n=37, generator=True):
    rng = np.random.default_rng(n)
    R = model.random_rows(rng, n)
    w, m, v = (rng.integers(0, 1 << 32, 12412, dtype=np.uint32).view(np.float32) for _ in range(3))
    return dict(fingerprint=fingerprint(), iterations_done=12, games_played=(1 << 33) + 5, weights=w, m=m, v=v, step=(1 << 40) + 3, replay=R,
                digest_trainer=0xFEDCBA9876543210, digest_replay=0x8000000000000001,
                torch_generator=rng.integers(0, 256, 5056, dtype=np.uint8) if generator else None)


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def assert_same_state(got, want):
    assert set(got) == set(want)
    for k in ("iterations_done", "games_played", "step", "digest_trainer", "digest_replay", "fingerprint"):
        assert got[k] == want[k] and type(got[k]) is type(want[k]), k
    for k in ("weights", "m", "v"):
        assert same(got[k], want[k]), k
    for k in ("my", "op", "gid", "pi", "v"):
        assert same(got["replay"][k], want["replay"][k]), k
    if want["torch_generator"] is None:
        assert got["torch_generator"] is None
    else:
        assert same(got["torch_generator"], want["torch_generator"])


@pytest.mark.parametrize("n,generator", ((37, True), (0, False)))
def test_pack_unpack_round_trips_every_field(n, generator):
    from synthesis_amd.learner import pack_state, unpack_state

    S = a_state(n, generator)
    assert S["replay"]["gid"].max(initial=0) > (1 << 32) or n == 0
    arrays = pack_state(S)
    assert all(isinstance(a, np.ndarray) and a.dtype != object for a in arrays.values())
    assert_same_state(unpack_state(arrays), S)


def test_file_round_trip_and_replace(tmp_path):
    from synthesis_amd.learner import read_state_file, write_state_file

    path = tmp_path / "run.npz"
    write_state_file(path, a_state(5))
    S = a_state(37)
    write_state_file(path, S)    # replaces the older file
    assert os.listdir(tmp_path) == ["run.npz"]
    assert_same_state(read_state_file(path), S)
    with np.load(path, allow_pickle=False) as z:   # numpy alone reads it, nothing pickled
        assert int(z["format_version"]) == 1 and z["replay_gid"].dtype == np.int64


def test_a_failed_write_leaves_the_old_file_and_no_partial_one(tmp_path, monkeypatch):
    from synthesis_amd.learner import read_state_file, write_state_file

    path = tmp_path / "run.npz"
    S = a_state(5)
    write_state_file(path, S)
    bad = a_state(6)
    bad["replay"]["pi"] = bad["replay"]["pi"][:-1]
    with pytest.raises(ValueError, match="same number of rows"):
        write_state_file(path, bad)

    def disk_full(f, **arrays):   # a write that dies half way through
        f.write(b"PK\x03\x04 half a file")
        raise OSError(28, "No space left on device")

    monkeypatch.setattr(np, "savez", disk_full)
    with pytest.raises(OSError, match="No space left"):
        write_state_file(path, a_state(6))
    monkeypatch.undo()
    assert os.listdir(tmp_path) == ["run.npz"]
    assert_same_state(read_state_file(path), S)


def test_a_truncated_file_is_refused(tmp_path):
    from synthesis_amd.learner import read_state_file, write_state_file

    path = tmp_path / "run.npz"
    write_state_file(path, a_state(37))
    raw = path.read_bytes()
    for keep in (len(raw) // 2, len(raw) - 1, 10, 0):
        path.write_bytes(raw[:keep])
        with pytest.raises(ValueError, match="not a complete LearningLoop state file"):
            read_state_file(path)
        assert os.listdir(tmp_path) == ["run.npz"]
    with pytest.raises(FileNotFoundError):
        read_state_file(tmp_path / "absent.npz")
    assert os.listdir(tmp_path) == ["run.npz"]


def test_a_foreign_version_or_file_is_refused(tmp_path):
    from synthesis_amd.learner import pack_state, read_state_file, unpack_state

    arrays = pack_state(a_state(5))
    arrays["format_version"] = np.int64(2)
    path = tmp_path / "future.npz"
    np.savez(path, **arrays)
    with pytest.raises(ValueError, match="format version 2; this library reads version 1"):
        read_state_file(path)
    np.savez(tmp_path / "other.npz", x=np.zeros(3))
    with pytest.raises(ValueError, match="not a LearningLoop state file"):
        read_state_file(tmp_path / "other.npz")
    assert sorted(os.listdir(tmp_path)) == ["future.npz", "other.npz"]
    arrays = pack_state(a_state(5))
    del arrays["replay_gid"]
    with pytest.raises(ValueError, match="'replay_gid' is missing"):
        unpack_state(arrays)
    arrays = pack_state(a_state(5))
    arrays["replay_gid"] = arrays["replay_gid"].astype(np.int32)
    with pytest.raises(ValueError, match="'replay_gid' is int32"):
        unpack_state(arrays)


@pytest.mark.parametrize("field,other", (("net", "conv"), ("seed", 8), ("precision", "bf16"), ("batch_mode", "micro"), ("sampler", "device"),
                                         ("flip", True), ("symmetry", "none"), ("holdout", 0.5), ("reanalyse", 0.25), ("reanalyse_explores", 40),
                                         ("reanalyse_value_mix", 0.0), ("lr_schedule", [[1, 1e-3]]),
                                         ("hyper", dict(weight_decay=1e-5, policy_weight=1.0, value_weight=1.0, beta1=0.9, beta2=0.999, eps=1e-8)),
                                         ("network_arithmetic", "f16x2"), ("world", 2)))
def test_a_fingerprint_mismatch_names_its_field(field, other):
    from synthesis_amd.learner import FINGERPRINT_FIELDS, check_fingerprint, pack_state, unpack_state

    assert field in FINGERPRINT_FIELDS and "replay" not in FINGERPRINT_FIELDS
    saved = unpack_state(pack_state(a_state(5)))["fingerprint"]
    check_fingerprint(saved, fingerprint())
    check_fingerprint(saved, fingerprint(lr_schedule=((1, 1e-3), (20, 3e-4))))    # a tuple in the constructor, a list in the file
    with pytest.raises(ValueError, match=rf"\b{field}="):
        check_fingerprint(saved, fingerprint(**{field: other}))
