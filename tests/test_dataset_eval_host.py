"""Held-out evaluation without a GPU: the numpy restatement (tests/dataset_eval_model.py) and its self-checks, the holdout hash against
hand-computed values, the C ABI (header, ABI_SYMBOLS, the built library, the ctypes mirror) and LearningLoop's argument checks."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import dataset_eval_model as dm
from tests import sampler_model as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = {"syn_dataset_set": 6, "syn_dataset_get": 7, "syn_dataset_evaluate": 11, "syn_replay_set_holdout": 3, "syn_dataset_counts": 3}


def header_text():
    with open(os.path.join(ROOT, "include", "synthesis_amd.h")) as f:
        return f.read()


# ---- the C ABI
def test_new_symbols_in_header_abi_list_library_and_ctypes():
    from synthesis_amd.engine import ABI_SYMBOLS, load_library

    h = header_text()
    lib = load_library()
    exported = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "synthesis_amd", "libsynthesis_amd.so")]).decode()
    for name, n_args in NEW_SYMBOLS.items():
        protos = re.findall(rf"^int {name}\(([^;]*)\);", h, re.M)
        assert len(protos) == 1, name
        params = [p.strip() for p in protos[0].split(",")]
        assert len(params) == n_args and params[0] == "syn_engine* h", (name, params)
        assert name in ABI_SYMBOLS
        assert len(getattr(lib, name).argtypes) == n_args, name
        assert re.search(rf"\bT {name}\b", exported), name
    assert re.search(r"SYN_DATASET_TRAIN = 0, SYN_DATASET_EVAL = 1", h)
    assert f"HOLDOUT_TAG = 0x{dm.HOLDOUT_TAG:016X}" in h
    csrc = open(os.path.join(ROOT, "synthesis_amd", "csrc", "replay_kernels.cuh")).read()
    assert f"HOLDOUT_TAG = 0x{dm.HOLDOUT_TAG:016X}ull" in csrc


def test_metrics_struct_matches_the_header():
    from synthesis_amd.engine import DATASETS, CDatasetMetrics

    body = re.search(r"typedef struct syn_dataset_metrics \{(.*?)\} syn_dataset_metrics;", header_text(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    ctype = {"double": C.c_double, "uint64_t": C.c_uint64, "uint32_t": C.c_uint32}
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            ty, names = decl.split(None, 1)
            fields += [(n.strip(), ctype[ty]) for n in names.split(",")]
    assert fields == [(n, t) for n, t in CDatasetMetrics._fields_]
    assert C.sizeof(CDatasetMetrics) == 72 and CDatasetMetrics.rows.offset == 32 and CDatasetMetrics.grid.offset == 64
    assert DATASETS == {"train": 0, "eval": 1}


# ---- the restatement of the metrics
def test_argmax_rules():
    assert dm.argmax_first([1.0, 3.0, 3.0, 2.0]) == 1 and dm.argmax_first([0.0, 0.0, 0.0]) == 0
    assert dm.argmax_first([np.float32("nan"), 1.0]) == 0       # nothing compares greater than the first entry
    x = np.arange(9, dtype=np.float32)
    assert dm.argmax_legal(x, 0) == 8
    assert dm.argmax_legal(x, 1 << (6 + 7 * 8)) == 7              # column 8 full
    assert dm.argmax_legal(x, (1 << (5 + 7 * 8))) == 8            # its top cell is free: legal
    assert dm.argmax_legal(np.zeros(9, np.float32), 1 << 6) == 1  # first maximum among the legal ones
    full = sum(1 << (6 + 7 * c) for c in range(9))
    assert dm.argmax_legal(x, full) == 9
    ph, vh = dm.row_hits(np.array([[0, 0, 5, 0, 0, 0, 0, 0, 0, 1, 2, 0]], np.float32), [1 << (6 + 14)], [0], np.eye(9, dtype=np.float32)[2][None],
                         np.eye(3, dtype=np.float32)[1][None])
    assert ph.tolist() == [0] and vh.tolist() == [1]


def test_block_rows_and_losses():
    assert dm.block_rows(1).tolist() == [1] and dm.block_rows(32).tolist() == [32] and dm.block_rows(33).tolist() == [32, 1]
    assert dm.block_rows(95).tolist() == [32, 32, 31] and dm.block_rows(0).size == 0
    rng = np.random.default_rng(0)
    kl = rng.random((95, 2), np.float32)
    got = dm.block_losses(kl)
    for j, r in enumerate((32, 32, 31)):
        acc = np.float32(0)
        for b in range(r):
            acc = np.float32(acc + kl[32 * j + b, 0])
        assert got[j, 0] == np.float32(np.float32(1) / np.float32(r)) * acc
    assert abs(float(got[2, 1]) - kl[64:, 1].astype(np.float64).mean()) < 1e-6
    # a minibatch of one: the loss is the row's KL
    assert np.array_equal(dm.block_losses(kl[:1]), kl[:1])


def test_reduction_order_is_chunks_of_256_blocks():
    rng = np.random.default_rng(1)
    nb = 256 * 2 + 37
    n = 32 * (nb - 1) + 5
    rows = dm.block_rows(n)
    assert rows.size == nb and rows[-1] == 5
    losses = (rng.random(nb) * 10).astype(np.float32)
    got = dm.reduce_sum(rows, losses)
    prod = rows.astype(np.float64) * losses.astype(np.float64)
    assert np.all(prod == np.array([float(r) * float(l) for r, l in zip(rows, losses)]))   # exact products
    chunks = []
    for c0 in (0, 256, 512):
        s = 0.0
        for p in prod[c0:c0 + 256]:
            s += float(p)
        chunks.append(s)
    assert got == (0.0 + chunks[0]) + chunks[1] + chunks[2]
    # ... which is not the plain ascending chain's bits for these values, and never far from the exact sum
    import math

    exact = math.fsum(prod.tolist())
    assert abs(got - exact) <= 1e-9 * exact
    t = dm.totals(n, np.stack([losses, losses], 1), np.ones(n, np.uint32), np.zeros(n, np.uint32))
    assert t["rows"] == n and t["blocks"] == nb and t["pi_hits"] == n and t["v_hits"] == 0
    assert dm.f64_bits(t["mean_pi"]) == dm.f64_bits(got / np.float64(n)) and t["sum_v"] == got
    z = dm.totals(0, np.zeros((0, 2), np.float32), [], [])
    assert all(z[k] == 0 for k in z)


# ---- the holdout hash
def py_finalise(z):
    m = (1 << 64) - 1
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
    return z ^ (z >> 31)


def py_sm(seed, idx):
    return py_finalise((seed + ((idx + 1) & 0xFFFFFFFF) * 0x9E3779B97F4A7C15) & ((1 << 64) - 1))


def test_holdout_hash_against_hand_computed_values():
    # sm itself, in Python integers: sm(0, 0) is splitmix64's first output for the seed 0
    assert py_sm(0, 0) == 0xE220A8397B1DCDAF
    assert int(sm.sm(np.uint64(0), np.uint64(0))) == 0xE220A8397B1DCDAF
    assert py_sm(5, 0xFFFFFFFF) == py_finalise(5)      # idx + 1 wraps to 0 in 32 bits
    for key, gid in ((0, 0), (1, 0), (0x1234567890ABCDEF, 77), (7 << 32, (3 << 32) + 9), (0xFFFFFFFFFFFFFFFF, -1), (42, -(1 << 40))):
        g = gid & ((1 << 64) - 1)
        want = py_sm(py_sm((key ^ dm.HOLDOUT_TAG) & ((1 << 64) - 1), g >> 32), g & 0xFFFFFFFF) >> 32
        assert int(dm.holdout_hash(key, np.array([gid], np.int64))[0]) == want, (key, gid)
        assert bool(dm.holdout_flags(key, np.array([gid], np.int64), want + 1)[0]) and not bool(dm.holdout_flags(key, np.array([gid], np.int64), want)[0])
    assert int(dm.holdout_hash(0, np.array([0], np.int64))[0]) == py_sm(py_sm(dm.HOLDOUT_TAG, 0), 0) >> 32


def test_holdout_is_by_game_and_about_the_fraction():
    gid = np.repeat(np.arange(20000, dtype=np.int64), 3)
    f = dm.holdout_flags(99, gid, dm.holdout_threshold(0.05))
    assert np.array_equal(f[0::3], f[1::3]) and np.array_equal(f[0::3], f[2::3])
    assert abs(f.mean() - 0.05) < 0.01
    assert not dm.holdout_flags(99, gid, 0).any() and dm.holdout_flags(99, gid, 1 << 32).all()
    assert dm.holdout_threshold(0.25) == 1 << 30 and dm.holdout_threshold(0.0) == 0
    # a larger threshold holds out a superset; another key another set
    g = dm.holdout_flags(99, gid, dm.holdout_threshold(0.10))
    assert (g | ~f).all() and not np.array_equal(f, dm.holdout_flags(100, gid, dm.holdout_threshold(0.05)))


def test_seen_partition():
    tmy = np.array([1, 1, 4, 9], np.uint64); top = np.array([2, 7, 0, 9], np.uint64)
    my = np.array([0, 1, 1, 4, 9, 10], np.uint64); op = np.array([5, 7, 3, 0, 8, 0], np.uint64)
    seen = dm.is_seen(my, op, tmy, top)
    assert seen.tolist() == [False, True, False, True, False, False]
    D = dict(my_bb=my, op_bb=op, pis=np.arange(54, dtype=np.float32).reshape(6, 9), vs=np.arange(18, dtype=np.float32).reshape(6, 3))
    E, n_unseen = dm.unseen_first(D, seen)
    assert n_unseen == 4 and E["my_bb"].tolist() == [0, 1, 9, 10, 1, 4] and E["op_bb"].tolist() == [5, 3, 8, 0, 7, 0]
    assert E["pis"][4].tolist() == D["pis"][1].tolist() and E["vs"][1].tolist() == D["vs"][2].tolist()


def test_the_loops_own_hash_is_the_models():
    from synthesis_amd.learner import HOLDOUT_TAG, _holdout_key, holdout_flags

    assert HOLDOUT_TAG == dm.HOLDOUT_TAG and _holdout_key(7) == 7 << 32 and _holdout_key((1 << 32) + 3) == 3 << 32
    gid = np.concatenate([np.arange(3000, dtype=np.int64), np.array([-1, 1 << 33, (1 << 40) + 5], np.int64)])
    for key, t in ((0, 1 << 30), (_holdout_key(7), dm.holdout_threshold(0.05)), (0xFFFFFFFFFFFFFFFF, 1 << 31)):
        assert np.array_equal(holdout_flags(key, t, gid), dm.holdout_flags(key, gid, t))


# ---- LearningLoop's argument checks (raised before anything touches the engine)
@pytest.mark.parametrize("bad", [-0.1, 1.0, 1.5, "0.1", None, True, float("nan")])
def test_learning_loop_refuses_a_bad_holdout(bad):
    from synthesis_amd.learner import LearningLoop

    with pytest.raises(ValueError, match="holdout"):
        LearningLoop(None, "mlp", np.zeros(30492, np.float32), holdout=bad)
