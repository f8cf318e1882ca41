"""The device-side epoch sampler without a GPU: its C ABI (header, ABI_SYMBOLS, the built library, the ctypes mirror), the properties
of its definition on the numpy model (tests/sampler_model.py restates include/synthesis_amd.h), and LearningLoop's argument checks."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import sampler_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("syn_train_epochs_sampled", "syn_debug_sampler")


def header_text():
    with open(os.path.join(ROOT, "include", "synthesis_amd.h")) as f:
        return f.read()


def test_new_symbols_in_header_abi_list_and_library():
    from synthesis_amd.engine import ABI_SYMBOLS

    declared = set(re.findall(r"\b(syn_[a-z0-9_]+)\s*\(", header_text()))
    exported = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "synthesis_amd", "libsynthesis_amd.so")]).decode()
    exported = {line.split()[-1] for line in exported.splitlines() if line.strip()}
    for s in NEW_SYMBOLS:
        assert s in declared, s
        assert s in ABI_SYMBOLS, s
        assert s in exported, s


def test_ctypes_struct_matches_the_header():
    from synthesis_amd.engine import CSamplerConfig

    body = re.search(r"typedef struct syn_sampler_config \{(.*?)\} syn_sampler_config;", header_text(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [tuple(d.split()) for d in body.split(";") if d.strip()]
    ctype = {"uint64_t": C.c_uint64, "uint32_t": C.c_uint32, "int32_t": C.c_int32}
    assert [(name, ctype[t]) for t, name in fields] == list(CSamplerConfig._fields_)
    assert [name for _, name in fields] == ["key", "first_epoch", "flip"]
    assert C.sizeof(CSamplerConfig) == 16
    assert (CSamplerConfig.key.offset, CSamplerConfig.first_epoch.offset, CSamplerConfig.flip.offset) == (0, 8, 12)
    h = header_text()
    assert re.search(r"SYN_SAMPLER_FLIP_NONE = 0, SYN_SAMPLER_FLIP_RANDOM = 1", h)
    assert "0x5AD3C0DE5EED1E55" in h and model.SAMPLER_TAG == 0x5AD3C0DE5EED1E55


def test_model_arithmetic_wraps_as_the_header_says():
    # splitmix64's published first output from state 0 is finalise(GOLDEN): sm(0, 0)
    assert int(model.sm(0, 0)) == 0xE220A8397B1DCDAF
    # idx + 1 in 32 bits: idx = 2^32 - 1 gives finalise(seed)
    assert int(model.sm(5, 0xFFFFFFFF)) == int(model.finalise(np.uint64(5)))
    assert int(model.epoch_key(model.M64, 1)) == int(model.sm((model.M64 ^ model.SAMPLER_TAG), 1))


def test_keys_distinct_at_2_pow_20():
    k = model.sort_keys(0x1234, 3, 1 << 20)
    assert k.dtype == np.uint64 and np.unique(k).size == 1 << 20


@pytest.mark.parametrize("n", [1, 2, 33, 1000])
def test_perm_is_a_permutation_and_epochs_differ(n):
    for key in (0, 1, model.M64):
        for e in (0, 1, 0xFFFFFFFE):
            p0, f0 = model.sampler(key, e, n)
            p1, f1 = model.sampler(key, e + 1, n)
            assert p0.dtype == np.int32 and np.array_equal(np.sort(p0), np.arange(n))
            assert np.array_equal(np.sort(p1), np.arange(n))
            assert set(np.unique(f0)) <= {0, 1} and f0.shape == (n,)
            if n >= 33:   # (n <= 2 has at most two orders: equal by chance is no defect)
                assert not np.array_equal(p0, p1) and not np.array_equal(f0, f1)
            assert int(model.epoch_key(key, e)) != int(model.epoch_key(key, e + 1))


def run_statistics(runs):
    """(chi-square of where row 0 lands, chi-square of the row that lands first, fraction of flipped rows) over (key, epoch) runs at n = 64"""
    pos0, first, flipped = np.zeros(64), np.zeros(64), 0
    for key, epoch in runs:
        p, f = model.sampler(key, epoch, 64)
        pos0[int(np.flatnonzero(p == 0)[0])] += 1
        first[int(p[0])] += 1
        flipped += int(f.sum())
    return model.chi_square(pos0), model.chi_square(first), flipped / (64.0 * len(runs))


@pytest.mark.parametrize("name, runs, expect", [
    ("keys 0..19999 at epoch 0", [(k, 0) for k in range(20000)], (69.3, 81.7, 0.49982)),
    ("key 7 at epochs 0..19999", [(7, e) for e in range(20000)], (66.5, 61.4, 0.50034)),
])
def test_order_is_uniform_over_64_cells(name, runs, expect):
    """The 99.9 % point of chi-square with 63 degrees of freedom is about 103: both statistics stay below 110, and the flip fraction
    within 0.5 +- 0.002. The figures of this definition are pinned too (they are deterministic)."""
    c_pos, c_first, frac = run_statistics(runs)
    print(name, c_pos, c_first, frac)
    assert c_pos < 110 and c_first < 110
    assert abs(frac - 0.5) < 0.002
    assert (round(c_pos, 1), round(c_first, 1), round(frac, 5)) == expect


def test_sampler_key_of_the_loop():
    from synthesis_amd.learner import _sampler_key

    assert _sampler_key(0, 0) == 0 and _sampler_key(1, 2) == (1 << 32) | 2
    assert _sampler_key(-1, 5) == (0xFFFFFFFF << 32) | 5 and 0 <= _sampler_key(1 << 40, 1 << 33) < 1 << 64
    assert len({_sampler_key(s, i) for s in range(4) for i in range(4)}) == 16


def test_learning_loop_argument_validation_needs_no_engine():
    from synthesis_amd.learner import LearningLoop

    blob = np.zeros(30492, np.float32)
    with pytest.raises(ValueError, match="sampler"):
        LearningLoop(None, "mlp", blob, sampler="gpu")
    for sampler in ("numpy", "torch"):
        with pytest.raises(ValueError, match="flip"):
            LearningLoop(None, "mlp", blob, sampler=sampler, flip=True)
    with pytest.raises(ValueError, match="replay"):
        LearningLoop(None, "mlp", blob, sampler="device", flip=True, replay="disk")
    # sampler="device" with flip passes the argument checks: the next thing the constructor does is use the engine
    with pytest.raises(AttributeError):
        LearningLoop(None, "mlp", blob, sampler="device", flip=True)
