"""Held-out evaluation in other arithmetics (syn_dataset_evaluate_arith), what needs no GPU:
  head model   tests/dataset_eval_arith_model.head equals the oracle's train_gradients / convtrain_gradients losses for single rows on
               checkpoints whose weights are all zero and whose last-layer biases are chosen values (the raw outputs are then the biases
               in any arithmetic): one-hot, all-zero and subnormal targets
  agreement    synthesis_amd.arena.dataset_agreement against the model's restatement and on hand-made rows
  surface      the ABI symbol, the enum values, LearningLoop's refusal of an unknown holdout_arith name
"""
import os
import re

import numpy as np
import pytest

from tests import dataset_eval_arith_model as am
from tests import f16x2_checkpoints as fc
from tests import learner_f32_family as lf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

BIASES = (np.array([0.25, -1.5, 3.0, 0.0, 2.999, -7.25, 0.125, 1.0, 3.0, -0.5, 0.75, 0.75], np.float32),
          np.array([-20.0, 40.0, 1e-3, -1e-3, 0.0, 0.0, 12.5, -3.0, 39.5, 88.0, -88.0, 0.0], np.float32),
          np.zeros(12, np.float32))


def zero_weights_with_bias(net, bias):
    w = np.zeros(lf.family(net)["zero"].size, np.float32)
    (fc.mlp_views(w)[4][1] if net == "mlp" else fc.conv_views(w)[3])[:] = bias
    return w


def target_rows():
    """(name, tpi [9], tv [3])"""
    rec = lf.recorded()
    sub = rec[2][5].copy(); sub[int(np.argmin(sub))] = np.float32(1e-42)
    half = (rec[2][9] * np.float32(0.5)).astype(np.float32)
    return (("recorded", rec[2][3].copy(), rec[3][3].copy()), ("onehot", np.eye(9, dtype=np.float32)[4], np.eye(3, dtype=np.float32)[2]),
            ("zero", np.zeros(9, np.float32), np.zeros(3, np.float32)), ("subnormal", sub, rec[3][5].copy()),
            ("half", half, np.array([0.5, 0.0, 0.25], np.float32)))


@pytest.mark.parametrize("net", lf.NETS)
def test_head_model_equals_the_oracle_on_bias_only_checkpoints(oracle, net):
    rec = lf.recorded()
    for bi, bias in enumerate(BIASES):
        w = zero_weights_with_bias(net, bias)
        for name, tpi, tv in target_rows():
            for pos in (0, 17):
                b = (rec[0][pos:pos + 1], rec[1][pos:pos + 1], tpi[None], tv[None])
                _, want = lf.oracle_gradients(oracle, net, w, "default", b)
                got = am.row_kl(oracle, bias[None], tpi[None], tv[None])[0]
                assert fc.same_bits(got, want), (net, bi, name, pos, got, want)
                if name == "zero":
                    assert not got.view(np.uint32).any()


def test_head_model_rows_are_independent(oracle):
    """the vectorised model on many rows is the model on every row alone"""
    rs = np.random.RandomState(3)
    raw = (rs.standard_normal((40, 12)) * 4).astype(np.float32)
    my, op, tpi, tv = lf.batch("subnormal_t", 40)
    all_rows = am.row_kl(oracle, raw, tpi, tv)
    for i in (0, 7, 39):
        assert fc.same_bits(all_rows[i], am.row_kl(oracle, raw[i:i + 1], tpi[i:i + 1], tv[i:i + 1])[0])


def full_column(col):
    return sum(1 << (r + 7 * col) for r in (0, 2, 4, 6)), sum(1 << (r + 7 * col) for r in (1, 3, 5))


def test_dataset_agreement_hand_made_rows():
    from synthesis_amd.arena import dataset_agreement

    rs = np.random.RandomState(1)
    a = rs.standard_normal((6, 12)).astype(np.float32)
    empty = np.zeros(6, np.uint64)
    z = dataset_agreement(a, a, empty, empty)
    assert z["rows"] == 6 and all(z[k] == 0.0 for k in z if k != "rows")
    # a swapped maximum on a FULL column does not count: column 4 is full, a's largest logit sits there, b's elsewhere on the full column's
    # side only
    my4, op4 = full_column(4)
    a = np.zeros((1, 12), np.float32); b = np.zeros((1, 12), np.float32)
    a[0, :9] = [0, 1, 0, 0, 9, 0, 0, 0, 0]; b[0, :9] = [0, 1, 0, 0, -9, 0, 0, 0, 0]
    r = dataset_agreement(a, b, np.array([my4], np.uint64), np.array([op4], np.uint64))
    assert r["pi_argmax_differs"] == 0.0 and r["mean_kl_pi"] == 0.0 and r["max_abs_diff"] == 18.0 and r["mean_abs_diff"] == 1.5
    # ... and does on an empty board
    r = dataset_agreement(a, b, np.zeros(1, np.uint64), np.zeros(1, np.uint64))
    assert r["pi_argmax_differs"] == 1.0 and r["mean_kl_pi"] > 1.0
    # two equal maxima: the first one is the arg-max (columns 2 and 6 tie in a -> 2; b prefers 6 by a hair -> differs; c prefers 2 -> same)
    a = np.zeros((1, 12), np.float32); a[0, 2] = a[0, 6] = 1.0
    b = a.copy(); b[0, 6] = np.nextafter(np.float32(1.0), np.float32(2.0))
    c = a.copy(); c[0, 2] = np.nextafter(np.float32(1.0), np.float32(2.0))
    e1 = np.zeros(1, np.uint64)
    assert dataset_agreement(a, b, e1, e1)["pi_argmax_differs"] == 1.0 and dataset_agreement(a, c, e1, e1)["pi_argmax_differs"] == 0.0
    a = np.zeros((1, 12), np.float32); a[0, 10] = a[0, 11] = 2.0
    b = a.copy(); b[0, 11] = 2.5
    assert dataset_agreement(a, b, e1, e1)["v_argmax_differs"] == 1.0 and dataset_agreement(a, a, e1, e1)["v_argmax_differs"] == 0.0
    # a row without a legal column: no arg-max difference, KL 0
    full_my = sum(full_column(c)[0] for c in range(9)); full_op = sum(full_column(c)[1] for c in range(9))
    r = dataset_agreement(a, b, np.array([full_my], np.uint64), np.array([full_op], np.uint64))
    assert r["pi_argmax_differs"] == 0.0 and r["mean_kl_pi"] == 0.0
    assert dataset_agreement(a[:0], a[:0], e1[:0], e1[:0])["rows"] == 0


def test_dataset_agreement_equals_the_restatement():
    from synthesis_amd.arena import dataset_agreement

    rs = np.random.RandomState(7)
    my, op, _, _ = lf.batch("empty_board", 64)
    my = my.copy(); op = op.copy()
    my[5], op[5] = full_column(0)
    a = (rs.standard_normal((64, 12)) * 3).astype(np.float32)
    b = (a + rs.standard_normal((64, 12)).astype(np.float32) * np.float32(0.5)).astype(np.float32)
    got, want = dataset_agreement(a, b, my, op), am.dataset_agreement(a, b, my, op)
    assert set(got) == set(want) and got["rows"] == want["rows"] == 64
    assert 0.0 < got["pi_argmax_differs"] < 1.0 and got["mean_kl_pi"] > 0.0
    for k in want:
        assert abs(got[k] - want[k]) <= 1e-12 * max(1.0, abs(want[k])), (k, got[k], want[k])


def test_abi_symbol_and_enum_values():
    from synthesis_amd import engine

    assert "syn_dataset_evaluate_arith" in engine.ABI_SYMBOLS and hasattr(engine.load_library(), "syn_dataset_evaluate_arith")
    assert engine.EVAL_ARITHMETICS == {"f32": 0, "f16x2": 1, "bf16": 2}
    header = open(os.path.join(ROOT, "include", "synthesis_amd.h")).read()
    for name, value in (("SYN_EVAL_ARITH_F32", 0), ("SYN_EVAL_ARITH_F16X2", 1), ("SYN_EVAL_ARITH_BF16", 2)):
        assert re.search(rf"\b{name} = {value}\b", header), name
    assert "int syn_dataset_evaluate_arith(syn_engine* h, int which, size_t first_row, size_t n_rows, const float* blob, size_t n_floats, " \
           "int arithmetic," in header
    assert "Out of scope: evaluation in the f16x2 arithmetic" not in header


def test_learning_loop_refuses_an_unknown_holdout_arith():
    from synthesis_amd.learner import HOLDOUT_ARITHMETICS, LearningLoop

    assert HOLDOUT_ARITHMETICS == ("f32", "f16x2", "bf16")
    blob = np.zeros(30492, np.float32)
    for bad in (("f64",), ("f32", "fp16"), "f16"):
        with pytest.raises(ValueError, match="holdout_arith"):
            LearningLoop(None, "mlp", blob, holdout=0.25, holdout_arith=bad)
    with pytest.raises(ValueError, match="bf16"):
        LearningLoop(None, "mlp", blob, holdout=0.25, holdout_arith=("f32", "bf16"))
