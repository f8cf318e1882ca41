"""GPU tests of SYN_NET_ARITH_F16X2 on the stress family of tests/f16x2_checkpoints.py: parameter sets that push the per-checkpoint plan
(f16x2_tile.cuh build_f16x2_image, conv_f16x2_tile.cuh build_conv_f16x2_image) to its caps, to negative exponents, to subnormal `lo`
halves and to the edges of the window outside which a load is refused — where the four committed parameter sets never go.

Bars, for every member:
  * a load into an engine that is already in f16x2 reports the plan the restatement chose (oracle/nn_f16x2.hpp; tests/cpp/conv_f16x2_model.cpp);
  * the stand-alone evaluation (ragged sizes, tile boundaries, more than one workgroup) and an evaluation context give the restatement's
    bits, and meet the float64 bars of fc.check_f64_bars;
  * the fused kernels — free-running waves (Connect4Net) and lane-per-tree — play the oracle's search driven by that arithmetic, the
    launch shape asserted;
  * a learner's publish from two of the members arrives in the arithmetic as the restatement evaluates it;
  * the refused members are refused with SYN_ERR_UNSUPPORTED from either side and change nothing.
"""
import numpy as np
import pytest

from tests import f16x2_checkpoints as fc
from tests.test_gpu_parity import assert_search_equal, random_positions

pytestmark = pytest.mark.gpu

EVAL_SIZES = (1, 15, 16, 17, 33, 600)
ROOTS, EXPLORES = 64, 40
LANE_REPLICAS = 65     # 65 x 64 roots = 4,160 trees: more than 16 per CU, so Connect4Net's search leaves the free-running shape


@pytest.fixture(scope="module")
def fixtures():
    return fc.load_fixtures()


@pytest.fixture(scope="module")
def families(fixtures):
    blob, trained, cblob, ctrained = fixtures
    return dict(mlp=fc.mlp_family(blob, trained), conv=fc.conv_family(cblob, ctrained), refused=fc.refused_family(blob))


@pytest.fixture(scope="module")
def positions(oracle):
    my, op = random_positions(oracle, 600, seed=2027)
    my[0] = 0; op[0] = 0
    return my, op


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    from tests import conv_f16x2_model

    return conv_f16x2_model.load(tmp_path_factory.mktemp("conv_f16x2_model"))


@pytest.fixture(scope="module")
def restated(oracle, model, families, positions):
    """restated(net, name) -> (logits, value, plan) of the CPU restatement on `positions`, computed once per member."""
    cache = {}

    def get(net, name, blob=None):
        if (net, name) not in cache or blob is not None:
            w = families[net][name] if blob is None else blob
            my, op = positions
            if net == "mlp":
                l, v = oracle.c4net_eval(w, my, op, mode=oracle.ACC_F16X2)
                p = oracle.f16x2_plan(w)
                p = p if p["ok"] else None
            else:
                l, v = model.eval(w, my, op)
                p = model.plan(w)
            if blob is not None:
                return l, v, p
            cache[(net, name)] = (l, v, p)
        return cache[(net, name)]

    return get


@pytest.fixture(scope="module")
def mlp_engine(fixtures):
    import synthesis_amd as sa

    eng = sa.Engine(concurrent_games=ROOTS * LANE_REPLICAS, max_explores=EXPLORES, device=0)
    eng.load_weights(fixtures[0])
    eng.set_network_arithmetic("f16x2")
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def conv_engine(fixtures):
    import synthesis_amd as sa

    eng = sa.Engine(concurrent_games=256, max_explores=EXPLORES, device=0)
    eng.load_weights_conv(fixtures[2])
    eng.set_network_arithmetic("f16x2")
    yield eng
    eng.close()


def _load(eng, net, w):
    (eng.load_weights if net == "mlp" else eng.load_weights_conv)(w)


def _same_plan(got, want):
    return got is not None and want is not None and all(got[k] == want[k] for k in ("activation_exp", "weight_exp", "out_exp", "bound"))


def _check_evaluation(eng, net, w, ref, positions, oracle, f64, name):
    """The engine holds `w` in f16x2: plan, bits at every size and through a context, the f64 bars."""
    my, op = positions
    ref_l, ref_v, ref_plan = ref
    arith, plan = eng.network_arithmetic()
    assert arith == "f16x2" and _same_plan(plan, ref_plan), (name, plan, ref_plan)
    for n in EVAL_SIZES:
        l, v = eng.policy_eval(my[:n], op[:n])
        assert l.shape == (n, 9) and fc.same_bits(l, ref_l[:n]) and fc.same_bits(v, ref_v[:n]), (name, n)
    ctx = eng.eval_context()
    try:
        cl, cv = ctx.eval(my, op)
    finally:
        ctx.close()
    assert fc.same_bits(cl, ref_l) and fc.same_bits(cv, ref_v), name
    if net == "mlp":
        fl, _ = oracle.c4net_eval(w, my, op, mode=oracle.ACC_FMA)
    else:
        fl, _ = oracle.c4conv_eval(w, my, op, mode=oracle.ACC_FMA)
    fc.check_f64_bars(f"{net} {name}", l, v, fl, *f64(w, my, op))


@pytest.mark.parametrize("name", fc.MLP_MEMBERS)
def test_f16x2_family_member_evaluates_as_restated(mlp_engine, oracle, families, restated, positions, name):
    w = families["mlp"][name]
    mlp_engine.load_weights(w)
    _check_evaluation(mlp_engine, "mlp", w, restated("mlp", name), positions, oracle, fc.mlp_f64, name)


@pytest.mark.parametrize("name", fc.CONV_MEMBERS)
def test_conv_f16x2_family_member_evaluates_as_restated(conv_engine, oracle, families, restated, positions, name):
    w = families["conv"][name]
    conv_engine.load_weights_conv(w)
    _check_evaluation(conv_engine, "conv", w, restated("conv", name), positions, oracle, fc.conv_f64, name)


def _search_exempt(ref):
    """A member whose restated outputs contain a non-finite number has no defined search (computed, not listed)."""
    return not (np.isfinite(ref[0]).all() and np.isfinite(ref[1]).all())


@pytest.mark.parametrize("name", fc.MLP_MEMBERS)
def test_f16x2_family_member_searches_as_the_oracle(mlp_engine, oracle, families, restated, positions, name):
    """Both fused launch shapes of Connect4Net in f16x2: 64 roots run as free-running waves, 65 copies of them (4,160 trees) in the
    lane-per-tree kernel; every copy is the oracle's search."""
    import synthesis_amd as sa
    from tests.oracle_lib import parity_mcts_config

    w = families["mlp"][name]
    if _search_exempt(restated("mlp", name)):
        print(f"{name}: non-finite restated outputs, no search")
        return
    my, op = positions[0][:ROOTS], positions[1][:ROOTS]
    mlp_engine.load_weights(w)
    ref = oracle.c4_mcts_search(parity_mcts_config(), w, my, op, EXPLORES, nn_mode=oracle.ACC_F16X2)
    got = mlp_engine.mcts_search(sa.parity_mcts_config(), my, op, EXPLORES)
    assert mlp_engine.last_launch_shape()[0] == 7
    assert_search_equal(got, ref, f"{name}: free-running")
    got = mlp_engine.mcts_search(sa.parity_mcts_config(), np.tile(my, LANE_REPLICAS), np.tile(op, LANE_REPLICAS), EXPLORES)
    assert mlp_engine.last_launch_shape()[0] == 4
    tiled = {k: np.concatenate([np.asarray(v)] * LANE_REPLICAS, axis=0) for k, v in ref.items()}
    assert_search_equal(got, tiled, f"{name}: lane-per-tree")


@pytest.mark.parametrize("name", fc.CONV_MEMBERS)
def test_conv_f16x2_family_member_searches_as_the_oracle(conv_engine, model, families, restated, positions, name):
    import synthesis_amd as sa
    from tests.oracle_lib import parity_mcts_config

    w = families["conv"][name]
    if _search_exempt(restated("conv", name)):
        print(f"{name}: non-finite restated outputs, no search")
        return
    my, op = positions[0][:ROOTS], positions[1][:ROOTS]
    conv_engine.load_weights_conv(w)
    got = conv_engine.mcts_search(sa.parity_mcts_config(), my, op, EXPLORES)
    assert conv_engine.last_launch_shape()[0] == 4
    assert_search_equal(got, model.mcts_search(parity_mcts_config(), w, my, op, EXPLORES), f"{name}: lane-per-tree")


@pytest.mark.parametrize("net,name", fc.PUBLISH_MEMBERS)
def test_f16x2_publish_from_a_family_member_arrives_as_restated(oracle, families, restated, positions, net, name):
    """The path every iteration of the learning loop takes: a trainer started from the member, three optimiser steps, publish — a fresh
    plan for parameters nobody has seen, evaluated as the restatement evaluates them."""
    import synthesis_amd as sa

    w = families[net][name]
    my, op = positions
    rs = np.random.RandomState(4)
    tpi = rs.dirichlet(np.ones(9), 32).astype(np.float32); tv = rs.dirichlet(np.ones(3), 32).astype(np.float32)
    eng = sa.Engine(concurrent_games=256, max_explores=EXPLORES, device=0)
    try:
        _load(eng, net, w)
        eng.set_network_arithmetic("f16x2")
        (eng.trainer_init if net == "mlp" else eng.trainer_init_conv)(w)
        for _ in range(3):
            eng.train_step(my[:32], op[:32], tpi, tv, 1e-2)
        eng.trainer_publish_weights()
        now = eng.trainer_state()["weights"]
        assert np.abs(now - w).max() > 1e-3
        ref = restated(net, name, blob=now)
        arith, plan = eng.network_arithmetic()
        assert arith == "f16x2" and _same_plan(plan, ref[2]), (plan, ref[2])
        l, v = eng.policy_eval(my, op)
        assert fc.same_bits(l, ref[0]) and fc.same_bits(v, ref[1])
    finally:
        eng.close()


@pytest.mark.parametrize("name", fc.REFUSED_MEMBERS)
def test_f16x2_refused_member_changes_nothing(mlp_engine, families, restated, positions, name):
    """No plan: the load into an f16x2 engine and the switch coming from f32 both fail with SYN_ERR_UNSUPPORTED (-5); after the refused
    load the engine still evaluates the previous member, bit for bit, in the arithmetic and with the plan it had."""
    import synthesis_amd as sa

    my, op = positions
    bad = families["refused"][name]
    prev = "init_b1_plus300"
    ref_l, ref_v, ref_plan = restated("mlp", prev)
    mlp_engine.load_weights(families["mlp"][prev])
    try:
        with pytest.raises(sa.SynthesisAmdError) as e:
            mlp_engine.load_weights(bad)
        assert e.value.code == -5
        arith, plan = mlp_engine.network_arithmetic()
        assert arith == "f16x2" and _same_plan(plan, ref_plan)
        l, v = mlp_engine.policy_eval(my, op)
        assert fc.same_bits(l, ref_l) and fc.same_bits(v, ref_v)
        mlp_engine.set_network_arithmetic("f32")
        mlp_engine.load_weights(bad)   # (f32 takes any parameters)
        with pytest.raises(sa.SynthesisAmdError) as e:
            mlp_engine.set_network_arithmetic("f16x2")
        assert e.value.code == -5
        assert mlp_engine.network_arithmetic() == ("f32", None)
    finally:   # the shared engine goes on in f16x2 with parameters that have a plan
        mlp_engine.set_network_arithmetic("f32")
        mlp_engine.load_weights(families["mlp"][prev])
        mlp_engine.set_network_arithmetic("f16x2")
    l, v = mlp_engine.policy_eval(my, op)
    assert fc.same_bits(l, ref_l) and fc.same_bits(v, ref_v)
