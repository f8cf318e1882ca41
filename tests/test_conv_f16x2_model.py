"""Connect4ConvNet in the f16x2 arithmetic, host side (no GPU): the product's plan (syn_f16x2_plan_of_blob on a 12,412-float blob: the code
behind syn_set_network_arithmetic for the conv network) against the CPU model's independent restatement (tests/cpp/conv_f16x2_model.cpp),
the model itself against the canonical slimnn-order evaluation, and the learning loop's arithmetic argument."""
import os

import numpy as np
import pytest

from tests import f16x2_checkpoints as fc


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    from tests import conv_f16x2_model

    return conv_f16x2_model.load(tmp_path_factory.mktemp("conv_f16x2_model"))


@pytest.fixture(scope="module")
def blobs(golden_dir):
    from bench import make_conv_weights

    return make_conv_weights(), np.load(os.path.join(golden_dir, "c4conv_trained_f32.npy"))


def test_product_plan_is_the_models_plan(model, blobs):
    """Exponent for exponent and bound for bound, on both blobs and on rescaled copies; layer 0 = the conv layer (inputs unscaled), layer 1
    = the head, entries 2..4 zero; a blob with a non-finite parameter has no plan on either side."""
    from synthesis_amd.engine import f16x2_plan_of_blob

    rand, trained = blobs
    for w in (rand, trained, (rand * np.float32(37.5)).astype(np.float32), (trained * np.float32(2.0 ** -9)).astype(np.float32)):
        a, b = f16x2_plan_of_blob(w), model.plan(w)
        assert a is not None and b is not None
        assert a["network"] == "Connect4ConvNet"
        assert a["activation_exp"] == b["activation_exp"] and a["weight_exp"] == b["weight_exp"] and a["out_exp"] == b["out_exp"]
        assert a["bound"] == b["bound"]
        assert a["activation_exp"][0] == 0 and a["activation_exp"][2:] == [0, 0, 0] and a["bound"][2:] == [0.0, 0.0, 0.0]
    for at in (5, 300, 1000, 12411):   # a conv weight, a conv bias, a head weight, a head bias
        bad = rand.copy(); bad[at] = np.inf
        assert f16x2_plan_of_blob(bad) is None and model.plan(bad) is None
    assert f16x2_plan_of_blob(np.load(os.path.join(os.path.dirname(__file__), "golden", "c4net_blob_f32.npy")))["network"] == "Connect4Net"


def test_model_is_within_tolerance_of_the_slimnn_order(model, oracle, blobs):
    """The definition itself (before any GPU is involved): the random-init network within 1e-5 / 3 of slimnn's own loop order, the
    trained checkpoint within 2e-6 of its logits' scale."""
    from tests.test_gpu_parity import random_positions

    rand, trained = blobs
    my, op = random_positions(oracle, 400, seed=12)
    my[0] = 0; op[0] = 0
    l, v = model.eval(rand, my, op)
    sl, sv = oracle.c4conv_eval(rand, my, op, mode=oracle.ACC_SLIMNN)
    assert np.abs(l - sl).max() < 1e-5 / 3 and np.abs(v - sv).max() < 1e-5 / 3
    l, v = model.eval(trained, my, op)
    sl, sv = oracle.c4conv_eval(trained, my, op, mode=oracle.ACC_SLIMNN)
    assert np.abs(l - sl).max() / max(1.0, float(np.abs(sl).max())) < 2e-6 and np.abs(v - sv).max() < 1e-5


# ---- the stress family (tests/f16x2_checkpoints.py) -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def family(blobs):
    return fc.conv_family(*blobs)


@pytest.fixture(scope="module")
def family_positions(oracle):
    from tests.test_gpu_parity import random_positions

    return random_positions(oracle, 1000, seed=2026)


def test_f64_reference_is_the_conv_network(oracle, blobs, family_positions):
    """The yardstick itself (fc.conv_f64, plain numpy float64) computes the function of the oracle's slimnn-order Connect4ConvNet."""
    my, op = family_positions
    my = np.concatenate([np.zeros(1, np.uint64), my[:300]]); op = np.concatenate([np.zeros(1, np.uint64), op[:300]])   # + the empty board
    for w, tol in zip(blobs, (2e-6, 5e-5)):
        raw, v = fc.conv_f64(w, my, op)
        sl, sv, sraw = oracle.c4conv_eval(w, my, op, mode=oracle.ACC_SLIMNN, raw=True)
        assert np.abs(raw - sraw).max() < tol and np.abs(v - sv).max() < 2e-6


@pytest.mark.parametrize("name", fc.CONV_MEMBERS)
def test_conv_f16x2_family_member_meets_the_f64_bars(model, oracle, family, family_positions, name):
    """Every member, 1,000 reachable positions: the CPU model of the definition against float64 (fc.check_f64_bars)."""
    my, op = family_positions
    w = family[name]
    l, v = model.eval(w, my, op)
    fl, _ = oracle.c4conv_eval(w, my, op, mode=oracle.ACC_FMA)
    raw, v64 = fc.conv_f64(w, my, op)
    fc.check_f64_bars("conv " + name, l, v, fl, raw, v64)


def test_conv_family_plans_agree_between_the_product_and_the_model(model, blobs, family):
    """syn_f16x2_plan_of_blob against the model's plan on every member and on init x 2^k for every k in -30..30: the same verdict, the
    same exponents and bounds. The family reaches both caps (tc and th at 40, s1 at 24), negative exponents and both signs of the
    rescale exponent s1 - tc."""
    from synthesis_amd.engine import f16x2_plan_of_blob

    def same(w, ctx):
        a, b = f16x2_plan_of_blob(w), model.plan(w)
        assert (a is None) == (b is None), ctx
        if a is not None:
            assert a["activation_exp"] == b["activation_exp"] and a["weight_exp"] == b["weight_exp"] and a["out_exp"] == b["out_exp"], ctx
            assert a["bound"] == b["bound"], ctx
            assert abs(b["weight_exp"][0]) <= 60 and abs(b["activation_exp"][1] + b["weight_exp"][1]) <= 60, ctx
            assert b["out_exp"] == -(b["activation_exp"][1] + b["weight_exp"][1]), ctx
        return b

    plans = {name: same(w, name) for name, w in family.items()}
    assert all(p is not None for p in plans.values())
    every = list(plans.values())
    assert any(p["activation_exp"][1] == 24 for p in every)                                            # the s cap
    assert any(p["weight_exp"][0] == 40 for p in every) and any(p["weight_exp"][1] == 40 for p in every)   # the t cap, conv and head
    assert plans["zero"]["weight_exp"][:2] == [0, 0] and plans["init_convW_zero"]["weight_exp"][0] == 0
    assert any(p["activation_exp"][1] < 0 for p in every) and any(min(p["weight_exp"][:2]) < 0 for p in every)
    cexp = [p["activation_exp"][1] - p["weight_exp"][0] for p in every]
    assert min(cexp) < 0 < max(cexp)
    rand = blobs[0]
    ok_p, edges = fc.accept_edges(lambda w: f16x2_plan_of_blob(w) is not None, rand)
    ok_m, _ = fc.accept_edges(lambda w: model.plan(w) is not None, rand)
    assert ok_p == ok_m
    for k in ok_p:
        same(rand * np.float32(2.0) ** np.float32(k), k)
    print(f"Connect4ConvNet init x 2^k: accepted for k in [{edges['last_accepted_down']}, {edges['last_accepted_up']}], "
          f"refused at {edges['first_refused_down']} and {edges['first_refused_up']}")
    assert edges["first_refused_down"] == edges["last_accepted_down"] - 1   # (upwards every k of the sweep has a plan)
    assert all(ok_p[k] for k in range(edges["last_accepted_down"], 31))


def test_conv_f16x2_family_replays_device_bits_and_plans(model, golden_dir, family):
    """What an MI355X computed for every member (64 positions; tests/golden/make_f16x2_family_golden.py): the model reproduces every
    bit and the plan's exponents."""
    g = np.load(os.path.join(golden_dir, "f16x2_family_device.npz"))
    my, op = g["my_bb"], g["op_bb"]
    for name, w in family.items():
        l, v = model.eval(w, my, op)
        assert fc.same_bits(l, g[f"conv.{name}.logits"]) and fc.same_bits(v, g[f"conv.{name}.value"]), name
        plan = model.plan(w)
        assert plan["activation_exp"] + plan["weight_exp"] + [plan["out_exp"]] == g[f"conv.{name}.plan"].tolist(), name


def test_learning_loop_runs_self_play_in_the_chosen_arithmetic():
    """LearningLoop(network_arithmetic=...) hands the choice to its engine once, after the first load; the default leaves it alone."""
    from bench import make_conv_weights
    from synthesis_amd.learner import LearningLoop

    class Recording:
        def __init__(self):
            self.calls = []

        def __getattr__(self, name):
            return lambda *a, **k: self.calls.append((name, a))

    for arith, want in (("f16x2", [("set_network_arithmetic", ("f16x2",))]), ("f32", [])):
        eng = Recording()
        LearningLoop(eng, "conv", make_conv_weights(), network_arithmetic=arith)
        names = [c[0] for c in eng.calls]
        assert names[0] == "load_weights_conv" and "trainer_init_conv" in names
        assert [c for c in eng.calls if c[0] == "set_network_arithmetic"] == want
