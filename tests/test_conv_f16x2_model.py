"""Connect4ConvNet in the f16x2 arithmetic, host side (no GPU): the product's plan (syn_f16x2_plan_of_blob on a 12,412-float blob: the code
behind syn_set_network_arithmetic for the conv network) against the CPU model's independent restatement (tests/cpp/conv_f16x2_model.cpp),
the model itself against the canonical slimnn-order evaluation, and the learning loop's arithmetic argument."""
import os

import numpy as np
import pytest


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
