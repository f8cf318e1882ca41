"""GPU parity tests of Connect4ConvNet in the f16x2 arithmetic (synthesis_amd/csrc/conv_f16x2_tile.cuh; syn_set_network_arithmetic with
the conv network loaded).

Bars:
  * the network: EXACTLY the CPU model of the definition (tests/cpp/conv_f16x2_model.cpp on oracle/nn_f16x2.hpp's model of
    v_mfma_f32_16x16x32_f16), within north_star's 1e-5 of slimnn's loop order on the random-init network, as close to it as the f32
    arithmetic relative to the logits' scale on the trained checkpoint;
  * searches and whole games: bit-exact against the oracle's MCTS / run_game driven by that model, on every launch shape shipped;
  * the stand-alone evaluation and the fused kernels produce the same bits (a search's priors are the stand-alone softmax).
"""
import os

import numpy as np
import pytest

from tests.test_gpu_convnet import conv_blob
from tests.test_gpu_parity import SELFPLAY_KEYS, assert_search_equal, assert_selfplay_equal, random_positions

pytestmark = pytest.mark.gpu

NN_TOL = 1e-5   # north_star: "policy/value outputs within 1e-5 fp32"


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    from tests import conv_f16x2_model

    return conv_f16x2_model.load(tmp_path_factory.mktemp("conv_f16x2_model"))


@pytest.fixture(scope="module")
def cblob():
    return conv_blob()


@pytest.fixture(scope="module")
def trained(golden_dir):
    return np.load(os.path.join(golden_dir, "c4conv_trained_f32.npy"))


@pytest.fixture(scope="module")
def engine(cblob):
    import synthesis_amd as sa

    eng = sa.Engine(concurrent_games=1100, max_explores=800, device=0)
    eng.load_weights_conv(cblob)
    eng.set_network_arithmetic("f16x2")
    yield eng
    eng.close()


def _bits_equal(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


def test_conv_f16x2_network_is_the_models_bits_and_within_tolerance(engine, oracle, model, cblob):
    name, plan = engine.network_arithmetic()
    want = model.plan(cblob)
    assert name == "f16x2" and plan["network"] == "Connect4ConvNet"
    assert all(plan[k] == want[k] for k in ("activation_exp", "weight_exp", "out_exp", "bound"))
    my, op = random_positions(oracle, 3000, seed=3)
    my[0] = 0; op[0] = 0
    logits, value = engine.policy_eval(my, op)
    ref_l, ref_v = model.eval(cblob, my, op)
    assert _bits_equal(logits, ref_l) and _bits_equal(value, ref_v)
    sl, sv = oracle.c4conv_eval(cblob, my, op, mode=oracle.ACC_SLIMNN)
    err = max(float(np.abs(logits - sl).max()), float(np.abs(value - sv).max()))
    print(f"conv f16x2 against the slimnn order: max error {err:.3e}, margin {NN_TOL / max(err, 1e-30):.1f}x under 1e-5")
    assert err < NN_TOL
    # ragged sizes and tile boundaries; evaluation contexts run the same arithmetic
    for n in (0, 1, 15, 16, 17, 33, 2999):
        l, v = engine.policy_eval(my[:n], op[:n])
        assert l.shape == (n, 9) and _bits_equal(l, ref_l[:n]) and _bits_equal(v, ref_v[:n])
    ctx = engine.eval_context()
    for n in (1, 700, 3000):
        l, v = ctx.eval(my[:n], op[:n])
        assert _bits_equal(l, ref_l[:n]) and _bits_equal(v, ref_v[:n])
    ctx.close()
    # a large batch: every tile of the grid-stride loop gives the first tile's answer
    big_l, big_v = engine.policy_eval(np.tile(my[:2048], 160), np.tile(op[:2048], 160))
    assert np.array_equal(big_l.reshape(160, 2048, 9), np.broadcast_to(ref_l[:2048], (160, 2048, 9)))
    assert np.array_equal(big_v.reshape(160, 2048, 3), np.broadcast_to(ref_v[:2048], (160, 2048, 3)))


def test_conv_f16x2_trained_checkpoint_is_as_close_to_the_slimnn_order_as_f32(oracle, model, trained):
    import synthesis_amd as sa

    my, op = random_positions(oracle, 3000, seed=9)
    eng = sa.Engine(concurrent_games=256, max_explores=64, device=0)
    try:
        eng.load_weights_conv(trained)
        f32_l, f32_v = eng.policy_eval(my, op)
        eng.set_network_arithmetic("f16x2")
        l, v = eng.policy_eval(my, op)
        ref_l, ref_v = model.eval(trained, my, op)
        assert _bits_equal(l, ref_l) and _bits_equal(v, ref_v)
        sl, sv = oracle.c4conv_eval(trained, my, op, mode=oracle.ACC_SLIMNN)
        scale = max(1.0, float(np.abs(sl).max()))
        print(f"trained conv checkpoint: logit scale {scale:.1f}, f16x2 error {np.abs(l - sl).max():.3e}, f32 error {np.abs(f32_l - sl).max():.3e}")
        assert np.abs(l - sl).max() / scale < 2e-6 and np.abs(v - sv).max() < NN_TOL
        assert np.abs(l - sl).max() <= 4.0 * max(float(np.abs(f32_l - sl).max()), 1e-7)
        eng.set_network_arithmetic("f32")
        b_l, b_v = eng.policy_eval(my[:500], op[:500])
        assert np.array_equal(b_l, f32_l[:500]) and np.array_equal(b_v, f32_v[:500])
    finally:
        eng.close()


def test_conv_f16x2_searches_match_the_model_driven_oracle(engine, oracle, model, cblob):
    import synthesis_amd as sa
    from tests.oracle_lib import parity_mcts_config

    my, op = random_positions(oracle, 64, seed=7)
    my[0] = 0; op[0] = 0
    for explores in (0, 1, 37, 200):
        got = engine.mcts_search(sa.parity_mcts_config(), my, op, explores)
        ref = model.mcts_search(parity_mcts_config(), cblob, my, op, explores)
        assert_search_equal(got, ref, f"explores={explores}")
    # the root's priors are the stand-alone kernel's softmax: fused == stand-alone, bit for bit
    got = engine.mcts_search(sa.parity_mcts_config(), my[:24], op[:24], 1)
    l, _ = engine.policy_eval(my[:24], op[:24])
    for i in range(24):
        legal = [c for c in range(9) if not ((int(my[i]) | int(op[i])) >> (6 + 7 * c)) & 1]
        e = np.exp(l[i][legal] - l[i][legal].max())
        assert np.allclose(got["child_P"][i][legal], e / e.sum(), rtol=1e-6, atol=1e-7)


def test_conv_f16x2_selfplay_matches_the_model_driven_oracle(engine, oracle, model, cblob):
    import synthesis_amd as sa
    from tests.oracle_lib import parity_mcts_config, parity_rollout_config

    got = engine.selfplay(sa.parity_rollout_config(800), base_seed=11, n_games=12, counters=True)
    ref = model.selfplay(parity_rollout_config(800), cblob, 11, 12, threads=8)
    assert_selfplay_equal(got, ref, "parity configuration, 800 explores")
    for k in ("explores", "select_levels", "expansions", "new_nodes", "policy_evals", "backprop_levels"):
        assert got["counters"][k] == ref["counters"][k], k
    # the reference's self-play configuration (Fpu::Normal(1.0, 0.1), FAST = 2 family) with PolicyWithCache, at a moderate size
    eng = sa.Engine(concurrent_games=256, max_explores=100, device=0, policy_cache_log2=14)
    try:
        eng.load_weights_conv(cblob)
        eng.set_network_arithmetic("f16x2")
        cfg = sa.parity_rollout_config(100)
        cfg.mcts_cfg = sa.reference_selfplay_mcts_config()
        got = eng.selfplay(cfg, base_seed=4, n_games=300)   # (refills included: 300 games over 256 slots)
        rcfg = parity_rollout_config(100, mcts=parity_mcts_config(fpu=2, fpu_value=1.0, fpu_std=0.1))
        ref = model.selfplay(rcfg, cblob, 4, 300, threads=8, use_cache=True)
        assert_selfplay_equal(got, ref, "reference configuration with the policy cache")
        hits, misses = eng.last_cache_stats()
        assert hits > 0 and misses > 0
    finally:
        eng.close()


@pytest.mark.parametrize("nw", [4, 8])
def test_conv_f16x2_every_wave_count_plays_the_same_games(oracle, model, trained, monkeypatch, nw):
    import synthesis_amd as sa
    from tests.oracle_lib import parity_mcts_config, parity_rollout_config

    monkeypatch.setenv("SYN_DEBUG", "1")
    monkeypatch.setenv("SYN_LANES", str(nw))
    my, op = random_positions(oracle, 40, seed=21)
    ref_s = model.mcts_search(parity_mcts_config(), trained, my, op, 200)
    ref_g = model.selfplay(parity_rollout_config(80), trained, 5, 150, threads=8)
    eng = sa.Engine(concurrent_games=64 * nw, max_explores=200, device=0)
    try:
        eng.load_weights_conv(trained)
        eng.set_network_arithmetic("f16x2")
        assert_search_equal(eng.mcts_search(sa.parity_mcts_config(), my, op, 200), ref_s, f"nw={nw}")
        assert_selfplay_equal(eng.selfplay(sa.parity_rollout_config(80), base_seed=5, n_games=150), ref_g, f"nw={nw}")
        shape = eng.last_launch_shape()
        assert shape[0] == 4 and shape[2] == 64 * nw, shape
        # the self-play instantiation with the event counters at this wave count
        got = eng.selfplay(sa.parity_rollout_config(80), base_seed=5, n_games=60, counters=True)
        ref = model.selfplay(parity_rollout_config(80), trained, 5, 60, threads=8)
        assert_selfplay_equal(got, ref, f"nw={nw} with counters")
        for k in ("explores", "select_levels", "expansions", "new_nodes", "policy_evals", "backprop_levels"):
            assert got["counters"][k] == ref["counters"][k], k
        if nw == 4:   # the runtime-switched family (Uct + ParentQ) runs at 4 waves: search, self-play, self-play with counters
            got = eng.mcts_search(sa.parity_mcts_config(exploration=sa.Exploration.Uct, c=1.5, fpu=sa.Fpu.ParentQ), my, op, 150)
            ref = model.mcts_search(parity_mcts_config(exploration=0, c=1.5, fpu=1), trained, my, op, 150)
            assert_search_equal(got, ref, "Uct/ParentQ")
            cfg = sa.parity_rollout_config(60)
            cfg.mcts_cfg = sa.parity_mcts_config(exploration=sa.Exploration.Uct, c=1.5, fpu=sa.Fpu.ParentQ)
            rcfg = parity_rollout_config(60, mcts=parity_mcts_config(exploration=0, c=1.5, fpu=1))
            ref = model.selfplay(rcfg, trained, 6, 60, threads=8)
            for counters in (False, True):
                got = eng.selfplay(cfg, base_seed=6, n_games=60, counters=counters)
                assert eng.last_launch_shape()[2] == 256
                assert_selfplay_equal(got, ref, f"Uct/ParentQ self-play, counters={counters}")
            assert got["counters"]["policy_evals"] == ref["counters"]["policy_evals"]
    finally:
        eng.close()


def test_conv_f16x2_bench_shape_plays_the_models_games(model, cblob, monkeypatch):
    """The with_conv_policy leg's engine (262,144 slots, bench.make_conv_weights, the headline configuration) in the f16x2 arithmetic:
    slices of its games equal the model-driven oracle's."""
    import synthesis_amd as sa
    from tests.oracle_lib import parity_rollout_config

    for k in ("SYN_DEBUG", "SYN_LANES", "SYN_LANES2", "SYN_QUADS", "SYN_LANE_THRESH", "SYN_PROFILE", "SYN_PC", "SYN_FREE", "SYN_POOL"):
        monkeypatch.delenv(k, raising=False)
    conc, seed = 262144, 20260
    n_games = 140000
    big = sa.Engine(concurrent_games=conc, max_explores=800, device=0)
    try:
        big.load_weights_conv(cblob)
        big.set_network_arithmetic("f16x2")
        got = big.selfplay(sa.parity_rollout_config(800), base_seed=seed, n_games=n_games)
        shape, grid, threads = big.last_launch_shape()
        assert shape == 4 and threads == 512
    finally:
        big.close()
    for first in (0, 65536 + 5, grid * threads - 4, n_games - 8):
        ref = model.selfplay(parity_rollout_config(800), cblob, seed, 8, first_game=first, threads=8)
        sub = {k: got[k][first:first + 8] for k in SELFPLAY_KEYS}
        assert_selfplay_equal(sub, ref, f"bench shape, games {first}..{first + 7}")


def test_conv_f16x2_switches_cleanly(oracle, model, cblob, trained):
    """f16x2 and back returns the f32 conv bits; loads and a conv learner's publish arrive in the chosen arithmetic; parameters without a
    plan and engines for more explores than the lane kernels address are refused, and a refused call changes nothing."""
    import synthesis_amd as sa
    from tests.oracle_lib import parity_mcts_config

    my, op = random_positions(oracle, 32, seed=33)
    eng = sa.Engine(concurrent_games=256, max_explores=200, device=0, policy_cache_log2=10)
    try:
        eng.load_weights_conv(cblob)
        a = eng.mcts_search(sa.parity_mcts_config(), my, op, 200)
        eng.set_network_arithmetic("f16x2")
        b = eng.mcts_search(sa.parity_mcts_config(), my, op, 200)
        eng.set_network_arithmetic("f32")
        c = eng.mcts_search(sa.parity_mcts_config(), my, op, 200)
        assert_search_equal(a, oracle.c4_mcts_search(parity_mcts_config(), cblob, my, op, 200, nn_mode=oracle.ACC_FMA, net="conv"), "f32")
        assert_search_equal(b, model.mcts_search(parity_mcts_config(), cblob, my, op, 200), "f16x2")
        assert_search_equal(c, a, "f32 again")
        l, v = eng.policy_eval(my, op)
        rl, rv = oracle.c4conv_eval(cblob, my, op, mode=oracle.ACC_FMA)
        assert _bits_equal(l, rl) and _bits_equal(v, rv)
        # weights loaded after the choice are evaluated in it
        eng.set_network_arithmetic("f16x2")
        eng.load_weights_conv(trained)
        l, v = eng.policy_eval(my, op)
        rl, rv = model.eval(trained, my, op)
        assert _bits_equal(l, rl) and _bits_equal(v, rv)
        # a load without a plan is refused and changes nothing (policy_eval, a context and a search still see `trained` in f16x2)
        bad = cblob.copy(); bad[3] = np.inf
        with pytest.raises(sa.SynthesisAmdError):
            eng.load_weights_conv(bad)
        assert eng.network_arithmetic()[0] == "f16x2"
        l, v = eng.policy_eval(my, op)
        assert _bits_equal(l, rl) and _bits_equal(v, rv)
        ctx = eng.eval_context()
        cl, cv = ctx.eval(my, op)
        ctx.close()
        assert _bits_equal(cl, rl) and _bits_equal(cv, rv)
        got = eng.mcts_search(sa.parity_mcts_config(), my[:8], op[:8], 60)
        assert_search_equal(got, model.mcts_search(parity_mcts_config(), trained, my[:8], op[:8], 60), "after a refused load")
        # from the f32 side: the switch itself is refused for parameters without a plan (a conv bias of 1e30 puts the head's scale
        # outside the window, though f32 evaluates the network finitely) and the engine stays in f32, with the f32 bits
        eng.set_network_arithmetic("f32")
        wide = cblob.copy(); wide[288] = np.float32(1e30)
        assert model.plan(wide) is None
        eng.load_weights_conv(wide)
        with pytest.raises(sa.SynthesisAmdError):
            eng.set_network_arithmetic("f16x2")
        assert eng.network_arithmetic()[0] == "f32"
        l, v = eng.policy_eval(my, op)
        rl, rv = oracle.c4conv_eval(wide, my, op, mode=oracle.ACC_FMA)
        assert np.isfinite(l).all() and _bits_equal(l, rl) and _bits_equal(v, rv)
        # a conv learner's publish keeps the engine's arithmetic
        eng.load_weights_conv(cblob)
        eng.set_network_arithmetic("f16x2")
        eng.trainer_init_conv(cblob)
        rs = np.random.RandomState(4)
        tpi = rs.dirichlet(np.ones(9), 32).astype(np.float32); tv = rs.dirichlet(np.ones(3), 32).astype(np.float32)
        for _ in range(5):
            eng.train_step(my, op, tpi, tv, 1e-2)
        eng.trainer_publish_weights()
        assert eng.network_arithmetic()[0] == "f16x2"
        now = eng.trainer_state()["weights"]
        assert np.abs(now - cblob).max() > 1e-3
        l, v = eng.policy_eval(my, op)
        rl, rv = model.eval(now, my, op)
        assert _bits_equal(l, rl) and _bits_equal(v, rv)
        got = eng.mcts_search(sa.parity_mcts_config(), my[:8], op[:8], 100)
        assert_search_equal(got, model.mcts_search(parity_mcts_config(), now, my[:8], op[:8], 100), "published")
    finally:
        eng.close()
    # an 8,000-explore engine (past the lane kernels' node addressing) takes neither the conv network nor the f16x2 arithmetic, in
    # either order, and stays as it was
    big = sa.Engine(concurrent_games=16, max_explores=8000, device=0)
    try:
        with pytest.raises(sa.SynthesisAmdError) as e:
            big.set_network_arithmetic("f16x2")
        assert e.value.code == -5 and big.network_arithmetic() == ("f32", None)
        with pytest.raises(sa.SynthesisAmdError) as e:
            big.load_weights_conv(cblob)
        assert e.value.code == -5 and big.network_arithmetic() == ("f32", None)
        with pytest.raises(sa.SynthesisAmdError):
            big.policy_eval(my, op)   # (still no network)
    finally:
        big.close()


def test_conv_f16x2_data_parallel_learner_publishes_into_the_chosen_arithmetic(oracle, model, cblob):
    """DataParallelLearner(network_arithmetic="f16x2"): the engine's self-play evaluates each published conv network in f16x2."""
    import synthesis_amd as sa
    from synthesis_amd.learner import DataParallelLearner

    my, op = random_positions(oracle, 32, seed=41)
    rs = np.random.RandomState(5)
    tpi = rs.dirichlet(np.ones(9), 32).astype(np.float32); tv = rs.dirichlet(np.ones(3), 32).astype(np.float32)
    eng = sa.Engine(concurrent_games=256, max_explores=64, device=0)
    try:
        eng.load_weights_conv(cblob)
        learner = DataParallelLearner(eng, cblob, net="conv", network_arithmetic="f16x2")
        name, plan = eng.network_arithmetic()
        assert name == "f16x2" and plan["network"] == "Connect4ConvNet"
        for _ in range(3):
            learner.step(my, op, tpi, tv, 1e-2)
        learner.publish()
        now = learner.state()["weights"]
        assert np.abs(now - cblob).max() > 1e-4 and eng.network_arithmetic()[0] == "f16x2"
        l, v = eng.policy_eval(my, op)
        rl, rv = model.eval(now, my, op)
        assert _bits_equal(l, rl) and _bits_equal(v, rv)
    finally:
        eng.close()
