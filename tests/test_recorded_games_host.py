"""Recorded games, the parts that need no GPU: the plain-Python model of the definition (tests/recorded_games_model.py) against the
plain-Python run_game it generalises (tests/selfplay_py.py), the record mask, RecordConfig and LearningLoop(exploring_starts=...)
validation, the optional field of the run's fingerprint, and the threshold arithmetic."""
import os

import numpy as np
import pytest

from tests import recorded_games_model as model


@pytest.fixture(scope="module")
def blob(golden_dir):
    return np.load(os.path.join(golden_dir, "c4net_blob_f32.npy")).astype(np.float32).ravel()


VARIANTS = [dict(), dict(value_target=0), dict(value_target=2, vt_p=0.3), dict(value_target=3, vt_from=0.1, vt_to=0.9),
            dict(stop_games_when_solved=1), dict(action=0, sample_actions_until=4)]


@pytest.mark.parametrize("variant", range(len(VARIANTS)))
def test_model_from_the_empty_board_is_run_game(oracle, blob, variant):
    """one blob on both sides, the empty board, a full mask: the model is tests/selfplay_py.run_game, for every ValueTarget, the stop
    rule and ActionSelection::Q — rows == plies, and every array of the game"""
    from tests import selfplay_py
    from tests.oracle_lib import parity_rollout_config

    cfg = parity_rollout_config(16, **VARIANTS[variant])
    side = model.Side(blob, cfg.mcts, 16, action=cfg.action, nn_mode=oracle.ACC_FMA)
    for seed in (300 + variant, 9000 + 17 * variant):
        want = selfplay_py.run_game(oracle, blob, cfg, seed, nn_mode=oracle.ACC_FMA)
        got = model.run_game(oracle, [side], 0, 0, 0, 0, seed, model.rules_of_rollout(cfg, 1))
        n = want["plies"]
        assert got["plies"] == got["rows"] == n and got["row_plies"] == list(range(n)), (variant, seed)
        assert got["actions"] == want["actions"] == got["moves"] and got["states"] == want["states"], (variant, seed)
        assert got["root_nodes"] == want["tree_sizes"] and got["final_kind"] == want["final_kind"], (variant, seed)
        assert np.array_equal(got["pis"].view(np.uint32), want["pis"].view(np.uint32)), (variant, seed)
        assert np.array_equal(got["vs"].view(np.uint32), want["vs"].view(np.uint32)), (variant, seed)


def test_mask_of_the_first_mover_drops_the_odd_plies_and_keeps_the_games_t_and_z(oracle, blob, golden_dir):
    """two players, record_mask = the first mover only: the game is the one both masks play, its rows are the even plies' rows of the
    full record — with t = (ply + 1) / ALL plies and z by parity from the game's last position"""
    from tests.oracle_lib import parity_mcts_config

    trained = np.load(os.path.join(golden_dir, "c4net_trained_f32.npy")).astype(np.float32).ravel()
    sides = [model.Side(trained, parity_mcts_config(), 12, nn_mode=oracle.ACC_FMA), model.Side(blob, parity_mcts_config(c=1.5), 10, nn_mode=oracle.ACC_FMA)]
    for vt in (dict(value_target=0), dict(value_target=3, vt_from=0.2, vt_to=0.8)):
        both = model.run_game(oracle, sides, 0, 1, 0, 0, 77, model.record_rules(1, 30, record_mask=3, **vt))
        only = model.run_game(oracle, sides, 0, 1, 0, 0, 77, model.record_rules(1, 30, record_mask=1, **vt))
        n = both["plies"]
        assert only["plies"] == n and only["moves"] == both["moves"] and only["rng_words"] == both["rng_words"] and n > 4
        assert both["rows"] == n and only["row_plies"] == list(range(0, n, 2)) and only["rows"] == (n + 1) // 2
        for k in ("pis", "vs"):
            assert np.array_equal(only[k].view(np.uint32), both[k][0::2].view(np.uint32)), k
        assert only["states"] == both["states"][0::2] and only["actions"] == both["actions"][0::2]
        if vt["value_target"] == 0:   # z: one-hot, alternating Win / Lose (or Draw throughout) back from the last position
            kinds = both["vs"].argmax(axis=1)
            last = 2 - both["final_kind"]
            assert all(kinds[k] == (last if (n - 1 - k) % 2 == 0 else 2 - last) for k in range(n))
    second = model.run_game(oracle, sides, 0, 1, 0, 0, 77, model.record_rules(1, 30, record_mask=2))
    assert second["row_plies"] == list(range(1, second["plies"], 2))
    nobody = model.run_game(oracle, sides, 0, 1, 0, 0, 77, model.record_rules(1, 30, record_mask=0))
    assert nobody["rows"] == 0 and nobody["plies"] == second["plies"]


def test_record_config_validation_and_from_rollout():
    import synthesis_amd as sa
    from synthesis_amd.config import CRecordConfig

    cfg = sa.parity_rollout_config(12, value_target=sa.ValueTarget.QtoZ, value_target_from=0.25, value_target_to=0.75, stop_games_when_solved=True)
    rec = sa.RecordConfig.from_rollout(cfg, record_mask=5)
    assert (rec.random_actions_until, rec.sample_actions_until, rec.stop_games_when_solved, rec.record_mask) == (1, 30, True, 5)
    c = rec.to_c()
    assert isinstance(c, CRecordConfig) and (c.value_target, c.value_target_from, c.value_target_to, c.record_mask) == (3, 0.25, 0.75, 5)
    assert (c.random_actions_until, c.sample_actions_until, c.stop_games_when_solved, c.reserved) == (1, 30, 1, 0)
    assert sa.RecordConfig(record_mask=(1 << 64) - 1).to_c().record_mask == (1 << 64) - 1
    for bad in (dict(random_actions_until=-1), dict(sample_actions_until=-3), dict(sample_actions_until=1.5), dict(random_actions_until=True),
                dict(record_mask=-1), dict(record_mask=1 << 64), dict(value_target=4), dict(value_target=-1)):
        with pytest.raises(ValueError):
            sa.RecordConfig(**bad)


def test_learning_loop_exploring_starts_validation():
    from synthesis_amd.learner import LearningLoop

    for bad in (-0.1, 1.0, 1.5, True, "0.25", None, float("nan")):
        with pytest.raises(ValueError, match="exploring_starts"):
            LearningLoop(None, "mlp", np.zeros(1, np.float32), exploring_starts=bad)


def test_exploring_threshold_arithmetic_and_key():
    from synthesis_amd.learner import _exploring_key, _reanalyse_key, exploring_threshold

    assert exploring_threshold(16, 1000) == (16 << 32) // 1000 == 68719476
    assert exploring_threshold(16, 16) == (1 << 32) - 1 == exploring_threshold(17, 16) == exploring_threshold(10**9, 1)   # capped
    assert exploring_threshold(0, 1000) == 0 and exploring_threshold(16, 0) == 0
    assert exploring_threshold(1, (1 << 31) - 1) == 2 and exploring_threshold(3, 7) == (3 << 32) // 7
    with pytest.raises(ValueError):
        exploring_threshold(-1, 10)
    keys = {_exploring_key(7, it) for it in range(50)} | {_reanalyse_key(7, it) for it in range(50)}
    assert len(keys) == 100 and all(0 <= k < 1 << 64 for k in keys)   # a tag of its own: no iteration shares a key with a reanalysis


def _fingerprint(**kw):
    fp = dict(net="mlp", seed=7, precision="f32", batch_mode="chained", sampler="numpy", flip=False, symmetry="none", holdout=0.0,
              reanalyse=0.0, reanalyse_explores=None, reanalyse_value_mix=0.0, lr_schedule=[[1, 1e-3]], hyper=dict(eps=1e-8),
              network_arithmetic="f32", world=1)
    fp.update(kw)
    return fp


def _state(fp):
    z1, z3 = np.zeros(4, np.float32), np.zeros(0, np.uint64)
    return dict(fingerprint=fp, iterations_done=2, games_played=128, weights=z1, m=z1, v=z1, step=5,
                replay=dict(my=z3, op=z3, gid=np.zeros(0, np.int64), pi=np.zeros((0, 9), np.float32), v=np.zeros((0, 3), np.float32)),
                digest_trainer=1, digest_replay=2)


def test_the_fingerprints_optional_field(tmp_path):
    """exploring_starts is in a state file only when non-zero; a missing field reads as 0.0; a loop with another value refuses the file
    and names the field — in both directions. FINGERPRINT_FIELDS and the format version are what they were."""
    from synthesis_amd import learner as L

    assert "exploring_starts" not in L.FINGERPRINT_FIELDS and L.FINGERPRINT_OPTIONAL == dict(exploring_starts=0.0) and L.STATE_FORMAT_VERSION == 1
    plain, zero, quarter = _fingerprint(), _fingerprint(exploring_starts=0.0), _fingerprint(exploring_starts=0.25)
    files = {}
    for name, fp in (("plain", plain), ("zero", zero), ("quarter", quarter)):
        files[name] = str(tmp_path / f"{name}.npz")
        L.write_state_file(files[name], _state(fp))
    got = {name: L.read_state_file(path)["fingerprint"] for name, path in files.items()}
    assert got["plain"] == got["zero"] and "exploring_starts" not in got["plain"]        # the file of a run that does not use it
    with np.load(files["plain"]) as a, np.load(files["zero"]) as b:
        assert a["fingerprint"].tobytes() == b["fingerprint"].tobytes()
    assert got["quarter"]["exploring_starts"] == 0.25 and {k: v for k, v in got["quarter"].items() if k != "exploring_starts"} == got["plain"]
    L.check_fingerprint(got["plain"], zero)
    L.check_fingerprint(got["quarter"], quarter)
    with pytest.raises(ValueError, match="exploring_starts=0.25.*exploring_starts=0.0"):
        L.check_fingerprint(got["quarter"], plain)          # saved with exploring starts, continued without
    with pytest.raises(ValueError, match="exploring_starts=0.0.*exploring_starts=0.25"):
        L.check_fingerprint(got["plain"], quarter)          # and the other way round
    with pytest.raises(ValueError, match="exploring_starts=0.25.*exploring_starts=0.5"):
        L.check_fingerprint(got["quarter"], _fingerprint(exploring_starts=0.5))
    with pytest.raises(ValueError, match="seed"):           # a required field still comes first
        L.check_fingerprint(got["quarter"], _fingerprint(seed=8))
