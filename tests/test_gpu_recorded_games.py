"""GPU tests of recorded device games (Engine.games_run_recorded = syn_games_run_recorded, record_kernels.cuh), of
Engine.replay_select_positions and of LearningLoop(exploring_starts=...). Every comparison is bit for bit: against Engine.selfplay from
the empty board, against the plain-Python model of the definition (tests/recorded_games_model.py, the oracle's search per ply) from
given starts, against the one-game call, against reanalyse_flags, and between the two replay modes of the loop."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import recorded_games_model as model

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = -1, -5
EXPLORES = 12
ROW_KEYS = ("states", "pis", "vs", "actions", "root_nodes")


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.fixture(scope="module")
def blobs(golden_dir):
    """(the trained Connect4Net checkpoint, the random-init one, the trained Connect4ConvNet checkpoint)"""
    return tuple(np.load(os.path.join(golden_dir, f)).astype(np.float32).ravel()
                 for f in ("c4net_trained_f32.npy", "c4net_blob_f32.npy", "c4conv_trained_f32.npy"))


@pytest.fixture(scope="module")
def engine(blobs):
    import synthesis_amd as sa

    eng = sa.Engine(concurrent_games=64, max_explores=32)
    eng.load_weights(blobs[0])
    yield eng
    eng.close()


def player(blob, explores=EXPLORES, c=3.0, action=1, arithmetic=None):
    import synthesis_amd as sa
    from synthesis_amd import match

    return match.Player("p", explores, sa.MCTSConfig(c=c), action=sa.ActionSelection(action), weights=blob, arithmetic=arithmetic)


def side_of(oracle, p):
    """the model's description of a match.Player (f32 sides and engines only, or an explicit f16x2 side)"""
    from tests.oracle_lib import parity_mcts_config

    return model.Side(p.weights, parity_mcts_config(c=p.mcts_cfg.c), p.explores, action=int(p.action),
                      nn_mode=oracle.ACC_F16X2 if p.arithmetic == "f16x2" else oracle.ACC_FMA)


def rules_of(rec):
    return model.record_rules(rec.random_actions_until, rec.sample_actions_until, int(rec.stop_games_when_solved), int(rec.value_target),
                              rec.value_target_p, rec.value_target_from, rec.value_target_to, rec.record_mask)


# ---- 1
def assert_equals_selfplay(eng, blob, cfg, n=300, base_seed=11, first_game=5):
    """one player on both sides, the empty board, seeds = base_seed + first_game + g: all seven outputs of Engine.selfplay. (A padded
    slot beyond a game's plies is compared nowhere: self-play leaves there what an earlier launch wrote.)"""
    import synthesis_amd as sa

    sp = eng.selfplay(cfg, base_seed=base_seed, n_games=n, first_game=first_game)
    zeros = np.zeros(n, np.int32)
    seeds = (base_seed + first_game + np.arange(n)).astype(np.uint64)
    me = player(blob, cfg.num_explores, cfg.mcts_cfg.c, int(cfg.action))
    got = eng.games_run_recorded([me], zeros, zeros, np.zeros(n, np.uint64), np.zeros(n, np.uint64), seeds,
                                 record=sa.RecordConfig.from_rollout(cfg, 1))
    assert same(got["rows"], sp["plies"]) and same(got["plies"], sp["plies"]) and same(got["final_kind"], sp["final_kind"])
    # (four in a row needs seven plies; a solved game may stop before the board decides it)
    assert sp["plies"].min() >= (1 if cfg.stop_games_when_solved else 7) and len(set(sp["plies"].tolist())) > 5
    mask = np.arange(63)[None, :] < sp["plies"][:, None]
    for k in ROW_KEYS:
        a, b = got[k][mask], sp["states_bb" if k == "states" else k][mask]
        assert same(a, b), f"{k}: {int((a != b).reshape(a.shape[0], -1).any(axis=1).sum())} of {a.shape[0]} rows differ"
        assert not got[k][~mask].any(), f"{k}: a slot no row reaches is not zero"
    # the game loop's own outputs: the moves are the rows' actions, a stream position per draw
    assert same(got["moves"][mask], sp["actions"][mask]) and (got["moves"][~mask] == 255).all()
    drawn = np.minimum(sp["plies"], max(cfg.random_actions_until, cfg.sample_actions_until))
    assert (got["rng_words"] <= drawn).all() and (got["rng_words"] >= 1).all()
    return got


@pytest.mark.parametrize("arithmetic", ["f32", "f16x2"])
def test_equals_selfplay_connect4net(blobs, arithmetic):
    import synthesis_amd as sa

    with sa.Engine(concurrent_games=64, max_explores=32) as eng:
        eng.load_weights(blobs[0])
        eng.set_network_arithmetic(arithmetic)
        got = assert_equals_selfplay(eng, blobs[0], sa.parity_rollout_config(EXPLORES))
        assert eng.network_arithmetic()[0] == arithmetic
        ms, launches = eng.last_timing()
        assert launches == 4 * int(got["plies"].max()) + 1 and ms > 0.0   # one group: search, advance, count, scatter per ply; the finish


def test_equals_selfplay_convnet(blobs):
    import synthesis_amd as sa

    with sa.Engine(concurrent_games=64, max_explores=32) as eng:
        eng.load_weights_conv(blobs[2])
        assert_equals_selfplay(eng, blobs[2], sa.parity_rollout_config(EXPLORES))


@pytest.mark.parametrize("variant", ["z", "qz_average", "q_to_z", "stop_when_solved", "action_q"])
def test_equals_selfplay_rollout_variants(engine, blobs, variant):
    import synthesis_amd as sa

    kw = dict(z=dict(value_target=sa.ValueTarget.Z), qz_average=dict(value_target=sa.ValueTarget.QZaverage, value_target_p=0.3),
              q_to_z=dict(value_target=sa.ValueTarget.QtoZ, value_target_from=0.1, value_target_to=0.9),
              stop_when_solved=dict(stop_games_when_solved=True), action_q=dict(action=sa.ActionSelection.Q, sample_actions_until=4))[variant]
    engine.load_weights(blobs[0])
    assert_equals_selfplay(engine, blobs[0], sa.parity_rollout_config(EXPLORES, **kw))


# ---- 2
def grid_position(owner, empty):
    """(my, op) of a board given as owner[row][col] in {0, 1} with the cells of `empty` taken out; 0 = the side to move"""
    bb = [0, 0]
    for r in range(7):
        for c in range(9):
            if (r, c) not in empty:
                bb[owner[r][c]] |= 1 << (r + 7 * c)
    return bb


def special_starts():
    """One move from a full board, filled as a draw; one move from a full board, filled by a winning move; an immediate win; two
    forced moves from a full board that the SECOND mover fills as a draw (its reward is +0.0, not -0.0).
    The full boards come from the pattern owner = (col // 2 + row) % 2, which has no four in a row in any direction."""
    from tests.frozen_py import Game, won

    draw = [[(c // 2 + r) % 2 for c in range(9)] for r in range(7)]
    a = grid_position(draw, {(6, 8)})
    win = [row[:] for row in draw]
    win[6][4], win[6][6], win[6][7] = 1, 0, 0      # row 6: the mover holds columns 5, 6, 7 and fills column 8
    b = grid_position(win, {(6, 8)})
    c = [sum(1 << (r + 7 * 0) for r in range(3)), sum(1 << (r + 7 * 1) for r in range(3))]   # three in column 0, the mover's
    d = grid_position([[1 - x for x in row] for row in draw], {(5, 8), (6, 8)})   # column 8 alone is free: both moves are forced
    for my, op in (a, b, c, d):
        assert not won(my) and not won(op) and not my & op
    g, over = Game(*d).step(8)
    assert Game(*d).actions() == [8] and not over and g.actions() == [8] and g.step(8)[1] and not won(g.step(8)[0].op)
    for (my, op), wins in ((a, False), (b, True)):
        g = Game(my, op)
        assert g.actions() == [8]
        after, over = g.step(8)
        assert over and won(after.op) == wins
    assert won(Game(*c).step(0)[0].op)
    return np.array([a[0], b[0], c[0], d[0]], np.uint64), np.array([a[1], b[1], c[1], d[1]], np.uint64)


@pytest.fixture(scope="module")
def openings24():
    from synthesis_amd import arena

    return arena.random_openings(24, 8, seed=5)


@pytest.mark.parametrize("case", ["mask_both", "mask_first", "mixed_arithmetic", "q_to_z_stop"])
def test_equals_the_model_from_given_starts(engine, blobs, oracle, openings24, case):
    """24 games from 8-ply openings between two different checkpoints, the trained one first in the even games"""
    import synthesis_amd as sa

    engine.load_weights(blobs[1])          # (the engine's own network is neither side's business)
    engine.set_network_arithmetic("f32")
    mixed = case == "mixed_arithmetic"
    players = [player(blobs[0], 12, 3.0, arithmetic="f16x2" if mixed else None), player(blobs[1], 10, 1.5, arithmetic="f32" if mixed else None)]
    rec = sa.RecordConfig(random_actions_until=1, sample_actions_until=30, record_mask=1 if case == "mask_first" else 3)
    if case == "q_to_z_stop":
        rec = sa.RecordConfig(1, 30, True, sa.ValueTarget.QtoZ, 0.0, 0.2, 0.8, 3)
    my, op = openings24
    first = (np.arange(24) % 2).astype(np.int32)
    second = 1 - first
    seeds = (1000 + 7 * np.arange(24)).astype(np.uint64)
    got = engine.games_run_recorded(players, first, second, my, op, seeds, record=rec)
    want = model.run_games(oracle, [side_of(oracle, p) for p in players], first, second, my, op, seeds, rules_of(rec))
    model.assert_records_equal(got, want, case)
    assert (got["rows"] < got["plies"]).all() if case == "mask_first" else same(got["rows"], got["plies"])
    assert got["plies"].max() > 10 and len(set(got["rewards"].tolist())) >= 2 and (got["rng_words"] > 1).any()


@pytest.mark.parametrize("sampling", [False, True])
def test_equals_the_model_at_the_end_of_the_board(engine, blobs, oracle, sampling):
    """one-ply games: the board filled as a draw (the draw column of z), filled by a winning move, an immediate win (t = 1 / 1); and
    a board the second mover fills as a draw"""
    import synthesis_amd as sa

    engine.load_weights(blobs[0])
    engine.set_network_arithmetic("f32")
    my, op = special_starts()
    players = [player(blobs[0], 12, 3.0), player(blobs[1], 10, 1.5)]
    first, second = np.array([0, 1, 0, 1], np.int32), np.array([1, 0, 1, 0], np.int32)
    for vt in (sa.ValueTarget.Z, sa.ValueTarget.QtoZ):
        rec = sa.RecordConfig(1 if sampling else 0, 30 if sampling else 0, False, vt, 0.0, 0.25, 0.75, 3)
        seeds = np.array([5, 6, 7, 8], np.uint64) if sampling else None
        got = engine.games_run_recorded(players, first, second, my, op, seeds, record=rec)
        want = model.run_games(oracle, [side_of(oracle, p) for p in players], first, second, my, op, seeds, rules_of(rec))
        model.assert_records_equal(got, want, f"sampling={sampling} {vt!r}")
        assert got["plies"][:2].tolist() == [1, 1] and got["rewards"][:2].tolist() == [0.0, 1.0] and got["final_kind"][:2].tolist() == [1, 0]
        if vt == sa.ValueTarget.Z:
            assert got["vs"][0, 0].tolist() == [0.0, 1.0, 0.0] and got["vs"][1, 0].tolist() == [0.0, 0.0, 1.0]
        assert got["plies"][3] == 2 and got["rows"][3] == 2 and got["final_kind"][3] == 1 and got["rewards"][3:].tobytes() == np.zeros(1, np.float32).tobytes()
        if not sampling:
            assert got["plies"][2] == 1 and got["rewards"][2] == 1.0 and not got["rng_words"].any()


# ---- 3
def test_nine_pairings_every_game_is_its_one_game_call(engine, blobs, openings24):
    """three players, all nine ordered pairings from five openings in one call: every game's whole record — rows and stream position
    included — is what the call for that game alone returns"""
    import synthesis_amd as sa
    from tests import f16x2_checkpoints as ck

    blob, trained, _, _ = ck.load_fixtures()
    third = np.asarray(ck.mlp_family(blob, trained)["trained_outlier_4096"], np.float32).ravel()
    engine.load_weights(blobs[0])
    engine.set_network_arithmetic("f32")
    players = [player(blobs[0], 12, 3.0), player(blobs[1], 10, 1.5, arithmetic="f16x2"), player(third, 14, 2.0, action=0)]
    first = np.tile(np.repeat(np.arange(3), 3), 5).astype(np.int32)
    second = np.tile(np.tile(np.arange(3), 3), 5).astype(np.int32)
    opening = np.repeat(np.arange(5), 9)
    my, op = openings24[0][opening], openings24[1][opening]
    seeds = (77 + np.arange(45)).astype(np.uint64)
    rec = sa.RecordConfig(random_actions_until=1, sample_actions_until=30, value_target=sa.ValueTarget.QZaverage, value_target_p=0.4, record_mask=0b101)
    got = engine.games_run_recorded(players, first, second, my, op, seeds, record=rec)
    assert (got["rows"][(first == 1) & (second == 1)] == 0).all() and same(got["rows"][(first != 1) & (second != 1)], got["plies"][(first != 1) & (second != 1)])
    for g in range(45):
        one = engine.games_run_recorded(players, first[g:g + 1], second[g:g + 1], my[g:g + 1], op[g:g + 1], seeds[g:g + 1], record=rec)
        model.assert_records_equal({k: got[k][g:g + 1] for k in model.RECORD_KEYS}, one, f"game {g} ({first[g]} against {second[g]})")
    moves = {(int(first[g]), int(second[g])): got["moves"][g].tobytes() for g in range(9)}
    assert len(set(moves.values())) >= 6     # the pairings of one opening play different games: a game searched as another player would show


# ---- 4
def test_append_compacts_exactly_the_rows(engine, blobs, openings24):
    import synthesis_amd as sa

    engine.load_weights(blobs[0])
    engine.set_network_arithmetic("f32")
    players = [player(blobs[0], 12, 3.0), player(blobs[1], 10, 1.5)]
    first = np.array([0, 1, 1, 0, 1, 0], np.int32)
    second = np.array([1, 0, 1, 0, 1, 1], np.int32)      # games 2 and 4: player 1 against itself, which the mask does not record
    my, op = openings24[0][:6], openings24[1][:6]
    seeds = np.arange(6).astype(np.uint64) + np.uint64(40)
    got = engine.games_run_recorded(players, first, second, my, op, seeds, record=sa.RecordConfig(1, 30, record_mask=1))
    assert got["rows"][[2, 4]].tolist() == [0, 0] and (got["rows"][[0, 1, 3, 5]] > 0).all()
    engine.replay_reserve(6 * 63)
    engine.replay_clear()
    n = engine.replay_append_selfplay(first_gid=1000)
    R = engine.replay_read()
    mask = np.arange(63)[None, :] < got["rows"][:, None]
    assert n == int(got["rows"].sum()) == R["my"].size
    assert same(R["my"], got["states"][..., 0][mask]) and same(R["op"], got["states"][..., 1][mask])
    assert same(R["pi"], got["pis"][mask]) and same(R["v"], got["vs"][mask])
    assert same(R["gid"], (1000 + np.arange(6, dtype=np.int64))[:, None].repeat(63, 1)[mask])
    # a refused call leaves nothing to compact
    with pytest.raises(sa.SynthesisAmdError) as e:
        engine.games_run_recorded(players, first, second, my, op, seeds, record=sa.RecordConfig(1, 30, record_mask=4))
    assert e.value.code == INVALID
    with pytest.raises(sa.SynthesisAmdError) as e:
        engine.replay_append_selfplay(first_gid=2000)
    assert e.value.code == INVALID and engine.replay_size() == n
    engine.replay_clear()


# ---- 5, 6
@pytest.fixture(scope="module")
def observed(engine, blobs):
    """the engine with a trainer that has stepped, a replay buffer, both data sets: observe() = everything a recorded call must leave"""
    import synthesis_amd as sa

    engine.set_network_arithmetic("f32")
    engine.load_weights(blobs[1])
    engine.selfplay(sa.parity_rollout_config(EXPLORES), base_seed=3, n_games=40, outputs=False)
    engine.replay_reserve(40 * 63)
    engine.replay_clear()
    engine.replay_append_selfplay(first_gid=100)
    R = engine.replay_read()
    engine.trainer_init(blobs[1])
    engine.train_set_data(R["my"][:200], R["op"][:200], R["pi"][:200], R["v"][:200])
    engine.train_epoch(np.arange(192), 32, 1e-3)
    engine.dataset_set(R["my"][200:300], R["op"][200:300], R["pi"][200:300], R["v"][200:300])
    engine.load_weights(blobs[0])

    def observe():
        logits, value = engine.policy_eval(R["my"][:64], R["op"][:64])
        return ([engine.state_digest(w) for w in ("trainer", "network", "replay", "train_data", "eval_data")], engine.network_arithmetic()[0],
                logits.tobytes(), value.tobytes())

    return observe


def test_the_engine_is_only_observed(engine, blobs, openings24, observed):
    import synthesis_amd as sa

    before = observed()
    players = [player(blobs[1], 12, 3.0, arithmetic="f16x2"), player(blobs[0], 10, 1.5)]
    first = (np.arange(24) % 2).astype(np.int32)
    got = engine.games_run_recorded(players, first, 1 - first, *openings24, np.arange(24).astype(np.uint64), record=sa.RecordConfig(1, 30, record_mask=3))
    assert got["rows"].sum() > 200
    assert observed() == before


def test_refusals_before_anything_changes(engine, blobs, openings24, observed):
    import synthesis_amd as sa
    from synthesis_amd import match

    before = observed()
    my, op = openings24[0][:4], openings24[1][:4]
    zeros, seeds = np.zeros(4, np.int32), np.arange(4).astype(np.uint64)
    ok = player(blobs[0])
    sampling = sa.RecordConfig(1, 30)
    finished_my = my.copy()
    finished_my[2] = np.uint64(0b1111)      # four in column 0
    finished_op = op.copy()
    finished_op[2] = np.uint64(0b111 << 7)
    noisy = match.Player("n", EXPLORES, sa.MCTSConfig(root_policy_noise=sa.PolicyNoise.Dirichlet, noise_alpha=0.3, noise_weight=0.25), weights=blobs[0])
    normal = match.Player("f", EXPLORES, sa.reference_selfplay_mcts_config(), weights=blobs[0])
    cases = [("a baseline side", dict(players=[ok, match.vanilla_player(64)], second=np.ones(4, np.int32)), UNSUPPORTED),
             ("Dirichlet noise", dict(players=[noisy]), UNSUPPORTED), ("FPU_NORMAL", dict(players=[normal]), UNSUPPORTED),
             ("a mask bit at n_players", dict(record=sa.RecordConfig(1, 30, record_mask=2)), INVALID),
             ("a mask bit above n_players", dict(record=sa.RecordConfig(1, 30, record_mask=1 | 1 << 40)), INVALID),
             ("seeds=None with sampling on", dict(seeds=None), INVALID),
             ("seeds=None with random moves on", dict(seeds=None, record=sa.RecordConfig(1, 0)), INVALID),
             ("a finished start position", dict(start_my=finished_my, start_op=finished_op), INVALID),
             ("a player index outside the call", dict(second=np.array([0, 0, 1, 0], np.int32)), INVALID)]
    for what, kw, code in cases:
        args = dict(players=[ok], first=zeros, second=zeros, start_my=my, start_op=op, seeds=seeds, record=sampling)
        args.update(kw)
        with pytest.raises(sa.SynthesisAmdError) as e:
            engine.games_run_recorded(**args)
        assert e.value.code == code, (what, e.value)
        assert observed() == before, what
        with pytest.raises(sa.SynthesisAmdError):
            engine.replay_append_selfplay(first_gid=0)
    # an unknown value target and negative horizons never leave Python as a RecordConfig: the C entry point itself
    from synthesis_amd.config import CRecordConfig
    from synthesis_amd.engine import CMatchSide, CRecordOutputs

    side, keep = engine.match_side(ok)
    arr = (CMatchSide * 1)(side)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    rewards, plies = np.zeros(4, np.float32), np.zeros(4, np.int32)
    for bad in (CRecordConfig(1, 30, 0, 4, 0, 0, 0, 0, 1), CRecordConfig(-1, 30, 0, 1, 0, 0, 0, 0, 1), CRecordConfig(1, -1, 0, 1, 0, 0, 0, 0, 1)):
        rc = engine._lib.syn_games_run_recorded(engine._h, arr, 1, p(zeros), p(zeros), p(my), p(op), p(seeds), 4, C.byref(bad), p(rewards), p(plies),
                                                None, None, None, C.byref(CRecordOutputs()))
        assert rc == INVALID
    assert engine._lib.syn_games_run_recorded(engine._h, arr, 1, p(zeros), p(zeros), p(my), p(op), p(seeds), 4, None, p(rewards), p(plies),
                                              None, None, None, None) == INVALID
    assert observed() == before and not plies.any()
    # and after the refusals the call still plays
    got = engine.games_run_recorded([ok], zeros, zeros, my, op, seeds, record=sampling, outputs=False)
    assert (got["rows"] == got["plies"]).all() and got["plies"].min() > 0 and "states" not in got
    assert observed() == before


# ---- 7
def test_replay_select_positions_is_reanalyse_flags(engine, observed):
    import synthesis_amd as sa
    from synthesis_amd.learner import exploring_threshold, reanalyse_flags

    before = observed()
    R = engine.replay_read()
    n = R["my"].size
    assert n > 600
    for key, threshold, before_gid in ((3, 1 << 31, None), (4, exploring_threshold(16, n), 120), (5, 1 << 32, None), (6, 1 << 32, 100), (7, 0, None)):
        sel = reanalyse_flags(key, threshold, before_gid, R["gid"], R["my"], R["op"])
        got = engine.replay_select_positions(key, threshold=threshold, before_gid=before_gid)
        assert same(got["my"], R["my"][sel]) and same(got["op"], R["op"][sel]) and got["skipped"] == 0, (key, threshold, before_gid)
    assert 0.4 * n < engine.replay_select_positions(3, fraction=0.5)["my"].size < 0.6 * n
    assert engine.replay_select_positions(5, threshold=1 << 32)["my"].size == n and engine.replay_select_positions(6, threshold=1 << 32, before_gid=100)["my"].size == 0
    # capacity too small: an error that writes nothing, and says how many there are
    my, op = np.full(10, 77, np.uint64), np.full(10, 78, np.uint64)
    count, skipped = C.c_size_t(), C.c_size_t()
    rc = engine._lib.syn_replay_select_positions(engine._h, 5, 1 << 32, (1 << 63) - 1, my.ctypes.data_as(C.c_void_p), op.ctypes.data_as(C.c_void_p), 10,
                                                 C.byref(count), C.byref(skipped))
    assert rc == -6 and count.value == n and (my == 77).all() and (op == 78).all()
    with pytest.raises(sa.SynthesisAmdError) as e:
        engine.replay_select_positions(5, threshold=(1 << 32) + 1)
    assert e.value.code == INVALID
    assert observed() == before and same(engine.replay_read()["pi"], R["pi"])


# ---- 8
LOOP_SHAPE = (64, 150, 1, 32)     # games per iteration, games to keep, epochs, batch


def run_loop(net, blob, iterations, restore=None, save=None, **kw):
    import synthesis_amd as sa
    from synthesis_amd.learner import LearningLoop

    with sa.Engine(concurrent_games=64, max_explores=32) as eng:
        loop = LearningLoop(eng, net, blob, seed=7, digests=True, **kw)
        if restore:
            loop.restore_state(restore)
        cfg = sa.parity_rollout_config(EXPLORES)
        recs = [loop.iteration(cfg, *LOOP_SHAPE) for _ in range(iterations)]
        if save:
            loop.save_state(save)
        R = eng.replay_read() if loop.replay == "device" else loop.R
        return dict(recs=[{k: v for k, v in r.items() if k != "seconds"} for r in recs], seconds=[set(r["seconds"]) for r in recs],
                    weights=loop.weights.copy(), buffer={k: R[k].copy() for k in ("my", "op", "gid", "pi", "v")})


def assert_same_run(a, b, what):
    assert same(a["weights"], b["weights"]), f"{what}: weights"
    for k in a["buffer"]:
        assert same(a["buffer"][k], b["buffer"][k]), f"{what}: buffer {k}"
    assert a["recs"] == b["recs"], f"{what}: records"


_runs = {}


def exploring_run(net, blobs, replay):
    """three iterations with exploring_starts=0.25; one run per network and replay mode, shared by the cases below, never modified"""
    if (net, replay) not in _runs:
        _runs[(net, replay)] = run_loop(net, blobs[0] if net == "mlp" else blobs[2], 3, replay=replay, exploring_starts=0.25)
    return _runs[(net, replay)]


@pytest.mark.parametrize("net", ["mlp", "conv"])
def test_learning_loop_exploring_starts_host_equals_device(net, blobs):
    host, device = exploring_run(net, blobs, "host"), exploring_run(net, blobs, "device")
    assert_same_run(host, device, "replay host against device")
    assert host["seconds"] == device["seconds"] and all("exploring" in s for s in host["seconds"])
    games = [r["exploring_games"] for r in device["recs"]]
    rows = [r["exploring_rows"] for r in device["recs"]]
    print("exploring games per iteration", games, "rows", rows, "buffer rows", [r["steps_in_buffer"] for r in device["recs"]])
    # n_t = 16 of 64 games; the hash draws about 16 of the buffer's rows (a binomial count: 4 .. 40 is beyond four deviations)
    assert games[0] == 0 and rows[0] == 0 and 4 <= games[1] <= 40 and 4 <= games[2] <= 40 and all(r >= g for r, g in zip(rows, games))
    gid = device["buffer"]["gid"]
    assert (gid[(gid >= 64) & (gid < 128)] < 64 + 48 + games[1]).all() and ((gid >= 64 + 48) & (gid < 128)).any()
    assert len(set(r["digests"]["replay"] for r in device["recs"])) == 3


@pytest.mark.parametrize("net", ["mlp", "conv"])
def test_learning_loop_exploring_starts_zero_is_the_loop_without_it(net, blobs):
    blob = blobs[0] if net == "mlp" else blobs[2]
    off, plain = run_loop(net, blob, 3, replay="device", exploring_starts=0.0), run_loop(net, blob, 3, replay="device")
    assert_same_run(off, plain, "exploring_starts=0.0 against no argument")
    assert off["seconds"] == plain["seconds"] and "exploring_games" not in off["recs"][1]
    assert not same(off["weights"], exploring_run(net, blobs, "device")["weights"])


@pytest.mark.parametrize("net", ["mlp", "conv"])
def test_learning_loop_exploring_starts_resumes(net, blobs, tmp_path):
    """2 + 1 iterations through save_state / restore_state (saved under replay="device", continued under "host") equal 3 iterations;
    a loop without exploring starts refuses the file and names the field"""
    import synthesis_amd as sa
    from synthesis_amd.learner import LearningLoop

    blob = blobs[0] if net == "mlp" else blobs[2]
    device = exploring_run(net, blobs, "device")
    path = str(tmp_path / "state.npz")
    run_loop(net, blob, 2, save=path, replay="device", exploring_starts=0.25)
    resumed = run_loop(net, blob, 1, restore=path, replay="host", exploring_starts=0.25)
    assert same(resumed["weights"], device["weights"]) and resumed["recs"] == device["recs"][2:]
    for k in device["buffer"]:
        assert same(resumed["buffer"][k], device["buffer"][k]), k
    with sa.Engine(concurrent_games=64, max_explores=32) as eng:
        with pytest.raises(ValueError, match="exploring_starts"):
            LearningLoop(eng, net, blob, seed=7, digests=True, replay="device").restore_state(path)
