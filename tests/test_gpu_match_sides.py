"""GPU tests of the match sides (Engine.match_run_sides = syn_match_run_sides, match_kernels.cuh): a side is a network in an arithmetic
of its own, or the evaluator's rollout baseline with one generator per game. Bar: moves, ply counts, rewards, final positions and stream
positions equal, game for game, to games built on the CPU from the oracle (ply by ply from oracle.c4_mcts_search / c4_frozen_search
with the mover's parameters and the mover's nn_mode, and the oracle's own match loops c4_mcts_vs_mcts / c4_eval_against_rollout), and to
the host path (match.play_match, arena.host_match) on the same engine."""
import ctypes as C
import os
from dataclasses import replace

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KEYS = ("moves", "plies", "rewards", "final_bb")
A_EXPLORES, A_C = 32, 3.0      # the two sides differ in explores and in c, so a side that searched with the other's settings shows
B_EXPLORES, B_C = 20, 1.5
INVALID, UNSUPPORTED, CAPACITY = -1, -5, -6
# Cross arithmetic, held to the oracle: the checkpoints and openings were chosen on the CPU, with the oracle alone, so that the expected
# games differ from the games of one arithmetic on both sides (cross_guard). CROSS_A / CROSS_B name members of tests/f16x2_checkpoints.py
CROSS_A, CROSS_B, CROSS_OPENINGS = "trained_outlier_4096", "trained_outlier_4096", 12


def net_players(**kw):
    import synthesis_amd as sa
    from synthesis_amd import match

    return (match.Player("A", A_EXPLORES, sa.MCTSConfig(c=A_C), **kw), match.Player("B", B_EXPLORES, sa.MCTSConfig(c=B_C), **kw))


def rollout_cfgs():
    import synthesis_amd as sa
    from tests.oracle_lib import parity_mcts_config

    return (sa.MCTSConfig(exploration=sa.Exploration.Uct, c=2.0, auto_extend=False, fpu=sa.Fpu.Const, fpu_value=float("inf")),
            parity_mcts_config(exploration=0, c=2.0, auto_extend=0, fpu_value=float("inf")))


def net_side(blob, c, explores, nn_mode, net="mlp"):
    from tests.oracle_lib import parity_mcts_config

    return dict(kind="net", blob=blob, cfg=parity_mcts_config(c=c), explores=explores, nn_mode=nn_mode, net=net)


def baseline_side(explores, action):
    return dict(kind="baseline", cfg=rollout_cfgs()[1], explores=explores, action=action)


def oracle_match(oracle, sides, start_my, start_op, seeds=None):
    """The expected games: ply k of every live game is one oracle search with side k % 2's description — c4_mcts_search with the side's
    blob, configuration, explores and nn_mode, or c4_frozen_search on the game's own generator (seeds[g], from the word the game's last
    baseline ply left) — the move is its best_action, the rules are match.step's (numpy). Engine.match_run_sides' dict."""
    from synthesis_amd import match

    my = np.array(start_my, np.uint64).ravel(); op = np.array(start_op, np.uint64).ravel()
    n = my.size
    seeds = np.zeros(n, np.uint64) if seeds is None else np.asarray(seeds, np.uint64)
    words = np.zeros(n, np.uint64)
    alive = np.ones(n, bool)
    out = dict(rewards=np.zeros(n, np.float32), plies=np.zeros(n, np.int32), moves=np.full((n, 63), 255, np.uint8),
               final_bb=np.zeros((n, 2), np.uint64))
    for ply in range(63):
        idx = np.nonzero(alive)[0]
        if idx.size == 0:
            break
        s = sides[ply % 2]
        if s["kind"] == "baseline":
            r = oracle.c4_frozen_search(s["cfg"], seeds[idx], words[idx], my[idx], op[idx], s["explores"], action_selection=s["action"])
            words[idx] = r["rng_words"]
            col = r["best_action"]
        else:
            col = oracle.c4_mcts_search(s["cfg"], s["blob"], my[idx], op[idx], s["explores"], nn_mode=s["nn_mode"], net=s["net"])["best_action"]
        out["moves"][idx, ply] = col
        my[idx], op[idx], over, w = match.step(my[idx], op[idx], col)
        out["plies"][idx] += 1
        first_moved = ply % 2 == 0
        out["rewards"][idx[over & w]] = 1.0 if first_moved else -1.0
        done = idx[over]
        out["final_bb"][done, 0] = op[done] if first_moved else my[done]   # (after the move the mover's stones are `op`)
        out["final_bb"][done, 1] = my[done] if first_moved else op[done]
        alive[done] = False
    out["rng_words"] = words
    return out


def assert_games_equal(got, want, what, n=None, keys=KEYS):
    for k in keys:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        if n is not None:
            w = w[:n]
        assert g.shape == w.shape, f"{what}: {k} has shape {g.shape}, expected {w.shape}"
        if g.shape[0] == 0:
            continue
        bad = np.nonzero(np.any((g != w).reshape(g.shape[0], -1), axis=1))[0]
        assert bad.size == 0, f"{what}: {k} differs in games {bad[:8]} ({bad.size} of {g.shape[0]})"


def games_differ(a, b):
    return int(np.any(a["moves"] != b["moves"], axis=1).sum())


@pytest.fixture(scope="module")
def blobs(golden_dir):
    """two different Connect4Net checkpoints: A = the trained one, B = the random-init one"""
    return (np.load(os.path.join(golden_dir, "c4net_trained_f32.npy")).astype(np.float32).ravel(),
            np.load(os.path.join(golden_dir, "c4net_blob_f32.npy")).astype(np.float32).ravel())


@pytest.fixture(scope="module")
def openings():
    """100 openings of 4 plies: more than a wave, more than a 32-slot engine holds at once"""
    from synthesis_amd import arena

    return arena.random_openings(100, 4, seed=3)


@pytest.fixture(scope="module")
def expected_17(oracle, blobs, openings):
    """A (first) against B on the first 17 openings, both in f32, from the oracle: what a match after a refusal must still play"""
    a, b = blobs
    sides = (net_side(a, A_C, A_EXPLORES, oracle.ACC_FMA), net_side(b, B_C, B_EXPLORES, oracle.ACC_FMA))
    return oracle_match(oracle, sides, openings[0][:17], openings[1][:17])


def small_engine(slots, max_explores, arithmetic="f32"):
    import synthesis_amd as sa

    eng = sa.Engine(concurrent_games=slots, max_explores=max_explores)
    eng.set_network_arithmetic(arithmetic)
    return eng


@pytest.fixture(scope="module")
def engine32():
    eng = small_engine(32, 64)
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def engine32_f16():
    """an engine whose own arithmetic is f16x2 (it holds no network: a match needs none)"""
    eng = small_engine(32, 64, "f16x2")
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def engine_eval():
    """the evaluator's explore counts: a 100-explore policy"""
    eng = small_engine(32, 100)
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def engine_tiny():
    """16 slots and one-explore trees: the node pool holds 36 baseline trees of 400 explores, fewer than the 40 games of a match"""
    eng = small_engine(16, 1)
    yield eng
    eng.close()


# ---- 1
@pytest.mark.parametrize("which", ["f32", "f16x2"])
def test_default_sides_are_match_run(engine32, engine32_f16, blobs, openings, which):
    eng = engine32 if which == "f32" else engine32_f16
    assert eng.network_arithmetic()[0] == which
    pa, pb = net_players()
    a, b = blobs
    want = eng.match_run(pa, pb, a, b, *openings)
    got = eng.match_run_sides(replace(pa, weights=a), replace(pb, weights=b), *openings)
    for k in KEYS:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), k
    assert not got["rng_words"].any()                      # no baseline side: no generator moved
    assert want["plies"].min() >= 1 and ((want["moves"] != 255).sum(axis=1) == want["plies"]).all()
    again = eng.match_run(pa, pb, a, b, *openings)         # and the wrapper's own call is what it was after a sides call
    for k in KEYS:
        assert np.array_equal(again[k], want[k]), k


# ---- 2
def test_timing_counts_four_launches_per_ply_with_a_baseline_side(engine32, blobs, openings):
    """syn_last_timing's documented count, a network side against a baseline: one group per ply whichever kind of search it launches"""
    from synthesis_amd import match

    pa, _ = net_players()
    got = engine32.match_run_sides(replace(pa, weights=blobs[0]), match.vanilla_player(30), openings[0][:17], openings[1][:17],
                                   seeds=np.arange(17, dtype=np.uint64))
    ms, launches = engine32.last_timing()
    assert ms > 0.0
    assert got["plies"].min() >= 1
    assert launches == 4 * int(got["plies"].max())


@pytest.fixture(scope="module")
def cross(oracle):
    """blob A in f32 against blob B in f16x2, A first and B first, and the same games with one arithmetic on both sides — all from the
    oracle, computed once, shared, never modified"""
    from synthesis_amd import arena
    from tests import f16x2_checkpoints as ck

    blob, trained, _, _ = ck.load_fixtures()
    fam = ck.mlp_family(blob, trained)
    a, b = fam[CROSS_A], fam[CROSS_B]
    my, op = arena.random_openings(100, 4, seed=3)
    my, op = my[:CROSS_OPENINGS], op[:CROSS_OPENINGS]
    F, H = oracle.ACC_FMA, oracle.ACC_F16X2

    def games(mode_a, mode_b, a_first):
        sa_, sb_ = net_side(a, A_C, A_EXPLORES, mode_a), net_side(b, B_C, B_EXPLORES, mode_b)
        return oracle_match(oracle, (sa_, sb_) if a_first else (sb_, sa_), my, op)

    return dict(a=a, b=b, my=my, op=op,
                want={True: games(F, H, True), False: games(F, H, False)},
                all_f32={True: games(F, F, True), False: games(F, F, False)},
                all_f16={True: games(H, H, True), False: games(H, H, False)})


def test_cross_guard_from_the_oracle_alone(cross):
    """without this the cross-arithmetic test could not see which arithmetic ran"""
    for a_first in (True, False):
        assert games_differ(cross["want"][a_first], cross["all_f32"][a_first]) >= 1, "B's arithmetic does not show: choose other blobs / openings"
        assert games_differ(cross["want"][a_first], cross["all_f16"][a_first]) >= 1, "A's arithmetic does not show: choose other blobs / openings"


@pytest.mark.parametrize("which", ["f32", "f16x2"])
def test_cross_arithmetic_is_the_oracles_games(engine32, engine32_f16, cross, which):
    eng = engine32 if which == "f32" else engine32_f16
    pa, pb = net_players()
    pa, pb = replace(pa, weights=cross["a"], arithmetic="f32"), replace(pb, weights=cross["b"], arithmetic="f16x2")
    for a_first in (True, False):
        first, second = (pa, pb) if a_first else (pb, pa)
        got = eng.match_run_sides(first, second, cross["my"], cross["op"])
        assert_games_equal(got, cross["want"][a_first], f"engine in {which}, A first {a_first}: device match vs oracle")
        assert games_differ(got, cross["all_f32"][a_first]) >= 1 and games_differ(got, cross["all_f16"][a_first]) >= 1
    assert eng.network_arithmetic()[0] == which


# ---- 3
@pytest.mark.parametrize("which", ["f32", "f16x2"])
def test_cross_arithmetic_conv_is_the_host_path(openings, which):
    import synthesis_amd as sa
    from bench import make_conv_weights
    from synthesis_amd import arena

    a, b = make_conv_weights(), make_conv_weights(seed=7)
    pa, pb = net_players()
    pa, pb = replace(pa, weights=a, arithmetic="f32"), replace(pb, weights=b, arithmetic="f16x2")
    with sa.Engine(concurrent_games=32, max_explores=64) as eng:
        eng.load_weights_conv(b)     # the engine's network kind is the kind of the blobs a match takes
        eng.set_network_arithmetic(which)
        for first, second in ((pa, pb), (pb, pa)):
            got = eng.match_run_sides(first, second, *openings)
            host = arena.host_match(eng, first, second, *openings)
            assert eng.network_arithmetic()[0] == which
            assert_games_equal(got, host, f"conv, engine in {which}: device match vs host path")
        # the arithmetic of a side is what the host path says it is: both sides in the engine's own arithmetic is match_run
        same = eng.match_run_sides(replace(pa, arithmetic=which), replace(pb, arithmetic=which), *openings)
        assert_games_equal(same, eng.match_run(pa, pb, a, b, *openings), "conv: both sides in the engine's arithmetic")


# ---- 4
@pytest.mark.parametrize("which", ["f32", "f16x2"])
def test_nothing_leaks_into_or_out_of_the_engine(oracle, blobs, openings, monkeypatch, which):
    """An engine with a 2^16-entry policy cache that holds a THIRD network: its evaluations and one search give the same bits before and
    after the same checkpoint meets itself, f32 against f16x2 and the reverse. The lane-per-tree kernel is forced (small engines run the
    row kernels, which never use the cache); the searched positions are the match's own openings."""
    import synthesis_amd as sa
    from tests.oracle_lib import parity_mcts_config

    monkeypatch.setenv("SYN_DEBUG", "1")   # developer knobs are honoured only with SYN_DEBUG=1
    monkeypatch.setenv("SYN_LANES", "4")
    a = blobs[0]
    third = np.random.RandomState(11).normal(0.0, 0.2, a.size).astype(np.float32)
    my, op = openings
    cfg = sa.parity_mcts_config()
    pa, pb = net_players()
    p32, p16 = replace(pa, weights=a, arithmetic="f32"), replace(pb, weights=a, arithmetic="f16x2")
    with sa.Engine(concurrent_games=64, max_explores=64, policy_cache_log2=16) as eng:
        eng.load_weights(third)
        eng.set_network_arithmetic(which)
        plan0 = eng.network_arithmetic()
        ev0 = eng.policy_eval(my, op)
        s0 = eng.mcts_search(cfg, my, op, 32)
        assert eng.last_launch_shape()[0] == 4 and eng.last_cache_stats()[1] > 0      # the cache is in use: misses were inserted
        s0b = eng.mcts_search(cfg, my, op, 32)
        assert eng.last_cache_stats()[0] > 0
        g1 = eng.match_run_sides(p32, p16, my, op)
        assert eng.last_cache_stats() == (0, 0)
        g2 = eng.match_run_sides(p16, p32, my, op)
        assert eng.network_arithmetic() == plan0
        ev1 = eng.policy_eval(my, op)
        s1 = eng.mcts_search(cfg, my, op, 32)
        assert eng.last_cache_stats()[0] > 0                                           # the table still answers: it was not emptied
        for x, y in zip(ev0, ev1):
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
        for k in s0:
            for before in (s0, s0b):
                assert np.array_equal(np.asarray(before[k]).view(np.uint32), np.asarray(s1[k]).view(np.uint32)), k
        ref = oracle.c4_mcts_search(parity_mcts_config(), third, my, op, 32,
                                    nn_mode=oracle.ACC_F16X2 if which == "f16x2" else oracle.ACC_FMA)
        assert np.array_equal(s1["child_N"], ref["child_N"]) and np.array_equal(s1["best_action"], ref["best_action"])
    with sa.Engine(concurrent_games=64, max_explores=64) as plain:
        assert_games_equal(g1, plain.match_run_sides(p32, p16, my, op), "engine with a cache vs engine without")
        assert_games_equal(g2, plain.match_run_sides(p16, p32, my, op), "engine with a cache vs engine without, colours swapped")


# ---- 5
VS = ((200, 100, 0), (50, 400, 1))     # (first explores, second explores, action selection): Q and NumVisits


@pytest.fixture(scope="module")
def expected_vs(oracle):
    """oracle.c4_mcts_vs_mcts for 40 games per pairing, seeds 100 + g: (reward, moves, words) per game"""
    ocfg = rollout_cfgs()[1]
    return {(e1, e2, sel): [oracle.c4_mcts_vs_mcts(ocfg, 0, e1, e2, 100 + g, rollout_action=sel) for g in range(40)] for e1, e2, sel in VS}


def assert_oracle_games(reward, plies, record, want, what):
    for g, (r, moves, words) in enumerate(want):
        assert plies[g] == moves.size and np.array_equal(record["moves"][g, :moves.size], moves), f"{what}: game {g}"
        assert (record["moves"][g, moves.size:] == 255).all(), f"{what}: game {g}"
        assert reward[g] == r and record["rng_words"][g] == words[-1], f"{what}: game {g}"


@pytest.mark.parametrize("engine_name", ["engine32", "engine_tiny"])
def test_mcts_vs_mcts_on_the_device(request, expected_vs, engine_name):
    """evaluator.rs:200-228 without the host between the plies: two baseline sides, one generator per game shared by both. engine_tiny:
    40 games on 16 slots, and a pool that holds 36 trees of 400 explores (lanes take further roots in a grid-stride loop)."""
    from synthesis_amd import match

    eng = request.getfixturevalue(engine_name)
    for e1, e2, sel in VS:
        first, second = match.vanilla_player(e1, action=sel), match.vanilla_player(e2, action=sel)
        rec = {}
        reward, plies = match.play_match_device(eng, first, second, 40, seed=100, record=rec)
        assert eng.last_launch_shape()[0] == 5
        assert_oracle_games(reward, plies, rec, expected_vs[(e1, e2, sel)], f"{engine_name} {e1} vs {e2}")
        host_rec = {}
        host_reward, host_plies = match.play_match(eng, first, second, 40, seed=100, record=host_rec)
        assert np.array_equal(reward, host_reward) and np.array_equal(plies, host_plies)
        assert np.array_equal(rec["moves"], host_rec["moves"]) and np.array_equal(rec["rng_words"], host_rec["rng_words"])


# ---- 6
@pytest.mark.parametrize("arithmetic", ["f32", "f16x2"])
def test_eval_against_rollout_on_the_device(engine_eval, oracle, blobs, arithmetic):
    """evaluator.rs:163-198: the network's MCTS::exploit on one side, the vanilla baseline on the other, both colours; a network ply
    leaves the game's generator where it was"""
    import synthesis_amd as sa
    from synthesis_amd import match
    from tests.oracle_lib import parity_mcts_config

    blob = blobs[1]
    nn_mode = oracle.ACC_F16X2 if arithmetic == "f16x2" else oracle.ACC_FMA
    net = match.Player("net", 100, sa.parity_mcts_config(), weights=blob, arithmetic=arithmetic)
    ocfg = rollout_cfgs()[1]
    for net_moves_first in (True, False):
        sel = 0 if net_moves_first else 1   # rollout_action: Q (the reference's choice) and NumVisits
        van = match.vanilla_player(150, action=sel)
        first, second = (net, van) if net_moves_first else (van, net)
        rec = {}
        reward, plies = match.play_match_device(engine_eval, first, second, 24, seed=7, record=rec)
        want = [oracle.c4_eval_against_rollout(parity_mcts_config(), 100, blob, ocfg, 0 if net_moves_first else 1, 150, 7 + g,
                                               rollout_action=sel, nn_mode=nn_mode) for g in range(24)]
        assert_oracle_games(reward, plies, rec, want, f"network {arithmetic}, moves first {net_moves_first}")
    assert engine_eval.network_arithmetic()[0] == "f32"


# ---- 7
@pytest.fixture(scope="module")
def one_game_per_ply(oracle, blobs):
    """Starts, seeds and the oracle's games of network A (f32, first) against VanillaMCTS40: harvested from deep random openings so that
    exactly one game ends after 1, 2, ..., K plies, in an order of game indices that is not the order of ending."""
    from synthesis_amd import arena

    my, op = [], []
    for plies, seed in ((12, 5), (14, 6), (16, 7), (18, 8)):
        m, o = arena.random_openings(60, plies, seed)
        my.append(m); op.append(o)
    # one move from a win: first has the bottom row of columns 0..2, column 3 wins
    my.append(np.array([0b1 | 1 << 7 | 1 << 14], np.uint64)); op.append(np.array([0b10 | 1 << 8 | 1 << 15], np.uint64))
    my, op = np.concatenate(my), np.concatenate(op)
    seeds = np.arange(my.size, dtype=np.uint64) * np.uint64(977) + np.uint64(13)
    sides = (net_side(blobs[0], A_C, A_EXPLORES, oracle.ACC_FMA), baseline_side(40, 0))
    want = oracle_match(oracle, sides, my, op, seeds)
    pick = []
    for r in range(1, 64):
        idx = np.nonzero(want["plies"] == r)[0]
        if idx.size == 0:
            break
        pick.append(int(idx[0]))
    order = np.array(pick)[np.random.RandomState(1).permutation(len(pick))]
    return my, op, seeds, want, order


def test_the_generator_follows_the_game(engine32, blobs, one_game_per_ply):
    import synthesis_amd as sa
    from synthesis_amd import match

    my, op, seeds, want, order = one_game_per_ply
    assert order.size >= 8, "the starts do not end at every ply from 1 to 8"
    keys = KEYS + ("rng_words",)
    net = match.Player("A", A_EXPLORES, sa.MCTSConfig(c=A_C), weights=blobs[0])
    van = match.vanilla_player(40)
    # the live set shrinks by exactly one game per ply, K, K - 1, ..., 1: every survivor keeps its own generator
    got = engine32.match_run_sides(net, van, my[order], op[order], seeds=seeds[order])
    assert sorted(got["plies"].tolist()) == list(range(1, order.size + 1))
    assert got["rng_words"][got["plies"] >= 2].min() > 0       # (a game of one ply ended on the network's move: no playout)
    assert_games_equal(got, {k: want[k][order] for k in keys}, "one game ends per ply: device vs oracle", keys=keys)
    rec = {}
    reward, plies = match.play_match(engine32, net, van, seeds=seeds[order], starts=(my[order], op[order]), record=rec)
    assert np.array_equal(rec["rng_words"], got["rng_words"]) and np.array_equal(rec["moves"], got["moves"])
    assert np.array_equal(reward, got["rewards"]) and np.array_equal(plies, got["plies"])
    # all starts, then the same games in another order with their seeds: per-game records are identical
    full = engine32.match_run_sides(net, van, my, op, seeds=seeds)
    assert_games_equal(full, want, "all starts: device vs oracle", keys=keys)
    perm = np.random.RandomState(2).permutation(my.size)
    shuffled = engine32.match_run_sides(net, van, my[perm], op[perm], seeds=seeds[perm])
    assert_games_equal(shuffled, {k: full[k][perm] for k in keys}, "permuted games", keys=keys)
    # ... and the seed is the game's: the same order with the seeds left where they were plays other games
    assert games_differ(engine32.match_run_sides(net, van, my[perm], op[perm], seeds=seeds), shuffled) >= 1


# ---- 8
def test_refusals_leave_the_next_match_identical(blobs, openings, expected_17):
    import synthesis_amd as sa
    from synthesis_amd import match
    from synthesis_amd.engine import CMatchSide, Engine
    from tests import f16x2_checkpoints as ck

    a, b = blobs
    pa, pb = net_players()
    pa, pb = replace(pa, weights=a), replace(pb, weights=b)
    my, op = openings[0][:17].copy(), openings[1][:17].copy()
    seeds = np.arange(17, dtype=np.uint64)
    dcfg = rollout_cfgs()[0]
    van = match.vanilla_player(30)
    with sa.Engine(concurrent_games=32, max_explores=64, policy_cache_log2=10) as eng:
        eng.load_weights(b)
        state0 = (eng.network_arithmetic(), eng.policy_eval(my, op))

        def untouched():
            arith, ev = eng.network_arithmetic(), eng.policy_eval(my, op)
            assert arith == state0[0] and all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(ev, state0[1]))
            assert_games_equal(eng.match_run_sides(pa, pb, my, op), expected_17, "match after a refusal")

        def refused(code, first=pa, second=pb, seeds=seeds, text=None):
            with pytest.raises(sa.SynthesisAmdError) as e:
                eng.match_run_sides(first, second, my, op, seeds=seeds)
            assert e.value.code == code and (text is None or text in str(e.value)), str(e.value)
            untouched()

        def refused_c(code, side_first, side_second):
            with pytest.raises(sa.SynthesisAmdError) as e:
                eng.match_run_sides_c(side_first, side_second, my, op, seeds)
            assert e.value.code == code, str(e.value)
            untouched()

        untouched()
        poly = replace(van, mcts_cfg=replace(dcfg, exploration=sa.Exploration.PolynomialUct))
        refused(UNSUPPORTED, second=poly, text="Uct only")
        refused(UNSUPPORTED, first=poly, text="Uct only")
        refused(UNSUPPORTED, second=replace(van, mcts_cfg=replace(dcfg, fpu=sa.Fpu.ParentQ)), text="Fpu::Const only")
        refused(CAPACITY, second=match.vanilla_player(300000), text="needs up to")          # beyond 21 bits of node index
        refused(CAPACITY, first=match.vanilla_player(2**30))                                # ... and beyond any pool
        refused(INVALID, second=van, seeds=None, text="seeds")
        refused(INVALID, first=van, second=van, seeds=None, text="seeds")
        sa_, ka = Engine.match_side(pa)
        sb_, kb = Engine.match_side(pb)
        for field, value in (("kind", 2), ("kind", -1), ("arithmetic", 3), ("arithmetic", -1)):
            bad = CMatchSide.from_buffer_copy(sb_)
            setattr(bad, field, value)
            refused_c(INVALID, sa_, bad)
            refused_c(INVALID, bad, sa_)
        no_plan = ck.refused_family(b)["init_x2^24"]
        refused(UNSUPPORTED, second=replace(pb, weights=no_plan, arithmetic="f16x2"), text="f16x2 plan")
        refused(UNSUPPORTED, first=replace(pa, weights=no_plan, arithmetic="f16x2"), text="f16x2 plan")
        assert_games_equal(eng.match_run_sides(pa, replace(pb, weights=no_plan, arithmetic="f32"), my[:3], op[:3]),
                           eng.match_run(pa, pb, a, no_plan, my[:3], op[:3]), "the same blob is playable in f32")
        normal = match.Player("n", A_EXPLORES, sa.MCTSConfig(fpu=sa.Fpu.Func, fpu_value=1.0, fpu_std=0.1), weights=a)       # SYN_FPU_NORMAL
        refused(UNSUPPORTED, first=normal, text="deterministic")
        refused(UNSUPPORTED, first=van, second=normal, text="deterministic")
        refused(INVALID, second=replace(pb, weights=b[:-1]))
        refused(INVALID, first=replace(pa, weights=a[:12412]))                              # Connect4ConvNet's size on a Connect4Net engine
        refused(CAPACITY, first=replace(pa, explores=65))                                   # a network side: the engine's max_explores is 64
        keep = (ka, kb)   # noqa: F841  (the hand-made structs point into these arrays)
        # n_games == 0 with a baseline side
        empty = eng.match_run_sides(pa, van, my[:0], op[:0], seeds=seeds[:0])
        assert empty["rewards"].shape == (0,) and empty["rng_words"].shape == (0,) and empty["moves"].shape == (0, 63)


# ---- 9
def test_evaluation_round_on_the_device_is_the_host_paths_text(engine_eval, blobs):
    import synthesis_amd as sa
    from synthesis_amd import match

    blob = blobs[1]
    old_w = np.random.RandomState(3).normal(0, 0.2, blob.size).astype(np.float32)
    cfg = match.EvaluationConfig(policy_num_explores=80, policy_mcts_cfg=sa.parity_mcts_config(), num_games_against_rollout=2,
                                 rollout_num_explores=(60, 120, 240))
    for i_iter in (4, 5):
        name = f"model_{i_iter}.ot"
        host = match.evaluation_round(engine_eval, cfg, i_iter, name, blob, [("model_1.ot", old_w)])
        dev = match.evaluation_round(engine_eval, cfg, i_iter, name, blob, [("model_1.ot", old_w)], device=True)
        assert dev == host and dev.count("[Result") == 2 + 2 * 2 * 3 + 2
