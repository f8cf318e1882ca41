"""GPU tests of the device-resident tournament (Engine.tournament_run = syn_tournament_run, tournament_kernels.cuh): K players, one call.
Bar: every game's record — moves, ply count, reward, final position, stream position — equal to the one-game match between its two
players: to games built on the CPU from the oracle where the players are networks in f32, and to Engine.match_run_sides on the same
engine for the other kinds. The stable multi-way regroup is also tested alone (syn_debug_tournament_regroup) against numpy's stable
sort."""
from dataclasses import replace

import numpy as np
import pytest

from tests.test_gpu_match_sides import KEYS, assert_games_equal, games_differ, net_side, oracle_match, rollout_cfgs

pytestmark = pytest.mark.gpu

ALL_KEYS = KEYS + ("rng_words",)
INVALID, UNSUPPORTED, CAPACITY = -1, -5, -6
SETTINGS = ((32, 3.0), (20, 1.5), (24, 2.0))    # (explores, c) of P0, P1, P2: all different, so a game searched as another player shows


@pytest.fixture(scope="module")
def blobs3(golden_dir):
    """P0 = the trained checkpoint, P1 = the random-init one, P2 = the stress family's trained_outlier_4096"""
    from tests import f16x2_checkpoints as ck

    blob, trained, _, _ = ck.load_fixtures()
    return (np.asarray(trained, np.float32).ravel(), np.asarray(blob, np.float32).ravel(),
            np.asarray(ck.mlp_family(blob, trained)["trained_outlier_4096"], np.float32).ravel())


def players3(blobs3, **kw):
    import synthesis_amd as sa
    from synthesis_amd import match

    return [match.Player(f"P{i}", e, sa.MCTSConfig(c=c), weights=b, **kw) for i, ((e, c), b) in enumerate(zip(SETTINGS, blobs3))]


@pytest.fixture(scope="module")
def openings17():
    from synthesis_amd import arena

    my, op = arena.random_openings(100, 4, seed=3)
    return my[:17].copy(), op[:17].copy()


@pytest.fixture(scope="module")
def expected_nine(oracle, blobs3, openings17):
    """{(i, j): the oracle's 17 games of Pi (first) against Pj}, all nine ordered pairings: computed once, shared, never modified"""
    sides = [net_side(b, c, e, oracle.ACC_FMA) for (e, c), b in zip(SETTINGS, blobs3)]
    return {(i, j): oracle_match(oracle, (sides[i], sides[j]), *openings17) for i in range(3) for j in range(3)}


def nine_schedule():
    """153 games: for every opening all nine ordered pairings — interleaved by opening, not grouped by pairing"""
    first = np.tile(np.repeat(np.arange(3), 3), 17).astype(np.int32)
    second = np.tile(np.tile(np.arange(3), 3), 17).astype(np.int32)
    return first, second, np.repeat(np.arange(17), 9)


def expected_of_schedule(expected_nine, first, second, opening):
    n = first.size
    out = dict(rewards=np.zeros(n, np.float32), plies=np.zeros(n, np.int32), moves=np.full((n, 63), 255, np.uint8),
               final_bb=np.zeros((n, 2), np.uint64), rng_words=np.zeros(n, np.uint64))
    for g in range(n):
        e = expected_nine[(int(first[g]), int(second[g]))]
        for k in ALL_KEYS:
            out[k][g] = e[k][opening[g]]
    return out


@pytest.fixture(scope="module")
def engine32():
    import synthesis_amd as sa

    eng = sa.Engine(concurrent_games=32, max_explores=64)
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def engine32_f16():
    import synthesis_amd as sa

    eng = sa.Engine(concurrent_games=32, max_explores=64)
    eng.set_network_arithmetic("f16x2")
    yield eng
    eng.close()


# ---- 1
def key_patterns(n, n_keys):
    rng = np.random.default_rng(1000 * n_keys + n)
    pats = {"all one key": np.full(n, n_keys - 1), "all dropped": np.full(n, n_keys),
            "ascending": np.arange(n) * (n_keys + 1) // n, "descending": (n - 1 - np.arange(n)) * (n_keys + 1) // n,
            "uniform": rng.integers(0, n_keys + 1, n)}
    once = np.full(n, n_keys)
    where = rng.permutation(n)[:n_keys]
    once[where] = rng.permutation(n_keys)[:where.size]
    pats["every key exactly once"] = once
    last = rng.integers(0, n_keys - 1, n) if n_keys > 1 else np.full(n, n_keys)
    last[n - 1] = n_keys - 1
    pats["one key in the last lane of the last workgroup only"] = last
    return {k: v.astype(np.int32) for k, v in pats.items()}


@pytest.mark.parametrize("n_keys", [1, 2, 5, 64])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1000, 70001])
def test_regroup_is_numpys_stable_sort(engine32, n, n_keys):
    import synthesis_amd as sa

    for what, keys in key_patterns(n, n_keys).items():
        assert keys.min() >= 0 and keys.max() <= n_keys
        order = np.argsort(keys, kind="stable")
        want_seg = np.searchsorted(keys[order], np.arange(n_keys + 1), side="left")
        survivors = int(want_seg[n_keys])
        perm, seg = engine32.debug_tournament_regroup(keys, n_keys)
        assert np.array_equal(seg, want_seg), f"{what}: seg"
        assert np.array_equal(perm[:survivors], order[:survivors]), f"{what}: the survivors' permutation"
        assert (perm[survivors:] == -1).all(), f"{what}: a dropped job was copied"
    with pytest.raises(sa.SynthesisAmdError) as e:
        engine32.debug_tournament_regroup(np.full(3, n_keys + 1, np.int32), n_keys)
    assert e.value.code == INVALID


# ---- 2
def test_guard_any_two_pairings_differ_in_most_openings(expected_nine):
    """asserted on the oracle's games before the device is asked: a game searched with another player's blob or settings cannot pass"""
    pairings = sorted(expected_nine)
    fewest = min(games_differ(expected_nine[a], expected_nine[b]) for i, a in enumerate(pairings) for b in pairings[i + 1:])
    assert fewest >= 9, f"two pairings differ in only {fewest} of 17 openings: choose other players / openings"
    for e in expected_nine.values():
        assert not e["rng_words"].any()


def test_tournament_is_the_oracles_pairwise_games(engine32, blobs3, openings17, expected_nine):
    first, second, opening = nine_schedule()
    assert first.size == 153 and len(set(zip(first[:9].tolist(), second[:9].tolist()))) == 9
    my, op = openings17
    got = engine32.tournament_run(players3(blobs3), first, second, my[opening], op[opening])
    assert_games_equal(got, expected_of_schedule(expected_nine, first, second, opening), "nine pairings in one call vs oracle", keys=KEYS)
    assert not got["rng_words"].any()
    ms, launches = engine32.last_timing()
    assert ms > 0 and launches >= 2 * int(got["plies"].max())


# ---- 3
@pytest.mark.parametrize("which", ["f32", "f16x2"])
def test_mixed_kinds_are_match_run_sides(engine32, engine32_f16, blobs3, which):
    from synthesis_amd import arena, match

    eng = engine32 if which == "f32" else engine32_f16
    p2 = players3(blobs3)[2]
    players = [replace(p2, arithmetic="f32"), replace(p2, arithmetic="f16x2"), match.vanilla_player(50, action=0),
               match.vanilla_player(20, action=1)]
    my, op = arena.random_openings(100, 4, seed=3)
    my, op = my[:12], op[:12]
    first = np.tile(np.repeat(np.arange(4), 4), 12).astype(np.int32)
    second = np.tile(np.tile(np.arange(4), 4), 12).astype(np.int32)
    opening = np.repeat(np.arange(12), 16)
    seeds = np.arange(first.size, dtype=np.uint64) * np.uint64(7919) + np.uint64(5)
    got = eng.tournament_run(players, first, second, my[opening], op[opening], seeds=seeds)
    assert eng.network_arithmetic()[0] == which
    for a in range(4):
        for b in range(4):
            g = np.nonzero((first == a) & (second == b))[0]
            want = eng.match_run_sides(players[a], players[b], my[opening[g]], op[opening[g]], seeds=seeds[g])
            assert_games_equal({k: got[k][g] for k in ALL_KEYS}, want, f"engine in {which}: pairing {a} vs {b}", keys=ALL_KEYS)
            assert (want["rng_words"] > 0).any() == (a >= 2 or b >= 2)     # a generator moves where a baseline plays, and only there


# ---- 4
def test_the_order_of_the_games_does_not_matter(engine32, blobs3, openings17, expected_nine):
    first, second, opening = nine_schedule()
    my, op = openings17
    perm = np.random.default_rng(4).permutation(first.size)
    seeds = np.arange(first.size, dtype=np.uint64) + np.uint64(11)     # (no baseline plays: carried, never read)
    got = engine32.tournament_run(players3(blobs3), first[perm], second[perm], my[opening[perm]], op[opening[perm]], seeds=seeds[perm])
    want = expected_of_schedule(expected_nine, first, second, opening)
    assert_games_equal(got, {k: want[k][perm] for k in ALL_KEYS}, "permuted schedule", keys=ALL_KEYS)


# ---- 5
def pattern_board():
    """A full 9x7 board without four in a row: cell (row, col) belongs to side (col // 2 + row) % 2"""
    side = [0, 0]
    for col in range(9):
        for row in range(7):
            side[(col // 2 + row) % 2] |= 1 << (row + 7 * col)
    return side


@pytest.fixture(scope="module")
def special(oracle, blobs3, openings17, expected_nine):
    """Hand-made and harvested starts over three playing players (and a fourth that plays nothing): a win in one, a forced draw on a
    62-stone board, and the tails of the oracle's P0-against-P1 games, so that games of every length from 1 ply up are in one call.
    Returns (my, op, first, second, the oracle's games)."""
    from synthesis_amd import match

    starts = [(0b1 | 1 << 7 | 1 << 14, 0b10 | 1 << 8 | 1 << 15)]                       # one move from a win
    s = pattern_board()
    top, mine = 1 << (6 + 7 * 8), (8 // 2 + 6) % 2
    starts.append((s[mine] & ~top, s[1 - mine]))                                      # one free cell: a draw at ply 1
    e = expected_nine[(0, 1)]
    for g in range(17):
        my, op = np.array([openings17[0][g]], np.uint64), np.array([openings17[1][g]], np.uint64)
        p = int(e["plies"][g])
        for j in range(p):
            if p - j <= 12:
                starts.append((int(my[0]), int(op[0])))
            my, op, _, _ = match.step(my, op, e["moves"][g, j:j + 1].astype(np.int64))
    my = np.array([a for a, _ in starts], np.uint64); op = np.array([b for _, b in starts], np.uint64)
    n = my.size
    cyc = [(0, 1), (1, 2), (2, 0), (1, 0), (2, 2), (0, 2)]
    first = np.array([cyc[g % 6][0] for g in range(n)], np.int32); second = np.array([cyc[g % 6][1] for g in range(n)], np.int32)
    sides = [net_side(b, c, x, oracle.ACC_FMA) for (x, c), b in zip(SETTINGS, blobs3)]
    want = dict(rewards=np.zeros(n, np.float32), plies=np.zeros(n, np.int32), moves=np.full((n, 63), 255, np.uint8),
                final_bb=np.zeros((n, 2), np.uint64), rng_words=np.zeros(n, np.uint64))
    for a, b in set(cyc):
        g = np.nonzero((first == a) & (second == b))[0]
        r = oracle_match(oracle, (sides[a], sides[b]), my[g], op[g])
        for k in ALL_KEYS:
            want[k][g] = r[k]
    return my, op, first, second, want


def test_groups_that_empty_at_different_plies(engine32, blobs3, special):
    my, op, first, second, want = special
    assert want["plies"][0] == 1 and want["rewards"][0] == 1.0
    assert want["plies"][1] == 1 and want["rewards"][1] == 0.0 and want["final_bb"][1].sum() == (1 << 63) - 1
    assert set(range(1, 11)) <= set(want["plies"].tolist()), "the starts do not end at every ply from 1 to 10"
    # who still moves at ply t: a playing player's group is empty while others live, and the last live game is alone
    emptied = False
    for t in range(int(want["plies"].max())):
        live = want["plies"] > t
        movers = set(np.where(t % 2 == 0, first, second)[live].tolist())
        emptied |= 0 < len(movers) < 3
    assert emptied and (want["plies"] == want["plies"].max()).sum() == 1
    players = players3(blobs3)
    players.append(replace(players[0], name="idle", explores=7))      # appears in no game
    got = engine32.tournament_run(players, first, second, my, op)
    assert_games_equal(got, want, "special starts over three players", keys=ALL_KEYS)


# ---- 6
def test_more_than_one_workgroup_per_ply(engine32, blobs3):
    """600 games over five network players at 4 explores: ply 0's regroup spans three 256-thread workgroups, every key in each"""
    import synthesis_amd as sa
    from synthesis_amd import arena, match

    my, op = arena.random_openings(120, 4, seed=3)
    players = [match.Player(f"Q{i}", 4, sa.MCTSConfig(c=1.0 + 0.5 * i), weights=blobs3[i % 3]) for i in range(5)]
    k = np.arange(600) // 5
    first = (np.arange(600) % 5).astype(np.int32)
    second = (k % 5).astype(np.int32)
    grouped_second = second[np.argsort(first, kind="stable")]     # ply 0's job order: what the first regroup reads
    for b in range(3):
        assert set(grouped_second[256 * b:256 * (b + 1)].tolist()) == set(range(5))
    got = engine32.tournament_run(players, first, second, my[k], op[k])
    assert got["plies"].min() >= 1
    for a in range(5):
        for b in range(5):
            g = np.nonzero((first == a) & (second == b))[0]
            assert g.size == 24
            want = engine32.match_run_sides(players[a], players[b], my[k[g]], op[k[g]])
            assert_games_equal({key: got[key][g] for key in ALL_KEYS}, want, f"pairing {a} vs {b}", keys=ALL_KEYS)


# ---- 7
def test_refusals_leave_the_next_calls_identical(blobs3, openings17, expected_nine):
    import synthesis_amd as sa
    from synthesis_amd import match
    from synthesis_amd.engine import CMatchSide, Engine
    from tests import f16x2_checkpoints as ck

    my, op = openings17
    players = players3(blobs3)
    pa, pb = players[0], players[1]
    i17 = np.arange(17)
    first, second = np.zeros(17, np.int32), np.ones(17, np.int32)
    seeds = np.arange(17, dtype=np.uint64)
    dcfg = rollout_cfgs()[0]
    van = match.vanilla_player(30)
    with sa.Engine(concurrent_games=32, max_explores=64, policy_cache_log2=10) as eng:
        eng.load_weights(blobs3[1])
        state0 = (eng.network_arithmetic(), eng.policy_eval(my, op))

        def untouched():
            arith, ev = eng.network_arithmetic(), eng.policy_eval(my, op)
            assert arith == state0[0] and all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(ev, state0[1]))
            assert_games_equal(eng.tournament_run(players, first, second, my, op), expected_nine[(0, 1)], "tournament after a refusal")
            assert_games_equal(eng.match_run(pb, pa, blobs3[1], blobs3[0], my, op), expected_nine[(1, 0)], "match_run after a refusal")

        def refused(code, ps=players, first=first, second=second, my=my, op=op, seeds=seeds, text=None):
            with pytest.raises(sa.SynthesisAmdError) as e:
                eng.tournament_run(ps, first, second, my, op, seeds=seeds)
            assert e.value.code == code and (text is None or text in str(e.value)), str(e.value)
            untouched()

        def refused_c(code, sides, n_players=None, text=None):
            with pytest.raises(sa.SynthesisAmdError) as e:
                eng.tournament_run_c(sides, first, second, my, op, seeds, n_players=n_players)
            assert e.value.code == code and (text is None or text in str(e.value)), str(e.value)
            untouched()

        def with_player(p, at=2):
            ps = list(players)
            ps[at] = p
            return ps

        untouched()
        # a refusal of match_run_sides is a refusal here, for a player that plays (index 1) and for one that does not (index 2)
        for at in (1, 2):
            refused(UNSUPPORTED, with_player(replace(van, mcts_cfg=replace(dcfg, exploration=sa.Exploration.PolynomialUct)), at), text="Uct only")
            refused(INVALID, with_player(van, at), seeds=None, text="seeds")
        refused(UNSUPPORTED, with_player(replace(van, mcts_cfg=replace(dcfg, fpu=sa.Fpu.ParentQ))), text="Fpu::Const only")
        refused(CAPACITY, with_player(match.vanilla_player(300000)), text="needs up to")
        normal = match.Player("n", 32, sa.MCTSConfig(fpu=sa.Fpu.Func, fpu_value=1.0, fpu_std=0.1), weights=blobs3[0])       # SYN_FPU_NORMAL
        refused(UNSUPPORTED, with_player(normal, 0), text="deterministic")
        refused(UNSUPPORTED, with_player(replace(pa, mcts_cfg=replace(pa.mcts_cfg, root_policy_noise=sa.PolicyNoise.Dirichlet))), text="deterministic")
        refused(INVALID, with_player(replace(pa, action=7), 1), text="action")
        refused(INVALID, with_player(replace(van, action=7)), text="action")
        refused(INVALID, with_player(replace(pb, weights=blobs3[1][:-1])))
        refused(INVALID, with_player(replace(pa, weights=blobs3[0][:12412]), 0))           # Connect4ConvNet's size on a Connect4Net engine
        refused(CAPACITY, with_player(replace(pa, explores=65)))                           # the engine's max_explores is 64
        no_plan = ck.refused_family(blobs3[1])["init_x2^24"]
        refused(UNSUPPORTED, with_player(replace(pb, weights=no_plan, arithmetic="f16x2")), text="f16x2 plan")
        sides, keep = zip(*(Engine.match_side(p) for p in players))
        for field, value in (("kind", 2), ("kind", -1), ("arithmetic", 3), ("arithmetic", -1)):
            bad = CMatchSide.from_buffer_copy(sides[1])
            setattr(bad, field, value)
            refused_c(INVALID, [sides[0], bad, sides[2]], text=field if field == "kind" else "arithmetic")
        # the tournament's own refusals
        refused_c(INVALID, list(sides), n_players=0, text="n_players")
        refused_c(INVALID, list(sides) * 22, n_players=65, text="n_players")
        for arr in ("first", "second"):
            for value in (-1, 3):
                idx = {"first": first.copy(), "second": second.copy()}
                idx[arr][5] = value
                refused(INVALID, first=idx["first"], second=idx["second"], text="game 5")
        bad_my = my.copy(); bad_my[3] = np.uint64(0b10)                                     # a floating stone
        refused(INVALID, my=bad_my, text="start 3")
        won_my = my.copy(); won_op = op.copy()
        won_my[4], won_op[4] = np.uint64(0b1 | 1 << 7 | 1 << 14 | 1 << 21), np.uint64(0b10 | 1 << 8 | 1 << 15)
        refused(INVALID, my=won_my, op=won_op, text="finished game")
        assert keep is not None
        # n_games == 0 after the refusals, and 64 players are accepted
        empty = eng.tournament_run(players, i17[:0], i17[:0], my[:0], op[:0])
        assert empty["rewards"].shape == (0,) and empty["moves"].shape == (0, 63)
        with pytest.raises(sa.SynthesisAmdError):
            eng.tournament_run(with_player(replace(pa, explores=65)), i17[:0], i17[:0], my[:0], op[:0])
        many = eng.tournament_run_c(list(sides) * 21 + [sides[0]], np.full(17, 63, np.int32), np.full(17, 3, np.int32), my, op, None)   # both are P0
        assert_games_equal(many, expected_nine[(0, 0)], "64 players, the last one playing", keys=ALL_KEYS)


# ---- 8
def test_nothing_leaks_into_or_out_of_the_engine(oracle, blobs3, monkeypatch):
    """The arena's cache test with a tournament in the middle: an engine with a 2^16-entry policy cache that holds a FOURTH network
    gives the same evaluations and the same search, bit for bit, before and after; the searched positions are the tournament's own
    openings. The lane-per-tree kernel is forced (small engines run the row kernels, which never use the cache)."""
    import synthesis_amd as sa
    from synthesis_amd import arena
    from tests.oracle_lib import parity_mcts_config

    monkeypatch.setenv("SYN_DEBUG", "1")   # developer knobs are honoured only with SYN_DEBUG=1
    monkeypatch.setenv("SYN_LANES", "4")
    other = np.random.RandomState(11).normal(0.0, 0.2, blobs3[0].size).astype(np.float32)
    my, op = arena.random_openings(100, 4, seed=3)
    cfg = sa.parity_mcts_config()
    players = players3(blobs3)
    players[2] = replace(players[2], arithmetic="f16x2")
    first = (np.arange(100) % 3).astype(np.int32); second = ((np.arange(100) // 3) % 3).astype(np.int32)
    with sa.Engine(concurrent_games=64, max_explores=64, policy_cache_log2=16) as eng:
        eng.load_weights(other)
        plan0 = eng.network_arithmetic()
        ev0 = eng.policy_eval(my, op)
        s0 = eng.mcts_search(cfg, my, op, 32)
        assert eng.last_launch_shape()[0] == 4 and eng.last_cache_stats()[1] > 0      # the cache is in use: misses were inserted
        s0b = eng.mcts_search(cfg, my, op, 32)
        assert eng.last_cache_stats()[0] > 0
        got = eng.tournament_run(players, first, second, my, op)
        assert eng.last_cache_stats() == (0, 0) and eng.network_arithmetic() == plan0
        ev1 = eng.policy_eval(my, op)
        s1 = eng.mcts_search(cfg, my, op, 32)
        assert eng.last_cache_stats()[0] > 0                                           # the table still answers: it was not emptied
        for x, y in zip(ev0, ev1):
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
        for k in s0:
            for before in (s0, s0b):
                assert np.array_equal(np.asarray(before[k]).view(np.uint32), np.asarray(s1[k]).view(np.uint32)), k
        ref = oracle.c4_mcts_search(parity_mcts_config(), other, my, op, 32, nn_mode=oracle.ACC_FMA)
        assert np.array_equal(s1["child_N"], ref["child_N"]) and np.array_equal(s1["best_action"], ref["best_action"])
    with sa.Engine(concurrent_games=64, max_explores=64) as plain:
        assert_games_equal(got, plain.tournament_run(players, first, second, my, op), "engine with a cache vs engine without", keys=ALL_KEYS)


# ---- 9
def test_round_robin_is_compare_pair_by_pair(engine32, blobs3, openings17):
    from synthesis_amd import arena

    players = players3(blobs3)
    players[1] = replace(players[1], arithmetic="f32")      # (compare then goes through match_run_sides for the pairs with P1)
    res = arena.round_robin(engine32, players, openings17)
    assert res["pairs"] == [(0, 1), (0, 2), (1, 2)] and res["games"]["rewards"].shape == (2 * 3 * 17,)
    for a, b in res["pairs"]:
        want = arena.compare(engine32, blobs3[a], blobs3[b], openings17, players[a], players[b])
        st = res["stats"][(a, b)]
        assert set(st) == set(want)
        for k, w in want.items():
            if isinstance(w, np.ndarray):
                assert np.array_equal(st[k], w), (a, b, k)
            else:
                assert st[k] == w or (st[k] != st[k] and w != w), (a, b, k)
    fit = arena.ratings(res, prior_draws=1.0, bootstrap=50)
    assert fit["elo"][0] == 0.0 and np.isfinite(fit["elo"]).all() and (fit["elo_lo"] <= fit["elo_hi"]).all()
