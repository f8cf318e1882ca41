"""GPU tests of the device-resident match (Engine.match_run = syn_match_run, match_kernels.cuh). Bar: moves, ply counts, rewards and
final positions equal, game for game, to games built ply by ply on the CPU from oracle.c4_mcts_search with the mover's parameters, and
to the host path of match.play_match on the same engine.

play_match itself starts every game from the empty board, so from other starts the host path is arena.host_match: play_match's per-ply
steps (load_weights of the mover's blob, one mcts_search over the live games, match.step) from given positions. From the empty board
play_match itself is the comparison (test_empty_board_game_is_eval_against_old)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KEYS = ("moves", "plies", "rewards", "final_bb")
A_EXPLORES, A_C = 32, 3.0      # the two sides differ in explores and in c, so a side that searched with the other's settings shows
B_EXPLORES, B_C = 20, 1.5


def device_players():
    import synthesis_amd as sa
    from synthesis_amd import match

    return (match.Player("A", A_EXPLORES, sa.MCTSConfig(c=A_C)), match.Player("B", B_EXPLORES, sa.MCTSConfig(c=B_C)))


def oracle_sides(blob_first, blob_second):
    from tests.oracle_lib import parity_mcts_config

    return ((blob_first, parity_mcts_config(c=A_C), A_EXPLORES), (blob_second, parity_mcts_config(c=B_C), B_EXPLORES))


def oracle_match(oracle, sides, start_my, start_op, nn_mode=1, net="mlp"):
    """The expected games: ply k of every live game is one oracle.c4_mcts_search with side k % 2's (blob, config, explores), the move
    is its best_action, the rules are match.step's (numpy). Same dict as Engine.match_run."""
    from synthesis_amd import match

    my = np.array(start_my, np.uint64).ravel(); op = np.array(start_op, np.uint64).ravel()
    n = my.size
    alive = np.ones(n, bool)
    out = dict(rewards=np.zeros(n, np.float32), plies=np.zeros(n, np.int32), moves=np.full((n, 63), 255, np.uint8),
               final_bb=np.zeros((n, 2), np.uint64))
    for ply in range(63):
        idx = np.nonzero(alive)[0]
        if idx.size == 0:
            break
        blob, cfg, explores = sides[ply % 2]
        col = oracle.c4_mcts_search(cfg, blob, my[idx], op[idx], explores, nn_mode=nn_mode, net=net)["best_action"]
        out["moves"][idx, ply] = col
        my[idx], op[idx], over, w = match.step(my[idx], op[idx], col)
        out["plies"][idx] += 1
        first_moved = ply % 2 == 0
        out["rewards"][idx[over & w]] = 1.0 if first_moved else -1.0
        done = idx[over]
        out["final_bb"][done, 0] = op[done] if first_moved else my[done]   # (after the move the mover's stones are `op`)
        out["final_bb"][done, 1] = my[done] if first_moved else op[done]
        alive[done] = False
    return out


def assert_games_equal(got, want, what, n=None):
    for k in KEYS:
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


def with_weights(player, blob):
    from dataclasses import replace

    return replace(player, weights=blob)


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
def expected_ab(oracle, blobs, openings):
    """A (first) against B on the 100 openings, from the oracle: computed once, shared, never modified"""
    return oracle_match(oracle, oracle_sides(*blobs), *openings)


@pytest.fixture(scope="module")
def engine32():
    import synthesis_amd as sa

    eng = sa.Engine(concurrent_games=32, max_explores=64)
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def engine16():
    import synthesis_amd as sa

    eng = sa.Engine(concurrent_games=16, max_explores=64)
    yield eng
    eng.close()


def test_match_is_the_oracles_games_move_for_move(engine32, oracle, blobs, openings, expected_ab):
    from synthesis_amd import arena

    pa, pb = device_players()
    got = engine32.match_run(pa, pb, blobs[0], blobs[1], *openings)     # (the engine holds no network of its own: it needs none)
    assert_games_equal(got, expected_ab, "device match vs oracle")
    assert got["plies"].min() >= 1 and (got["moves"][np.arange(100), got["plies"] - 1] < 9).all()
    assert ((got["moves"] != 255).sum(axis=1) == got["plies"]).all()
    assert engine32.last_kernel_ms() > 0.0
    host = arena.host_match(engine32, with_weights(pa, blobs[0]), with_weights(pb, blobs[1]), *openings)
    assert_games_equal(host, expected_ab, "host path vs oracle")
    assert_games_equal(got, host, "device match vs host path")


def test_empty_board_game_is_eval_against_old(engine32, oracle, blobs):
    """evaluator.rs:129-160: one policy configuration for both sides, from the empty board, both colours"""
    import synthesis_amd as sa
    from synthesis_amd import match
    from tests.oracle_lib import parity_mcts_config

    z = np.zeros(1, np.uint64)
    for first, second in ((blobs[0], blobs[1]), (blobs[1], blobs[0])):
        p = match.Player("net", 40, sa.parity_mcts_config())
        got = engine32.match_run(p, p, first, second, z, z)
        r, moves = oracle.c4_eval_against_old(parity_mcts_config(), 40, first, second, nn_mode=oracle.ACC_FMA)
        assert got["plies"][0] == moves.size and np.array_equal(got["moves"][0, :moves.size], moves) and got["rewards"][0] == r
        rec = {}
        reward, plies = match.play_match(engine32, with_weights(p, first), with_weights(p, second), 1, record=rec)
        assert plies[0] == got["plies"][0] and reward[0] == got["rewards"][0] and np.array_equal(rec["moves"], got["moves"])


def test_both_networks_really_play(engine32, oracle, blobs, openings, expected_ab):
    """Openings chosen on the CPU, with the oracle, where the two networks' first moves differ under the first player's settings: there
    a match that searched both sides with one network, or gave the sides each other's network, plays another first move."""
    pa, pb = device_players()
    a, b = blobs
    cfg_first = oracle_sides(a, b)[0][1]
    first_a = oracle.c4_mcts_search(cfg_first, a, *openings, A_EXPLORES, nn_mode=oracle.ACC_FMA)["best_action"]
    first_b = oracle.c4_mcts_search(cfg_first, b, *openings, A_EXPLORES, nn_mode=oracle.ACC_FMA)["best_action"]
    chosen = np.nonzero(first_a != first_b)[0]
    assert chosen.size >= 5, "the two golden checkpoints agree on (nearly) every opening: choose other openings"
    my, op = openings
    ab = engine32.match_run(pa, pb, a, b, my, op)
    ba = engine32.match_run(pa, pb, b, a, my, op)
    aa = engine32.match_run(pa, pb, a, a, my, op)
    bb = engine32.match_run(pa, pb, b, b, my, op)
    assert_games_equal(ab, expected_ab, "A vs B")
    assert np.array_equal(ab["moves"][chosen, 0], first_a[chosen]) and np.array_equal(aa["moves"][chosen, 0], first_a[chosen])
    assert np.array_equal(ba["moves"][chosen, 0], first_b[chosen]) and np.array_equal(bb["moves"][chosen, 0], first_b[chosen])
    assert games_differ(ab, ba) >= chosen.size          # swapping the blobs changes every chosen game (and at least one: the issue's bar)
    assert games_differ(ab, aa) >= 1 and games_differ(ab, bb) >= chosen.size and games_differ(aa, bb) >= chosen.size
    # the second player's network matters as well: A vs A and A vs B share every first move and still part ways
    assert np.array_equal(ab["moves"][:, 0], aa["moves"][:, 0])


def test_nothing_leaks_into_or_out_of_the_engine(oracle, blobs, openings, expected_ab, monkeypatch):
    """An engine with a policy cache that holds a THIRD network: its evaluations and one search give the same bits before and after a
    match, the cache still answers from that network's entries, and the match's games are those of an engine without a cache. The
    lane-per-tree kernel is forced (small engines run the row kernels, which never use the cache); the searched positions are the
    match's own openings, so an entry the match had written or read would be one of theirs."""
    import synthesis_amd as sa
    from tests.oracle_lib import parity_mcts_config

    monkeypatch.setenv("SYN_DEBUG", "1")   # developer knobs are honoured only with SYN_DEBUG=1
    monkeypatch.setenv("SYN_LANES", "4")
    pa, pb = device_players()
    third = np.random.RandomState(11).normal(0.0, 0.2, blobs[0].size).astype(np.float32)
    my, op = openings
    cfg = sa.parity_mcts_config()
    with sa.Engine(concurrent_games=64, max_explores=64, policy_cache_log2=16) as eng:
        eng.load_weights(third)
        ev0 = eng.policy_eval(my, op)
        s0 = eng.mcts_search(cfg, my, op, 32)
        assert eng.last_launch_shape()[0] == 4 and eng.last_cache_stats()[1] > 0      # the cache is in use: misses were inserted
        s0b = eng.mcts_search(cfg, my, op, 32)
        hits_before = eng.last_cache_stats()[0]
        assert hits_before > 0
        got = eng.match_run(pa, pb, blobs[0], blobs[1], my, op)
        assert eng.last_launch_shape()[0] == 4 and eng.last_cache_stats() == (0, 0)
        ev1 = eng.policy_eval(my, op)
        s1 = eng.mcts_search(cfg, my, op, 32)
        # the table still answers (it was not emptied). How many lookups hit is not a fixed number — trees of one launch race for each
        # other's fresh entries — so the check of WHAT it answers is the bits below: an entry of the match's networks would change them
        assert eng.last_cache_stats()[0] > 0
        for x, y in zip(ev0, ev1):
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
        for k in s0:
            for before in (s0, s0b):
                assert np.array_equal(np.asarray(before[k]).view(np.uint32), np.asarray(s1[k]).view(np.uint32)), k
        ref = oracle.c4_mcts_search(parity_mcts_config(), third, my, op, 32, nn_mode=oracle.ACC_FMA)
        assert np.array_equal(s1["child_N"], ref["child_N"]) and np.array_equal(s1["best_action"], ref["best_action"])
    with sa.Engine(concurrent_games=64, max_explores=64) as plain:
        assert_games_equal(got, plain.match_run(pa, pb, blobs[0], blobs[1], my, op), "engine with a cache vs engine without")
    assert_games_equal(got, expected_ab, "match on the lane-per-tree kernel vs oracle")


@pytest.mark.parametrize("n", [0, 1, 17, 100])
def test_game_counts_on_a_16_slot_engine(engine16, blobs, openings, expected_ab, n):
    pa, pb = device_players()
    got = engine16.match_run(pa, pb, blobs[0], blobs[1], openings[0][:n], openings[1][:n])
    assert got["rewards"].shape == (n,) and got["moves"].shape == (n, 63) and got["final_bb"].shape == (n, 2)
    assert_games_equal(got, expected_ab, f"{n} games", n=n)


def test_timing_counts_four_launches_per_ply(engine32, blobs, openings, expected_ab):
    """syn_last_timing's documented count for a match: every ply has one group, so one search, one advance and the regroup's count and
    scatter — four launches for every ply the longest game lasted"""
    pa, pb = device_players()
    got = engine32.match_run(pa, pb, blobs[0], blobs[1], openings[0][:17], openings[1][:17])
    assert_games_equal(got, expected_ab, "17 games", n=17)
    ms, launches = engine32.last_timing()
    assert ms > 0.0
    assert launches == 4 * int(got["plies"].max())


def pattern_board():
    """A full 9x7 board without four in a row: cell (row, col) belongs to side (col // 2 + row) % 2 — columns alternate row by row,
    rows run in pairs, both diagonals read 0110 / 0011. Returns the two sides' bitboards."""
    side = [0, 0]
    for col in range(9):
        for row in range(7):
            side[(col // 2 + row) % 2] |= 1 << (row + 7 * col)
    return side


def special_starts(expected_ab, openings):
    """(my, op, what) of hand-made and harvested starts, `first` to move in each"""
    from synthesis_amd import arena, match

    starts = []
    # one move from a win: first has the bottom row of columns 0..2, column 3 wins
    starts.append((0b1 | 1 << 7 | 1 << 14, 0b10 | 1 << 8 | 1 << 15, "one move from a win"))
    # ... and one move from losing: the OPPONENT threatens it (first must block, or loses at ply 2)
    starts.append((0b10 | 1 << 8 | 1 << 56, 0b1 | 1 << 7 | 1 << 14, "must block"))
    s = pattern_board()
    top = 1 << (6 + 7 * 8)
    mine = (8 // 2 + 6) % 2
    starts.append((s[mine] & ~top, s[1 - mine], "one free cell: a draw at ply 1"))
    cols01 = (1 << 14) - 1
    starts.append((s[0] & cols01, s[1] & cols01, "two full columns"))
    cols = ((1 << 7) - 1) | (((1 << 7) - 1) << 28) | (((1 << 7) - 1) << 56)
    starts.append((s[1] & cols, s[0] & cols, "three full columns, apart"))
    # the tails of the oracle's A-first games: `first` = A is to move after an even number of plies, and the rest of the game is the
    # game's own rest, so a start taken r plies before the end ends at ply r (odd distances: B's turn in the original; the oracle says)
    my0, op0 = openings
    for g in range(24):
        my, op = np.array([my0[g]], np.uint64), np.array([op0[g]], np.uint64)
        p = int(expected_ab["plies"][g])
        for j in range(p):
            if p - j <= 12:
                starts.append((int(my[0]), int(op[0]), f"game {g}, {p - j} plies before its end"))
            my, op, _, _ = match.step(my, op, expected_ab["moves"][g, j:j + 1].astype(np.int64))
    for plies, seed in ((3, 8), (5, 9), (6, 10)):   # odd and even stone counts
        m, o = arena.random_openings(6, plies, seed)
        starts += [(int(a), int(b), f"{plies}-ply opening") for a, b in zip(m, o)]
    return (np.array([s[0] for s in starts], np.uint64), np.array([s[1] for s in starts], np.uint64), [s[2] for s in starts])


@pytest.fixture(scope="module")
def special(oracle, blobs, openings, expected_ab):
    my, op, what = special_starts(expected_ab, openings)
    return my, op, what, oracle_match(oracle, oracle_sides(*blobs), my, op)


def test_special_starts(engine16, blobs, special):
    """wins in one, a forced draw at ply 1, full columns, odd and even stone counts, games of every length from 1 ply up in one call"""
    pa, pb = device_players()
    my, op, what, want = special
    assert want["plies"][0] == 1 and want["rewards"][0] == 1.0, what[0]
    assert want["plies"][2] == 1 and want["rewards"][2] == 0.0 and want["final_bb"][2].sum() == (1 << 63) - 1, what[2]
    assert set(range(1, 11)) <= set(want["plies"].tolist()), "the starts do not end at every ply from 1 to 10"
    assert {bin(int(a | b)).count("1") % 2 for a, b in zip(my, op)} == {0, 1}
    got = engine16.match_run(pa, pb, blobs[0], blobs[1], my, op)
    assert_games_equal(got, want, "special starts")


def test_compaction_at_every_live_count_down_to_one(engine16, blobs, special):
    """K starts that end after 1, 2, ..., K plies, one each: the live set shrinks by exactly one game per ply, K, K - 1, ..., 1, in
    an order of game indices that is not the order of ending."""
    pa, pb = device_players()
    my, op, _, want = special
    pick = []
    for r in range(1, 64):
        idx = np.nonzero(want["plies"] == r)[0]
        if idx.size == 0:
            break
        pick.append(int(idx[0]))
    assert len(pick) >= 10
    order = np.array(pick)[np.random.RandomState(1).permutation(len(pick))]
    got = engine16.match_run(pa, pb, blobs[0], blobs[1], my[order], op[order])
    assert sorted(got["plies"].tolist()) == list(range(1, len(pick) + 1))
    assert_games_equal(got, {k: want[k][order] for k in KEYS}, "one game ends per ply")


def test_refusals_leave_the_next_match_identical(engine32, blobs, openings, expected_ab):
    import synthesis_amd as sa
    from synthesis_amd import match

    pa, pb = device_players()
    a, b = blobs
    my, op = openings[0][:17].copy(), openings[1][:17].copy()
    s = pattern_board()

    def refused(code, first=pa, second=pb, blob_first=a, blob_second=b, start_my=my, start_op=op):
        with pytest.raises(sa.SynthesisAmdError) as e:
            engine32.match_run(first, second, blob_first, blob_second, start_my, start_op)
        assert e.value.code == code, str(e.value)
        assert_games_equal(engine32.match_run(pa, pb, a, b, my, op), expected_ab, "match after a refusal", n=17)

    INVALID, UNSUPPORTED, CAPACITY = -1, -5, -6
    won_start = my.copy(); won_op = op.copy()
    won_start[9], won_op[9] = 0b1111, 0b1110000000                       # the side to move already has four in a column
    refused(INVALID, start_my=won_start, start_op=won_op)
    won_start[9], won_op[9] = 0b1110000000, 0b1111                       # ... or the other side has
    refused(INVALID, start_my=won_start, start_op=won_op)
    floating = my.copy(); floating[16] |= np.uint64(1 << (5 + 7 * 8))    # a stone in the air above column 8
    refused(INVALID, start_my=floating)
    full_my, full_op = my.copy(), op.copy()
    full_my[0], full_op[0] = s[0], s[1]                                  # no free column
    refused(INVALID, start_my=full_my, start_op=full_op)
    refused(INVALID, blob_first=a[:12412], blob_second=b[:12412])        # Connect4ConvNet's size on a Connect4Net engine
    refused(INVALID, blob_first=a[:-1], blob_second=b[:-1])
    normal = match.Player("n", A_EXPLORES, sa.MCTSConfig(fpu=sa.Fpu.Func, fpu_value=1.0, fpu_std=0.1))          # SYN_FPU_NORMAL
    refused(UNSUPPORTED, first=normal)
    refused(UNSUPPORTED, second=normal)
    dirichlet = match.Player("d", B_EXPLORES, sa.MCTSConfig(root_policy_noise=sa.PolicyNoise.Dirichlet, noise_alpha=0.3, noise_weight=0.25))
    refused(UNSUPPORTED, second=dirichlet)
    refused(CAPACITY, first=match.Player("deep", 65, sa.MCTSConfig(c=A_C)))   # the engine's max_explores is 64
    refused(CAPACITY, second=match.Player("deep", 65, sa.MCTSConfig(c=B_C)))


def test_f16x2_blob_without_a_plan_is_refused_before_anything_changes(blobs, openings, expected_ab, oracle):
    import synthesis_amd as sa

    pa, pb = device_players()
    a, b = blobs
    my, op = openings[0][:9], openings[1][:9]     # (the oracle's f16x2 network costs seconds per hundred games)
    bad = a.copy(); bad[5] = np.inf
    with sa.Engine(concurrent_games=32, max_explores=64) as eng:
        eng.load_weights(b)
        eng.set_network_arithmetic("f16x2")
        before = eng.policy_eval(my, op)
        with pytest.raises(sa.SynthesisAmdError) as e:
            eng.match_run(pa, pb, a, bad, my, op)
        assert e.value.code == -5
        after = eng.policy_eval(my, op)
        assert all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(before, after))
        want = oracle_match(oracle, oracle_sides(a, b), my, op, nn_mode=oracle.ACC_F16X2)
        assert_games_equal(eng.match_run(pa, pb, a, b, my, op), want, "f16x2 match after a refusal")


@pytest.mark.parametrize("net,arithmetic,n", [("conv", "f32", 100), ("mlp", "f16x2", 40), ("conv", "f16x2", 100)])
def test_other_network_and_arithmetic(oracle, blobs, openings, net, arithmetic, n):
    """The oracle comparison for Connect4ConvNet, and for Connect4Net in the f16x2 arithmetic (the oracle's ACC_F16X2, as the f16x2
    search tests use it); both also against the host path under the same network and arithmetic. (f16x2: 40 openings, still more than
    the engine's 32 slots — the oracle's f16x2 network is the slow part of this test.) Connect4ConvNet in f16x2 has no oracle mode
    (its searches are held to a CPU model elsewhere, tests/test_gpu_conv_f16x2.py): that case is held to the host path alone."""
    openings = (openings[0][:n], openings[1][:n])
    import synthesis_amd as sa
    from bench import make_conv_weights
    from synthesis_amd import arena

    pa, pb = device_players()
    a, b = (make_conv_weights(), make_conv_weights(seed=7)) if net == "conv" else blobs
    nn_mode = oracle.ACC_F16X2 if arithmetic == "f16x2" else oracle.ACC_FMA
    want = None if (net, arithmetic) == ("conv", "f16x2") else oracle_match(oracle, oracle_sides(a, b), *openings, nn_mode=nn_mode, net=net)
    with sa.Engine(concurrent_games=32, max_explores=64) as eng:
        if net == "conv":
            eng.load_weights_conv(b)     # the engine's network kind is the kind of the blobs a match takes
        eng.set_network_arithmetic(arithmetic)
        got = eng.match_run(pa, pb, a, b, *openings)
        if want is not None:
            assert_games_equal(got, want, f"{net} {arithmetic}: device match vs oracle")
        host = arena.host_match(eng, with_weights(pa, a), with_weights(pb, b), *openings)
        assert_games_equal(got, host, f"{net} {arithmetic}: device match vs host path")
        swapped = eng.match_run(pa, pb, b, a, *openings)
        assert games_differ(got, swapped) >= 1
