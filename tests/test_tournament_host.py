"""Host-side checks of the tournament (syn_tournament_run, arena.tournament / round_robin / gauntlet / ratings): the schedule builders,
the Bradley-Terry fit against closed forms, its refusals, the bootstrap, and the header / ctypes / ABI_SYMBOLS agreement. No device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_text():
    return open(os.path.join(ROOT, "include", "synthesis_amd.h")).read()


# ---- schedule builders
def test_schedule_has_each_pair_once_per_colour_and_opening():
    from synthesis_amd import arena

    for pairs, k in ((arena.round_robin_pairs(5), 5), (arena.gauntlet_pairs(3, 2), 5), ([(2, 0)], 3)):
        sch = arena.schedule(pairs, 7, k)
        n = 2 * len(pairs) * 7
        assert all(sch[f].shape == (n,) for f in ("first", "second", "opening", "pair", "a_first"))
        assert sch["first"].dtype == np.int32 and sch["second"].dtype == np.int32
        assert sch["first"].min() >= 0 and sch["second"].min() >= 0 and max(sch["first"].max(), sch["second"].max()) < k
        games = sorted(zip(sch["first"].tolist(), sch["second"].tolist(), sch["opening"].tolist()))
        want = sorted([(a, b, o) for a, b in pairs for o in range(7)] + [(b, a, o) for a, b in pairs for o in range(7)])
        assert games == want and len(set(games)) == n
        for g in range(n):   # the bookkeeping of a game agrees with its players
            a, b = sch["pairs"][sch["pair"][g]]
            assert (sch["first"][g], sch["second"][g]) == ((a, b) if sch["a_first"][g] else (b, a))
        assert np.array_equal(sch["opening"], np.repeat(np.arange(7), 2 * len(pairs)))   # interleaved by opening, not grouped by pairing
        again = arena.schedule(pairs, 7, k)
        assert all(np.array_equal(sch[f], again[f]) for f in ("first", "second", "opening", "pair", "a_first"))
    assert arena.round_robin_pairs(4) == [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
    assert arena.gauntlet_pairs(2, 2) == [(0, 2), (0, 3), (1, 2), (1, 3)]
    for bad in ([(0, 0)], [(0, 1), (1, 0)], [(0, 5)], [(-1, 0)]):
        with pytest.raises(ValueError):
            arena.schedule(bad, 3, 4)


def test_tournament_is_one_call_and_splits_the_rewards_by_pair():
    from synthesis_amd import arena

    calls = []

    class FakeEngine:
        def tournament_run(self, players, first, second, start_my, start_op, seeds=None):
            calls.append((players, np.array(first), np.array(second), np.array(start_my), np.array(start_op), seeds))
            # a game's reward names it: + for the lower index moving first
            r = np.where(np.asarray(first) < np.asarray(second), 1.0, 0.0).astype(np.float32)
            return dict(rewards=r, plies=np.asarray(first, np.int32) * 10 + np.asarray(second, np.int32))

    my, op = np.array([1, 2, 3], np.uint64), np.array([128, 256, 384], np.uint64)
    players = ["p0", "p1", "p2"]
    res = arena.round_robin(FakeEngine(), players, (my, op), seeds=[5, 6, 7])
    assert len(calls) == 1 and calls[0][0] is players
    assert np.array_equal(calls[0][3], np.repeat(my, 6)) and np.array_equal(calls[0][4], np.repeat(op, 6))
    assert np.array_equal(calls[0][5], np.repeat(np.array([5, 6, 7], np.uint64), 6)) and calls[0][5].dtype == np.uint64
    assert res["pairs"] == [(0, 1), (0, 2), (1, 2)] and res["n_players"] == 3
    for (a, b), st in res["stats"].items():
        want = arena.pair_statistics(np.ones(3), np.zeros(3))
        assert st["score"] == want["score"] == 0.75 and (st["wins"], st["draws"], st["losses"]) == (3, 3, 0)
        assert np.array_equal(st["plies_a_first"], [a * 10 + b] * 3) and np.array_equal(st["plies_b_first"], [b * 10 + a] * 3)
    g = arena.gauntlet(FakeEngine(), ["c0", "c1"], ["a0"], (my, op))
    assert calls[1][0] == ["c0", "c1", "a0"] and g["pairs"] == [(0, 2), (1, 2)] and calls[1][5] is None


# ---- ratings
def test_ratings_of_two_players_are_the_closed_form():
    from synthesis_amd import arena

    r1 = np.array([1, 1, 0, -1, 1, 1, 0, 1], np.float32)
    r2 = np.array([-1, 1, 0, 1, -1, 0, 0, -1], np.float32)
    st = arena.pair_statistics(r1, r2)
    res = dict(n_players=2, pairs=[(0, 1)], stats={(0, 1): st})
    out = arena.ratings(res, anchor=1, bootstrap=0)
    assert out["elo"][1] == 0.0 and abs(out["elo"][0] - arena.elo(st["score"])) < 1e-6
    s = st["score"]
    assert out["gamma"][0] / out["gamma"][1] == pytest.approx(s / (1 - s), rel=1e-9)
    assert out["score"][(0, 1)] == pytest.approx(s, rel=1e-15)
    # results_from_pair_scores restates what ratings reads
    out2 = arena.ratings(arena.results_from_pair_scores(2, {(0, 1): st["pair_scores"]}), anchor=1, bootstrap=0)
    assert np.array_equal(out2["elo"], out["elo"])


def test_ratings_recover_four_players_from_their_expected_scores():
    from synthesis_amd import arena

    true = np.array([0.0, 120.0, -75.0, 310.0])
    gam = 10.0 ** (true / 400.0)
    n = 64
    scores = {}
    for a, b in arena.round_robin_pairs(4):
        if (a, b) == (0, 3):
            continue   # an incomplete round-robin: still connected
        scores[(a, b)] = np.full(n, gam[a] / (gam[a] + gam[b]))   # the exact Bradley-Terry expectation, every opening
    out = arena.ratings(arena.results_from_pair_scores(4, scores), anchor=0, bootstrap=0)
    assert np.abs(out["elo"] - true).max() < 1e-6, out["elo"]
    # another anchor shifts every rating by one constant
    for anchor in (1, 2, 3):
        shifted = arena.ratings(arena.results_from_pair_scores(4, scores), anchor=anchor, bootstrap=0)
        assert shifted["elo"][anchor] == 0.0
        assert np.abs((shifted["elo"] - out["elo"]) - (shifted["elo"][0] - out["elo"][0])).max() < 1e-6
        assert abs((shifted["elo"][0] - out["elo"][0]) + true[anchor]) < 1e-6


def test_ratings_refuse_what_has_no_finite_maximum():
    from synthesis_amd import arena

    n = 16
    loser = arena.results_from_pair_scores(3, {(0, 1): np.full(n, 0.5), (0, 2): np.ones(n), (1, 2): np.ones(n)})
    with pytest.raises(ValueError, match="player 2"):
        arena.ratings(loser, bootstrap=0)
    fit = arena.ratings(loser, prior_draws=1.0, bootstrap=0)
    assert np.isfinite(fit["elo"]).all() and fit["elo"][2] < -400 and abs(fit["elo"][0] - fit["elo"][1]) < 1e-6
    winner = arena.results_from_pair_scores(2, {(0, 1): np.ones(n)})
    with pytest.raises(ValueError, match="player 0"):
        arena.ratings(winner, bootstrap=0)
    apart = arena.results_from_pair_scores(5, {(0, 1): np.full(n, 0.5), (2, 3): np.full(n, 0.25), (3, 4): np.full(n, 0.5)})
    with pytest.raises(ValueError, match=r"not connected.*\[0, 1\]"):
        arena.ratings(apart, prior_draws=1.0, bootstrap=0)
    with pytest.raises(ValueError, match="anchor"):
        arena.ratings(winner, anchor=2, prior_draws=1.0)


def test_bootstrap_intervals():
    from synthesis_amd import arena

    rng = np.random.default_rng(5)
    n = 4096
    r1 = rng.choice([1.0, 0.0, -1.0], size=n, p=[0.5, 0.2, 0.3])
    r2 = rng.choice([1.0, 0.0, -1.0], size=n, p=[0.35, 0.25, 0.4])
    st = arena.pair_statistics(r1, r2)
    res = dict(n_players=2, pairs=[(0, 1)], stats={(0, 1): st})
    a = arena.ratings(res, anchor=1, bootstrap=400, seed=3)
    b = arena.ratings(res, anchor=1, bootstrap=400, seed=3)
    c = arena.ratings(res, anchor=1, bootstrap=400, seed=4)
    assert np.array_equal(a["elo_lo"], b["elo_lo"]) and np.array_equal(a["elo_hi"], b["elo_hi"])
    assert not np.array_equal(a["elo_lo"], c["elo_lo"])
    assert (a["elo_lo"] <= a["elo"]).all() and (a["elo"] <= a["elo_hi"]).all() and a["elo_lo"][0] < a["elo_hi"][0]
    assert a["elo_lo"][1] == a["elo_hi"][1] == 0.0
    # the bootstrap's own relative error is 1 / sqrt(2 * 400) = 3.5 %: 15 % is more than four of those
    sd = a["score_sd"][(0, 1)]
    print(f"bootstrap sd {sd:.6f}, pair_statistics se {st['se']:.6f}, ratio {sd / st['se']:.4f}")
    assert abs(sd / st["se"] - 1.0) < 0.15
    # three players: the same resampled openings for every pair (a pair resampled on its own would not reproduce this)
    sc = {(0, 1): st["pair_scores"], (1, 2): 1.0 - st["pair_scores"], (0, 2): np.full(n, 0.5)}
    three = arena.ratings(arena.results_from_pair_scores(3, sc), bootstrap=50, seed=1)
    assert abs(three["score_sd"][(0, 1)] - three["score_sd"][(1, 2)]) < 1e-15 and three["score_sd"][(0, 2)] == 0.0
    assert (three["elo_lo"] <= three["elo"] + 1e-9).all() and (three["elo"] <= three["elo_hi"] + 1e-9).all()
    with pytest.raises(ValueError, match="same openings"):
        arena.ratings(arena.results_from_pair_scores(3, {(0, 1): np.full(4, 0.5), (1, 2): np.full(5, 0.5)}))


# ---- ABI
def test_the_symbols_are_declared_listed_and_typed():
    from synthesis_amd import engine as E

    h = header_text()
    declared = set(re.findall(r"\b(syn_[a-z0-9_]+)\s*\(", h))
    for name in ("syn_tournament_run", "syn_debug_tournament_regroup"):
        assert name in declared and name in E.ABI_SYMBOLS
    assert re.search(r"#define SYN_TOURNAMENT_MAX_PLAYERS 64\b", h) and E.TOURNAMENT_MAX_PLAYERS == 64
    decl = re.search(r"int syn_tournament_run\((.*?)\);", h, re.S).group(1)
    decl = re.sub(r"/\*.*?\*/", "", decl, flags=re.S)
    params = [" ".join(p.split()) for p in decl.split(",")]
    assert params == ["syn_engine* h", "const syn_match_side* players", "int n_players", "const int32_t* first", "const int32_t* second",
                      "const uint64_t* start_my", "const uint64_t* start_op", "const uint64_t* seeds", "int n_games", "float* rewards",
                      "int32_t* plies", "uint8_t* moves", "uint64_t* final_bb", "uint64_t* rng_words"]
    src = open(os.path.join(ROOT, "synthesis_amd", "engine.py")).read()
    sig = re.search(r"lib\.syn_tournament_run\.argtypes = \[(.*?)\]\n", src, re.S).group(1)
    types = [t.strip() for t in sig.replace("\n", " ").split(",")]
    want = ["C.c_void_p", "C.POINTER(CMatchSide)", "C.c_int"] + ["C.c_void_p"] * 5 + ["C.c_int"] + ["C.c_void_p"] * 5
    assert types == want and len(types) == len(params)
    sig = re.search(r"lib\.syn_debug_tournament_regroup\.argtypes = \[(.*?)\]\n", src, re.S).group(1)
    assert [t.strip() for t in sig.split(",")] == ["C.c_void_p", "C.c_void_p", "C.c_int", "C.c_int", "C.c_void_p", "C.c_void_p"]
    decl = re.search(r"int syn_debug_tournament_regroup\((.*?)\);", h, re.S).group(1)
    assert [" ".join(p.split()) for p in decl.split(",")] == ["syn_engine* h", "const int32_t* keys", "int n", "int n_keys",
                                                              "int32_t* perm_out", "int32_t* seg_out"]


def test_tournament_run_reuses_match_side():
    """the players of a tournament go through Engine.match_side, unchanged: the same structs a match gets, in player order, one array"""
    import synthesis_amd as sa
    from synthesis_amd import match
    from synthesis_amd.engine import CMatchSide, Engine, decode_match_side

    blob = np.arange(30492, dtype=np.float32)
    players = [match.Player("a", 7, sa.parity_mcts_config(), weights=blob, arithmetic="f16x2"), match.vanilla_player(300),
               match.Player("b", 9, weights=blob)]
    seen = {}

    class Probe(Engine):
        def __init__(self):   # no library, no device
            pass

        def tournament_run_c(self, sides, first, second, start_my, start_op, seeds=None, n_players=None):
            seen["sides"] = sides
            return "out"

        def __del__(self):
            pass

    assert Probe().tournament_run(players, [0], [1], [0], [0], seeds=[1]) == "out"
    want = [Engine.match_side(p)[0] for p in players]
    assert [decode_match_side(s) for s in seen["sides"]] == [("network", "f16x2"), ("baseline", None), ("network", None)]
    for got, w in zip(seen["sides"], want):
        assert isinstance(got, CMatchSide) and got.player.explores == w.player.explores and got.n_floats == w.n_floats
        assert bytes(got.player) == bytes(w.player)
    with pytest.raises(ValueError, match="weights"):
        Probe().tournament_run([match.Player("net", 5)], [0], [0], [0], [0])
    assert C.sizeof(CMatchSide) == 88
