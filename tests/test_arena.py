"""CPU-only tests of the arena's host side (synthesis_amd/arena.py): the openings, the statistics on hand-made result vectors against
closed-form values, the order in which `compare` gives the colours, and the header <-> ctypes layout of syn_match_player."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def popcount(a):
    return np.array([bin(int(x)).count("1") for x in np.asarray(a).ravel()])


def reachable(my, op):
    """disjoint, inside the 63 cells, every column filled from the bottom"""
    occ = int(my) | int(op)
    if int(my) & int(op) or occ >> 63:
        return False
    return all(((occ >> (7 * c)) & 0x7F) & (((occ >> (7 * c)) & 0x7F) + 1) == 0 for c in range(9))


@pytest.mark.parametrize("plies", [3, 4, 7])
def test_random_openings_properties(plies):
    from synthesis_amd import arena, match

    n = 100
    my, op = arena.random_openings(n, plies, seed=5)
    assert my.dtype == np.uint64 and op.dtype == np.uint64 and my.shape == (n,) and op.shape == (n,)
    # `plies` stones, the side to move has the smaller half
    assert (popcount(my) == plies // 2).all() and (popcount(op) == plies - plies // 2).all()
    assert all(reachable(a, b) for a, b in zip(my, op))
    assert not match.won(my).any() and not match.won(op).any()
    # pairwise distinct up to the left-right mirror
    keys = set()
    for a, b, ma, mb in zip(my, op, arena.mirror(my), arena.mirror(op)):
        keys.add(min((int(a), int(b)), (int(ma), int(mb))))
    assert len(keys) == n
    # deterministic in the seed, and the seed matters
    my2, op2 = arena.random_openings(n, plies, seed=5)
    assert np.array_equal(my, my2) and np.array_equal(op, op2)
    my3, op3 = arena.random_openings(n, plies, seed=6)
    assert not (np.array_equal(my, my3) and np.array_equal(op, op3))
    # a prefix request is a prefix of the answer only by accident of the round size: it is the SEED AND N that name a set
    assert arena.random_openings(0, plies, seed=5)[0].shape == (0,)


def test_mirror_is_the_column_reversal():
    from synthesis_amd import arena

    bb = np.array([1 << (2 + 7 * 1), (1 << 0) | (1 << (6 + 7 * 8)), 0x7F << 28], np.uint64)
    want = np.array([1 << (2 + 7 * 7), (1 << (7 * 8)) | (1 << 6), 0x7F << 28], np.uint64)
    assert np.array_equal(arena.mirror(bb), want)
    assert np.array_equal(arena.mirror(arena.mirror(bb)), bb)


def test_random_openings_raise_when_the_depth_has_too_few_positions():
    from synthesis_amd import arena

    # one ply: nine positions, five up to mirror
    my, op = arena.random_openings(5, 1, seed=0)
    assert sorted(popcount(op)) == [1] * 5 and (my == 0).all()
    with pytest.raises(ValueError, match="distinct openings"):
        arena.random_openings(6, 1, seed=0)
    with pytest.raises(ValueError):
        arena.random_openings(3, 63, seed=0)


def test_pair_statistics_closed_form():
    from synthesis_amd import arena

    # opening:            0    1    2    3
    r_a_first = np.array([1, 1, 0, -1], np.float32)     # A's games as first mover: win, win, draw, loss
    r_b_first = np.array([-1, 1, 0, 1], np.float32)     # B's reward as first mover: A wins, loses, draws, loses
    s = arena.pair_statistics(r_a_first, r_b_first)
    assert np.array_equal(s["pair_scores"], [1.0, 0.5, 0.5, 0.0])
    assert (s["wins"], s["draws"], s["losses"], s["openings"]) == (3, 2, 3, 4)
    assert s["score"] == 0.5 and s["elo"] == 0.0
    se = math.sqrt((0.25 + 0.0 + 0.0 + 0.25) / 3.0) / 2.0
    assert s["se"] == pytest.approx(se, rel=1e-12)
    lo, hi = 0.5 - 1.96 * se, 0.5 + 1.96 * se
    assert s["score_lo"] == pytest.approx(lo, rel=1e-12) and s["score_hi"] == pytest.approx(hi, rel=1e-12)
    assert s["elo_lo"] == pytest.approx(-400.0 * math.log10(1.0 / lo - 1.0), rel=1e-12)
    assert s["elo_hi"] == pytest.approx(-s["elo_lo"], rel=1e-9)

    # every quarter value of a pair score
    q = arena.pair_statistics([1, 1, 0, -1, -1], [0, 1, 0, 0, 1])
    assert np.array_equal(q["pair_scores"], [0.75, 0.5, 0.5, 0.25, 0.0])
    assert q["score"] == pytest.approx(0.4) and q["elo"] == pytest.approx(-400.0 * math.log10(1.0 / 0.4 - 1.0))

    # a clean sweep: no spread, the Elo is the clipped one of match.score
    w = arena.pair_statistics(np.ones(10), -np.ones(10))
    assert w["score"] == 1.0 and w["se"] == 0.0 and (w["wins"], w["draws"], w["losses"]) == (20, 0, 0)
    clipped = -400.0 * math.log10(1.0 / 0.999 - 1.0)
    assert w["elo"] == pytest.approx(clipped) and w["elo_lo"] == pytest.approx(clipped) and w["elo_hi"] == pytest.approx(clipped)
    from synthesis_amd import match
    assert match.score(np.ones(10))[4] == pytest.approx(w["elo"])
    # an interval that leaves [0, 1] is clipped too
    x = arena.pair_statistics([1, 1, 1, 0], [-1, -1, -1, -1])
    assert x["score_hi"] > 1.0 and x["elo_hi"] == pytest.approx(clipped)
    # one opening has no error bar
    one = arena.pair_statistics([1], [0])
    assert one["pair_scores"][0] == 0.75 and math.isnan(one["se"]) and math.isnan(one["elo_lo"])
    with pytest.raises(ValueError):
        arena.pair_statistics([1, 0], [1])


def test_compare_plays_each_colour_in_one_call():
    from synthesis_amd import arena

    calls = []

    class FakeEngine:
        def match_run(self, first, second, blob_first, blob_second, start_my, start_op):
            calls.append((first, second, blob_first, blob_second, tuple(start_my), tuple(start_op)))
            r = np.array([1, 0, -1], np.float32) if len(calls) == 1 else np.array([1, 1, -1], np.float32)
            return dict(rewards=r, plies=np.array([7, 8, 9], np.int32) + len(calls))

    my, op = np.array([1, 2, 3], np.uint64), np.array([4, 5, 6], np.uint64)
    out = arena.compare(FakeEngine(), "blobA", "blobB", (my, op), "playerA", "playerB")
    assert calls == [("playerA", "playerB", "blobA", "blobB", (1, 2, 3), (4, 5, 6)),
                     ("playerB", "playerA", "blobB", "blobA", (1, 2, 3), (4, 5, 6))]
    assert np.array_equal(out["pair_scores"], [0.5, 0.25, 0.5])
    assert (out["wins"], out["draws"], out["losses"]) == (2, 1, 3)
    assert np.array_equal(out["plies_a_first"], [8, 9, 10]) and np.array_equal(out["plies_b_first"], [9, 10, 11])


def test_match_player_layout_matches_the_header():
    from synthesis_amd.config import CMctsConfig
    from synthesis_amd.engine import ABI_SYMBOLS, CMatchPlayer

    h = open(os.path.join(ROOT, "include", "synthesis_amd.h")).read()
    body = re.search(r"typedef struct syn_match_player \{(.*?)\} syn_match_player;", h, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    decls = [d.split() for d in body.split(";") if d.strip()]
    assert decls == [["int32_t", "explores"], ["int32_t", "action"], ["syn_mcts_config", "mcts_cfg"]]
    assert [f[0] for f in CMatchPlayer._fields_] == [d[1] for d in decls]
    assert [f[1] for f in CMatchPlayer._fields_] == [C.c_int32, C.c_int32, CMctsConfig]
    # (syn_mcts_config holds a function pointer: 8-byte alignment, no padding after two int32)
    assert (CMatchPlayer.explores.offset, CMatchPlayer.action.offset, CMatchPlayer.mcts_cfg.offset) == (0, 4, 8)
    assert C.sizeof(CMatchPlayer) == 8 + C.sizeof(CMctsConfig) == 64
    # the prototype, argument for argument
    proto = re.search(r"int syn_match_run\((.*?)\);", h, re.S).group(1)
    args = [re.sub(r"\s+", " ", a).strip() for a in proto.split(",")]
    assert args == ["syn_engine* h", "const syn_match_player* first", "const syn_match_player* second", "const float* blob_first",
                    "const float* blob_second", "size_t n_floats", "const uint64_t* start_my", "const uint64_t* start_op", "int n_games",
                    "float* rewards", "int32_t* plies", "uint8_t* moves", "uint64_t* final_bb"]
    assert "syn_match_run" in ABI_SYMBOLS
    from synthesis_amd.engine import load_library

    lib = load_library()
    assert len(lib.syn_match_run.argtypes) == len(args)
    assert lib.syn_match_run.argtypes[1]._type_ is CMatchPlayer and lib.syn_match_run.argtypes[5] is C.c_size_t
