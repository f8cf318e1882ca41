"""Host-side checks of the match sides (syn_match_run_sides): the struct's layout against the header, the zero-initialisation rule, the
Python refusals that need no device, the statistics compare_baseline shares with compare, and the per-call arithmetic of the launch
selection (tests/cpp/match_sides_plan_harness.cpp, built with g++)."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_text():
    return open(os.path.join(ROOT, "include", "synthesis_amd.h")).read()


def header_fields(struct):
    """[(type, name)] of a struct of the header, in order"""
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), header_text(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return [(m.group(1).strip(), m.group(2)) for m in re.finditer(r"([A-Za-z_][A-Za-z_0-9 ]*?[ \*]+)([a-z_A-Z0-9]+);", body)]


def test_match_side_layout_is_the_headers():
    from synthesis_amd.engine import CMatchPlayer, CMatchSide

    fields = header_fields("syn_match_side")
    assert [name for _, name in fields] == [f[0] for f in CMatchSide._fields_]
    # sizeof from the header's field order: natural alignment of each member, the struct padded to its widest
    size_align = {"int32_t": (4, 4), "syn_match_player": (C.sizeof(CMatchPlayer), C.alignment(CMatchPlayer)),
                  "const float*": (C.sizeof(C.c_void_p), C.alignment(C.c_void_p)), "size_t": (C.sizeof(C.c_size_t), C.alignment(C.c_size_t))}
    at, widest = 0, 1
    for ctype, name in fields:
        size, align = size_align[ctype.replace(" *", "*")]
        at = (at + align - 1) // align * align
        assert getattr(CMatchSide, name).offset == at, name
        at += size
        widest = max(widest, align)
    assert C.sizeof(CMatchSide) == (at + widest - 1) // widest * widest == 88
    # the enums the mirror's tables restate
    h = header_text()
    assert re.search(r"SYN_MATCH_SIDE_NETWORK = 0, SYN_MATCH_SIDE_BASELINE = 1", h)
    assert re.search(r"SYN_MATCH_ARITH_ENGINE = 0, SYN_MATCH_ARITH_F32 = 1, SYN_MATCH_ARITH_F16X2 = 2", h)


def test_the_symbol_is_declared_and_listed():
    from synthesis_amd.engine import ABI_SYMBOLS

    declared = set(re.findall(r"\b(syn_[a-z0-9_]+)\s*\(", header_text()))
    assert "syn_match_run_sides" in declared and "syn_match_run_sides" in ABI_SYMBOLS and "syn_match_run" in ABI_SYMBOLS


def test_zero_filled_side_is_a_network_side_in_the_engines_arithmetic():
    from synthesis_amd.engine import MATCH_ARITHMETICS, MATCH_SIDE_KINDS, CMatchSide, decode_match_side

    side = CMatchSide()
    assert bytes(side) == bytes(C.sizeof(CMatchSide))
    assert decode_match_side(side) == ("network", None)
    assert MATCH_SIDE_KINDS == {"network": 0, "baseline": 1} and MATCH_ARITHMETICS == {None: 0, "f32": 1, "f16x2": 2}


def test_sides_from_players():
    import synthesis_amd as sa
    from synthesis_amd import match
    from synthesis_amd.engine import Engine, decode_match_side

    blob = np.arange(30492, dtype=np.float32)
    p = match.Player("net", 77, sa.parity_mcts_config(), weights=blob)
    assert p.arithmetic is None
    side, keep = Engine.match_side(p)
    assert decode_match_side(side) == ("network", None) and side.player.explores == 77 and side.n_floats == 30492 and side.blob == keep.ctypes.data
    for name in ("f32", "f16x2"):
        side, _ = Engine.match_side(match.Player("net", 5, weights=blob, arithmetic=name))
        assert decode_match_side(side) == ("network", name)
    van = match.vanilla_player(300)
    side, keep = Engine.match_side(van)
    assert decode_match_side(side) == ("baseline", None) and keep is None and not side.blob and side.player.explores == 300
    assert side.player.action == int(sa.ActionSelection.Q) and side.player.mcts_cfg.c == 2.0
    with pytest.raises(ValueError, match="arithmetic"):
        Engine.match_side(match.Player("net", 5, weights=blob, arithmetic="bf16"))
    with pytest.raises(ValueError, match="weights"):
        Engine.match_side(match.Player("net", 5))


def test_play_match_device_refuses_a_rollout_player():
    """before the engine is touched: the engine here is None"""
    from synthesis_amd import match

    van, roll = match.vanilla_player(50), match.rollout_player(50)
    for first, second in ((roll, van), (van, roll)):
        with pytest.raises(ValueError, match="keyed by ply x batch size"):
            match.play_match_device(None, first, second, 4)
    with pytest.raises(ValueError, match="n_games or starts"):
        match.play_match_device(None, van, van)


def test_play_match_device_is_one_call_with_play_matchs_seeds_and_record():
    from synthesis_amd import match

    calls = []

    class FakeEngine:
        def match_run_sides(self, first, second, start_my, start_op, seeds=None):
            calls.append((first, second, np.array(start_my), np.array(start_op), np.array(seeds)))
            n = len(start_my)
            return dict(rewards=np.arange(n, dtype=np.float32), plies=np.full(n, 9, np.int32), moves=np.full((n, 63), 3, np.uint8),
                        final_bb=np.zeros((n, 2), np.uint64), rng_words=np.arange(n, dtype=np.uint64) + np.uint64(100))

    a, b = match.vanilla_player(20), match.vanilla_player(10)
    rec = {}
    r, plies = match.play_match_device(FakeEngine(), a, b, 3, seed=7, record=rec)
    assert len(calls) == 1 and calls[0][0] is a and calls[0][1] is b
    assert np.array_equal(calls[0][2], np.zeros(3, np.uint64)) and np.array_equal(calls[0][3], np.zeros(3, np.uint64))
    assert np.array_equal(calls[0][4], [7, 8, 9]) and calls[0][4].dtype == np.uint64
    assert np.array_equal(r, [0, 1, 2]) and np.array_equal(plies, [9, 9, 9])
    assert set(rec) == {"moves", "rng_words"} and np.array_equal(rec["rng_words"], [100, 101, 102])
    my, op = np.array([1, 2], np.uint64), np.array([128, 256], np.uint64)
    match.play_match_device(FakeEngine(), a, b, starts=(my, op), seeds=[5, 5])
    assert np.array_equal(calls[1][2], my) and np.array_equal(calls[1][3], op) and np.array_equal(calls[1][4], [5, 5])
    with pytest.raises(ValueError, match="disagree"):
        match.play_match_device(FakeEngine(), a, b, 3, starts=(my, op))


def test_compare_passes_the_arithmetic_through():
    from synthesis_amd import arena, match

    calls = []

    class FakeEngine:
        def match_run(self, first, second, blob_first, blob_second, start_my, start_op):
            calls.append(("run", first, second))
            return dict(rewards=np.zeros(2, np.float32), plies=np.ones(2, np.int32))

        def match_run_sides(self, first, second, start_my, start_op, seeds=None):
            calls.append(("sides", first, second, seeds))
            return dict(rewards=np.zeros(2, np.float32), plies=np.ones(2, np.int32))

    my, op = np.array([1, 2], np.uint64), np.array([128, 256], np.uint64)
    pa, pb = match.Player("A", 30), match.Player("B", 20)
    arena.compare(FakeEngine(), "blobA", "blobB", (my, op), pa, pb)
    assert [c[0] for c in calls] == ["run", "run"]           # players without an arithmetic of their own: the call compare always made
    del calls[:]
    pa16 = match.Player("A", 30, arithmetic="f16x2")
    arena.compare(FakeEngine(), "blobA", "blobB", (my, op), pa16, pb)
    assert [c[0] for c in calls] == ["sides", "sides"]
    (_, f1, s1, _), (_, f2, s2, _) = calls
    assert (f1.arithmetic, f1.weights, f1.explores, s1.arithmetic, s1.weights, s1.explores) == ("f16x2", "blobA", 30, None, "blobB", 20)
    assert (f2.arithmetic, f2.weights, s2.arithmetic, s2.weights) == (None, "blobB", "f16x2", "blobA")   # the arithmetic follows the player
    del calls[:]
    van = match.vanilla_player(40)
    out = arena.compare_baseline(FakeEngine(), "blobA", (my, op), pa, van, [3, 4])
    assert [c[0] for c in calls] == ["sides", "sides"] and calls[0][2] is van and calls[1][1] is van and calls[0][3] == [3, 4]
    assert out["score"] == 0.5 and out["openings"] == 2


def test_pair_statistics_is_unchanged():
    """the numbers of tests/test_arena.py's closed-form case"""
    from synthesis_amd import arena

    s = arena.pair_statistics(np.array([1, 1, 0, -1], np.float32), np.array([-1, 1, 0, 1], np.float32))
    assert np.array_equal(s["pair_scores"], [1.0, 0.5, 0.5, 0.0])
    assert (s["wins"], s["draws"], s["losses"], s["openings"]) == (3, 2, 3, 4)
    assert s["score"] == 0.5 and s["elo"] == 0.0
    assert s["se"] == pytest.approx(math.sqrt((0.25 + 0.0 + 0.0 + 0.25) / 3.0) / 2.0, rel=1e-12)
    q = arena.pair_statistics([1, 1, 0, -1, -1], [0, 1, 0, 0, 1])
    assert np.array_equal(q["pair_scores"], [0.75, 0.5, 0.5, 0.25, 0.0]) and q["score"] == pytest.approx(0.4)


@pytest.mark.parametrize("flags", [[], ["-DSYN_DEBUG_SHAPES"]])
def test_per_call_arithmetic_reaches_the_launch_plan(tmp_path, flags):
    exe = str(tmp_path / "match_sides_plan_harness")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror"] + flags +
                          ["-o", exe, os.path.join(ROOT, "tests", "cpp", "match_sides_plan_harness.cpp")])
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.startswith("ok "), p.stdout[-2000:] + p.stderr[-2000:]
    assert int(p.stdout.split()[1]) > 1000
