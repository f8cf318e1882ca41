"""The mirror-symmetric replay de-duplication's surface, as far as it can be checked without a GPU: header <-> ctypes <-> library
agreement of the three entry points, the Engine methods, the argument checks of LearningLoop and examples/train_connect4.py, the two
synthesis_amd.hpp methods with their symmetry argument in a host-only C++ translation unit — and tests/symmetry_py.py, the numpy
restatement of the specification the GPU tests compare against, held to the CPU oracle's Connect4."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import symmetry_py as sym

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_ENTRY_POINTS = {"syn_positions_mirror": 8, "syn_replay_deduplicate_symmetric": 13, "syn_replay_deduplicate_to_trainer_symmetric": 3}


def test_new_entry_points_agree_between_header_ctypes_and_library():
    from synthesis_amd.engine import ABI_SYMBOLS, load_library

    header = open(os.path.join(ROOT, "include", "synthesis_amd.h")).read()
    lib = load_library()
    exported = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "synthesis_amd", "libsynthesis_amd.so")]).decode()
    for name, n_args in NEW_ENTRY_POINTS.items():
        protos = re.findall(rf"^int {name}\(([^)]*)\);", header, re.M)
        assert len(protos) == 1, name
        params = [p.strip() for p in protos[0].split(",")]
        assert len(params) == n_args and params[0] == "syn_engine* h", (name, params)
        assert name in ABI_SYMBOLS
        assert len(getattr(lib, name).argtypes) == n_args, name
        assert re.search(rf"\bT {name}\b", exported), name
    # the symmetric form takes syn_replay_deduplicate's arguments, with one more count in front of the last
    plain = re.findall(r"^int syn_replay_deduplicate\(([^)]*)\);", header, re.M)[0]
    symm = re.findall(r"^int syn_replay_deduplicate_symmetric\(([^)]*)\);", header, re.M)[0]
    norm = lambda s: [" ".join(p.split()) for p in s.split(",")]
    assert norm(symm) == norm(plain)[:-1] + ["size_t* out_canonical", "size_t* out_count"]
    import ctypes as C

    assert lib.syn_positions_mirror.argtypes[4] is C.c_size_t and lib.syn_replay_deduplicate_symmetric.argtypes[5] is C.c_size_t


def test_engine_has_the_symmetry_methods():
    import inspect

    from synthesis_amd.engine import Engine

    assert callable(Engine.positions_mirror)
    for m in ("replay_deduplicate", "replay_deduplicate_to_trainer"):
        p = inspect.signature(getattr(Engine, m)).parameters
        assert p["symmetry"].default == "none", m   # the default is today's call
    for m, args in (("replay_deduplicate", (None, [], [], [], [])), ("replay_deduplicate_to_trainer", (None,))):
        with pytest.raises(ValueError, match="symmetry"):   # refused before the library is touched (no handle here)
            getattr(Engine, m)(*args, symmetry="rotate")


class StandIn:
    """what LearningLoop's constructor touches of an engine"""

    def load_weights(self, blob):
        pass

    def trainer_init(self, blob, **hyper):
        pass


def test_learning_loop_rejects_an_unknown_symmetry():
    from synthesis_amd.engine import NUM_PARAMS
    from synthesis_amd.learner import LearningLoop

    blob = np.full(NUM_PARAMS, 0.5, np.float32)
    with pytest.raises(ValueError, match="symmetry"):
        LearningLoop(StandIn(), "mlp", blob, symmetry="rotate")
    for ok in ("none", "mirror"):
        for replay in ("host", "device"):
            assert LearningLoop(StandIn(), "mlp", blob, symmetry=ok, replay=replay).symmetry == ok
    assert LearningLoop(StandIn(), "mlp", blob).symmetry == "none"   # the default is today's path


def test_example_rejects_an_unknown_symmetry():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "train_connect4.py"), "--symmetry", "rotate"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "invalid choice" in r.stderr and "--symmetry" in r.stderr
    h = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "train_connect4.py"), "--help"],
                       capture_output=True, text=True, timeout=120)
    assert h.returncode == 0 and "--symmetry {none,mirror}" in h.stdout


CPP = r"""
#include "synthesis_amd.hpp"
#include <cstdio>
// host-only: the two de-duplications with their symmetry argument, and without it (the default is Symmetry::None)
static size_t device_iteration(synthesis::Engine& e, synthesis::DeviceReplayBuffer& buffer, size_t games, size_t* canonical) {
    const syn_rollout_config rc = synthesis::RolloutConfig().to_c();
    e.check(syn_selfplay_run(e.handle(), &rc, 0, buffer.total_games_played(), (int)games, nullptr, nullptr, nullptr, nullptr, nullptr,
                             nullptr, nullptr, nullptr));
    buffer.extend_from_selfplay(games);
    const size_t plain = buffer.deduplicate_to_trainer();
    const size_t also_plain = buffer.deduplicate_to_trainer(synthesis::Symmetry::None);
    const size_t both = buffer.deduplicate_to_trainer(synthesis::Symmetry::Mirror, canonical);
    return plain == also_plain ? both : 0;
}
static size_t host_dedup(synthesis::Engine& e, const synthesis::ReplayBuffer& buffer) {
    size_t canonical = 0;
    const synthesis::FlatBatch a = buffer.deduplicate(e);
    const synthesis::FlatBatch b = buffer.deduplicate(e, synthesis::Symmetry::Mirror, &canonical);
    const synthesis::FlatBatch c = buffer.deduplicate(e, synthesis::Symmetry::Mirror);
    return a.games.size() + b.games.size() + c.pis.size() + canonical;
}
int main() {
    try {
        synthesis::Engine e(64, 64);
        synthesis::DeviceReplayBuffer buffer(e, 64 * 63);
        synthesis::ReplayBuffer host;
        size_t canonical = 0;
        std::printf("%zu %zu %zu\n", device_iteration(e, buffer, 16, &canonical), canonical, host_dedup(e, host));
    } catch (const synthesis::Error& err) {
        std::printf("error %d %s\n", err.code, err.what());
        return 3;
    }
    return 0;
}
"""


def test_hpp_symmetry_arguments_compile_host_only(tmp_path):
    """ReplayBuffer::deduplicate and DeviceReplayBuffer::deduplicate_to_trainer with and without the symmetry argument in a plain g++
    translation unit (-Wall -Werror, no HIP headers), linked against the library; without a GPU the program fails loudly at the Engine."""
    import torch

    src = tmp_path / "symmetry.cpp"
    src.write_text(CPP)
    exe = str(tmp_path / "symmetry")
    lib = os.path.join(ROOT, "synthesis_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe,
                           "-L" + lib, "-lsynthesis_amd", "-Wl,-rpath," + lib, "-pthread"])
    if not torch.cuda.is_available():
        p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        assert p.returncode == 3 and p.stdout.startswith("error -2 ")


# ---- tests/symmetry_py.py on its own

def test_mirror_is_an_involution_that_moves_columns():
    rng = np.random.default_rng(5)
    bb = rng.integers(0, 1 << 63, size=4096, dtype=np.uint64)
    m = sym.mirror(bb)
    assert np.array_equal(sym.mirror(m), bb)
    assert not np.array_equal(m, bb) and (m >> np.uint64(63) == 0).all()
    for col in range(9):
        for row in range(7):
            one = np.array([1 << (row + 7 * col)], np.uint64)
            assert int(sym.mirror(one)[0]) == 1 << (row + 7 * (8 - col))
    assert np.array_equal(sym.mirror(bb | np.uint64(1 << 63)), m | np.uint64(1 << 63))   # bit 63 is not part of the board
    pi = rng.random((7, 9), dtype=np.float32)
    assert np.array_equal(sym.reverse(pi)[:, 2], pi[:, 6]) and np.array_equal(sym.reverse(sym.reverse(pi)), pi)


def random_lines(rng, count):
    """random move sequences from the empty board, and the centre-column lines (their positions are self-symmetric)"""
    lines = [[4] * k for k in range(8)] + [[4, 4, 0, 8], [0, 8], [3, 5, 4]]
    for _ in range(count):
        lines.append(list(rng.integers(0, 9, size=int(rng.integers(1, 40)))))
    return lines


def legal_prefix(oracle, moves):
    """the longest prefix that is a legal game (it may end with the move that ends the game)"""
    for i in range(len(moves)):   # (one move at a time: the oracle's step is never asked to go on behind an illegal move)
        r = oracle.c4_play(moves[: i + 1])
        if not r["legal_before"][i]:
            return moves[:i]
        if r["over"][i]:
            return moves[: i + 1]
    return moves


def legal_mask(oracle, moves):
    return np.array([bool(oracle.c4_play(moves + [c])["legal_before"][-1]) for c in range(9)])


def test_mirror_against_the_oracle_game(oracle):
    """A reachable position and the position the mirrored moves reach: the bitboards are each other's mirror, the legal-move mask is
    reversed, the win status is the same, the feature planes are flipped left to right."""
    rng = np.random.default_rng(17)
    seen_over = seen_sym = 0
    for line in random_lines(rng, 120):
        a = legal_prefix(oracle, [int(m) for m in line])
        b = [8 - m for m in a]
        if not a:
            pa = pb = dict(my_bb=0, op_bb=0, winner=-1)
            over = False
        else:
            pa, pb = oracle.c4_play(a), oracle.c4_play(b)
            over = bool(pa["over"][-1])
            assert over == bool(pb["over"][-1])
            assert pa["winner"] == pb["winner"] and pa["player"] == pb["player"]
        my, op = np.array([pa["my_bb"]], np.uint64), np.array([pa["op_bb"]], np.uint64)
        assert int(sym.mirror(my)[0]) == pb["my_bb"] and int(sym.mirror(op)[0]) == pb["op_bb"], a
        for bb in (my, op):
            assert oracle.c4_won(int(bb[0])) == oracle.c4_won(int(sym.mirror(bb)[0]))
        if not over:
            assert np.array_equal(legal_mask(oracle, a)[::-1], legal_mask(oracle, b)), a
        fa = oracle.c4_features(my, op).reshape(7, 9)
        fb = oracle.c4_features(sym.mirror(my), sym.mirror(op)).reshape(7, 9)
        assert np.array_equal(fa[:, ::-1], fb), a
        seen_over += over
        seen_sym += bool(sym.self_symmetric(my, op)[0])
        assert bool(sym.self_symmetric(my, op)[0]) == (pa["my_bb"] == pb["my_bb"] and pa["op_bb"] == pb["op_bb"])
    assert seen_over > 0 and seen_sym >= 8


def test_symmetric_deduplicate_in_numpy_against_the_oracle_dedup(oracle):
    """symmetry_py.symmetric_deduplicate over the CPU oracle's de-duplication (sorted into ascending (my, op) order): the properties the
    definitions promise — U + M <= 2n, sum(num[:U]) == n, the states closed under mirror, row U + k the exact permutation of its class."""
    rng = np.random.default_rng(23)
    base_my = rng.integers(0, 1 << 63, size=40, dtype=np.uint64)
    base_op = rng.integers(0, 1 << 63, size=40, dtype=np.uint64) & ~base_my
    base_my[:6] = np.array([0, 1 << 28, 1 | 1 << 56, 1 << 30, 3 << 28, 1 << 7 | 1 << 49], np.uint64)   # self-symmetric ones
    base_op[:6] = np.array([0, 1 << 29, 1 << 31, 0, 1 << 14 | 1 << 42, 1 << 28], np.uint64)
    pick = rng.integers(0, 40, size=300)
    flip = rng.random(300) < 0.5
    my = np.where(flip, sym.mirror(base_my[pick]), base_my[pick])
    op = np.where(flip, sym.mirror(base_op[pick]), base_op[pick])
    pi, v = rng.random((300, 9), dtype=np.float32), rng.random((300, 3), dtype=np.float32)

    def plain(my, op, pi, v):
        D = oracle.dedup(my, op, pi, v)
        o = np.lexsort((D["op_bb"], D["my_bb"]))
        return {k: a[o] for k, a in D.items()}

    S = sym.symmetric_deduplicate(plain, my, op, pi, v)
    U, total = S["canonical"], S["num"].size
    assert U < 300 and U <= 40 and U < total <= 2 * U
    assert int(S["num"][:U].sum()) == 300
    assert not sym.flipped(S["my_bb"][:U], S["op_bb"][:U]).any()
    states = set(zip(S["my_bb"].tolist(), S["op_bb"].tolist()))
    assert len(states) == total
    assert states == set(zip(sym.mirror(S["my_bb"]).tolist(), sym.mirror(S["op_bb"]).tolist()))
    e = np.flatnonzero(~sym.self_symmetric(S["my_bb"][:U], S["op_bb"][:U]))
    assert e.size == total - U and e.size < U
    assert np.array_equal(S["pis"][U:].view(np.uint32), S["pis"][e][:, ::-1].view(np.uint32))
    assert np.array_equal(S["vs"][U:].view(np.uint32), S["vs"][e].view(np.uint32)) and np.array_equal(S["num"][U:], S["num"][e])
    # the de-duplication does not depend on the orientation a record arrived in — except that a self-symmetric state's record is its
    # own canonical form in both orientations, so its averaged pi arrives reversed
    S2 = sym.symmetric_deduplicate(plain, sym.mirror(my), sym.mirror(op), sym.reverse(pi), v)
    ss = sym.self_symmetric(S["my_bb"], S["op_bb"])
    for k in ("my_bb", "op_bb", "vs", "num"):
        assert np.array_equal(S[k], S2[k]), k
    assert np.array_equal(S["pis"][~ss].view(np.uint32), S2["pis"][~ss].view(np.uint32))
    assert np.array_equal(S["pis"][ss].view(np.uint32), S2["pis"][ss][:, ::-1].view(np.uint32))
