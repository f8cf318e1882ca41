"""The replay / data-set layouts (synthesis_amd/csrc/position_layout.hpp) on a CPU: tests/cpp/position_layout_harness.cpp, built with
g++, prints a layout for each query on stdin. The de-duplication work area's total is held to the two hand-summed formulas that the
size query had before the layout was stated once (restated here in Python, not read from the header), the reanalyse scratch to a
restatement of its carve, and the column offsets to the figures of the stored formats: my | op | gid | pi | v at 0, 8, 16, 24 and 60
bytes times the capacity in the replay buffer, my | op | pi | v at 0, 8, 16 and 52 times n in a data set."""
import itertools
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "position_layout_harness.cpp")
NS = [1, 2, 31, 32, 33, 255, 256, 257, 65537, 0x3FFFFFFF]
TMPS = [0, 1, 255, 256, 4097]
SEARCH_RESULT_BYTES = 372   # 93 four-byte words: include/synthesis_amd.h syn_search_result


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("position_layout") / "harness")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-o", exe, SRC])

    def ask(queries):
        text = "".join(" ".join(str(int(x)) if not isinstance(x, str) else x for x in q) + "\n" for q in queries)
        out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
        assert len(out) == len(queries)
        return [[int(x) for x in l.split()] for l in out]

    return ask


def a256(x):
    return (x + 255) & ~255


def parent_dedup_total(n, tmp, mirror):
    """dedup_work_bytes as it was summed by hand: the plain form, then the mirrored one."""
    if not mirror:
        return 2 * a256(n * 8) + 2 * a256(n * 4) + 3 * a256(n * 4) + 2 * a256(n * 8) + a256(n * 36) + a256(n * 12) + a256(n * 4) + a256(tmp)
    r = 2 * n
    return (2 * a256(n * 8) + 2 * a256(n * 4) + 3 * a256(n * 4) + 2 * a256(r * 8) + a256(r * 36) + a256(r * 12) + a256(r * 4) + a256(tmp)
            + 2 * a256(n * 8) + 3 * a256(n * 4))


def check_sections(offsets, payloads, total, what):
    """Sections in carve order: 256-byte aligned, disjoint, each at least as long as its payload, the last one ending inside `total`."""
    assert offsets[0] == 0, what
    for i, (o, p) in enumerate(zip(offsets, payloads)):
        end = offsets[i + 1] if i + 1 < len(offsets) else total
        assert o % 256 == 0, f"{what}: section {i} at {o}"
        assert end - o >= p, f"{what}: section {i} has {end - o} bytes for a payload of {p}"
        assert end - o < p + 256, f"{what}: section {i} is padded by a whole line or more"
    assert total % 256 == 0, what


def test_dedup_layout(harness):
    cases = list(itertools.product(NS, TMPS, (0, 1)))
    for (n, tmp, mirror), row in zip(cases, harness([("dedup", *c) for c in cases])):
        what = f"dedup n={n} tmp={tmp} mirror={mirror}"
        sections, rows, total = row[:18], row[18], row[19]
        assert rows == (2 * n if mirror else n), what
        payloads = [n * 8, n * 8, n * 4, n * 4, n * 4, n * 4, n * 4, rows * 8, rows * 8, rows * 36, rows * 12, rows * 4, tmp]
        if mirror:
            payloads += [n * 8, n * 8, n * 4, n * 4, n * 4]
            assert all(o >= 0 for o in sections), what
            check_sections(sections, payloads, total, what)
        else:
            assert sections[13:] == [-1] * 5, f"{what}: mirror sections without mirror"
            check_sections(sections[:13], payloads, total, what)
        assert total == parent_dedup_total(n, tmp, mirror), what


def test_reanalyse_layout(harness):
    chunks = [0, 1, 33, 65536]
    cases = list(itertools.product(NS, TMPS, chunks))
    for (n, tmp, chunk), row in zip(cases, harness([("reanalyse", *c) for c in cases])):
        what = f"reanalyse n={n} tmp={tmp} chunk={chunk}"
        payloads = [n * 4, n * 4, n * 4, n * 8, n * 8, n * 4, n * 4, n * 4, 16, tmp, chunk * SEARCH_RESULT_BYTES]
        check_sections(row[:11], payloads, row[11], what)
        at, want = 0, []
        for p in payloads:   # the carve, restated
            want.append(at)
            at += a256(p)
        assert row[:11] == want and row[11] == at, what


@pytest.mark.parametrize("cap", [1, 300, 2**31 - 1])
def test_columns_at(harness, cap):
    with_gid, without = harness([("columns", cap, 1, 0), ("columns", cap, 0, 0)])
    assert with_gid[:5] == [0, 8 * cap, 16 * cap, 24 * cap, 60 * cap]
    assert without[:5] == [0, 8 * cap, -1, 16 * cap, 52 * cap]
    # columns_from(.., 7): seven rows on in every column, a null game id stays null
    assert with_gid[5:10] == [56, 56, 56, 7 * 36, 7 * 12]
    assert without[5:10] == [56, 56, -1, 7 * 36, 7 * 12]
    assert with_gid[10:] == [64, 72] and without[10:] == [64, 72]
    # the last column ends where the allocation does
    assert with_gid[4] + 12 * cap == 72 * cap and without[4] + 12 * cap == 64 * cap


def test_carve_columns(harness):
    """The staged columns of the host entry points: my | op | [pi] | [v], a column that is left out takes no room and reads as null."""
    for n in NS:
        full, no_v, boards = harness([("carve", n, 1, 1), ("carve", n, 1, 0), ("carve", n, 0, 0)])
        s8, s36, s12 = a256(n * 8), a256(n * 36), a256(n * 12)
        assert full == [0, s8, 2 * s8, 2 * s8 + s36, 2 * s8 + s36 + s12, 0, 0, 1, 0, 0]
        assert no_v == [0, s8, 2 * s8, -1, 2 * s8 + s36, 0, 0, 1, 0, 1]
        assert boards == [0, s8, -1, -1, 2 * s8, 0, 0, 1, 1, 1]
