"""Layer 1's operand tables (synthesis_amd/csrc/l1_tables.cuh) checked on the host by tests/cpp/l1_tables_check.cpp: the spread
table on every 7-bit column pattern x 9 columns, the quad table on every 8-bit index x 4 lane groups, and the composed path
(transpose, then quad lookups) on all 64 operands of the empty board, full boards and 120,000 positions of random games,
against the cell-by-cell definition of Game::features. Built plain and with the address and undefined-behaviour sanitizers."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "l1_tables_check.cpp")


@pytest.mark.parametrize("flags", [["-O1"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "sanitized"])
def test_l1_tables_match_the_feature_definition(tmp_path, flags):
    exe = str(tmp_path / "l1_tables_check")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", *flags, SRC, "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    lines = p.stdout.splitlines()
    assert len(lines) == 3 and all(line.endswith(": 0 mismatches") for line in lines), p.stdout
    assert lines[2].startswith("composed path, 12") and "reachable positions x 64 operands" in lines[2]
