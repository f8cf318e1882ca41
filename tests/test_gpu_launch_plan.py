"""The launch selection (synthesis_amd/csrc/launch_plan.hpp) as the library applies it, at the engine sizes that straddle its
thresholds: 16 and 17 workgroups' worth of trees per 16 CUs (row-per-tree, one / two workgroups per CU), 256 trees per CU and one
workgroup more (lane-per-tree kernel at 4 / 8 waves), the headline size (12 waves on 768 of 1,024 slots per CU); in the f16x2 arithmetic
the free-running kernel's last size and the first the lane kernel takes. tests/test_launch_plan.py holds the same rows on a CPU; here the
shapes are the engine's own and every shape plays the same games. Games of 8 explores on engines of max_explores=12: the lane-per-tree
kernel hands nodes out in blocks of four, so the root's and eight explores' expansions of up to nine children can take 27 blocks, which
max_explores=8 (21 blocks) does not hold and 12 (30 blocks) does; the largest pool is 0.94 GiB."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F32_ROWS = {4096: (1, 256, 256), 4112: (2, 257, 256), 65536: (4, 256, 256), 65552: (4, 129, 512), 262144: (4, 256, 768)}
F16_ROWS = {4096: (7, 256, 256), 4112: (4, 17, 256)}
KNOBS = ("SYN_DEBUG", "SYN_LANES", "SYN_LANES2", "SYN_QUADS", "SYN_LANE_THRESH", "SYN_PROFILE", "SYN_PC", "SYN_FREE", "SYN_POOL")


def play(blob, conc, f16x2):
    """(launch shape, plies, final_kind) of concurrent_games self-play games; of the outputs only these two arrays are fetched."""
    import synthesis_amd as sa
    from synthesis_amd.engine import _p

    eng = sa.Engine(concurrent_games=conc, max_explores=12, device=0)
    if f16x2:
        eng.set_network_arithmetic("f16x2")
    eng.load_weights(blob)
    plies, final = np.zeros(conc, np.int32), np.zeros(conc, np.uint8)
    cfg = sa.parity_rollout_config(8).to_c()
    eng._check(eng._lib.syn_selfplay_run(eng._h, C.byref(cfg), 7, 0, conc, _p(plies), None, None, None, None, None, _p(final), None))
    shape = eng.last_launch_shape()
    eng.close()
    return shape, plies, final


@pytest.mark.parametrize("f16x2,rows", [(False, F32_ROWS), (True, F16_ROWS)], ids=["f32", "f16x2"])
def test_shapes_at_the_thresholds_play_the_same_games(golden_dir, monkeypatch, f16x2, rows):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    blob = np.load(os.path.join(golden_dir, "c4net_blob_f32.npy"))
    got = {conc: play(blob, conc, f16x2) for conc in rows}
    for conc, expect in rows.items():
        assert got[conc][0] == expect, f"{conc} concurrent games"
    _, ref_plies, ref_final = got[max(rows)]
    assert ref_plies[:4112].min() >= 7 and ref_plies[:4112].max() <= 63
    for conc, (_, plies, final) in got.items():
        n = min(conc, 4112)
        assert np.array_equal(plies[:n], ref_plies[:n]) and np.array_equal(final[:n], ref_final[:n]), f"{conc} concurrent games"
