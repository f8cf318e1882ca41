"""Layer 1's operands by table (l1_tables.cuh) on the GPU: the two kernels whose tile reads them, held to the oracle bit for bit.

  * policy_eval_kernel (the throughput evaluation kernel, forced at every batch size with SYN_DEBUG=1 SYN_EVAL_THROUGHPUT=1) on
    1, 15, 16, 17 and 4,096 positions: the empty board, full boards, a full column each (top cells are bits on both sides of the
    32-bit boundary of both board layouts; column 4 straddles it in the column-major one), then random boards; two networks.
  * the lane-per-tree kernel: one self-play of 512 games at 64 explores in the parity configuration, on 256 trees (4 waves) and
    on 768 trees (the 12-wave instantiation), game for game equal to the oracle's.
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FULL = (1 << 63) - 1
EVAL_SIZES = (1, 15, 16, 17, 4096)


def eval_positions():
    """4,096 boards that obey gravity: index 0 empty, 1-2 full, 3-11 column c full over random other columns, the rest random."""
    rng = np.random.RandomState(424242)

    def random_board(fixed_col=None):
        heights = rng.randint(0, 8, 9)
        if fixed_col is not None:
            heights[fixed_col] = 7
        my = op = 0
        for c in range(9):
            for r in range(heights[c]):
                if rng.randint(2):
                    my |= 1 << (r + 7 * c)
                else:
                    op |= 1 << (r + 7 * c)
        return my, op

    a = 0
    for c in range(9):
        for r in range(7):
            if (c + r // 2) & 1:
                a |= 1 << (r + 7 * c)
    boards = [(0, 0), (a, FULL & ~a), (FULL & ~a, a)] + [random_board(c) for c in range(9)]
    while len(boards) < 4096:
        boards.append(random_board())
    my = np.array([b[0] for b in boards], np.uint64)
    op = np.array([b[1] for b in boards], np.uint64)
    return my, op


@pytest.mark.parametrize("weights", ["c4net_blob_f32", "c4net_trained_f32"])
def test_throughput_eval_kernel_is_bit_equal_to_the_oracle(oracle, golden_dir, monkeypatch, weights):
    import torch

    import synthesis_amd as sa

    w = np.load(os.path.join(golden_dir, weights + ".npy"))
    my, op = eval_positions()
    assert my[0] == 0 and (my[1] | op[1]) == FULL and all((int(my[3 + c]) | int(op[3 + c])) >> (6 + 7 * c) & 1 for c in range(9))
    ref_l, ref_v = oracle.c4net_eval(w, my, op, mode=oracle.ACC_FMA)
    monkeypatch.setenv("SYN_DEBUG", "1")  # developer knobs are honoured only with SYN_DEBUG=1
    monkeypatch.setenv("SYN_EVAL_THROUGHPUT", "1")
    eng = sa.Engine(concurrent_games=256, max_explores=64, device=0)
    try:
        eng.load_weights(w)
        d_my = torch.from_numpy(my.view(np.int64)).cuda()
        d_op = torch.from_numpy(op.view(np.int64)).cuda()
        for n in EVAL_SIZES:
            d_l = torch.full((n, 9), float("nan"), dtype=torch.float32, device="cuda")
            d_v = torch.full((n, 3), float("nan"), dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            eng.policy_eval_device(d_my.data_ptr(), d_op.data_ptr(), n, d_l.data_ptr(), d_v.data_ptr(), sync=True)
            got_l, got_v = d_l.cpu().numpy(), d_v.cpu().numpy()
            assert np.array_equal(got_l.view(np.uint32), ref_l[:n].view(np.uint32)), (weights, n)
            assert np.array_equal(got_v.view(np.uint32), ref_v[:n].view(np.uint32)), (weights, n)
    finally:
        eng.close()


@pytest.fixture(scope="module")
def selfplay_reference(oracle, golden_dir):
    from tests.oracle_lib import parity_rollout_config

    blob = np.load(os.path.join(golden_dir, "c4net_blob_f32.npy"))
    return blob, oracle.c4_selfplay(parity_rollout_config(64), blob, 1234, 512, threads=8, nn_mode=oracle.ACC_FMA)


@pytest.mark.parametrize("trees,waves", [(256, 4), (768, 12)])
def test_lane_kernel_selfplay_is_the_oracles_game_for_game(selfplay_reference, monkeypatch, trees, waves):
    import synthesis_amd as sa
    from tests.test_gpu_parity import assert_selfplay_equal

    blob, ref = selfplay_reference
    monkeypatch.setenv("SYN_DEBUG", "1")
    monkeypatch.setenv("SYN_LANES", str(waves))
    eng = sa.Engine(concurrent_games=trees, max_explores=64, device=0)
    try:
        eng.load_weights(blob)
        got = eng.selfplay(sa.parity_rollout_config(64), base_seed=1234, n_games=512)
        assert eng.last_launch_shape()[0] == 4 and eng.last_launch_shape()[2] == 64 * waves
        assert_selfplay_equal(got, ref, f"{trees} trees, {waves} waves")   # plies, positions, visit distributions, value targets, actions
    finally:
        eng.close()
