"""GPU results behind the policy-evaluation selection (synthesis_amd/csrc/launch_plan.hpp plan_eval; its rows are held on a CPU by
tests/test_launch_plan.py::test_eval_plan_rows): every Connect4Net row of it gives the oracle's bits — the tile kernel, two and three
waves per SIMD in f32, two and four in f16x2, on either side of each threshold —, and an evaluation context that outlives loads and
arithmetic switches follows the engine's network through the one install path. No test looks at which kernel ran."""
import os

import numpy as np
import pytest

from tests.test_gpu_convnet import conv_blob
from tests.test_gpu_parity import random_positions

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def blob(golden_dir):
    return np.load(os.path.join(golden_dir, "c4net_blob_f32.npy"))


@pytest.fixture(scope="module")
def conv_model(tmp_path_factory):
    from tests import conv_f16x2_model

    return conv_f16x2_model.load(tmp_path_factory.mktemp("conv_f16x2_model"))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_every_connect4net_row_gives_the_oracles_bits(oracle, blob):
    import torch

    import synthesis_amd as sa

    cus = torch.cuda.get_device_properties(0).multi_processor_count
    t32, t16 = 16 * 48 * cus - 15, 16 * 64 * cus - 15   # first sizes of three (f32) / four (f16x2) waves per SIMD
    # 4,096: the tile kernel's last size; 32,769: the first that leaves the context path for the engine's own stream
    sizes = (4096, 4097, 32769, t32 - 1, t32, t16 - 1, t16)
    my, op = random_positions(oracle, 512, seed=11)
    my[0] = 0; op[0] = 0
    eng = sa.Engine(concurrent_games=64, max_explores=64, device=0)
    try:
        eng.load_weights(blob)
        for arith, mode in (("f32", oracle.ACC_FMA), ("f16x2", oracle.ACC_F16X2)):
            eng.set_network_arithmetic(arith)
            ref_l, ref_v = oracle.c4net_eval(blob, my, op, mode=mode)
            for n in sizes:
                l, v = eng.policy_eval(np.resize(my, n), np.resize(op, n))
                full, tail = n // 512, n % 512
                what = f"{arith}, n {n}"
                assert np.array_equal(_bits(l[:512]), _bits(ref_l)) and np.array_equal(_bits(v[:512]), _bits(ref_v)), what
                assert np.array_equal(_bits(l[:full * 512]).reshape(full, 512, 9), np.broadcast_to(_bits(ref_l), (full, 512, 9))), what
                assert np.array_equal(_bits(v[:full * 512]).reshape(full, 512, 3), np.broadcast_to(_bits(ref_v), (full, 512, 3))), what
                assert np.array_equal(_bits(l[full * 512:]), _bits(ref_l[:tail])), what
                assert np.array_equal(_bits(v[full * 512:]), _bits(ref_v[:tail])), what
    finally:
        eng.close()


def test_a_context_follows_the_engine_through_every_install(oracle, blob, conv_model):
    import synthesis_amd as sa

    cblob = conv_blob()
    my, op = random_positions(oracle, 1025, seed=12)
    my[0] = 0; op[0] = 0
    refs = {
        ("mlp", "f32"): oracle.c4net_eval(blob, my, op, mode=oracle.ACC_FMA),
        ("mlp", "f16x2"): oracle.c4net_eval(blob, my, op, mode=oracle.ACC_F16X2),
        ("conv", "f16x2"): conv_model.eval(cblob, my, op),
        ("conv", "f32"): oracle.c4conv_eval(cblob, my, op, mode=oracle.ACC_FMA),
    }
    eng = sa.Engine(concurrent_games=64, max_explores=64, device=0)
    try:
        ctx = eng.eval_context()   # one context for the whole sequence
        steps = (
            (lambda: eng.load_weights(blob), ("mlp", "f32")),
            (lambda: eng.set_network_arithmetic("f16x2"), ("mlp", "f16x2")),
            (lambda: eng.load_weights_conv(cblob), ("conv", "f16x2")),
            (lambda: eng.set_network_arithmetic("f32"), ("conv", "f32")),
            (lambda: eng.load_weights(blob), ("mlp", "f32")),
        )
        for i, (step, key) in enumerate(steps):
            step()
            ref_l, ref_v = refs[key]
            for n in (17, 1025):   # Connect4Net in f32: polled and not polled
                l, v = ctx.eval(my[:n], op[:n])
                assert np.array_equal(_bits(l), _bits(ref_l[:n])) and np.array_equal(_bits(v), _bits(ref_v[:n])), (i, key, n)
    finally:
        eng.close()
