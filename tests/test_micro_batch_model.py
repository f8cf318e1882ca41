"""The micro-batch learner step on a CPU: the model the GPU tests compare against (tests/micro_batch_model.py) held to the oracle's
chained gradient, and the launch choice (synthesis_amd/csrc/launch_plan.hpp: plan_micro_grads) through a g++ harness of its own
(tests/cpp/micro_plan_harness.cpp), driven like tests/test_launch_plan.py drives its harness."""
import os
import subprocess
from collections import namedtuple

import numpy as np
import pytest

from tests import micro_batch_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "micro_plan_harness.cpp")


def test_one_micro_batch_is_the_chained_step(oracle):
    """nb = 1: nothing is added to g_0 and inv = 1, so every bit — the sign of a zero included — is the chained step's."""
    blob = model.blob_of("mlp")
    idx = model.batch_indices(oracle, 32, seed=1)
    G, l = model.gradients(oracle, "mlp", blob, idx)
    g, lo = model.chained_gradients(oracle, "mlp", blob, idx)
    assert np.array_equal(G.view(np.uint32), g.view(np.uint32)) and np.array_equal(l.view(np.uint32), lo.view(np.uint32))
    z = np.array([-0.0, 0.0, 1.5], np.float32)
    assert np.array_equal(model.combine([z]).view(np.uint32), z.view(np.uint32))


@pytest.mark.parametrize("nb", [2, 4, 8])
def test_model_is_the_mean_gradient(oracle, nb):
    """The model and the oracle's chained gradient of the same B = 32 nb samples are two f32 evaluations of the same sums (a mean of
    equal-size block means is the mean), each inside the project's 1e-5 training bar: they agree within 2e-5 of each
    parameter block's largest gradient; the losses within 2e-5 of the loss."""
    blob = model.blob_of("mlp")
    idx = model.batch_indices(oracle, 32 * nb, seed=10 + nb)
    G, l = model.gradients(oracle, "mlp", blob, idx)
    g, lo = model.chained_gradients(oracle, "mlp", blob, idx)
    assert not np.array_equal(G, g)   # a different order of the same sums, not the same chain
    for blk in model.mlp_param_blocks():
        top = np.abs(g[blk]).max()
        assert top > 0
        assert np.abs(G[blk] - g[blk]).max() <= 2e-5 * top, (nb, blk)
    assert np.all(np.abs(l - lo) <= 2e-5 * np.abs(lo))


def test_pool_has_the_planted_target_rows(oracle):
    p = model.pool(oracle)
    assert not p["tpi"][model.ZERO_ROW].any()
    assert sorted(p["tpi"][model.ONE_HOT_ROW]) == [0.0] * 8 + [1.0]
    idx = model.batch_indices(oracle, 96, seed=3)
    assert idx[model.ZERO_ROW] == model.ZERO_ROW and idx[model.ONE_HOT_ROW] == model.ONE_HOT_ROW   # micro-batches 0 and 1


# ---- plan_micro_grads
Plan = namedtuple("Plan", "grid threads lds row_stride buffer_bytes reduce_grid reduce_threads")
MLP_STRIDE, CONV_STRIDE = 30528, 12416   # 30492 + 2 and 12412 + 2 floats, padded to a multiple of 64


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("micro_plan") / "harness")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-o", exe, SRC])

    def run(queries):
        text = "".join(" ".join(f"{k}={int(v)}" for k, v in q.items()) + "\n" for q in queries)
        out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
        assert len(out) == len(queries)
        return [Plan(*map(int, l.split())) for l in out]

    return run


def test_micro_plan_grid(plans):
    """grid = min(nb, cap); cap = max_workgroups, or the CU count when that is 0."""
    rows = [  # (query, grid)
        (dict(net=0, nb=1), 1), (dict(net=0, nb=7), 7), (dict(net=0, nb=255), 255), (dict(net=0, nb=256), 256), (dict(net=0, nb=257), 256),
        (dict(net=0, nb=263), 256), (dict(net=0, nb=1024), 256), (dict(net=0, nb=263, cus=304), 263), (dict(net=0, nb=400, cus=304), 304),
        (dict(net=0, nb=7, cap=1), 1), (dict(net=0, nb=7, cap=2), 2), (dict(net=0, nb=7, cap=3), 3), (dict(net=0, nb=7, cap=7), 7),
        (dict(net=0, nb=7, cap=8), 7), (dict(net=0, nb=1024, cap=300), 300),   # an explicit cap is the caller's, also above the CU count
        (dict(net=1, nb=128), 128), (dict(net=1, nb=300), 256), (dict(net=1, nb=300, cap=64), 64),
    ]
    got = plans([q for q, _ in rows])
    for (q, grid), p in zip(rows, got):
        assert p.grid == grid, q
        assert 1 <= p.grid <= q["nb"]   # a workgroup's first micro-batch j = blockIdx.x exists


def test_micro_plan_shapes_and_buffer(plans):
    mlp, conv = plans([dict(net=0, nb=5), dict(net=1, nb=5)])
    assert (mlp.threads, mlp.lds, mlp.row_stride) == (1024, 25792 * 4, MLP_STRIDE)
    # the conv learner's step holds the minibatch's activations in LDS: 157,568 B of the CU's 160 KB, so one workgroup per CU
    assert (conv.threads, conv.lds, conv.row_stride) == (512, 157568, CONV_STRIDE)
    assert 2 * conv.lds > 160 * 1024 >= conv.lds
    for p, stride, params in ((mlp, MLP_STRIDE, 30492), (conv, CONV_STRIDE, 12412)):
        assert stride % 64 == 0 and params + 2 <= stride < params + 2 + 64
        assert p.buffer_bytes == 5 * stride * 4
        assert p.reduce_threads == 64 and (p.reduce_grid - 1) * 64 < params + 2 <= p.reduce_grid * 64
    big = plans([dict(net=0, nb=1024), dict(net=1, nb=1024), dict(net=0, nb=1)])
    assert [p.buffer_bytes for p in big] == [1024 * MLP_STRIDE * 4, 1024 * CONV_STRIDE * 4, MLP_STRIDE * 4]
