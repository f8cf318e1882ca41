"""The launch selection (synthesis_amd/csrc/launch_plan.hpp: plan_launch) on a CPU: tests/cpp/launch_plan_harness.cpp, built with g++,
prints the plan for queries on stdin. The expected rows were derived by reading the launch code this selector replaced (the thresholds at
256 / 512 / 768 trees per CU, the 8-wave cap of the runtime-switched family, the 12-wave cap of the folded ones, the conv f16x2 caps),
and every plan of a sweep must name a kernel instantiation that lane_instances.h lists. The policy-evaluation selection (plan_eval) is
held the same way: rows read off the launch code it replaced (the tile kernel up to 4,096 positions, three waves per SIMD from 48 tiles
per CU, the f16x2 kernel's four from 64), the evaluation contexts' in-place and polling rules, and a sweep over the sizes."""
import itertools
import os
import subprocess
from collections import namedtuple

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "launch_plan_harness.cpp")
Plan = namedtuple("Plan", "error shape grid threads fast n policy tile prof slots lane_thresh nv path_entries listed")
CAP = 7212   # nodes per tree of a max_explores=800 engine


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    d = tmp_path_factory.mktemp("launch_plan")
    exes = {}
    for name, flags in (("default", []), ("debug_shapes", ["-DSYN_DEBUG_SHAPES"])):
        exes[name] = str(d / name)
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror"] + flags + ["-o", exes[name], SRC])

    def plans(queries, build="default"):
        text = "".join(" ".join(f"{k}={int(v)}" for k, v in q.items()) + "\n" for q in queries)
        out = subprocess.run([exes[build]], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
        assert len(out) == len(queries)
        return [Plan(*map(int, l.split())) for l in out]

    plans.exe = exes["default"]
    return plans


NETS = {"mlp f32": dict(net=0, f16=0), "mlp f16x2": dict(net=0, f16=1), "conv f32": dict(net=1, f16=0), "conv f16x2": dict(net=1, f16=1)}
FAM = {1: dict(fam=1, fpu=0), 2: dict(fam=2, fpu=2), "parentq": dict(fam=0, fpu=1), "dirichlet": dict(fam=0, fpu=0, noise=2)}


def query(net, fam, w, jobs=None, cap=CAP, **more):
    q = dict(slots=w, jobs=w if jobs is None else jobs, cap=cap, **NETS[net], **FAM[fam])
    q.update(more)
    return q


# (net / arithmetic, family, W, (shape, grid, threads), other plan fields)
ROWS = [
    ("mlp f32", 1, 4096, (1, 256, 256), {}),
    ("mlp f32", 1, 4112, (2, 257, 256), {}),
    ("mlp f32", 1, 8192, (2, 512, 256), {}),
    ("mlp f32", 1, 8208, (3, 171, 768), {}),
    ("mlp f32", 1, 12288, (3, 256, 768), {}),
    ("mlp f32", 1, 12304, (3, 193, 1024), {}),
    ("mlp f32", 1, 65520, (3, 1024, 1024), {}),
    ("mlp f32", 1, 65536, (4, 256, 256), dict(fast=1, policy=0, lane_thresh=48)),
    ("mlp f32", 1, 65552, (4, 129, 512), {}),
    ("mlp f32", 1, 131072, (4, 256, 512), {}),
    ("mlp f32", 1, 131088, (4, 171, 768), {}),
    ("mlp f32", 1, 196608, (4, 256, 768), dict(slots=196608)),
    ("mlp f32", 1, 262144, (4, 256, 768), dict(slots=196608)),
    ("mlp f32", "parentq", 262144, (4, 256, 512), dict(fast=0, slots=131072)),
    ("mlp f32", "parentq", 4096, (1, 256, 256), dict(fast=0)),
    ("mlp f32", 2, 16, (4, 1, 256), dict(fast=0)),   # no family-2 instantiation at 4 waves
    ("mlp f32", 2, 131072, (4, 256, 512), dict(fast=2)),
    ("mlp f32", 2, 262144, (4, 256, 768), dict(fast=2)),
    ("mlp f32", "dirichlet", 4096, (4, 16, 256), dict(fast=0)),
    ("mlp f16x2", 1, 4096, (7, 256, 256), {}),
    ("mlp f16x2", "parentq", 4096, (7, 256, 256), dict(fast=0)),
    ("mlp f16x2", 2, 4096, (4, 16, 256), dict(fast=2, policy=3, lane_thresh=64)),
    ("mlp f16x2", 1, 4112, (4, 17, 256), dict(policy=3, lane_thresh=64)),
    ("mlp f16x2", 1, 262144, (4, 256, 768), {}),
    ("mlp f16x2", "parentq", 262144, (4, 256, 512), dict(slots=131072)),
    ("conv f32", 1, 16, (4, 1, 256), dict(policy=2)),
    ("conv f32", 1, 262144, (4, 256, 1024), {}),
    ("conv f32", 2, 262144, (4, 256, 1024), dict(fast=0)),
    ("conv f32", "parentq", 262144, (4, 256, 512), dict(slots=131072)),
    ("conv f16x2", 1, 262144, (4, 256, 512), dict(policy=4, slots=131072)),
    ("conv f16x2", "parentq", 262144, (4, 256, 256), dict(fast=0, policy=4, slots=65536)),
    ("conv f16x2", 2, 262144, (4, 256, 256), dict(fast=0, policy=4, slots=65536)),
]


def test_plan_rows(harness):
    got = harness([query(net, fam, w) for net, fam, w, _, _ in ROWS])
    for (net, fam, w, sgt, other), p in zip(ROWS, got):
        what = f"{net}, family {fam}, {w} slots: {p}"
        assert not p.error and (p.shape, p.grid, p.threads) == sgt, what
        for k, v in other.items():
            assert getattr(p, k) == v, what
        assert p.listed == 1, what


def test_fewer_jobs_than_slots_plan_as_a_smaller_engine(harness):
    for net, fam, jobs in (("mlp f32", 1, 65537), ("mlp f32", 1, 4100), ("mlp f16x2", 1, 4090), ("conv f32", 1, 131073), ("mlp f32", 2, 1)):
        w = 16 * ((jobs + 15) // 16)
        a, b = harness([query(net, fam, 262144, jobs=jobs), query(net, fam, w)])
        assert a == b, (net, fam, jobs)


def test_capacity_beyond_the_lane_kernels(harness):
    big = 65540
    p, = harness([query("mlp f32", 1, 262144, cap=big)])
    assert not p.error and (p.shape, p.grid, p.threads, p.slots) == (3, 4096, 1024, 262144)   # no lane kernel
    for net, fam in (("mlp f32", 2), ("mlp f32", "dirichlet"), ("mlp f16x2", 1), ("conv f32", 1), ("conv f16x2", 1)):
        p, = harness([query(net, fam, 262144, cap=big)])
        assert p.error, (net, fam)
    p, = harness([dict(rollout=1, slots=4096, jobs=10000, cap=big)])
    assert p.error


def test_knobs(harness):
    sgt = lambda p: (p.shape, p.grid, p.threads)
    a, b, c, d = harness([query("mlp f32", 1, 262144, SYN_LANES=16), query("mlp f32", 1, 262144, SYN_LANES=0),
                          query("mlp f16x2", 1, 4096, SYN_FREE=0), query("mlp f32", 1, 65520, SYN_QUADS=0)])
    assert sgt(a) == (4, 256, 1024) and sgt(b) == (3, 4096, 1024) and sgt(c) == (4, 16, 256) and sgt(d) == (2, 4095, 256)
    a, b, c = harness([query("mlp f32", 1, 65536, SYN_LANE_THRESH=40), query("mlp f32", 1, 65536, SYN_LANE_THRESH=8),
                       query("mlp f16x2", 1, 65536, SYN_LANE_THRESH=8)])
    assert (a.lane_thresh, b.lane_thresh, c.lane_thresh) == (32, 48, 64)


def test_rollout_search_plan(harness):
    p, = harness([dict(rollout=1, slots=4096, jobs=10000, cap=CAP)])
    assert (p.shape, p.grid, p.threads, p.policy, p.fast, p.n, p.lane_thresh, p.listed) == (4, 8, 512, 1, 0, 8, 64, 1)


SWEEP_W = (16, 4096, 4112, 65536, 65552, 131072, 131088, 196608, 196624, 262144)
CALLS = (dict(mode=1, count=0, prof=0), dict(mode=0, count=0, prof=0), dict(mode=0, count=1, prof=0), dict(mode=0, count=0, prof=1))


def sweep_configs():
    """Every (fpu, noise) with the other switches folded or not; family as mcts.cuh's cfg_family derives it."""
    for fpu, noise, folded in itertools.product((0, 1, 2), (0, 1, 2), (True, False)):
        fam = {0: 1, 2: 2}.get(fpu, 0) if folded and noise == 0 else 0
        yield dict(fpu=fpu, noise=noise, fam=fam)


def plain_under_prof(p):
    """The kernels that have no profiled instantiation, so a profile run plays the plain one: the conv policies, Connect4Net f16x2
    outside the parity family's 12 and 16 waves, the free-running kernel's runtime-switched family."""
    return p.policy in (2, 4) or (p.policy == 3 and not (p.fast == 1 and p.n >= 12)) or (p.shape == 7 and p.fast == 0)


def test_every_plan_names_a_shipped_instantiation(harness):
    queries = [dict(slots=w, jobs=w, cap=CAP, **net, **cfg, **call, **lanes)
               for w in SWEEP_W for net in NETS.values() for cfg in sweep_configs() for call in CALLS
               for lanes in [{}] + [dict(SYN_LANES=n) for n in (4, 8, 12, 16)]]
    for q, p in zip(queries, harness(queries)):
        assert not p.error and p.listed in (1, 2), (q, p)
        if p.listed == 2:
            assert p.prof and plain_under_prof(p), (q, p)
        elif p.prof and p.shape in (4, 7):
            assert not plain_under_prof(p), (q, p)


def test_debug_shape_plans_name_shipped_instantiations(harness):
    """The forced-only shapes of DEBUG_SHAPES=1 builds: producer/consumer, two trees per lane, the pool kernel."""
    knobs = [dict(SYN_PC=2), dict(SYN_LANES2=8), dict(SYN_LANES2=12), dict(SYN_LANES2=8, SYN_L2_TILE=1), dict(SYN_POOL=96),
             dict(SYN_POOL=128, SYN_POOL_NW=8), dict(SYN_POOL=1)]
    queries = [dict(slots=w, jobs=w, cap=CAP, **net, **cfg, **call, **kn)
               for w in (16, 4096, 65552, 262144) for net in NETS.values() for cfg in sweep_configs() for call in CALLS for kn in knobs]
    got = harness(queries, build="debug_shapes")
    for q, p in zip(queries, got):
        assert not p.error and p.listed in (1, 2), (q, p)
        if p.listed == 2:
            assert p.prof and plain_under_prof(p), (q, p)
    assert {5, 6, 8} <= {p.shape for p in got}
    p, = harness([query("mlp f32", 1, 262144, SYN_POOL=96)], build="debug_shapes")
    assert (p.shape, p.grid, p.threads, p.nv, p.fast, p.n) == (8, 228, 768, 96, 1, 12)
    p, = harness([query("mlp f32", 1, 262144, SYN_LANES2=8)], build="debug_shapes")
    assert (p.shape, p.grid, p.threads) == (6, 256, 512)
    # the same knobs mean nothing to the default library
    assert harness([query("mlp f32", 1, 262144, SYN_POOL=96, SYN_LANES2=8, SYN_PC=2)])[0].shape == 4


# ---- plan_eval: which kernel evaluates a batch of n positions
EvalPlan = namedtuple("EvalPlan", "kernel threads grid lds f16_image in_place polled")
TILE, MLP_512, MLP_768, CONV_512, F16_512, F16_1024, CONV_F16_512 = range(7)
LDS = {TILE: 14 * 64 * 16, MLP_512: 30816 * 4, MLP_768: 30816 * 4, CONV_512: 16480 * 4, F16_512: 31080 * 4, F16_1024: 31080 * 4,
       CONV_F16_512: 16932 * 4}


def eval_plans(harness, queries):
    text = "".join(" ".join(f"{k}={int(v)}" for k, v in dict(q, eval=1).items()) + "\n" for q in queries)
    out = subprocess.run([harness.exe], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(queries)
    return [EvalPlan(*map(int, l.split())) for l in out]


# (net / arithmetic, CUs, n, kernel, threads, grid)
EVAL_ROWS = [
    ("mlp f32", 256, 1, TILE, 256, 1),
    ("mlp f32", 256, 16, TILE, 256, 1),
    ("mlp f32", 256, 17, TILE, 256, 2),
    ("mlp f32", 256, 4096, TILE, 256, 256),
    ("mlp f32", 256, 4097, MLP_512, 512, 33),          # 257 tiles over 8 waves
    ("mlp f32", 256, 196592, MLP_512, 512, 256),       # 12,287 tiles: one short of 48 per CU
    ("mlp f32", 256, 196593, MLP_768, 768, 256),
    ("conv f32", 256, 1, CONV_512, 512, 1),
    ("conv f32", 256, 1000000, CONV_512, 512, 256),
    ("mlp f16x2", 256, 1, F16_512, 512, 1),
    ("mlp f16x2", 256, 4096, F16_512, 512, 32),
    ("mlp f16x2", 256, 262128, F16_512, 512, 256),     # 16,383 tiles: one short of 64 per CU
    ("mlp f16x2", 256, 262129, F16_1024, 1024, 256),
    ("conv f16x2", 256, 1, CONV_F16_512, 512, 1),
    ("conv f16x2", 256, 1000000, CONV_F16_512, 512, 256),
    # the two wave-count thresholds scale with the CU count; the tile kernel's 4,096 positions do not
    ("mlp f32", 8, 4096, TILE, 256, 256),
    ("mlp f32", 8, 6128, MLP_512, 512, 8),
    ("mlp f32", 8, 6129, MLP_768, 768, 8),
    ("mlp f16x2", 8, 8176, F16_512, 512, 8),
    ("mlp f16x2", 8, 8177, F16_1024, 1024, 8),
]


def test_eval_plan_rows(harness):
    got = eval_plans(harness, [dict(NETS[net], cus=cus, n=n) for net, cus, n, _, _, _ in EVAL_ROWS])
    for (net, cus, n, kernel, threads, grid), p in zip(EVAL_ROWS, got):
        what = f"{net}, {cus} CUs, n {n}: {p}"
        assert (p.kernel, p.threads, p.grid) == (kernel, threads, grid), what
        assert p.lds == LDS[kernel] and p.f16_image == NETS[net]["f16"], what
        assert not p.in_place and not p.polled, what   # the engine's own launches: neither

    # the evaluation contexts' flags
    queries = [dict(net, n=n, poll_max=pm, zc_out=zc, poll_broken=br)
               for net in NETS.values() for n in (1, 17, 1024, 1025, 4096, 4097, 5000, 8192, 8193)
               for pm, zc in ((1024, 4096), (0, 4096), (1024, 0), (8192, 8192), (8192, 1024)) for br in (0, 1)]
    for q, p in zip(queries, eval_plans(harness, queries)):
        assert p.in_place == (q["n"] <= q["zc_out"]), (q, p)
        assert p.polled == (p.in_place and q["net"] == 0 and not q["f16"] and q["n"] <= q["poll_max"] and not q["poll_broken"]), (q, p)
        if p.polled:
            assert (p.kernel, p.threads, p.grid, p.lds) == (TILE, 256, (q["n"] + 15) // 16, LDS[TILE]), (q, p)
        else:   # the flags change nothing else
            assert p[:5] == eval_plans(harness, [dict(net=q["net"], f16=q["f16"], n=q["n"])])[0][:5], (q, p)
    # a polled call takes the tile kernel even past its 4,096 positions
    p, = eval_plans(harness, [dict(NETS["mlp f32"], n=5000, poll_max=8192, zc_out=8192)])
    assert p.polled and p.in_place and (p.kernel, p.grid) == (TILE, 313)
    p, = eval_plans(harness, [dict(NETS["mlp f32"], n=5000, poll_max=1024, zc_out=8192)])
    assert not p.polled and p.in_place and (p.kernel, p.grid) == (MLP_512, 40)

    # every size: the grid covers the tiles or fills the device, and the LDS fits a CU
    for cus, edges in ((256, (4096, 196592, 262128)), (8, (4096, 6128, 8176))):
        ns = sorted(set(range(1, 300001, 997)) | {n for e in edges for n in range(e - 40, e + 41)})
        for net in NETS.values():
            kernels = {(0, 0): (TILE, MLP_512, MLP_768), (0, 1): (F16_512, F16_1024), (1, 0): (CONV_512,), (1, 1): (CONV_F16_512,)}[net["net"], net["f16"]]
            for n, p in zip(ns, eval_plans(harness, [dict(net, cus=cus, n=n) for n in ns])):
                tiles, waves = (n + 15) // 16, p.threads // 64
                assert p.kernel in kernels and p.lds == LDS[p.kernel] <= 160 * 1024 and p.threads % 64 == 0, (net, cus, n, p)
                assert p.grid >= 1 and (p.grid * waves >= min(tiles, cus * waves) or p.grid == cus), (net, cus, n, p)
                assert p.kernel != TILE or p.grid == tiles, (net, cus, n, p)
