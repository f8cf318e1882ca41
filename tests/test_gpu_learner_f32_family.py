"""The f32 learners on the GPU against the oracle, bit for bit, over the stress family of tests/learner_f32_family.py: gradients, losses,
weights, m, v and step. Every chosen input is finite on the oracle — tests/test_learner_f32_family.py asserts it for the steps of the
table, and each test here asserts it for the oracle steps it adds (the step route's second step, the data-parallel route's second
gradient, micro mode) — so the comparison is exact equality (same_bits).

The table (lf.CASES; a case = network, member, target variant, batch size, hyper-parameter set, route, steps) is NOT the full cross
product. What is crossed, per network:

  route   kernels                                                        cases
  step    train_step: queued gradient kernels + the fused Adam           every member once, the 8 target variants, the batch sizes
          (Connect4Net) / adam_kernel; two steps, the state compared     (Connect4Net 1, 31, 32, 33, 100; Connect4ConvNet 1, 17, 32) and the 3
          after each                                                     hyper-parameter sets cycling along the member list (`duplicates`
                                                                         always at B = 32); plus the must-members below
  dp      train_gradients_device + train_apply_device (adam_kernel),     the must-members, and init / recorded / B = 32 / (1e-3, 0.7, 1.9)
          grad_scale = 0.5 at lr = 1e-3, then a second gradient and
          grad_scale = 0.25 at lr = 0 (the data-parallel route)
  epoch   train_set_data + train_epoch, 6 steps through a permutation    the must-members at B = 32 (Connect4ConvNet: 32 and 17), and
          that is not the identity: the persistent kernels; Connect4Net  init / tsum_half / default at B = 33 (Connect4Net) or 17; the last
          at B = 33 the queued launches                                  state is also held to the float64 bars
  micro   SYN_TRAIN_BATCH_MICRO at 96 positions (nb = 3), two steps      the must-members, and init / onehot / (1e-3, 0.7, 1.9)
          through train_step, against tests/micro_batch_model.combine
          of the oracle's per-32 gradients and oracle.train_adam
  child   the epoch route's cases in a fresh process with                trained, the first subnormal member and zero
          SYN_TRAIN_QUEUED=1 (Connect4Net) / SYN_TRAIN_CONV_MW=0

  must-members, always with weight_decay = 0, alternating between the zero_row and the subnormal_t batch: trained, the subnormal members
  (Connect4Net: mlp_init_x2^-30, mlp_init_x2^-28, init_x2^-16; Connect4ConvNet: conv_init_x2^-118), zero, and the gate-at-zero member.

Not crossed: most (member, variant) pairs; B = 1 and B = 100 run on the step route only, B = 31 on step only; the (1e-3, 0.7, 1.9) set
meets the subnormal members on no route (with a weight decay their gradients are normal numbers); the child route runs three members.
tests/test_learner_f32_family.py::test_the_table_covers_what_the_issue_lists asserts what every route must hold.
Which kernel ran is NOT observable: the engine may fall back from a persistent epoch kernel to the queued launches, or from the
four-workgroup conv kernel to the one-workgroup one (a failed start-up self-check, workgroups that cannot be co-resident), and has no
getter that reports it. `epoch` therefore means "train_epoch in the default mode" and `child` "train_epoch with the knob set": the bits
are held either way, but on an engine that fell back the two routes would cover the same kernel twice and this file could not tell.
The bf16 conv learner has its own model (tests/conv_bf16_learner_model.py); here only its Adam runs the weight_decay = 0 and subnormal-v
cases against oracle.train_adam, which it shares with the f32 learner.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import learner_f32_family as lf
from tests import micro_batch_model as mm
from tests.f16x2_checkpoints import same_bits

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATE = ("weights", "m", "v")


@pytest.fixture(scope="module")
def engines():
    import synthesis_amd as sa

    e = {}
    for net in lf.NETS:
        e[net] = sa.Engine(concurrent_games=64, max_explores=64)
        (e[net].load_weights if net == "mlp" else e[net].load_weights_conv)(lf.family(net)["init"])
    yield e
    for eng in e.values():
        eng.close()


init = lf.trainer_init


def where_differs(net, a, b):
    """Which blocks differ and in which magnitude class: the first thing to read when a comparison fails."""
    a = np.asarray(a, np.float32); b = np.asarray(b, np.float32)
    out = {}
    for name, sl in lf.BLOCKS[net].items():
        d = a[sl].view(np.uint32) != b[sl].view(np.uint32)
        if d.any():
            ref = np.abs(b[sl][d])
            out[name] = dict(entries=int(d.sum()), subnormal=int(((ref > 0) & (ref < lf.F32_TINY)).sum()), zero=int((ref == 0).sum()),
                             max_abs_diff=float(np.abs(a[sl][d].astype(np.float64) - b[sl][d]).max()))
    return out


def assert_state(tag, net, st, ref, losses=None, keys=STATE + ("grads",)):
    assert st["step"] == ref["step"], tag
    if losses is not None:
        assert same_bits(losses, ref["losses"]), (tag, "losses", losses, ref["losses"])
    for k in keys:
        assert same_bits(st[k], ref[k]), (tag, k, where_differs(net, st[k], ref[k]))


def assert_finite(tag, hist):
    assert all(np.isfinite(h[k]).all() for h in hist for k in STATE + ("grads", "losses")), tag


def ids(route):
    return dict(argvalues=lf.cases(route=route), ids=[c.id for c in lf.cases(route=route)])


# ---- step
@pytest.mark.parametrize("c", **ids("step"))
def test_train_step(engines, oracle, c):
    eng, bs = engines[c.net], lf.batches(c.variant, c.B, 2)
    hist = lf.oracle_steps(oracle, c.net, lf.family(c.net)[c.member], bs, c.hyper, [lf.LR, lf.LR])
    assert_finite(c.id, hist)   # the second step is not among the CPU file's: same_bits would take NaN for NaN
    init(eng, c)
    for s in range(2):
        l = eng.train_step(bs[0][s], bs[1][s], bs[2][s], bs[3][s], lf.LR)
        assert_state((c.id, s), c.net, eng.trainer_state(), hist[s], l)


# ---- dp
def to_device(b):
    import torch

    d = [torch.from_numpy(b[0].astype(np.int64)).cuda(), torch.from_numpy(b[1].astype(np.int64)).cuda(),
         torch.from_numpy(np.ascontiguousarray(b[2])).cuda(), torch.from_numpy(np.ascontiguousarray(b[3])).cuda()]
    torch.cuda.synchronize()
    return d


@pytest.mark.parametrize("c", **ids("dp"))
def test_gradients_device_then_apply_device(engines, oracle, c):
    import torch

    eng, bs, hp = engines[c.net], lf.batches(c.variant, c.B, 2), lf.oracle_hyper(c.hyper)
    w = np.array(lf.family(c.net)[c.member]); m, v, step = np.zeros_like(w), np.zeros_like(w), 0
    init(eng, c)
    for s, (lr, scale) in enumerate(((lf.LR, 0.5), (0.0, 0.25))):
        b = tuple(a[s] for a in bs)
        d = to_device(b)
        g = torch.full((w.size,), float("nan"), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        l = eng.train_gradients_device(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), c.B, g.data_ptr())
        go, lo = lf.oracle_gradients(oracle, c.net, w, c.hyper, b)
        gd = g.cpu().numpy()
        assert np.isfinite(go).all() and np.isfinite(lo).all(), (c.id, s)
        assert same_bits(gd, go), (c.id, s, where_differs(c.net, gd, go))
        assert same_bits(l, lo), (c.id, s, l, lo)
        eng.train_apply_device(g.data_ptr(), lr, grad_scale=scale)
        w_before = w
        w, m, v, step = oracle.train_adam(w, hp, go * np.float32(scale), lr, m, v, step)
        assert all(np.isfinite(a).all() for a in (w, m, v)), (c.id, s)
        assert_state((c.id, s), c.net, eng.trainer_state(), dict(weights=w, m=m, v=v, step=step), keys=STATE)
        if lr == 0.0:
            assert same_bits(w, w_before)   # (the oracle's own: w - 0 * (m / denom) with a finite quotient)


# ---- epoch
@pytest.mark.parametrize("c", **ids("epoch"))
def test_train_epoch(engines, oracle, c):
    eng = engines[c.net]
    ref = lf.final_state(lf.oracle_steps(oracle, c.net, lf.family(c.net)[c.member], lf.case_batches(c), c.hyper, [lf.LR] * c.steps))
    st, losses = lf.run_epoch(eng, c)
    assert_state(c.id, c.net, st, ref, losses)
    f64 = lf.case_reference(c)
    if not f64["gate_fragile"]:
        lf.check_bars(c.id, c.net, f64, dict(st, losses=losses))


# ---- micro
def micro_gradients(oracle, net, w, hyper, b):
    parts = [lf.oracle_gradients(oracle, net, w, hyper, tuple(a[o:o + mm.BLOCK] for a in b)) for o in range(0, lf.MICRO_B, mm.BLOCK)]
    return mm.combine([g for g, _ in parts]), mm.combine([l for _, l in parts])


@pytest.mark.parametrize("c", **ids("micro"))
def test_micro_mode(engines, oracle, c):
    eng, bs = engines[c.net], lf.case_batches(c)
    hist = lf.oracle_steps(oracle, c.net, lf.family(c.net)[c.member], bs, c.hyper, [lf.LR] * c.steps, gradients=micro_gradients)
    assert_finite(c.id, hist)
    init(eng, c)
    eng.trainer_set_batch_mode("micro")
    for s in range(c.steps):
        l = eng.train_step(bs[0][s], bs[1][s], bs[2][s], bs[3][s], lf.LR)
        assert_state((c.id, s), c.net, eng.trainer_state(), hist[s], l)
    assert eng.trainer_batch_mode() == ("micro", 0, lf.MICRO_B // mm.BLOCK)


# ---- child
CHILD = (
    "import sys, numpy as np\n"
    "sys.path.insert(0, sys.argv[1])\n"
    "import synthesis_amd as sa\n"
    "from tests import learner_f32_family as lf\n"
    "net = sys.argv[2]\n"
    "eng = sa.Engine(concurrent_games=64, max_explores=16)\n"
    "(eng.load_weights if net == 'mlp' else eng.load_weights_conv)(lf.family(net)['init'])\n"
    "out = {}\n"
    "for c in lf.cases(net, 'child'):\n"
    "    st, losses = lf.run_epoch(eng, c)\n"
    "    out.update({c.id + '.' + k: st[k] for k in ('weights', 'm', 'v', 'grads')})\n"
    "    out[c.id + '.losses'] = losses; out[c.id + '.step'] = np.int64(st['step'])\n"
    "eng.close()\n"
    "np.savez(sys.argv[3], **out)\n")
KNOBS = dict(mlp={"SYN_DEBUG": "1", "SYN_TRAIN_QUEUED": "1"}, conv={"SYN_DEBUG": "1", "SYN_TRAIN_CONV_MW": "0"})


@pytest.mark.parametrize("net", lf.NETS)
def test_persistent_kernel_alternatives_in_a_child(tmp_path, oracle, net):
    """The knobs are read once per process: a fresh child, under its own time limit, runs the three child cases through the queued
    launches (Connect4Net) / the one-workgroup kernel (Connect4ConvNet); the parent compares with the oracle."""
    env = {k: v for k, v in os.environ.items() if not k.startswith("SYN_")}
    env.update(KNOBS[net])
    path = str(tmp_path / "out.npz")
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT, net, path], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert r.returncode == 0, r.stdout.decode()[-2000:]
    out = np.load(path)
    for c in lf.cases(net, "child"):
        ref = lf.final_state(lf.oracle_steps(oracle, net, lf.family(net)[c.member], lf.case_batches(c), c.hyper, [lf.LR] * c.steps))
        st = {k: out[c.id + "." + k] for k in STATE + ("grads",)}
        st["step"] = int(out[c.id + ".step"])
        assert_state(c.id, net, st, ref, out[c.id + ".losses"])


# ---- the bf16 conv learner's Adam
def test_bf16_conv_adam_at_weight_decay_0_and_subnormal_v(engines, oracle):
    """Six bf16 steps from the subnormal member with weight_decay = 0: every step's weights, m and v are oracle.train_adam applied to the
    gradient the device reports for that step (the gradient itself belongs to tests/test_gpu_conv_bf16_learner.py)."""
    eng = engines["conv"]
    c = [c for c in lf.cases("conv", "epoch") if c.member == lf.SUBNORMAL_MEMBERS["conv"][0]][0]
    bs, hp = lf.case_batches(c), lf.oracle_hyper(c.hyper)
    assert c.hyper == "wd0"
    init(eng, c)
    eng.trainer_set_precision("bf16")
    w = np.array(lf.family("conv")[c.member]); m, v, step = np.zeros_like(w), np.zeros_like(w), 0
    seen = 0
    for s in range(c.steps):
        eng.train_step(bs[0][s], bs[1][s], bs[2][s], bs[3][s], lf.LR)
        st = eng.trainer_state()
        w, m, v, step = oracle.train_adam(w, hp, st["grads"], lf.LR, m, v, step)
        assert_state((c.id, "bf16", s), "conv", st, dict(weights=w, m=m, v=v, step=step), keys=STATE)
        seen = max(seen, lf.count_subnormal(v))
    assert seen >= 100, seen   # the premise: subnormal v entries did occur
    init(eng, c)   # leaves the engine in f32
