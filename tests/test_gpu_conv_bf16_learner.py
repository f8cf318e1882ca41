"""The bf16 variant of the Connect4ConvNet learner (train_conv_mfma.cuh: conv_grad_step_bf16 and the BF16 branches of the four-workgroup
epoch kernel) against the float64 rounded-operand model of tests/conv_bf16_learner_model.py, on its checkpoint and batch family.

Bars (conv_bf16_learner_model.py; none comes from a kernel): on the exact-forward members the losses and the 12 head-bias gradients are
the f32 oracle's bits and every other gradient is inside n * 2^-23 * sum|terms| + flips of the model; on every other member each
gradient is inside max(8 x the f32 random-order floor of its block, that derived term). Entries that must be exact zeros are compared as
bits, and the Adam half is oracle.train_adam applied to the device's own gradients, bit for bit. The figures of a run are printed (-s);
profiles/conv_bf16_learner_bars.txt keeps those of the run the bars were first held on."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import conv_bf16_learner_model as M
from tests.oracle_lib import default_train_hyper

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LR = 2e-3
EPOCH_CASES = (("trained", 32), ("trained", 17), ("grid", 32), ("grid", 17))
EPOCH_STEPS = 3


@pytest.fixture(scope="module")
def engine():
    import synthesis_amd as sa

    eng = sa.Engine(concurrent_games=64, max_explores=16, device=0)
    eng.load_weights_conv(M.family()["init"])
    yield eng
    eng.close()


def bf16_trainer(eng, blob, pw=1.0, vw=1.0):
    eng.trainer_init_conv(blob, policy_weight=pw, value_weight=vw)
    eng.trainer_set_precision("bf16")


def assert_adam(oracle, tag, before, after, hp, lr):
    """`after` is oracle.train_adam applied to `before` with the DEVICE's gradients (after["grads"]), bit for bit."""
    w, m, v, step = oracle.train_adam(before["weights"], hp, after["grads"], lr, before["m"], before["v"], before["step"])
    assert after["step"] == step, tag
    for k, ref in (("weights", w), ("m", m), ("v", v)):
        assert np.array_equal(after[k].view(np.uint32), ref.view(np.uint32)), (tag, k)


@pytest.mark.parametrize("member", M.MEMBERS)
def test_single_step_meets_the_model(engine, oracle, member):
    blob = M.family()[member]
    exact = member in M.EXACT_FORWARD
    zeros = M.exact_zero_entries(member)
    for B in M.BATCHES:
        c = M.case(member, B)
        my, op, tpi, tv = c["batch"]
        hp = default_train_hyper(policy_weight=c["pw"], value_weight=c["vw"])
        bf16_trainer(engine, blob, c["pw"], c["vw"])
        before = engine.trainer_state()
        losses = engine.train_step(my, op, tpi, tv, LR)
        st = engine.trainer_state()
        go, lo = oracle.convtrain_gradients(blob, hp, my, op, tpi, tv) if exact else (None, None)
        M.check_device(f"{member} B={B}", c, st["grads"], losses, go, lo, exact_forward=exact)
        assert not st["grads"].view(np.uint32)[zeros].any(), (member, B, "entries that must be exact zeros")
        if B > 1:
            assert not np.array_equal(st["grads"], oracle.convtrain_gradients(blob, hp, my, op, tpi, tv)[0])   # (it is the other arithmetic)
        assert_adam(oracle, f"{member} B={B}", before, st, hp, LR)


def epoch_data():
    """96 rows (the hand-made ones behind as many golden positions as fill it) and a permutation with repeated and out-of-order indices."""
    my, op, tpi, tv, _ = M.pool()
    rows = np.concatenate([np.arange(96 - (my.size - 256)), np.arange(256, my.size)])
    assert rows.size == 96 and my.size > 256
    perm = np.random.default_rng(7).integers(0, 96, size=EPOCH_STEPS * 32).astype(np.int32)
    assert np.unique(perm).size < perm.size and (np.diff(perm) < 0).any()
    return my[rows], op[rows], tpi[rows], tv[rows], perm


def epoch_runs(eng):
    """{(member, B): (losses of 1, 2, .. EPOCH_STEPS steps, states after them)}: the same epoch cut short after every step, each from a
    fresh trainer (deterministic: the shorter run's weights are the longer run's weights before its last step)."""
    my, op, tpi, tv, perm = epoch_data()
    out = {}
    for member, B in EPOCH_CASES:
        pw, vw = M.loss_weights(B)
        runs = []
        for n in range(1, EPOCH_STEPS + 1):
            bf16_trainer(eng, M.family()[member], pw, vw)
            eng.train_set_data(my, op, tpi, tv)
            losses = eng.train_epoch(perm[: n * B], B, LR)
            runs.append((losses, eng.trainer_state()))
        out[(member, B)] = runs
    return out


def save_epoch_runs(path):
    """The child-process half of test_epoch_kernels_meet_the_model (a debug knob selects the kernel; knobs are read once per process)."""
    import synthesis_amd as sa

    eng = sa.Engine(concurrent_games=64, max_explores=16, device=0)
    eng.load_weights_conv(M.family()["init"])
    flat = {}
    for (member, B), runs in epoch_runs(eng).items():
        for n, (losses, st) in enumerate(runs):
            flat[f"{member}|{B}|{n}|losses"] = losses
            for k in ("weights", "m", "v", "grads"):
                flat[f"{member}|{B}|{n}|{k}"] = st[k]
            flat[f"{member}|{B}|{n}|step"] = np.int64(st["step"])
    eng.close()
    np.savez(path, **flat)


_bars_at = {}   # (weights' bytes, member, B, step) -> measured_bars: the one-workgroup run reaches the four-workgroup run's weights


def check_epoch_runs(oracle, tag, runs_by_case):
    my, op, tpi, tv, perm = epoch_data()
    for (member, B), runs in runs_by_case.items():
        pw, vw = M.loss_weights(B)
        hp = default_train_hyper(policy_weight=pw, value_weight=vw)
        full_losses, last = runs[-1]
        assert last["step"] == EPOCH_STEPS and full_losses.shape == (EPOCH_STEPS, 2)
        w = M.family()[member]
        before = dict(weights=w, m=np.zeros_like(w), v=np.zeros_like(w), step=0)
        for n, (losses, st) in enumerate(runs):
            idx = perm[n * B:(n + 1) * B]
            batch = (my[idx], op[idx], tpi[idx], tv[idx])
            # the shorter runs are prefixes of the full one
            assert np.array_equal(losses.view(np.uint32), full_losses[: n + 1].view(np.uint32)), (tag, member, B, n)
            key = (before["weights"].tobytes(), member, B, n)
            if key not in _bars_at:
                _bars_at[key] = M.measured_bars(before["weights"], *batch, pw, vw)
            c = _bars_at[key]
            name = f"{tag} {member} B={B} step {n + 1}"
            if n == 0 and member in M.EXACT_FORWARD:   # exact logits: the oracle's H phase, bit for bit
                lo = oracle.convtrain_gradients(before["weights"], hp, *batch)[1]
                assert np.array_equal(losses[0].view(np.uint32), lo.view(np.uint32)), name
            M.check_device(name, c, st["grads"], losses[n])
            assert_adam(oracle, name, before, st, hp, LR)
            before = st


def test_epoch_kernels_meet_the_model(engine, oracle, tmp_path):
    """train_set_data + train_epoch: the four-workgroup kernel (the default) in this process, the one-workgroup kernel in a child. After
    every step of the epoch: the step's gradients and loss against the model at the weights before that step, and the Adam update."""
    inproc = epoch_runs(engine)
    check_epoch_runs(oracle, "four workgroups", inproc)
    path = str(tmp_path / "one_wg.npz")
    env = {k: v for k, v in os.environ.items() if not k.startswith("SYN_")}
    env.update(SYN_DEBUG="1", SYN_TRAIN_CONV_MW="0")
    code = f"import sys; sys.path.insert(0, {ROOT!r}); from tests.test_gpu_conv_bf16_learner import save_epoch_runs; save_epoch_runs({path!r})"
    r = subprocess.run([sys.executable, "-c", code], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert r.returncode == 0, r.stdout.decode()[-2000:]
    z = np.load(path)
    child = {}
    for member, B in EPOCH_CASES:
        child[(member, B)] = [(z[f"{member}|{B}|{n}|losses"],
                               dict({k: z[f"{member}|{B}|{n}|{k}"] for k in ("weights", "m", "v", "grads")}, step=int(z[f"{member}|{B}|{n}|step"])))
                              for n in range(EPOCH_STEPS)]
    check_epoch_runs(oracle, "one workgroup", child)


def test_eight_chained_steps_meet_the_model(engine, oracle, golden_dir):
    g = np.load(os.path.join(golden_dir, "conv_train_torch_goldens.npz"))
    hp = default_train_hyper()
    bf16_trainer(engine, M.family()["init"])
    before = engine.trainer_state()
    for s in range(8):
        batch = (g["my_bb"][s], g["op_bb"][s], g["target_pi"][s], g["target_v"][s])
        c = M.measured_bars(before["weights"], *batch, 1.0, 1.0)
        losses = engine.train_step(*batch, float(g["lrs"][s]))
        st = engine.trainer_state()
        M.check_device(f"chained step {s + 1}", c, st["grads"], losses)
        assert_adam(oracle, f"chained step {s + 1}", before, st, hp, float(g["lrs"][s]))
        before = st
    assert before["step"] == 8


def test_data_parallel_gradients_are_the_steps_bits(engine):
    """train_gradients_device (the data-parallel half) in bf16: the bits of train_step's gradients and losses, B = 17."""
    import torch

    c = M.case("trained", 17)
    my, op, tpi, tv = c["batch"]
    bf16_trainer(engine, c["blob"], c["pw"], c["vw"])
    d_my = torch.from_numpy(my.astype(np.int64)).cuda(); d_op = torch.from_numpy(op.astype(np.int64)).cuda()
    d_tpi = torch.from_numpy(np.ascontiguousarray(tpi)).cuda(); d_tv = torch.from_numpy(np.ascontiguousarray(tv)).cuda()
    d_g = torch.zeros(M.NUM, dtype=torch.float32, device="cuda")
    ld = engine.train_gradients_device(d_my.data_ptr(), d_op.data_ptr(), d_tpi.data_ptr(), d_tv.data_ptr(), 17, d_g.data_ptr())
    torch.cuda.synchronize()
    gd = d_g.cpu().numpy()
    assert engine.trainer_state()["step"] == 0
    ls = engine.train_step(my, op, tpi, tv, 0.0)
    gs = engine.trainer_state()["grads"]
    assert np.array_equal(gd.view(np.uint32), gs.view(np.uint32)) and np.array_equal(ld.view(np.uint32), ls.view(np.uint32))
    M.check_device("data-parallel trained B=17", c, gd, ld)
