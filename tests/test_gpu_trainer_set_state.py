"""syn_trainer_set_state (include/synthesis_amd.h): a learner that is read out, put into another engine and continued there leaves the
bits of the learner that never stopped — on every route a step can take, for both networks.

Per route: engine A runs K steps, its state is read (trainer_state) and A runs J more; engine B is initialised from a DIFFERENT blob,
given the same modes, then trainer_set_state and the same data set, and runs the same J; engine C runs the K + J steps without a
stop (the epoch routes: in ONE call). Parameters, moments, step count and every step's losses are compared bit for bit. The unit of
the sampled route is an epoch (10 steps over the 320 rows): K and J epochs."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

K, J, ROWS = 3, 5, 320
INVALID, NO_WEIGHTS = -1, -4
ROUTES = ("step", "epoch", "micro", "sampled", "bf16")


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.fixture(scope="module")
def blobs(golden_dir):
    from bench import make_conv_weights, make_weights

    return dict(mlp=(np.load(os.path.join(golden_dir, "c4net_blob_f32.npy")), make_weights(5)),
                conv=(make_conv_weights(), make_conv_weights(5)))


@pytest.fixture(scope="module")
def data():
    """320 rows of plausible training data, made once: boards, and targets that are distributions"""
    rng = np.random.default_rng(2024)
    my = rng.integers(0, 1 << 63, ROWS, dtype=np.uint64)
    op = rng.integers(0, 1 << 63, ROWS, dtype=np.uint64) & ~my
    pi = rng.random((ROWS, 9), dtype=np.float32)
    v = rng.random((ROWS, 3), dtype=np.float32)
    return my, op, pi / pi.sum(1, keepdims=True), v / v.sum(1, keepdims=True)


@pytest.fixture(scope="module")
def engines():
    import synthesis_amd as sa

    made = [sa.Engine(concurrent_games=64, max_explores=40) for _ in range(3)]
    yield made
    for e in made:
        e.close()


def start(eng, net, blob, route, data):
    (eng.trainer_init_conv if net == "conv" else eng.trainer_init)(blob)
    if route == "micro":
        eng.trainer_set_batch_mode("micro", 3)
    if route == "bf16":
        eng.trainer_set_precision("bf16")
    return eng


def run(eng, route, data, first, count):
    """steps (the sampled route: epochs) first .. first + count - 1 of the route; returns their losses"""
    my, op, pi, v = data
    if route == "step":
        return np.stack([eng.train_step(my[32 * s: 32 * s + 32], op[32 * s: 32 * s + 32], pi[32 * s: 32 * s + 32], v[32 * s: 32 * s + 32], 1e-3)
                         for s in range(first, first + count)])
    if route == "sampled":
        return eng.train_epochs_sampled(0xABCDEF0123, count, 32, 1e-3, first_epoch=first, flip=True)
    batch = 64 if route == "micro" else 32
    order = np.random.default_rng(11).integers(0, ROWS, (K + J) * batch)    # (micro: 512 draws from 320 rows, rows recur)
    return eng.train_epoch(order[first * batch: (first + count) * batch], batch, 1e-3)


def state(eng):
    S = eng.trainer_state()
    return S["weights"], S["m"], S["v"], S["step"]


# (the bf16 variant exists for the Connect4ConvNet learner only: syn_trainer_set_precision refuses Connect4Net)
@pytest.mark.parametrize("net,route", [(n, r) for n in ("mlp", "conv") for r in ROUTES if (n, r) != ("mlp", "bf16")])
def test_a_restored_learner_continues_bit_for_bit(engines, blobs, data, net, route):
    a, b, c = engines
    blob, other = blobs[net]
    per = 10 if route == "sampled" else 1    # optimiser steps per unit
    # A: K, read out, J more
    start(a, net, blob, route, data).train_set_data(*data)
    first_losses = run(a, route, data, 0, K)
    w, m, v, step = state(a)
    assert step == K * per and not same(w, blob) and np.abs(m).max() > 0
    a_losses = run(a, route, data, K, J)
    # B: another network's trainer, the same modes, A's state, then the data set
    start(b, net, other, route, data)
    b.trainer_set_state(w, m, v, step)
    got = state(b)
    assert same(got[0], w) and same(got[1], m) and same(got[2], v) and got[3] == step
    b.train_set_data(*data)
    b_losses = run(b, route, data, K, J)
    # C: never stopped
    start(c, net, blob, route, data).train_set_data(*data)
    c_losses = run(c, route, data, 0, K + J)
    assert same(b_losses, a_losses)
    assert same(c_losses.reshape(-1, 2), np.concatenate([first_losses.reshape(-1, 2), a_losses.reshape(-1, 2)]))
    A, B, Cn = state(a), state(b), state(c)
    assert A[3] == B[3] == Cn[3] == (K + J) * per
    for i, name in enumerate(("weights", "m", "v")):
        assert same(A[i], B[i]), (name, "restored")
        assert same(A[i], Cn[i]), (name, "never stopped")
    assert np.isfinite(A[0]).all() and not same(A[0], w)


@pytest.mark.parametrize("net", ("mlp", "conv"))
def test_set_then_get_and_what_stays(engines, blobs, data, net):
    eng = engines[0]
    blob, other = blobs[net]
    (eng.load_weights_conv if net == "conv" else eng.load_weights)(other)
    start(eng, net, blob, "micro", data).train_set_data(*data)
    eng.dataset_set(*(x[:33] for x in data))
    run(eng, "micro", data, 0, 1)                      # leaves a last gradient
    rng = np.random.default_rng(3)
    w, m, v = (rng.integers(0, 1 << 32, blob.size, dtype=np.uint32).view(np.float32) for _ in range(3))   # NaNs, infinities, -0.0: restored as they are
    my, op = data[0][:16], data[1][:16]
    before = [eng.trainer_state()["grads"].tobytes(), [x.tobytes() for x in eng.train_get_data().values()],
              [x.tobytes() for x in eng.dataset_get().values()], [x.tobytes() for x in eng.policy_eval(my, op)], eng.trainer_batch_mode(),
              eng.state_digest("network"), eng.dataset_counts()]
    step = (1 << 40) + 17
    eng.trainer_set_state(w, m, v, step)
    S = eng.trainer_state()
    assert same(S["weights"], w) and same(S["m"], m) and same(S["v"], v) and S["step"] == step
    after = [S["grads"].tobytes(), [x.tobytes() for x in eng.train_get_data().values()], [x.tobytes() for x in eng.dataset_get().values()],
             [x.tobytes() for x in eng.policy_eval(my, op)], eng.trainer_batch_mode(), eng.state_digest("network"), eng.dataset_counts()]
    assert after == before


def test_refusals_leave_the_trainer_alone(engines, blobs, data):
    import synthesis_amd as sa

    eng = engines[0]
    blob, other = blobs["mlp"]
    start(eng, "mlp", blob, "step", data)
    run(eng, "step", data, 0, 2)
    word = eng.state_digest("trainer")
    conv = blobs["conv"][0]
    for args in ((conv, conv, conv, 1), (other, other, other, -1), (other[:-1], other[:-1], other[:-1], 1)):
        with pytest.raises(sa.SynthesisAmdError) as e:
            eng.trainer_set_state(*args)
        assert e.value.code == INVALID
        assert eng.state_digest("trainer") == word
    p = other.ctypes.data_as(C.c_void_p)
    for ptrs in ((None, p, p), (p, None, p), (p, p, None)):
        assert eng._lib.syn_trainer_set_state(eng._h, *ptrs, other.size, 1) == INVALID
        assert eng.state_digest("trainer") == word
    with pytest.raises(ValueError):
        eng.trainer_set_state(other, other[:-1], other, 1)
    with sa.Engine(concurrent_games=64, max_explores=40) as fresh:
        with pytest.raises(sa.SynthesisAmdError) as e:
            fresh.trainer_set_state(other, other, other, 1)
        assert e.value.code == NO_WEIGHTS
