"""The device-side epoch sampler (include/synthesis_amd.h "Device-side epoch sampler"; csrc/sampler_kernels.cuh) on the GPU: the order
and the flags against the numpy model (tests/sampler_model.py), and syn_train_epochs_sampled against the existing call — a twin that
uploads the rows the model flips (positions_mirror) and runs train_epoch on the model's order — bit for bit on every route."""
import ctypes as C

import numpy as np
import pytest

from tests import micro_batch_model as data
from tests import sampler_model as model

pytestmark = pytest.mark.gpu

INVALID, NO_WEIGHTS = -1, -4
N, E, LR, KEY = 100, 3, 2e-3, 0xC0FFEE12345678


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def new_engine(net):
    import synthesis_amd as sa

    eng = sa.Engine(concurrent_games=64, max_explores=64)
    (eng.load_weights if net == "mlp" else eng.load_weights_conv)(data.blob_of(net))
    return eng


@pytest.fixture(scope="module")
def engines():
    e = {net: new_engine(net) for net in ("mlp", "conv")}
    yield e
    for eng in e.values():
        eng.close()


@pytest.fixture(scope="module")
def rows(oracle):
    """The first N pool rows (the all-zero and the one-hot policy target among them): (my, op, tpi, tv)"""
    p = data.pool(oracle)
    return tuple(np.array(p[k][:N]) for k in ("my", "op", "tpi", "tv"))


def start(eng, net, rows, mode="chained", precision="f32", n=N):
    """The learner at its start with the first n rows as its data set"""
    (eng.trainer_init if net == "mlp" else eng.trainer_init_conv)(data.blob_of(net), **data.HYPER)
    if precision != "f32":
        eng.trainer_set_precision(precision)
    if mode != "chained":
        eng.trainer_set_batch_mode(mode)
    eng.train_set_data(*(a[:n] for a in rows))


def assert_same_state(a, b, what=""):
    assert a["step"] == b["step"], what
    for k in ("weights", "m", "v"):
        assert same(a[k], b[k]), (what, k)


def twin_epochs(eng, rows, key, epochs, batch, lr, flip):
    """The existing call, epoch by epoch: the data set with the model's flagged rows mirrored, train_epoch on the model's order"""
    my, op, tpi, tv = rows
    n, n_steps = my.size, my.size // batch
    fmy, fop, fpi = eng.positions_mirror(my, op, tpi)
    losses = []
    for e in epochs:
        perm, flags = model.sampler(key, e, n)
        f = flags.astype(bool) if flip else np.zeros(n, bool)
        eng.train_set_data(np.where(f, fmy, my), np.where(f, fop, op), np.where(f[:, None], fpi, tpi), tv)
        losses.append(eng.train_epoch(perm[: n_steps * batch], batch, lr))
    return np.stack(losses)


# ---- the sampler alone
@pytest.mark.parametrize("n", [1, 2, 31, 32, 33, 255, 256, 257, 1000, 70001])
def test_debug_sampler_equals_the_model(engines, n):
    """one lane, one wave +- 1, one workgroup +- 1, several sort tiles; the extreme keys and epochs"""
    eng = engines["mlp"]
    for key in (0, 1, (1 << 64) - 1):
        for epoch in (0, 1, (1 << 32) - 1):
            perm, flags = eng.debug_sampler(key, epoch, n)
            want_perm, want_flags = model.sampler(key, epoch, n)
            assert perm.dtype == np.int32 and flags.dtype == np.uint8
            assert np.array_equal(perm, want_perm), (key, epoch)
            assert np.array_equal(flags, want_flags), (key, epoch)


# ---- epochs against the existing call
ROUTES = {
    "mlp-32": ("mlp", 32, "chained", "f32", False),           # persistent kernel: 3 steps, 4 rows dropped
    "mlp-7": ("mlp", 7, "chained", "f32", False),
    "mlp-64-chained": ("mlp", 64, "chained", "f32", False),   # queued launches
    "mlp-64-micro": ("mlp", 64, "micro", "f32", False),
    "conv-32-f32": ("conv", 32, "chained", "f32", False),
    "conv-32-bf16": ("conv", 32, "chained", "bf16", False),
    "conv-64-micro": ("conv", 64, "micro", "f32", False),
    "mlp-32-recovery": ("mlp", 32, "chained", "f32", True),   # SYN_DEBUG=1 SYN_TRAIN_FORCE_ABORT=1: snapshot, give-up, queued
}


@pytest.mark.parametrize("flip", [False, True], ids=["noflip", "flip"])
@pytest.mark.parametrize("route", list(ROUTES))
def test_sampled_epochs_equal_the_existing_call(engines, rows, monkeypatch, route, flip):
    net, batch, mode, precision, force_abort = ROUTES[route]
    eng = engines[net]
    start(eng, net, rows, mode, precision)
    before = eng.train_get_data()
    if force_abort:
        monkeypatch.setenv("SYN_DEBUG", "1")
        monkeypatch.setenv("SYN_TRAIN_FORCE_ABORT", "1")
    got_losses = eng.train_epochs_sampled(KEY, E, batch, LR, flip=flip)
    if force_abort:
        monkeypatch.delenv("SYN_TRAIN_FORCE_ABORT")
        monkeypatch.delenv("SYN_DEBUG")
    got = eng.trainer_state()
    after = eng.train_get_data()
    for k in before:   # the stored data set is never modified
        assert same(before[k], after[k]) if before[k].dtype == np.float32 else np.array_equal(before[k], after[k]), k
    assert got_losses.shape == (E, N // batch, 2) and got["step"] == E * (N // batch)

    start(eng, net, rows, mode, precision)
    want_losses = twin_epochs(eng, rows, KEY, range(E), batch, LR, flip)
    want = eng.trainer_state()
    assert same(got_losses, want_losses)
    assert_same_state(got, want, route)
    assert not same(got["weights"], data.blob_of(net))


def test_flip_trains_other_weights(engines, rows):
    """flip on and off train different weights on this data set (some flagged row is not its own mirror image)"""
    eng = engines["mlp"]
    out = []
    for flip in (False, True):
        start(eng, "mlp", rows)
        eng.train_epochs_sampled(KEY, 1, 32, LR, flip=flip)
        out.append(eng.trainer_state()["weights"])
    assert not same(out[0], out[1])


# ---- splitting
@pytest.mark.parametrize("net", ["mlp", "conv"])
def test_one_call_equals_one_call_per_epoch(engines, rows, net):
    eng = engines[net]
    start(eng, net, rows)
    all_losses = eng.train_epochs_sampled(KEY, E, 32, LR, flip=True)
    whole = eng.trainer_state()
    start(eng, net, rows)
    parts = [eng.train_epochs_sampled(KEY, 1, 32, LR, first_epoch=e, flip=True) for e in range(E)]
    assert same(all_losses, np.concatenate(parts))
    assert_same_state(whole, eng.trainer_state())
    # the last epoch number there is: first_epoch + n_epochs = 2^32 is inside the range
    start(eng, net, rows)
    last = eng.train_epochs_sampled(KEY, 1, 32, LR, first_epoch=(1 << 32) - 1)
    got = eng.trainer_state()
    start(eng, net, rows)
    assert same(last, twin_epochs(eng, rows, KEY, [(1 << 32) - 1], 32, LR, False))
    assert_same_state(got, eng.trainer_state())


# ---- degenerate cases and refusals through the C ABI itself
def raw_sampled(eng, cfg, n_epochs, batch, lr=LR):
    """(status, *n_steps) of syn_train_epochs_sampled with no loss array; *n_steps starts as a sentinel"""
    steps = C.c_size_t(12345)
    rc = eng._lib.syn_train_epochs_sampled(eng._h, None if cfg is None else C.byref(cfg), int(n_epochs), int(batch), float(lr), None,
                                           C.byref(steps))
    return rc, int(steps.value)


def config(key=KEY, first_epoch=0, flip=0):
    from synthesis_amd.engine import CSamplerConfig

    return CSamplerConfig(key, first_epoch, flip)


def test_degenerate_calls_leave_the_learner_unchanged(engines, rows):
    eng = engines["mlp"]
    start(eng, "mlp", rows, n=20)
    s0 = eng.trainer_state()
    assert raw_sampled(eng, config(), E, 32) == (0, 0)          # n = 20 < batch
    assert eng.train_epochs_sampled(KEY, E, 32, LR).shape == (E, 0, 2)
    assert_same_state(s0, eng.trainer_state())
    start(eng, "mlp", rows)
    assert raw_sampled(eng, config(), 0, 32) == (0, 0)          # n_epochs = 0
    assert eng.train_epochs_sampled(KEY, 0, 32, LR).shape == (0, 0, 2)
    assert_same_state(s0, eng.trainer_state())
    assert s0["step"] == 0 and same(s0["weights"], data.blob_of("mlp"))


@pytest.fixture(scope="module")
def reference_run(engines, rows):
    """What a sampled call of two flipped epochs leaves from the start"""
    eng = engines["mlp"]
    start(eng, "mlp", rows)
    losses = eng.train_epochs_sampled(KEY, 2, 32, LR, flip=True)
    return losses, eng.trainer_state()


def test_refusals_leave_the_learner_and_the_next_call_unchanged(engines, rows, reference_run):
    eng = engines["mlp"]
    start(eng, "mlp", rows)
    s0 = eng.trainer_state()
    refused = [
        ("null config", None, 2, 32),
        ("flip = 2", config(flip=2), 2, 32),
        ("flip = -1", config(flip=-1), 2, 32),
        ("n_epochs < 0", config(), -1, 32),
        ("batch = 0", config(), 2, 0),
        ("batch < 0", config(), 2, -32),
        ("epochs past 2^32", config(first_epoch=(1 << 32) - 1), 2, 32),
    ]
    for what, cfg, n_epochs, batch in refused:
        rc, steps = raw_sampled(eng, cfg, n_epochs, batch)
        assert rc == INVALID and steps == 0, what
        assert_same_state(s0, eng.trainer_state(), what)
    # the micro-batch mode's rules hold for the sampled call as for every other entry point
    eng.trainer_set_batch_mode("micro")
    assert raw_sampled(eng, config(), 2, 33)[0] == INVALID
    assert_same_state(s0, eng.trainer_state(), "micro batch 33")
    eng.trainer_set_batch_mode("chained")
    losses = eng.train_epochs_sampled(KEY, 2, 32, LR, flip=True)
    assert same(losses, reference_run[0])
    assert_same_state(eng.trainer_state(), reference_run[1])


def test_refusals_without_a_trainer_or_a_data_set(rows, reference_run):
    eng = new_engine("mlp")
    try:
        assert raw_sampled(eng, config(), 2, 32)[0] == NO_WEIGHTS               # no trainer
        eng.trainer_init(data.blob_of("mlp"), **data.HYPER)
        s0 = eng.trainer_state()
        rc, steps = raw_sampled(eng, config(), 2, 32)                           # no data set
        assert rc == INVALID and steps == 0
        assert_same_state(s0, eng.trainer_state())
        eng.train_set_data(*rows)
        losses = eng.train_epochs_sampled(KEY, 2, 32, LR, flip=True)
        assert same(losses, reference_run[0])
        assert_same_state(eng.trainer_state(), reference_run[1])
    finally:
        eng.close()


# ---- the loop
@pytest.mark.parametrize("net, flip", [("mlp", False), ("conv", False), ("mlp", True)])
def test_learning_loop_device_sampler_same_in_both_replay_modes(net, flip):
    """LearningLoop(sampler="device") for two iterations, replay="host" against replay="device": identical records and weights, one
    train_epochs_sampled call per iteration and no train_epoch call."""
    import synthesis_amd as sa
    from synthesis_amd.learner import LearningLoop

    class Recording(sa.Engine):
        calls = None

        def train_epochs_sampled(self, *a, **k):
            self.calls.append(("sampled", a[0], k.get("flip")))
            return super().train_epochs_sampled(*a, **k)

        def train_epoch(self, *a, **k):
            self.calls.append(("epoch",))
            return super().train_epoch(*a, **k)

    blob = data.blob_of(net)
    cfg = sa.parity_rollout_config(16)
    recs, weights, engines_ = {}, {}, {}
    try:
        for arm in ("host", "device"):
            eng = engines_[arm] = Recording(concurrent_games=64, max_explores=16)
            eng.calls = []
            loop = LearningLoop(eng, net, blob, seed=7, replay=arm, sampler="device", flip=flip)
            recs[arm] = [loop.iteration(cfg, 48, 64, 2, 32) for _ in range(2)]
            weights[arm] = loop.weights.copy()
            assert eng.calls == [("sampled", 7 << 32, flip), ("sampled", (7 << 32) | 1, flip)]
        for a, b in zip(recs["host"], recs["device"]):
            for k in ("steps_in_buffer", "unique", "optimiser_steps", "epoch_losses", "plies_per_game", "games", "lr", "iteration"):
                assert a[k] == b[k], (k, a[k], b[k])
            assert len(a["epoch_losses"]) == 2 and a["optimiser_steps"] == 2 * (a["unique"] // 32) > 0
        assert same(weights["host"], weights["device"])
        assert not same(weights["host"], blob)
    finally:
        for eng in engines_.values():
            eng.close()
