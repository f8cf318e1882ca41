"""The micro-batch learner step (SYN_TRAIN_BATCH_MICRO: csrc/train_micro.cuh) on the GPU against its model (tests/micro_batch_model.py:
the oracle's per-32 gradients, combined in numpy float32 in the order the header gives, oracle Adam). Every comparison is bit for bit."""
import numpy as np
import pytest

from tests import micro_batch_model as model

pytestmark = pytest.mark.gpu

NETS = ("mlp", "conv")
LRS = (2e-3, 2e-3, 5e-4, 5e-4)
INVALID, NO_WEIGHTS, UNSUPPORTED = -1, -4, -5


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def init(eng, net, blob=None):
    blob = model.blob_of(net) if blob is None else blob
    (eng.trainer_init if net == "mlp" else eng.trainer_init_conv)(blob, **model.HYPER)


@pytest.fixture(scope="module")
def engines():
    import synthesis_amd as sa

    e = {}
    for net in NETS:
        e[net] = sa.Engine(concurrent_games=64, max_explores=64)
        (e[net].load_weights if net == "mlp" else e[net].load_weights_conv)(model.blob_of(net))
    yield e
    for eng in e.values():
        eng.close()


@pytest.fixture(scope="module")
def device_pool(oracle):
    """The pool on the device, and a function that gathers a batch from it."""
    import torch

    p = model.pool(oracle)
    d = dict(my=torch.from_numpy(p["my"].astype(np.int64)).cuda(), op=torch.from_numpy(p["op"].astype(np.int64)).cuda(),
             tpi=torch.from_numpy(np.array(p["tpi"])).cuda(), tv=torch.from_numpy(np.array(p["tv"])).cuda())

    def batch(idx):
        i = torch.from_numpy(np.asarray(idx, np.int64)).cuda()
        b = {k: a.index_select(0, i).contiguous() for k, a in d.items()}
        torch.cuda.synchronize()
        return b

    return batch


def device_gradients(eng, b, n_params):
    """train_gradients_device on a gathered batch: (gradients, losses) on the host."""
    import torch

    g = torch.full((n_params,), float("nan"), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    l = eng.train_gradients_device(b["my"].data_ptr(), b["op"].data_ptr(), b["tpi"].data_ptr(), b["tv"].data_ptr(), b["my"].numel(), g.data_ptr())
    return g.cpu().numpy(), l


_STEPS = {}


def model_steps(oracle, net):
    """Four steps of B = 96 from the start: the reference of the whole-step tests, computed once per network."""
    if net not in _STEPS:
        idx = np.stack([model.batch_indices(oracle, 96, seed=40 + s) for s in range(4)])
        _STEPS[net] = (idx, model.steps(oracle, net, model.blob_of(net), idx, LRS))
    return _STEPS[net]


# ---- 1
@pytest.mark.parametrize("net", NETS)
@pytest.mark.parametrize("nb", [1, 2, 3, 5, 17])
def test_gradients_match_the_model(engines, oracle, device_pool, net, nb):
    eng, blob = engines[net], model.blob_of(net)
    idx = model.batch_indices(oracle, 32 * nb, seed=nb)
    b = device_pool(idx)
    init(eng, net)
    eng.trainer_set_batch_mode("micro")
    g, l = device_gradients(eng, b, blob.size)
    G, L = model.gradients(oracle, net, blob, idx)
    assert same(g, G) and same(l, L)
    assert eng.trainer_batch_mode() == ("micro", 0, nb)
    if nb == 1:   # nothing is added to g_0 and inv = 1: the chained mode's bits on the same engine
        eng.trainer_set_batch_mode("chained")
        gc, lc = device_gradients(eng, b, blob.size)
        assert same(g, gc) and same(l, lc)


# ---- 2
@pytest.mark.parametrize("net", NETS)
def test_result_does_not_depend_on_the_workgroup_count(engines, oracle, device_pool, net):
    """nb = 7 on 1, 2, 3 and 7 workgroups: the block loop with and without a remainder."""
    eng, blob = engines[net], model.blob_of(net)
    idx = model.batch_indices(oracle, 32 * 7, seed=70)
    b = device_pool(idx)
    init(eng, net)
    G, L = model.gradients(oracle, net, blob, idx)
    for cap, grid in ((1, 1), (2, 2), (3, 3), (0, 7)):
        eng.trainer_set_batch_mode("micro", max_workgroups=cap)
        g, l = device_gradients(eng, b, blob.size)
        assert eng.trainer_batch_mode() == ("micro", cap, grid)
        assert same(g, G) and same(l, L), cap


# ---- 3
def test_more_micro_batches_than_cus(engines, oracle, device_pool):
    import torch

    eng, blob, nb = engines["mlp"], model.blob_of("mlp"), 263
    idx = model.batch_indices(oracle, 32 * nb, seed=263)
    init(eng, "mlp")
    eng.trainer_set_batch_mode("micro")
    g, l = device_gradients(eng, device_pool(idx), blob.size)
    G, L = model.gradients(oracle, "mlp", blob, idx)
    assert same(g, G) and same(l, L)
    assert eng.trainer_batch_mode()[2] == torch.cuda.get_device_properties(0).multi_processor_count < nb


# ---- 4
def check_state(st, ref, losses):
    assert st["step"] == ref["step"] == len(LRS)
    assert same(losses, ref["losses"])
    for k in ("weights", "m", "v", "grads"):
        assert same(st[k], ref[k]), k


def check_publish(eng, oracle, net, weights):
    """trainer_publish_weights, then policy_eval: the model network's outputs (as the existing publish tests compare them)."""
    p = model.pool(oracle)
    eng.trainer_publish_weights()
    logits, value = eng.policy_eval(p["my"][:48], p["op"][:48])
    ev = oracle.c4net_eval if net == "mlp" else oracle.c4conv_eval
    fl, fv = ev(weights, p["my"][:48], p["op"][:48], mode=oracle.ACC_FMA)
    assert same(logits, fl) and same(value, fv)
    (eng.load_weights if net == "mlp" else eng.load_weights_conv)(model.blob_of(net))


@pytest.mark.parametrize("net", NETS)
def test_whole_steps_through_train_step(engines, oracle, net):
    eng, p = engines[net], model.pool(oracle)
    idx, ref = model_steps(oracle, net)
    init(eng, net)
    eng.trainer_set_batch_mode("micro")
    losses = np.stack([eng.train_step(p["my"][i], p["op"][i], p["tpi"][i], p["tv"][i], lr) for i, lr in zip(idx, LRS)])
    check_state(eng.trainer_state(), ref, losses)
    check_publish(eng, oracle, net, ref["weights"])


@pytest.mark.parametrize("net", NETS)
def test_whole_steps_through_train_epoch(engines, oracle, net):
    """The same four steps through syn_train_set_data + syn_train_epoch: the permutation (the steps' pool rows) is not the identity; per-step
    losses come from the reduce."""
    eng, p = engines[net], model.pool(oracle)
    idx, ref = model_steps(oracle, net)
    assert not np.array_equal(idx.ravel(), np.arange(idx.size))
    init(eng, net)
    eng.train_set_data(p["my"], p["op"], p["tpi"], p["tv"])
    eng.trainer_set_batch_mode("micro", max_workgroups=2)
    # one syn_train_epoch call per learning rate: two epochs of two steps, each step blocks, reduce and Adam queued in stream order
    losses, s = [], 0
    while s < len(LRS):
        e = s + 1
        while e < len(LRS) and LRS[e] == LRS[s]:
            e += 1
        losses.append(eng.train_epoch(idx[s:e].ravel(), 96, LRS[s]))
        s = e
    check_state(eng.trainer_state(), ref, np.concatenate(losses))
    assert eng.trainer_batch_mode() == ("micro", 2, 2)
    check_publish(eng, oracle, net, ref["weights"])


# ---- 5
@pytest.mark.parametrize("nb", [2, 5])
def test_bf16_conv_is_the_sum_of_its_own_blocks(engines, oracle, device_pool, nb):
    """The conv learner's bf16 variant: the micro-mode gradient is the ascending f32 sum, times inv, of the engine's own batch-32 bf16
    gradients of each block (the path tests/test_gpu_conv_bf16_learner.py holds to its model)."""
    eng, n = engines["conv"], model.blob_of("conv").size
    idx = model.batch_indices(oracle, 32 * nb, seed=500 + nb)
    init(eng, "conv")
    eng.trainer_set_precision("bf16")
    parts = [device_gradients(eng, device_pool(idx[o:o + 32]), n) for o in range(0, 32 * nb, 32)]
    eng.trainer_set_batch_mode("micro")
    g, l = device_gradients(eng, device_pool(idx), n)
    assert same(g, model.combine([pg for pg, _ in parts])) and same(l, model.combine([pl for _, pl in parts]))
    # and it is the bf16 arithmetic that ran, not the f32 one
    eng.trainer_set_precision("f32")
    g32, _ = device_gradients(eng, device_pool(idx), n)
    assert not same(g, g32)


# ---- 6
@pytest.mark.parametrize("net", NETS)
def test_enqueue_path_on_a_torch_stream(engines, oracle, device_pool, net):
    """train_gradients_enqueue + train_apply_enqueue on a non-default stream, two steps: the bits of the whole-step tests' first two."""
    import torch

    eng, n = engines[net], model.blob_of(net).size
    idx, ref = model_steps(oracle, net)
    init(eng, net)
    eng.trainer_set_batch_mode("micro")
    batches = [device_pool(idx[s]) for s in range(2)]
    buf = torch.zeros(n + 2, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    losses = []
    with torch.cuda.stream(stream):
        for s, b in enumerate(batches):
            eng.train_gradients_enqueue(stream.cuda_stream, b["my"].data_ptr(), b["op"].data_ptr(), b["tpi"].data_ptr(), b["tv"].data_ptr(), 96,
                                        buf.data_ptr(), buf.data_ptr() + 4 * n)
            eng.train_apply_enqueue(stream.cuda_stream, buf.data_ptr(), LRS[s])
            losses.append(buf[n:].clone())
    stream.synchronize()
    st = eng.trainer_state()
    w, m, v = ref["history"][1]
    assert st["step"] == 2
    assert same(st["weights"], w) and same(st["m"], m) and same(st["v"], v)
    assert same(torch.stack(losses).cpu().numpy(), ref["losses"][:2])


# ---- 7
def state_bits(eng):
    st = eng.trainer_state()
    return {k: (bits(a).copy() if isinstance(a, np.ndarray) else a) for k, a in st.items()}


def assert_refused(code, fn, *args, **kw):
    import synthesis_amd as sa

    with pytest.raises(sa.SynthesisAmdError) as ei:
        fn(*args, **kw)
    assert ei.value.code == code, ei.value


@pytest.mark.parametrize("net", NETS)
def test_refusals_leave_the_learner_alone(engines, oracle, device_pool, net):
    import torch

    eng, p, n = engines[net], model.pool(oracle), model.blob_of(net).size
    init(eng, net)
    eng.train_set_data(p["my"], p["op"], p["tpi"], p["tv"])
    eng.trainer_set_batch_mode("micro", max_workgroups=5)
    eng.train_step(p["my"][:64], p["op"][:64], p["tpi"][:64], p["tv"][:64], 1e-3)   # a state that is not the initial one
    before, mode = state_bits(eng), eng.trainer_batch_mode()
    g = torch.zeros(n, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()

    def batch_calls(B):
        i = np.arange(B) % p["my"].size
        b = device_pool(i)
        ptrs = (b["my"].data_ptr(), b["op"].data_ptr(), b["tpi"].data_ptr(), b["tv"].data_ptr(), B, g.data_ptr())
        return [lambda: eng.train_step(p["my"][i], p["op"][i], p["tpi"][i], p["tv"][i], 1e-3), lambda: eng.train_gradients_device(*ptrs),
                lambda: eng.train_gradients_enqueue(0, *ptrs), lambda: eng.train_epoch(i.astype(np.int32), B, 1e-3)]

    for B in (33, 31, 48, 1):   # not a multiple of 32
        for call in batch_calls(B):
            assert_refused(INVALID, call)
    for call in batch_calls(32 * 1025):   # more than 1024 micro-batches
        assert_refused(UNSUPPORTED, call)
    assert eng._lib.syn_trainer_set_batch_mode(eng._h, 2, 0) == INVALID   # unknown mode
    assert eng._lib.syn_trainer_set_batch_mode(eng._h, -1, 0) == INVALID
    assert_refused(INVALID, eng.trainer_set_batch_mode, "micro", max_workgroups=-1)
    with pytest.raises(ValueError):
        eng.trainer_set_batch_mode("blocked")
    torch.cuda.synchronize()
    after = state_bits(eng)
    assert eng.trainer_batch_mode() == mode == ("micro", 5, 2)
    assert before.keys() == after.keys()
    for k in before:
        assert np.array_equal(before[k], after[k]), k


def test_setter_needs_a_trainer_and_init_resets_the_mode(oracle):
    import synthesis_amd as sa

    eng = sa.Engine(concurrent_games=64, max_explores=64)
    try:
        assert_refused(NO_WEIGHTS, eng.trainer_set_batch_mode, "micro")
        assert_refused(NO_WEIGHTS, eng.trainer_batch_mode)
        init(eng, "conv")
        assert eng.trainer_batch_mode() == ("chained", 0, 0)   # no blocks launch yet
        eng.trainer_set_batch_mode("micro", max_workgroups=3)
        assert eng.trainer_batch_mode() == ("micro", 3, 0)
        init(eng, "mlp")
        assert eng.trainer_batch_mode()[:2] == ("chained", 0)
        eng.trainer_set_batch_mode("micro", max_workgroups=3)
        init(eng, "conv")
        assert eng.trainer_batch_mode()[:2] == ("chained", 0)
        # chained mode: Connect4ConvNet above 32 is still refused, as before
        p = model.pool(oracle)
        assert_refused(UNSUPPORTED, eng.train_step, p["my"][:64], p["op"][:64], p["tpi"][:64], p["tv"][:64], 1e-3)
    finally:
        eng.close()


# ---- 8
def test_default_mode_is_untouched(oracle):
    """With the setter never called, and again after micro then chained, train_epoch at batch 64 on Connect4Net gives the oracle's
    chained B = 64 bits."""
    import synthesis_amd as sa

    p, blob = model.pool(oracle), model.blob_of("mlp")
    idx = np.stack([model.batch_indices(oracle, 64, seed=800 + s) for s in range(2)])
    wo, mo, vo, so, lo = oracle.train_steps(blob, model.hyper(), p["X"][idx], p["tpi"][idx], p["tv"][idx], [1e-3] * 2)
    eng = sa.Engine(concurrent_games=64, max_explores=64)
    try:
        for toggled in (False, True):
            init(eng, "mlp")
            eng.train_set_data(p["my"], p["op"], p["tpi"], p["tv"])
            if toggled:
                eng.trainer_set_batch_mode("micro")
                eng.train_epoch(idx.ravel(), 64, 1e-3)
                assert not same(eng.trainer_state()["weights"], wo)   # the other definition
                init(eng, "mlp")
                eng.trainer_set_batch_mode("micro")
                eng.trainer_set_batch_mode("chained")
            losses = eng.train_epoch(idx.ravel(), 64, 1e-3)
            st = eng.trainer_state()
            assert st["step"] == so == 2 and same(losses, lo)
            assert same(st["weights"], wo) and same(st["m"], mo) and same(st["v"], vo)
    finally:
        eng.close()
