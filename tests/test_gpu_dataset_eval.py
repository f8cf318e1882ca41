"""Held-out evaluation on the device (syn_dataset_set / syn_dataset_get / syn_dataset_evaluate; csrc/dataset_eval.cuh), both networks:
  block losses   bit for bit the oracle's train_gradients / convtrain_gradients losses of every block as a minibatch, and the device's own
                 train_gradients_device losses for the same rows; row_kl = the oracle's losses of every row as a minibatch of one
  totals         the f64 bits of tests/dataset_eval_model.py's restatement; the hit counts = the restatement applied to the RETURNED
                 row_logits; row_logits within 1e-5 of the oracle's raw outputs
  hits           constructed cases: a full column with the largest logit, two equal maxima in the target, an all-zero target row
  grid           max_workgroups 1, 3 and 0 give the same bytes
  observer       trainer state, both data sets and a policy evaluation are byte-identical across evaluations and refusals
"""
import numpy as np
import pytest

from tests import dataset_eval_model as dm
from tests import f16x2_checkpoints as fc
from tests import learner_f32_family as lf
from tests.f16x2_checkpoints import same_bits

pytestmark = pytest.mark.gpu

SIZES = (1, 31, 32, 33, 95)
DATA_VARIANTS = ("recorded", "onehot", "zero_row", "subnormal_t", "empty_board")
MEMBERS = dict(mlp=("trained", lf.SUBNORMAL_MEMBERS["mlp"][0]), conv=("trained", lf.SUBNORMAL_MEMBERS["conv"][0]))
GRID_N = 95 + 32 * 7
TOTAL_KEYS = ("mean_pi", "mean_v", "sum_pi", "sum_v", "rows", "blocks", "pi_hits", "v_hits")


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


def trainer_init(eng, net, w):
    (eng.trainer_init if net == "mlp" else eng.trainer_init_conv)(w, **lf.HYPERS["default"])


def to_device(b):
    import torch

    d = [torch.from_numpy(b[0].astype(np.int64)).cuda(), torch.from_numpy(b[1].astype(np.int64)).cuda(),
         torch.from_numpy(np.ascontiguousarray(b[2])).cuda(), torch.from_numpy(np.ascontiguousarray(b[3])).cuda()]
    torch.cuda.synchronize()
    return d


def oracle_raw(oracle, net, w, my, op):
    """the twelve raw outputs [n][12] in the slimnn order"""
    if net == "conv":
        return oracle.c4conv_eval(w, my, op, mode=oracle.ACC_SLIMNN, raw=True)[2]
    x = oracle.c4_features(my, op)
    for l, (W, b) in enumerate(fc.mlp_views(np.ascontiguousarray(w, np.float32))):
        x = oracle.linear(W, b, x, mode=oracle.ACC_SLIMNN)
        if l < 4:
            x = oracle.relu(x).reshape(x.shape)
    return x


def assert_totals(tag, r, n, my, op, tpi, tv):
    ph, vh = dm.row_hits(r["row_logits"], my, op, tpi, tv)
    want = dm.totals(n, r["block_losses"], ph, vh)
    for k in TOTAL_KEYS:
        if isinstance(want[k], float):
            assert dm.f64_bits(r[k]) == dm.f64_bits(want[k]), (tag, k, r[k], want[k])
        else:
            assert r[k] == want[k], (tag, k, r[k], want[k])


def same_result(a, b):
    return all(a[k] == b[k] or (a[k] != a[k] and b[k] != b[k]) for k in TOTAL_KEYS) and all(
        np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)) for k in ("block_losses", "row_logits", "row_kl"))


CASES = [(net, member, variant) for net in lf.NETS for member in MEMBERS[net] for variant in DATA_VARIANTS]


@pytest.mark.parametrize("net,member,variant", CASES, ids=["-".join(c) for c in CASES])
def test_block_losses_rows_and_totals(engines, oracle, net, member, variant):
    import torch

    eng, w = engines[net], lf.family(net)[member]
    trainer_init(eng, net, w)
    g = torch.zeros(w.size, dtype=torch.float32, device="cuda")
    for n in SIZES:
        tag = (net, member, variant, n)
        b = lf.batch(variant, n)
        my, op, tpi, tv = b
        eng.dataset_set(*b)
        r = eng.dataset_evaluate("eval", blocks=True, rows=True)                      # the trainer's weights
        assert same_result(r, eng.dataset_evaluate("eval", blob=w, blocks=True, rows=True)), tag    # the same parameters as a blob
        eng.train_set_data(*b)
        assert same_result(r, eng.dataset_evaluate("train", blocks=True, rows=True)), tag
        assert r["rows"] == n and r["blocks"] == (n + 31) // 32 and r["block_losses"].shape == (r["blocks"], 2)
        for j in range(r["blocks"]):
            sl = slice(32 * j, min(32 * j + 32, n))
            blk = tuple(a[sl] for a in b)
            _, lo = lf.oracle_gradients(oracle, net, w, "default", blk)
            assert np.isfinite(lo).all(), tag
            assert same_bits(r["block_losses"][j], lo), (tag, j, r["block_losses"][j], lo)
            d = to_device(blk)
            ld = eng.train_gradients_device(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), sl.stop - sl.start, g.data_ptr())
            assert same_bits(r["block_losses"][j], ld), (tag, j, "device", r["block_losses"][j], ld)
        for i in range(n):
            _, lo = lf.oracle_gradients(oracle, net, w, "default", tuple(a[i:i + 1] for a in b))
            assert same_bits(r["row_kl"][i], lo), (tag, i, r["row_kl"][i], lo)
        assert same_bits(r["block_losses"], dm.block_losses(r["row_kl"])), tag
        assert_totals(tag, r, n, my, op, tpi, tv)
        raw = oracle_raw(oracle, net, w, my, op)
        assert np.abs(r["row_logits"].astype(np.float64) - raw).max() < 1e-5, tag
        # the zeroed rows of `zero_row`: KL exactly +0 in both heads
        if variant == "zero_row":
            for i in sorted({0, n - 1}):
                assert np.array_equal(r["row_kl"][i].view(np.uint32), np.zeros(2, np.uint32)), tag


# ---- constructed hit cases
def biased(net, w, entry, by=100.0):
    """`w` with the last layer's bias of output `entry` (0..8 policy, 9..11 value) raised by `by`"""
    w = np.array(w, np.float32)
    bias = fc.mlp_views(w)[4][1] if net == "mlp" else fc.conv_views(w)[3]
    bias[entry] += np.float32(by)
    return w


def full_column_position(col):
    """seven alternating stones in `col` (bit = row + 7 col), nothing else"""
    my = sum(1 << (r + 7 * col) for r in (0, 2, 4, 6))
    op = sum(1 << (r + 7 * col) for r in (1, 3, 5))
    return np.array([my], np.uint64), np.array([op], np.uint64)


@pytest.mark.parametrize("net", lf.NETS)
def test_constructed_hits(engines, net):
    eng, w = engines[net], lf.family(net)["trained"]
    onehot = lambda k, c: np.eye(k, dtype=np.float32)[c][None]
    # a full column whose logit is the largest: the prediction is the best LEGAL column
    my, op = full_column_position(4)
    wb = biased(net, w, 4)
    eng.dataset_set(my, op, onehot(9, 4), onehot(3, 0))
    r = eng.dataset_evaluate("eval", blob=wb, rows=True)
    lg = r["row_logits"][0, :9]
    assert int(np.argmax(lg)) == 4 and r["pi_hits"] == 0
    legal = [c for c in range(9) if c != 4]
    best = legal[int(np.argmax(lg[legal]))]
    eng.dataset_set(my, op, onehot(9, best), onehot(3, 0))
    assert eng.dataset_evaluate("eval", blob=wb)["pi_hits"] == 1
    other = [c for c in legal if c != best][0]
    eng.dataset_set(my, op, onehot(9, other), onehot(3, 0))
    assert eng.dataset_evaluate("eval", blob=wb)["pi_hits"] == 0
    # a target with two equal maxima: the first one is the target's arg-max
    empty = np.zeros(1, np.uint64)
    t = np.zeros((1, 9), np.float32); t[0, 1] = t[0, 3] = 0.5
    eng.dataset_set(empty, empty, t, onehot(3, 2))
    assert eng.dataset_evaluate("eval", blob=biased(net, w, 1))["pi_hits"] == 1
    assert eng.dataset_evaluate("eval", blob=biased(net, w, 3))["pi_hits"] == 0
    tv = np.zeros((1, 3), np.float32); tv[0, 1] = tv[0, 2] = 0.5
    eng.dataset_set(empty, empty, t, tv)
    assert eng.dataset_evaluate("eval", blob=biased(net, w, 10))["v_hits"] == 1
    assert eng.dataset_evaluate("eval", blob=biased(net, w, 11))["v_hits"] == 0
    # an all-zero target row: KL 0, and it still counts for the arg-max (entry 0)
    eng.dataset_set(empty, empty, np.zeros((1, 9), np.float32), np.zeros((1, 3), np.float32))
    r = eng.dataset_evaluate("eval", blob=biased(net, biased(net, w, 0), 9), blocks=True, rows=True)
    assert r["pi_hits"] == 1 and r["v_hits"] == 1 and not r["row_kl"].any() and not r["block_losses"].any() and r["mean_pi"] == 0.0
    r = eng.dataset_evaluate("eval", blob=biased(net, biased(net, w, 5), 10))
    assert r["pi_hits"] == 0 and r["v_hits"] == 0


# ---- grid independence
@pytest.mark.parametrize("net", lf.NETS)
def test_grid_independence(engines, net):
    eng, w = engines[net], lf.family(net)["trained"]
    b = lf.batch("recorded", GRID_N)
    eng.dataset_set(*b)
    rs = [eng.dataset_evaluate("eval", blob=w, max_workgroups=g, blocks=True, rows=True) for g in (1, 3, 0)]
    assert [r["grid"] for r in rs] == [1, 3, (GRID_N + 31) // 32]
    assert same_result(rs[0], rs[1]) and same_result(rs[0], rs[2])
    assert_totals((net, "grid"), rs[0], GRID_N, *b)
    # a sub-range is the range's own blocks: rows [33, 33 + 70)
    sub = eng.dataset_evaluate("eval", first_row=33, n_rows=70, blob=w, blocks=True, rows=True)
    assert np.array_equal(sub["row_kl"].view(np.uint32), rs[0]["row_kl"][33:103].view(np.uint32))
    assert_totals((net, "sub"), sub, 70, *(a[33:103] for a in b))
    ms, launches = eng.last_timing()
    assert ms > 0.0 and launches == 2


# ---- observer
def snapshot(eng, my, op):
    st = eng.trainer_state()
    return [st["weights"], st["m"], st["v"], st["grads"], np.array([st["step"]])] + list(eng.train_get_data().values()) + \
        list(eng.dataset_get().values()) + list(eng.policy_eval(my, op))


def same_snapshot(a, b):
    return all(x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b))


@pytest.mark.parametrize("net", lf.NETS)
def test_observer_and_refusals(engines, net):
    import synthesis_amd as sa
    from synthesis_amd.engine import SynthesisAmdError

    eng, fam = engines[net], lf.family(net)
    trainer_init(eng, net, fam["trained"])
    tr, ev = lf.batch("recorded", 96), lf.batch("onehot", 77, step=3)
    perm = np.random.default_rng(5).permutation(96).astype(np.int32)
    eng.train_set_data(*tr)
    eng.train_epoch(perm, 32, 1e-3)          # non-zero moments and step count
    eng.dataset_set(*ev)
    got = eng.dataset_get()
    assert all(np.array_equal(got[k], a) for k, a in zip(("my_bb", "op_bb", "pis", "vs"), ev))
    before = snapshot(eng, tr[0][:8], tr[1][:8])
    for which in ("train", "eval"):
        eng.dataset_evaluate(which, blocks=True, rows=True)
        eng.dataset_evaluate(which, blob=fam["init"], max_workgroups=2, rows=True)
    assert same_snapshot(before, snapshot(eng, tr[0][:8], tr[1][:8]))
    # every refusal leaves everything as it was
    n_params = fam["init"].size
    for kw, code in ((dict(which="eval", first_row=70, n_rows=8), -1), (dict(which="train", first_row=97, n_rows=0), -1),
                     (dict(which="eval", blob=fam["init"][: n_params - 1]), -1), (dict(which="eval", max_workgroups=-1), -1)):
        with pytest.raises(SynthesisAmdError) as ei:
            eng.dataset_evaluate(**kw)
        assert ei.value.code == code, kw
    z = eng.dataset_evaluate("eval", first_row=77, n_rows=0, blocks=True, rows=True)
    assert all(z[k] == 0 for k in TOTAL_KEYS) and z["block_losses"].shape == (0, 2) and z["row_kl"].shape == (0, 2)
    assert same_snapshot(before, snapshot(eng, tr[0][:8], tr[1][:8]))
    # a train_epoch after evaluations leaves the bits of one without them
    eng.train_epoch(perm, 32, 1e-3)
    after_with = eng.trainer_state()
    trainer_init(eng, net, fam["trained"])
    eng.train_set_data(*tr)
    eng.train_epoch(perm, 32, 1e-3)
    eng.train_epoch(perm, 32, 1e-3)
    after_without = eng.trainer_state()
    assert after_with["step"] == after_without["step"] == 6
    assert all(after_with[k].tobytes() == after_without[k].tobytes() for k in ("weights", "m", "v", "grads"))
    # no trainer, no weights, no data set: an engine of its own
    fresh = sa.Engine(concurrent_games=64, max_explores=64)
    try:
        for kw, code in ((dict(which="eval", blob=fam["init"]), -1), (dict(which="train", blob=fam["init"]), -1)):   # no data set
            with pytest.raises(SynthesisAmdError) as ei:
                fresh.dataset_evaluate(**kw)
            assert ei.value.code == code, kw
        fresh.dataset_set(*ev)
        with pytest.raises(SynthesisAmdError) as ei:
            fresh.dataset_evaluate("eval")                       # blob = None without a trainer
        assert ei.value.code == -4
        r = fresh.dataset_evaluate("eval", blob=fam["trained"], blocks=True, rows=True)    # needs neither trainer nor loaded weights
        eng.dataset_set(*ev)
        assert same_result(r, eng.dataset_evaluate("eval", blob=fam["trained"], blocks=True, rows=True))
        fresh.dataset_set(ev[0][:0], ev[1][:0], ev[2][:0], ev[3][:0])    # n = 0 empties the set
        assert fresh.dataset_get()["my_bb"].size == 0
    finally:
        fresh.close()
