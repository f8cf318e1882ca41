"""Held-out evaluation in the f16x2 and bf16 arithmetics (syn_dataset_evaluate_arith; csrc/dataset_eval.cuh), on the device:
  f16x2 raw      row_logits[:, :9] = policy_eval of a second engine holding the same parameters in the f16x2 arithmetic, and all twelve
                 = the references the f16x2 suites use (the oracle's ACC_F16X2; tests/conv_f16x2_model.py), bit for bit
  head, totals   row_kl = tests/dataset_eval_arith_model.head of the RETURNED row_logits; block_losses and the f64 totals =
                 tests/dataset_eval_model.py on the returned rows; the head model is calibrated on the f32 call
  bf16           block losses and row_kl = train_gradients_device in trainer_set_precision("bf16"), with the trainer left in either
                 precision; row_logits against tests/conv_bf16_learner_model.py's rounded-operand forward
  sources, grid, observer, refusals, the learning loop's holdout_arith
Row counts sit at the tile edge (16) and the block edge (32) of the new kernels.
"""
import ctypes as C

import numpy as np
import pytest

from tests import conv_bf16_learner_model as cbl
from tests import dataset_eval_arith_model as am
from tests import dataset_eval_model as dm
from tests import f16x2_checkpoints as fc
from tests import learner_f32_family as lf
from tests.f16x2_checkpoints import same_bits
from tests.oracle_lib import _p
from tests.test_gpu_dataset_eval import TOTAL_KEYS, assert_totals, same_result, to_device, trainer_init

pytestmark = pytest.mark.gpu

SIZES = (1, 15, 16, 17, 31, 32, 33, 95)
DATA_VARIANTS = ("recorded", "onehot", "zero_row", "subnormal_t", "empty_board")
# `trained` and the smallest- and largest-scale accepted members of tests/f16x2_checkpoints.py
F16_MEMBERS = dict(mlp=("trained", "init_x2^-16", "init_x2^16"), conv=("trained", "init_conv_x2^-30", "init_conv_x2^20"))
ARITHS = dict(mlp=("f32", "f16x2"), conv=("f32", "f16x2", "bf16"))
GRID_N = 319
CHUNK_N = 32 * 256 + 33
UNSUPPORTED, INVALID, NO_WEIGHTS = -5, -1, -4


@pytest.fixture(scope="module")
def engines():
    """per network: an engine in f32 with a trainer, and one in the f16x2 arithmetic"""
    import synthesis_amd as sa

    e = {}
    for net in lf.NETS:
        for arith in ("f32", "f16x2"):
            eng = e[net, arith] = sa.Engine(concurrent_games=64, max_explores=64, policy_cache_log2=10)
            (eng.load_weights if net == "mlp" else eng.load_weights_conv)(lf.family(net)["init"])
            eng.set_network_arithmetic(arith)
    yield e
    for eng in e.values():
        eng.close()


@pytest.fixture(scope="module")
def conv_model(tmp_path_factory):
    from tests import conv_f16x2_model

    return conv_f16x2_model.load(tmp_path_factory.mktemp("conv_f16x2_model"))


def f16x2_reference(oracle, conv_model, net, w, my, op):
    """the twelve raw outputs [n][12] of the f16x2 arithmetic on the CPU"""
    if net == "conv":
        return conv_model.eval(w, my, op, raw=True)[2]
    x = oracle.c4_features(my, op)
    out = np.zeros((my.size, 12), np.float32)
    w = np.ascontiguousarray(w, np.float32)
    oracle.lib.orc_c4net_forward_raw(_p(w), _p(x), C.c_int(int(my.size)), _p(out), C.c_int(oracle.ACC_F16X2))
    return out


def load(eng, net, w):
    (eng.load_weights if net == "mlp" else eng.load_weights_conv)(w)


def check_head_and_totals(tag, oracle, r, b):
    my, op, tpi, tv = b
    n = my.size
    assert r["rows"] == n and r["blocks"] == (n + 31) // 32
    want = am.row_kl(oracle, r["row_logits"], tpi, tv)
    assert same_bits(r["row_kl"], want), (tag, "row_kl", np.flatnonzero((r["row_kl"].view(np.uint32) != want.view(np.uint32)).any(axis=1))[:8])
    assert same_bits(r["block_losses"], dm.block_losses(r["row_kl"])), (tag, "block_losses")
    assert_totals(tag, r, n, my, op, tpi, tv)


# ---- f16x2: the raw outputs
F16_CASES = [(net, m) for net in lf.NETS for m in F16_MEMBERS[net]]


@pytest.mark.parametrize("net,member", F16_CASES, ids=["-".join(c) for c in F16_CASES])
def test_f16x2_raw_outputs(engines, oracle, conv_model, net, member):
    eng, e16, w = engines[net, "f32"], engines[net, "f16x2"], lf.family(net)[member]
    load(e16, net, w)
    assert e16.network_arithmetic()[0] == "f16x2"
    for i, n in enumerate(SIZES):
        b = lf.batch(DATA_VARIANTS[i % len(DATA_VARIANTS)], n, step=i)
        my, op = b[0], b[1]
        eng.dataset_set(*b)
        r = eng.dataset_evaluate("eval", blob=w, blocks=True, rows=True, arith="f16x2")
        assert r["arith"] == "f16x2" and r["row_logits"].shape == (n, 12)
        logits, _ = e16.policy_eval(my, op)
        assert same_bits(r["row_logits"][:, :9], logits), (net, member, n, "policy_eval")
        assert same_bits(r["row_logits"], f16x2_reference(oracle, conv_model, net, w, my, op)), (net, member, n, "reference")
        check_head_and_totals((net, member, n), oracle, r, b)


# ---- f16x2 (and the f32 calibration of the head model): head and totals on every data variant
HEAD_CASES = [(net, v) for net in lf.NETS for v in DATA_VARIANTS]


@pytest.mark.parametrize("net,variant", HEAD_CASES, ids=["-".join(c) for c in HEAD_CASES])
def test_head_and_totals(engines, oracle, net, variant):
    eng, w = engines[net, "f32"], lf.family(net)["trained"]
    for n in SIZES:
        b = lf.batch(variant, n)
        eng.dataset_set(*b)
        for arith in ARITHS[net]:   # "f32": the calibration of the head model on the kernels from before this arithmetic existed
            r = eng.dataset_evaluate("eval", blob=w, blocks=True, rows=True, arith=arith)
            check_head_and_totals((net, variant, n, arith), oracle, r, b)
            if variant == "zero_row":
                for i in sorted({0, n - 1}):
                    assert not r["row_kl"][i].view(np.uint32).any()
        assert same_result(eng.dataset_evaluate("eval", blob=w, blocks=True, rows=True),
                           eng.dataset_evaluate("eval", blob=w, blocks=True, rows=True, arith="f32"))


@pytest.mark.parametrize("net", lf.NETS)
def test_reduce_crosses_a_chunk(engines, oracle, net):
    eng, w = engines[net, "f32"], lf.family(net)["trained"]
    b = lf.batch("recorded", CHUNK_N)
    eng.dataset_set(*b)
    for arith in ARITHS[net][1:]:
        r = eng.dataset_evaluate("eval", blob=w, blocks=True, rows=True, arith=arith)
        assert r["blocks"] == 258
        check_head_and_totals((net, arith, CHUNK_N), oracle, r, b)


# ---- bf16
def bf16_forward_bar(blob, my, op, tpi, tv, exact):
    """(raw [n][12] f64 of the rounded-operand model, bar [n][12]). The device's chains run in f32 in the kernel's order: a chain of k
    terms is within k * 2^-23 * sum|terms| of the exact sum (conv_bf16_learner_model's derived bar) — the head's 1008 products + bias.
    An activation the model marks fragile (its f32 pre-activation may round to the neighbouring bf16 number, or fall on the other side of
    the gate) moves a logit by at most |w| * (one bf16 ulp of the activation + the pre-activation's own bound)."""
    m = cbl.conv_bf16_step(blob, my, op, tpi, tv, exact_forward=exact)
    bar = 1009 * cbl.U23 * m["raw_sumabs"]
    fr = m["fragile"]["act"] | m["fragile"]["gate"]
    if fr.any():
        t = cbl.conv_views(np.ascontiguousarray(blob, np.float32).astype(np.float64))
        X = cbl.tap_bits(my, op)
        rcw = cbl.round_bf16(t[0].reshape(16, 18))
        pre_sumabs = (np.abs(rcw[None, :, None, :] * X.transpose(0, 2, 1)[:, None, :, :]).sum(axis=-1) + np.abs(t[1])[None, :, None]).reshape(len(my), -1)
        bound = 18 * cbl.U23 * pre_sumabs
        move = np.where(fr, cbl.bf16_ulp(np.maximum(m["act"], bound)) + bound, 0.0)
        bar = bar + (np.abs(cbl.round_bf16(t[2]))[None, :, :] * move[:, None, :]).sum(axis=-1)
    return m["raw"], bar


@pytest.mark.parametrize("member", ["trained", "grid", "grid_sharp"])
def test_bf16_losses_are_the_bf16_learners(engines, oracle, member):
    """row_logits: the exact-forward members (grid, grid_sharp) bit for bit the model's raw outputs; `trained` within bf16_forward_bar."""
    import torch

    eng, w = engines["conv", "f32"], cbl.family()[member]
    trainer_init(eng, "conv", w)
    g = torch.zeros(w.size, dtype=torch.float32, device="cuda")
    grads = lambda d, k: eng.train_gradients_device(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), k, g.data_ptr())
    for i, n in enumerate(SIZES):
        tag = (member, n)
        b = lf.batch(DATA_VARIANTS[i % len(DATA_VARIANTS)], n, step=i)
        eng.dataset_set(*b)
        d = to_device(b)
        first = to_device(tuple(a[:min(n, 32)] for a in b))
        # the references: the learner itself in bf16, per block and per row
        eng.trainer_set_precision("bf16")
        blocks = np.stack([grads(to_device(tuple(a[32 * j:32 * j + 32] for a in b)), min(32, n - 32 * j)) for j in range((n + 31) // 32)])
        rows = np.stack([grads([d[0][k:k + 1], d[1][k:k + 1], d[2][k:k + 1].contiguous(), d[3][k:k + 1].contiguous()], 1) for k in range(n)])
        loss_bf16 = grads(first, min(n, 32))
        r_in_bf16 = eng.dataset_evaluate("eval", blocks=True, rows=True, arith="bf16")
        assert same_bits(grads(first, min(n, 32)), loss_bf16), tag      # the trainer is still in bf16
        eng.trainer_set_precision("f32")
        loss_f32 = grads(first, min(n, 32))
        r = eng.dataset_evaluate("eval", blocks=True, rows=True, arith="bf16")
        assert same_bits(grads(first, min(n, 32)), loss_f32), tag       # ... and still in f32
        assert same_result(r, r_in_bf16), tag
        assert same_result(r, eng.dataset_evaluate("eval", blob=w, blocks=True, rows=True, arith="bf16")), tag
        assert same_bits(r["block_losses"], blocks), (tag, r["block_losses"], blocks)
        assert same_bits(r["row_kl"], rows), tag
        f32 = eng.dataset_evaluate("eval", blocks=True, arith="f32")
        assert same_bits(f32["block_losses"][0], loss_f32), tag
        check_head_and_totals(tag, oracle, r, b)
        raw, bar = bf16_forward_bar(w, *b, exact=member in cbl.EXACT_FORWARD)
        if member in cbl.EXACT_FORWARD:
            assert same_bits(r["row_logits"], raw.astype(np.float32)), tag
        else:
            err = np.abs(r["row_logits"].astype(np.float64) - raw)
            print(f"bf16 {tag}: max |row_logits - model| {err.max():.3e}, smallest bar {bar.min():.3e}, largest err / bar {(err / bar).max():.3f}")
            assert (err <= bar).all(), (tag, float((err / bar).max()))
    if member == "trained":   # the arithmetic is visible: the bf16 losses are not the f32 ones
        assert not same_bits(r["block_losses"], f32["block_losses"])


# ---- sources of parameters, grid
@pytest.mark.parametrize("net", lf.NETS)
def test_sources_of_parameters(engines, net):
    eng, e16, w = engines[net, "f32"], engines[net, "f16x2"], lf.family(net)["trained"]
    b = lf.batch("recorded", 95, step=1)
    trainer_init(eng, net, w)
    eng.dataset_set(*b)
    eng.train_set_data(*b)
    e16.dataset_set(*b)
    for arith in ARITHS[net]:
        r = eng.dataset_evaluate("eval", blob=w, blocks=True, rows=True, arith=arith)
        assert same_result(r, eng.dataset_evaluate("eval", blocks=True, rows=True, arith=arith)), (net, arith, "trainer's weights")
        assert same_result(r, eng.dataset_evaluate("train", blocks=True, rows=True, arith=arith)), (net, arith, "train")
        assert same_result(r, eng.dataset_evaluate("train", blob=w, blocks=True, rows=True, arith=arith)), (net, arith, "train, blob")
        assert same_result(r, e16.dataset_evaluate("eval", blob=w, blocks=True, rows=True, arith=arith)), (net, arith, "engine in f16x2")
    f32, f16 = (eng.dataset_evaluate("eval", blob=w, rows=True, arith=a) for a in ("f32", "f16x2"))
    assert not same_bits(f32["row_logits"], f16["row_logits"]) and np.abs(f32["row_logits"] - f16["row_logits"]).max() < 1e-4


@pytest.mark.parametrize("net", lf.NETS)
def test_grid_independence(engines, oracle, net):
    eng, w = engines[net, "f32"], lf.family(net)["trained"]
    b = lf.batch("recorded", GRID_N)
    eng.dataset_set(*b)
    nb = (GRID_N + 31) // 32
    for arith in ARITHS[net]:
        rs = [eng.dataset_evaluate("eval", blob=w, max_workgroups=g, blocks=True, rows=True, arith=arith) for g in (1, 3, 0)]
        assert [r["grid"] for r in rs] == [1, 3, (nb + 3) // 4 if arith == "f16x2" else nb], arith
        assert same_result(rs[0], rs[1]) and same_result(rs[0], rs[2]), arith
        sub = eng.dataset_evaluate("eval", first_row=33, n_rows=70, blob=w, blocks=True, rows=True, arith=arith)
        assert same_bits(sub["row_kl"], rs[0]["row_kl"][33:103]) and same_bits(sub["row_logits"], rs[0]["row_logits"][33:103]), arith
        check_head_and_totals((net, arith, "sub"), oracle, sub, tuple(a[33:103] for a in b))
        ms, launches = eng.last_timing()
        assert ms > 0.0 and launches == 2


# ---- observer and refusals
def snapshot(eng, cfg, my, op):
    digests = [eng.state_digest(k) for k in ("trainer", "network", "replay", "train_data", "eval_data")]
    s = eng.mcts_search(cfg, my, op, 32)
    return dict(digests=digests, arithmetic=eng.network_arithmetic(), eval=[a.tobytes() for a in eng.policy_eval(my, op)],
                search=[s[k].tobytes() for k in ("child_N", "child_W", "best_action")], cache=eng.last_cache_stats())


@pytest.mark.parametrize("net,engine_arith", [(n, a) for n in lf.NETS for a in ("f32", "f16x2")])
def test_observer_and_refusals(engines, net, engine_arith):
    import synthesis_amd as sa
    from synthesis_amd.engine import SynthesisAmdError

    eng, fam = engines[net, engine_arith], lf.family(net)
    load(eng, net, fam["init"])
    trainer_init(eng, net, fam["trained"])
    tr, ev = lf.batch("recorded", 96), lf.batch("onehot", 77, step=3)
    eng.train_set_data(*tr)
    eng.train_epoch(np.random.default_rng(5).permutation(96).astype(np.int32), 32, 1e-3)
    eng.dataset_set(*ev)
    eng.replay_reserve(256)
    eng.replay_append(tr[0][:40], tr[1][:40], np.arange(40, dtype=np.int64), tr[2][:40], tr[3][:40])
    cfg = sa.parity_mcts_config()
    my, op = tr[0][:8], tr[1][:8]
    snapshot(eng, cfg, my, op)                  # (fills the policy cache: the searches below all find the same entries)
    before = snapshot(eng, cfg, my, op)
    assert before["arithmetic"][0] == engine_arith
    f32_before = eng.dataset_evaluate("eval", blocks=True, rows=True)
    for arith in ARITHS[net][1:]:
        for which in ("train", "eval"):
            eng.dataset_evaluate(which, blocks=True, rows=True, arith=arith)
            eng.dataset_evaluate(which, blob=fam["init"], max_workgroups=2, rows=True, arith=arith)
        assert snapshot(eng, cfg, my, op) == before, arith
        assert same_result(f32_before, eng.dataset_evaluate("eval", blocks=True, rows=True)), arith
    # refusals
    refusals = [(dict(arith=3), INVALID), (dict(arith=-1), INVALID), (dict(arith="f16x2", first_row=70, n_rows=8), INVALID),
                (dict(arith="f16x2", max_workgroups=-1), INVALID), (dict(arith="f16x2", blob=fam["init"][:-1]), INVALID)]
    if net == "mlp":
        refusals += [(dict(arith="bf16"), UNSUPPORTED), (dict(arith="bf16", blob=fam["init"]), UNSUPPORTED)]
        refused = fc.refused_family(fam["init"])
        assert tuple(refused) == fc.REFUSED_MEMBERS
        for name, w in refused.items():
            refusals.append((dict(arith="f16x2", blob=w), UNSUPPORTED))
    for kw, code in refusals:
        with pytest.raises(SynthesisAmdError) as ei:
            eng.dataset_evaluate("eval", **kw)
        assert ei.value.code == code and str(ei.value), kw
    if net == "mlp":
        with np.errstate(all="ignore"):
            for name, w in refused.items():
                r = eng.dataset_evaluate("eval", blob=w, arith="f32")        # f32 still answers (a number or a NaN, not a refusal)
                assert r["rows"] == 77, name
                z = eng.dataset_evaluate("eval", first_row=77, n_rows=0, blob=w, blocks=True, rows=True, arith="f16x2")
                assert all(z[k] == 0 for k in TOTAL_KEYS) and z["block_losses"].shape == (0, 2) and z["row_kl"].shape == (0, 2), name
    assert snapshot(eng, cfg, my, op) == before
    assert same_result(f32_before, eng.dataset_evaluate("eval", blocks=True, rows=True))
    if engine_arith == "f32":
        fresh = sa.Engine(concurrent_games=64, max_explores=64)
        try:
            fresh.dataset_set(*ev)
            for arith in ARITHS[net][1:]:
                with pytest.raises(SynthesisAmdError) as ei:
                    fresh.dataset_evaluate("eval", arith=arith)               # blob = None without a trainer
                assert ei.value.code == NO_WEIGHTS
                r = fresh.dataset_evaluate("eval", blob=fam["trained"], blocks=True, rows=True, arith=arith)   # no trainer, no weights loaded
                assert same_result(r, eng.dataset_evaluate("eval", blob=fam["trained"], blocks=True, rows=True, arith=arith)), arith
        finally:
            fresh.close()


# ---- the learning loop
METRIC_KEYS = ("rows", "mean_pi", "mean_v", "pi_acc", "v_acc")


@pytest.mark.parametrize("net", lf.NETS)
def test_loop_holdout_arith(net):
    import synthesis_amd as sa
    from bench import make_conv_weights, make_weights
    from synthesis_amd.learner import LearningLoop
    from tests.test_gpu_replay_device import EXPLORES

    blob = make_conv_weights(20260101) if net == "conv" else make_weights(20211003)
    cfg = sa.parity_rollout_config(EXPLORES)
    extra = ("f16x2", "bf16") if net == "conv" else ("f16x2",)
    recs, weights, engines = {}, {}, {}
    try:
        for arm, kw in (("host", dict(replay="host", holdout_arith=("f32",) + extra)), ("device", dict(replay="device", holdout_arith=("f32",) + extra)),
                        ("plain", dict(replay="device"))):
            eng = engines[arm] = sa.Engine(concurrent_games=512, max_explores=EXPLORES)
            loop = LearningLoop(eng, net, blob, seed=7, holdout=0.25, **kw)
            recs[arm] = []
            for _ in range(2):
                rec = loop.iteration(cfg, 601, 1000, 1, 32)
                recs[arm].append(rec)
                if arm != "plain":   # by hand: the saved weights on the stored evaluation set
                    n, u = rec["holdout_rows"], rec["holdout_unseen"]
                    assert 0 < u < n
                    for a in extra:
                        for name, rows in (("all", n), ("unseen", u)):
                            m = eng.dataset_evaluate("eval", 0, rows, blob=loop.weights, arith=a)
                            assert rec[f"holdout_after_{a}"][name] == {k: m[k] for k in METRIC_KEYS}, (arm, a, name)
                        assert rec[f"holdout_after_{a}"] != rec["holdout_after"] and rec[f"holdout_before_{a}"] != rec[f"holdout_after_{a}"]
            weights[arm] = loop.weights.copy()
        for a, b, p in zip(recs["host"], recs["device"], recs["plain"]):
            assert set(a) == set(b) == set(p) | {f"holdout_{w}_{x}" for w in ("before", "after") for x in extra}
            for k in a:
                if k != "seconds":
                    assert a[k] == b[k], (k, a[k], b[k])
            assert all(b[k] == p[k] for k in p if k != "seconds")      # the f32 keys are those of a loop without holdout_arith
        assert weights["host"].tobytes() == weights["device"].tobytes() == weights["plain"].tobytes()
    finally:
        for eng in engines.values():
            eng.close()


def test_loop_reports_none_without_a_plan():
    """an iteration whose weights have no f16x2 plan: that arithmetic's metrics are None and the run goes on"""
    import synthesis_amd as sa
    from bench import make_weights
    from synthesis_amd.learner import LearningLoop
    from tests.test_gpu_replay_device import EXPLORES

    blob = make_weights(20211003)
    with sa.Engine(concurrent_games=512, max_explores=EXPLORES) as eng:
        loop = LearningLoop(eng, "mlp", blob, seed=7, holdout=0.25, replay="device", holdout_arith=("f32", "f16x2"))
        rec = loop.iteration(sa.parity_rollout_config(EXPLORES), 601, 1000, 1, 32)
        assert rec["holdout_after_f16x2"] is not None
        st = eng.trainer_state()
        w = st["weights"].copy(); w[7] = np.float32(3e38)
        eng.trainer_set_state(w, st["m"], st["v"], st["step"])
        held = eng.dataset_counts()
        got = loop._holdout_metrics_arith("holdout_before", held)
        assert got == {"holdout_before_f16x2": None}
        assert loop._holdout_metrics(*held)["all"]["rows"] == held[0]


@pytest.mark.parametrize("net", lf.NETS)
def test_the_f32_entry_point_is_the_arith_call(engines, net):
    """syn_dataset_evaluate (the C entry point, which Engine.dataset_evaluate no longer goes through) = syn_dataset_evaluate_arith in f32"""
    from synthesis_amd.engine import CDatasetMetrics

    eng, w = engines[net, "f32"], np.ascontiguousarray(lf.family(net)["trained"], np.float32)
    b = lf.batch("recorded", 95, step=2)
    eng.dataset_set(*b)
    r = eng.dataset_evaluate("eval", blob=w, blocks=True, rows=True, arith="f32")
    m = CDatasetMetrics()
    bl, lg, kl = np.zeros((3, 2), np.float32), np.zeros((95, 12), np.float32), np.zeros((95, 2), np.float32)
    rc = eng._lib.syn_dataset_evaluate(eng._h, 1, 0, 95, _p(w), w.size, 0, C.byref(m), _p(bl), _p(lg), _p(kl))
    assert rc == 0 and (m.rows, m.blocks, m.pi_hits, m.v_hits, m.grid) == (95, 3, r["pi_hits"], r["v_hits"], r["grid"])
    assert dm.f64_bits(m.sum_pi) == dm.f64_bits(r["sum_pi"]) and dm.f64_bits(m.mean_v) == dm.f64_bits(r["mean_v"])
    assert same_bits(bl, r["block_losses"]) and same_bits(lg, r["row_logits"]) and same_bits(kl, r["row_kl"])
