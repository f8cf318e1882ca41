"""The f32 learners' stress family on the CPU (tests/learner_f32_family.py): the oracle (train_gradients / train_steps / convtrain_* /
train_adam) is held to the float64 bars on every case of the table, the subnormal members' premises are asserted on the oracle, every
mutation of the float64 model is caught by a named member and batch, and the table covers what the GPU routes must run."""
import numpy as np
import pytest

from tests import f16x2_checkpoints as fc
from tests import learner_f32_family as lf

_ORACLE_RUNS = {}


def oracle_history(oracle, c):
    if c.ref_key not in _ORACLE_RUNS:
        _ORACLE_RUNS[c.ref_key] = lf.oracle_steps(oracle, c.net, lf.family(c.net)[c.member], lf.case_batches(c), c.hyper, [lf.LR] * c.steps)
    return _ORACLE_RUNS[c.ref_key]


def barred_cases(net):
    seen, out = set(), []
    for c in lf.cases(net):
        if c.route in lf.BARRED_ROUTES and c.ref_key not in seen:
            seen.add(c.ref_key); out.append(c)
    return out


def test_model_forward_is_the_f64_reference_and_its_gradient_torchs():
    """mlp_step / conv_step compute mlp_f64 / conv_f64's outputs, and the first gradients / losses torch computed in float64."""
    my, op, tpi, tv = lf.batch("recorded", 32)
    for net, f64 in (("mlp", fc.mlp_f64), ("conv", fc.conv_f64)):
        for member in ("init", "trained", "zero"):
            w = lf.family(net)[member]
            raw = lf.STEP[net](w, my, op, tpi, tv, lf.HYPERS["default"])["raw"]
            ref = f64(w, my, op)[0]
            assert np.abs(raw - ref).max() <= 1e-13 * max(1.0, np.abs(ref).max()), (net, member)
    g = np.load(lf.GOLD)
    r = lf.mlp_step(lf.family("mlp")["init"], my, op, tpi, tv, lf.HYPERS["default"])
    assert np.abs(r["grads"] - g["grad0_f64"]).max() <= 1e-14 and np.abs(r["losses"] - g["losses_f64"][0]).max() <= 1e-13
    bs = tuple(g[k] for k in ("my_bb", "op_bb", "target_pi", "target_v"))
    run = lf.run_steps("mlp", lf.family("mlp")["init"], bs, lf.HYPERS["default"], g["lrs"])
    assert np.abs(run["weights"] - g["weights_f64"]).max() <= 1e-9 and np.abs(run["losses"] - g["losses_f64"]).max() <= 1e-9
    gc = np.load(lf.GOLD.replace("train_torch", "conv_train_torch"))
    bs = tuple(gc[k] for k in ("my_bb", "op_bb", "target_pi", "target_v"))
    run = lf.run_steps("conv", lf.family("conv")["init"], bs, lf.HYPERS["default"], gc["lrs"])
    assert np.abs(run["grads0"] - gc["first_grad_f64"]).max() <= 1e-13
    assert np.abs(run["weights"] - gc["final_weights_f64"]).max() <= 1e-9 and np.abs(run["losses"] - gc["losses_f64"]).max() <= 1e-9


@pytest.mark.parametrize("net", lf.NETS)
def test_oracle_meets_the_f64_bars_on_every_case(oracle, net):
    """Gradients, losses of every step, weights, m and v after the case's steps: max |oracle - f64| <= 8 x floor per parameter block. A
    gate-fragile case is not held to the bars; at most GATE_FRAGILE_CAP members may have one."""
    fragile = set()
    for c in barred_cases(net):
        ref = lf.case_reference(c)
        hist = oracle_history(oracle, c)
        assert all(np.isfinite(h[k]).all() for h in hist for k in ("weights", "m", "v", "grads", "losses")), c.id
        assert hist[-1]["step"] == c.steps == ref["f64"]["step"]
        if ref["gate_fragile"]:
            fragile.add(c.member)
            continue
        lf.check_bars(c.id, net, ref, lf.final_state(hist))
    print(net, "gate-fragile members:", sorted(fragile))
    assert len(fragile) <= lf.GATE_FRAGILE_CAP, fragile


@pytest.mark.parametrize("net", lf.NETS)
def test_oracle_step_loop_is_train_steps(oracle, net):
    """oracle_steps (gradients, then train_adam) gives the bits of train_steps / convtrain_steps, the calls the GPU suite compares with."""
    for c in lf.cases(net, "epoch")[:3]:
        bs, blob = lf.case_batches(c), lf.family(net)[c.member]
        if net == "mlp":
            X = np.stack([oracle.c4_features(bs[0][s], bs[1][s]) for s in range(c.steps)])
            w, m, v, step, lo = oracle.train_steps(blob, lf.oracle_hyper(c.hyper), X, bs[2], bs[3], [lf.LR] * c.steps)
        else:
            w, m, v, step, lo = oracle.convtrain_steps(blob, lf.oracle_hyper(c.hyper), *bs, [lf.LR] * c.steps)
        st = lf.final_state(oracle_history(oracle, c))
        assert step == st["step"] and fc.same_bits(lo, st["losses"])
        assert fc.same_bits(w, st["weights"]) and fc.same_bits(m, st["m"]) and fc.same_bits(v, st["v"]), c.id


def test_subnormal_members_are_subnormal_on_the_oracle(oracle):
    """The premise of each subnormal member, on the oracle with weight_decay = 0 and the recorded batches at B = 32. A member whose premise
    fails is a broken test."""
    for (net, member), floors in lf.SUBNORMAL_FLOORS.items():
        hist = lf.oracle_steps(oracle, net, lf.family(net)[member], lf.batches("recorded", 32, lf.EPOCH_STEPS), "wd0", [lf.LR] * lf.EPOCH_STEPS)
        got = dict(grad_subnormal=lf.count_subnormal(hist[0]["grads"]), grad_zero=int((hist[0]["grads"] == 0).sum()),
                   v6_subnormal=lf.count_subnormal(hist[-1]["v"]), m6_subnormal=lf.count_subnormal(hist[-1]["m"]),
                   v6_zero=int((hist[-1]["v"] == 0).sum()))
        print(net, member, got)
        for k, floor in floors.items():
            assert got[k] >= floor, (net, member, k, got[k], floor)
        # exactly-zero entries have m = v = 0: the update is 0 / eps and leaves the weight's bits alone
        z = (hist[-1]["v"] == 0) & (hist[-1]["m"] == 0)
        assert fc.same_bits(hist[-1]["weights"][z], lf.family(net)[member][z])
    # with the default weight decay none of this appears
    hist = lf.oracle_steps(oracle, "mlp", lf.family("mlp")["mlp_init_x2^-30"], lf.batches("recorded", 32, 1), "default", [lf.LR])
    assert lf.count_subnormal(hist[0]["m"]) == 0
    # the target edges: finite losses, and the logarithm does run on the subnormal entry
    assert oracle.det_logf(np.array([1e-42], np.float32))[0] == pytest.approx(np.log(np.float64(np.float32(1e-42))), rel=1e-6)


# (mutation, net, member, variant, B, hyper, steps): the case each mutation of the float64 model must break
MUTATION_CASES = (("gate_ge", "mlp", "mlp_init_l1_zero", "subnormal_t", 32, "wd0", 1), ("gate_ge", "conv", "conv_init_conv_zero", "subnormal_t", 17, "wd0", 1),
                  ("tsum_one", "mlp", "init", "tsum_half", 33, "default", 6), ("tsum_one", "conv", "init", "tsum_half", 17, "default", 6),
                  ("tsum_one", "mlp", "zero", "zero_row", 33, "wd0", 1), ("tsum_one", "conv", "zero", "zero_row", 32, "wd0", 1),
                  ("kl_keeps_t0", "mlp", "trained", "onehot", 31, "wd0", 1), ("kl_keeps_t0", "conv", "trained", "onehot", 17, "wd0", 1),
                  ("wd_when_zero", "mlp", "mlp_init_x2^-30", "zero_row", 32, "wd0", 6), ("wd_when_zero", "conv", "trained", "zero_row", 32, "wd0", 1),
                  ("wd_dropped", "mlp", "init_l2_x2^-20", "zero_row", 32, "weighted", 1), ("wd_dropped", "conv", "init_conv_x2^-30", "zero_row", 32, "weighted", 1),
                  ("bias_step_off_by_one", "mlp", "init", "recorded", 1, "default", 1), ("bias_step_off_by_one", "conv", "init", "recorded", 1, "default", 1))


@pytest.mark.parametrize("mutation,net,member,variant,B,hyper,steps", MUTATION_CASES, ids=lambda x: str(x))
def test_every_mutation_of_the_model_is_caught(mutation, net, member, variant, B, hyper, steps):
    """A model that is wrong in one definition leaves the bars of its named case (which is a case of the table: the oracle meets them)."""
    assert mutation in lf.MUTATIONS and {m[0] for m in MUTATION_CASES} == set(lf.MUTATIONS)
    key = (net, member, variant, B, hyper, steps)
    assert key in {c.ref_key for c in lf.CASES if c.route in lf.BARRED_ROUTES}, key
    ref = lf.reference(*key)
    assert not ref["gate_fragile"]
    bad = lf.run_steps(net, lf.family(net)[member], lf.batches(variant, B, steps), lf.HYPERS[hyper], [lf.LR] * steps, mutation=mutation)
    lf.check_bars("unmutated", net, ref, ref["f64"])
    with pytest.raises(AssertionError):
        lf.check_bars(mutation, net, ref, bad)


@pytest.mark.parametrize("net", lf.NETS)
def test_flushing_subnormals_round_the_oracles_adam_is_caught(oracle, net):
    """Subnormal g, m, v flushed to zero round oracle.train_adam, on the subnormal member's one-step case (after the first step the
    output biases have moved by lr and the gradients are normal numbers again): the gradient and m leave their float64 bars, and their
    bits differ from the oracle's (the comparison the GPU suite makes)."""
    c = [c for c in lf.cases(net, "step") if c.member == lf.SUBNORMAL_MEMBERS[net][0] and c.hyper == "wd0"][0]
    ref = lf.case_reference(c)
    good = lf.final_state(oracle_history(oracle, c))
    bad = lf.final_state(lf.oracle_steps(oracle, net, lf.family(net)[c.member], lf.case_batches(c), c.hyper, [lf.LR] * c.steps, flush=True))
    assert not fc.same_bits(good["m"], bad["m"]) and not fc.same_bits(good["grads"], bad["grads"])
    with pytest.raises(AssertionError):
        lf.check_bars("flush", net, ref, bad)


def test_the_table_covers_what_the_issue_lists():
    for net in lf.NETS:
        cs = lf.cases(net)
        assert {c.member for c in cs} == set(lf.family(net))
        assert {c.variant for c in cs} == set(lf.VARIANTS)
        assert {c.B for c in cs if c.route != "micro"} >= set(lf.BATCH_SIZES[net]) and {c.B for c in cs if c.route == "micro"} == {lf.MICRO_B}
        assert {c.hyper for c in cs} == set(lf.HYPERS)
        assert ("duplicates", 32) in {(c.variant, c.B) for c in cs}
        for route in lf.ROUTES:
            rc = lf.cases(net, route)
            members = {c.member for c in rc if c.hyper == "wd0"}
            need = {"trained", "zero"} | (set(lf.SUBNORMAL_MEMBERS[net]) if route != "child" else {lf.SUBNORMAL_MEMBERS[net][0]})
            assert members >= need, (net, route, need - members)
            assert {c.variant for c in rc} >= set(lf.EDGE_VARIANTS), (net, route)
        assert len(lf.cases(net, "child")) == 3 and all(c.hyper == "wd0" for c in lf.cases(net, "child"))
        assert all(c.B <= 100 and c.steps <= 6 for c in cs)
        # no degenerate case: a zeroed row as the only sample makes dz, every gradient, both losses and both moments exactly 0 ...
        assert not [c.id for c in cs if c.variant == "zero_row" and c.B == 1]
        # ... and every member has a case whose float64 first gradient is not identically zero, with non-zero floors to be held to
        for member in lf.family(net):
            live = [c for c in cs if c.member == member and c.route in lf.BARRED_ROUTES and np.any(lf.case_reference(c)["f64"]["grads0"] != 0)]
            assert live, (net, member)
            assert any(max(lf.case_reference(c)["floor"]["grads"].values()) > 0 for c in live), (net, member)
