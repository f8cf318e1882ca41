"""The float64 rounded-operand model of the bf16 conv learner (tests/conv_bf16_learner_model.py) against the references it can be held to
without a GPU — the torch float64 goldens and oracle/train.hpp::ConvTrainer with the rounding switched off, the oracle's logits on the
exact-forward members — the conditions that make its bars mean something, and mutations of the model that the bars must catch.

Mutations (test_mutations_move_the_model_beyond_its_own_bar; a mutation that the bars cannot see is listed in NO_EFFECT with the reason):
  trunc                    truncation instead of round-to-nearest-even                      caught
  dz_unrounded_dWh         unrounded dz in dWh                                              caught
  dY_unrounded_dbc         unrounded dY in dbc                                              caught
  drop_edge_tap            the tap reading the row below lost for the top row's cells       caught
  pad_rows                 rows >= B treated as live samples                                caught
  tsum_one                 the target's sum replaced by 1                                   caught
  act_rounded_before_gate  act rounded to bf16 before the ReLU gradient is taken            changes NOTHING: bf16 keeps f32's exponent range,
                           so rounding never moves a positive activation to zero (the gate is unchanged), and every consumer of act rounds
                           it anyway (rounding twice is rounding once)
"""
import os

import numpy as np
import pytest

from tests import conv_bf16_learner_model as M
from tests.f16x2_checkpoints import conv_views
from tests.oracle_lib import default_train_hyper

NO_EFFECT = ("act_rounded_before_gate",)
NON_GRID = tuple(m for m in M.MEMBERS if m not in M.EXACT_FORWARD)


def test_family_and_batches_hold_what_they_promise():
    fam = M.family()
    cw, cb, hw, hb = conv_views(fam["dead"])
    assert (cb[list(M.DEAD_CHANNELS)] == -40).all()
    init = fam["init"]
    assert np.array_equal(conv_views(fam["head_x2^-12"])[2] * np.float32(4096), conv_views(init)[2])
    assert np.array_equal(conv_views(fam["conv_x2^6"])[0], conv_views(init)[0] * np.float32(64))
    for name in M.EXACT_FORWARD:
        cw, cb, hw, hb = conv_views(fam[name].astype(np.float64))
        assert np.array_equal(cw * 8, np.round(cw * 8)) and np.array_equal(cb * 8, np.round(cb * 8))
        assert np.array_equal(hw * 64, np.round(hw * 64)) and np.array_equal(hb * 512, np.round(hb * 512))
    my, op, tpi, tv, names = M.pool()
    e, f = names["empty"], names["full_column_corners"]
    assert my[e] == 0 and op[e] == 0
    occ = int(my[f]) | int(op[f])
    assert all(occ >> bit & 1 for bit in (0, 6, 56, 62)) and (occ >> 28) & 0x7F == 0x7F and not int(my[f]) & int(op[f])
    assert (tpi[f] == 0).sum() == 3 and sorted(tv[f]) == [0, 0, 1]
    assert tpi[names["ulp_drift"]].astype(np.float64).sum() != 1.0 and abs(tpi[names["short_sum"]].sum() - 0.9) < 1e-6
    assert M.mirror_bb(np.uint64((1 << 0) | (1 << 8) | (1 << 62))) == np.uint64((1 << 56) | (1 << 50) | (1 << 6))
    for member in M.MEMBERS:
        for B in M.BATCHES:
            seed = M.BATCH_SEEDS.get((member, B), 0)
            idx = M.batch_indices(B, seed)
            bm, bo, bp, bv = M.batch(B, seed)
            assert idx.size == B == bm.size
            if B == 1:
                assert idx[0] == e
                continue
            r = int(np.flatnonzero(idx == M.MIRROR_ROW)[0])   # a mirrored pair (across the two 16-sample tiles from B = 19 on)
            assert M.mirror_bb(bm[r - 1]) == bm[r] and M.mirror_bb(bo[r - 1]) == bo[r] and bm[r] != bm[r - 1]
            assert np.array_equal(bp[r - 1][::-1], bp[r]) and (B < 19 or r == 16)
            if B > 2:   # every batch of 15 and more holds every hand-made row
                assert set(names.values()) <= set(idx.tolist()), B


def test_identity_rounding_is_the_torch_float64_step(golden_dir):
    g = np.load(os.path.join(golden_dir, "conv_train_torch_goldens.npz"))
    r = M.conv_bf16_step(M.family()["init"], g["my_bb"][0], g["op_bb"][0], g["target_pi"][0], g["target_v"][0], round="identity")
    assert np.abs(r["grads"] - g["first_grad_f64"]).max() <= 1e-12
    assert np.abs(r["losses"] - g["losses_f64"][0]).max() <= 1e-12


@pytest.mark.parametrize("B", M.BATCHES)
@pytest.mark.parametrize("member", M.MEMBERS)
def test_identity_rounding_is_the_f32_oracle_step(oracle, member, B):
    """Rounding switched off, the model is oracle/train.hpp::ConvTrainer within 1e-6 of each block's largest gradient."""
    blob = M.family()[member]
    my, op, tpi, tv = M.batch(B, M.BATCH_SEEDS.get((member, B), 0))
    pw, vw = M.loss_weights(B)
    r = M.conv_bf16_step(blob, my, op, tpi, tv, pw, vw, round="identity")
    go, lo = oracle.convtrain_gradients(blob, default_train_hyper(policy_weight=pw, value_weight=vw), my, op, tpi, tv)
    outside = []
    for name, sl in M.BLOCKS.items():
        scale = float(np.abs(r["grads"][sl]).max())
        err = float(np.abs(r["grads"][sl] - go[sl]).max())
        print(f"{member} B={B} {name}: |model - oracle| {err:.3e} = {err / max(scale, 1e-300):.3e} of the block's largest gradient")
        if not err <= 1e-6 * scale:
            outside.append((name, err / scale))
    assert np.abs(r["losses"] - lo).max() <= 1e-6 * max(1.0, float(np.abs(lo).max())), (member, B)
    z = M.exact_zero_entries(member)
    assert not r["grads"][z].any() and not go[z].any()
    for mode in ("f64", "f32"):   # and under bf16 rounding, in either accumulation: exact zeros stay exact zeros
        assert not M.conv_bf16_step(blob, my, op, tpi, tv, pw, vw, accumulate=mode, seed=3)["grads"][z].any()
    assert not outside, (member, B, outside)


@pytest.mark.parametrize("member", M.EXACT_FORWARD)
def test_exact_forward_members(oracle, member):
    """The f32 oracle, the float64 model and the f32 random-order variant compute the SAME logits; the activations are bf16 numbers;
    no partial sum of a logit can leave 20 bits; and the conditions of the derived bar hold: no fragile dz, fragile dY under 1 %."""
    blob = M.family()[member]
    peak = 0.0
    for B in M.BATCHES:
        c = M.case(member, B)
        my, op, tpi, tv = c["batch"]
        m = c["model"]
        peak = max(peak, float(np.abs(m["raw"]).max()))
        assert np.array_equal(m["raw"], m["raw"].astype(np.float32).astype(np.float64))
        assert np.array_equal(m["act"], M.round_bf16(m["act"])) and np.array_equal(m["act"] * 8, np.round(m["act"] * 8))
        assert m["raw_sumabs"].max() < 2.0 ** 11 and np.array_equal(m["raw"] * 512, np.round(m["raw"] * 512))
        v = M.conv_bf16_step(blob, my, op, tpi, tv, c["pw"], c["vw"], accumulate="f32", seed=B)
        for mode in (oracle.ACC_SLIMNN, oracle.ACC_FMA):
            raw = oracle.c4conv_eval(blob, my, op, mode=mode, raw=True)[2]
            assert np.array_equal(raw.view(np.uint32), m["raw"].astype(np.float32).view(np.uint32)), (member, B, mode)
            assert np.array_equal(raw.view(np.uint32), v["raw"].astype(np.float32).view(np.uint32)), (member, B, mode)
        # 3a: dz feeds every chain — none may be fragile, by the wider of 2^-20 relative and what an f32 H phase can move it by
        assert not m["fragile"]["dz"].any(), (member, B)
        assert not (M.boundary_distance(m["dz"]) <= 2.0 ** -20 * np.abs(m["dz"])).any(), (member, B)
        nz = int((m["dY"] != 0).sum()); nf = int(m["fragile"]["dY"].sum())
        print(f"{member} B={B}: max |logit| {np.abs(m['raw']).max():.2f}  fragile dY {nf} of {nz}")
        assert nf <= 0.01 * nz, (member, B, nf, nz)
        assert not m["fragile"]["act"].any() and not m["fragile"]["gate"].any()
    assert peak > 25.0 if member == "grid_sharp" else peak < 8.0, peak


@pytest.mark.parametrize("member", NON_GRID)
def test_measured_bar_is_far_below_the_bf16_effect(member):
    """3b: in every parameter block 8 x floor is at most 1/20 of what the bf16 rounding itself moves; a degenerate block (one whose
    bf16 effect is not above 20 x its own derived term, e.g. the head biases' gradients of head_x2^-12, the conv weights' under the
    empty board) is held to the derived bar instead. The losses carry no such condition: the rounding moves a loss by 1e-6 to 1e-4 of
    its value, next to an f32 H phase that moves it by 1e-7."""
    blob = M.family()[member]
    for B in M.BATCHES:
        c = M.case(member, B)
        my, op, tpi, tv = c["batch"]
        ident = M.conv_bf16_step(blob, my, op, tpi, tv, c["pw"], c["vw"], round="identity")
        eff, leff, fr = c["effect"], c["loss_effect"], c["model"]["fragile"]
        assert eff == M.block_maxima(c["model"]["grads"] - ident["grads"])
        print(f"{member} B={B}: " + "  ".join(f"{k} floor {c['floor'][k]:.2e} effect {eff[k]:.2e}" + (" (degenerate)" if c["degenerate"][k] else "")
                                              for k in M.BLOCKS)
              + f"  loss floor {c['loss_floor'].max():.2e} effect {leff.max():.2e}"
              + f"  fragile act {int(fr['act'].sum())} gate {int(fr['gate'].sum())} dz {int(fr['dz'].sum())} dY {int(fr['dY'].sum())}")
        der = M.derived_bar(c["model"])
        for name, sl in M.BLOCKS.items():
            if c["degenerate"][name]:
                assert eff[name] <= 20 * der[sl].max() and np.array_equal(c["bar"][sl], der[sl]), (member, B, name)
            else:
                assert 8 * c["floor"][name] <= eff[name] / 20, (member, B, name, c["floor"][name], eff[name])
                assert np.array_equal(c["bar"][sl], np.maximum(der[sl], 8 * c["floor"][name]))
        assert M.bar_means_something(c)
        assert (c["loss_bar"] >= 8 * c["loss_floor"]).all() and (c["loss_bar"] >= 32 * M.U23 * c["model"]["loss_sumabs"]).all()
    n_deg = sum(M.case(member, B)["degenerate"][k] for B in M.BATCHES for k in M.BLOCKS)
    print(f"{member}: {n_deg} degenerate blocks of {4 * len(M.BATCHES)}")


def test_mutations_move_the_model_beyond_its_own_bar():
    """Every mistake listed in the module docstring, made in the model, leaves the bar of the unmutated model on at least one non-grid
    member: the same mistake in a kernel would fail the GPU test."""
    fam = M.family()
    caught = {}
    for mut in M.MUTATIONS:
        for member in NON_GRID:
            for B in (17, 32, 2):
                c = M.case(member, B)
                my, op, tpi, tv = c["batch"]
                r = M.conv_bf16_step(fam[member], my, op, tpi, tv, c["pw"], c["vw"], mutation=mut)
                over = np.abs(r["grads"] - c["model"]["grads"]) / np.maximum(c["bar"], 1e-300)
                lover = np.abs(r["losses"] - c["model"]["losses"]) / np.maximum(c["loss_bar"], 1e-300)
                if over.max() > 1 or lover.max() > 1:
                    caught.setdefault(mut, (member, B, float(max(over.max(), lover.max()))))
                    break
            if mut in caught:
                break
    print("\n".join(f"{k}: caught on {v[0]} B={v[1]}, {v[2]:.3g} x the bar" for k, v in caught.items()))
    assert set(M.MUTATIONS) - set(caught) == set(NO_EFFECT), caught
    # the one that changes nothing changes NOTHING (not "too little to see")
    c = M.case("trained", 17)
    my, op, tpi, tv = c["batch"]
    r = M.conv_bf16_step(fam["trained"], my, op, tpi, tv, c["pw"], c["vw"], mutation="act_rounded_before_gate")
    assert np.array_equal(r["grads"], c["model"]["grads"]) and np.array_equal(r["losses"], c["model"]["losses"])


def test_oracle_adam_on_a_conv_parameter_vector(oracle, golden_dir):
    """The reference of the GPU tests' Adam half: oracle.train_adam on Connect4ConvNet's 12,412 floats is ConvTrainer's own update
    (two steps of convtrain_steps = gradients + train_adam, twice), bit for bit."""
    g = np.load(os.path.join(golden_dir, "conv_train_torch_goldens.npz"))
    hp = default_train_hyper(weight_decay=1e-3)
    w = M.family()["init"]; m = np.zeros_like(w); v = np.zeros_like(w); step = 0
    for s in range(2):
        gr, _ = oracle.convtrain_gradients(w, hp, g["my_bb"][s], g["op_bb"][s], g["target_pi"][s], g["target_v"][s])
        w, m, v, step = oracle.train_adam(w, hp, gr, float(g["lrs"][s]), m, v, step)
    wo, mo, vo, so, _ = oracle.convtrain_steps(M.family()["init"], hp, g["my_bb"][:2], g["op_bb"][:2], g["target_pi"][:2], g["target_v"][:2],
                                               g["lrs"][:2])
    assert step == so == 2 and w.size == M.NUM
    assert np.array_equal(w.view(np.uint32), wo.view(np.uint32)) and np.array_equal(m, mo) and np.array_equal(v, vo)
