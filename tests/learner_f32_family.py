"""A stress family for the f32 learners (Connect4Net: train_mfma.cuh / train_epoch.cuh / train_kernels.cuh / train_micro.cuh; Connect4ConvNet
f32: train_conv_mfma.cuh), a float64 model of the learner step of both networks, and the bars the oracle and the device are held to.
TEST INFRASTRUCTURE ONLY; numpy, no GPU. It shares no code with the engine or with oracle/train.hpp.

Checkpoints: every member of mlp_family / conv_family (tests/f16x2_checkpoints.py; the learner refuses none of them) plus the learner's
own — the learner has no f16x2 plan, so the +-2^24 window of that family does not apply:
  mlp_init_x2^-30, mlp_init_x2^-28   every W and b of the random-init Connect4Net x 2^-30 / 2^-28: the first gradient (weight_decay = 0) is
                                     mostly subnormal or exactly zero (x 2^-30 on the recorded batch 0: 14,464 subnormal and 13,259 zero
                                     entries of 30,492; test_learner_f32_family.py asserts the floors)
  conv_init_x2^-118                  every parameter of the random-init Connect4ConvNet x 2^-118. Found by a scan of head-weight and whole-blob
                                     scalings by 2^-k, k = 40, 42 .. 130, on the oracle (scan_conv_subnormal(); weight_decay = 0, recorded
                                     batch 0). dz = weight / B (softmax tsum - t) does not shrink with the network, so dWh = dz^T act turns
                                     subnormal only once the activations themselves are near 2^-120, and scaling the head alone reaches the
                                     subnormals only through dWc: head x 2^-60 gives 0 subnormal entries, head x 2^-118 117, head x 2^-120
                                     248 (and never more than 284 of the 304 conv entries). Whole blob x 2^-k: 0 up to k = 88, 125 at 108,
                                     665 at 112, 3,831 at 116, 7,157 at 118 (plus 2,861 exact zeros, of 12,412), 9,318 at 120; from k = 120
                                     on most parameters are subnormal themselves. k = 118 keeps most parameters normal (|w| >= 2^-8 before
                                     the scaling) with a subnormal tail, so both kinds of operand reach the matrix cores.
  mlp_init_l1_zero, conv_init_conv_zero   the first layer's W and b are zero, the rest is the random init: every pre-activation of that layer is
                                     exactly 0 with live weights behind it, so the ReLU gate `> 0` (not `>= 0`) alone decides the first layer's
                                     gradient (in `zero` the weights behind the gate are zero too and cannot tell the two apart)
Batches: positions and targets of tests/golden/train_torch_goldens.npz (12 x 32 recorded rows) with the target variants of VARIANTS.
Hyper-parameters: HYPERS.

The float64 model (mlp_step / conv_step + adam_step) is written from the definitions at the top of oracle/train.hpp: KL with 0 log 0 = 0,
tsum multiplying the softmax, ReLU gate > 0, Adam with the bias correction computed on the host in double. Its forward pass is the one
of mlp_f64 / conv_f64 (the CPU test asserts they agree). mode = "f32" sums every chain in float32 in a seeded random order, keeps every
intermediate in float32 and runs Adam's expression in unfused float32: that variant exists only to measure the reference's own noise floor.

Bars (none is taken from a kernel's output), per parameter block (Connect4Net: W1, b1 .. W5, b5; Connect4ConvNet: the four blocks of
conv_bf16_learner_model.BLOCKS):  max |x - f64| <= 8 x floor,  floor = the largest |f32 random-order variant - f64| of that block over 8
seeds; 8 is the margin the bf16 model uses, for the same reason (the kernel's order is one order among many). The same rule holds the two
losses of every step and the weights, m and v after the case's Adam steps (the floors then come from the f32 variant's whole chain).
A case is gate-fragile when some float64 pre-activation of its FIRST step lies no further from 0 than the f32 variants' spread at that unit:
there the bars are not asserted (the bit-for-bit comparison with the oracle still is); at most GATE_FRAGILE_CAP members per network may fall
out so. Later steps of a six-step case are not judged: a gate that flips in steps 2 to 6 shows as a missed bar, not as a fragile case.
"""
import functools
import os
from collections import OrderedDict

import numpy as np

from tests import conv_bf16_learner_model as cbl
from tests import f16x2_checkpoints as fc

GOLD = os.path.join(fc.GOLDEN, "train_torch_goldens.npz")
MLP_NUM = 30492
NETS = ("mlp", "conv")
MLP_OWN = ("mlp_init_x2^-30", "mlp_init_x2^-28", "mlp_init_l1_zero")
CONV_SUBNORMAL_EXP = -118
CONV_OWN = (f"conv_init_x2^{CONV_SUBNORMAL_EXP}", "conv_init_conv_zero")
SUBNORMAL_MEMBERS = dict(mlp=("mlp_init_x2^-30", "mlp_init_x2^-28", "init_x2^-16"), conv=CONV_OWN[:1])
GATE_ZERO_MEMBERS = dict(mlp="mlp_init_l1_zero", conv="conv_init_conv_zero")
VARIANTS = ("recorded", "onehot", "zero_row", "tsum_half", "subnormal_t", "tiny_t", "duplicates", "empty_board")
BATCH_SIZES = dict(mlp=(1, 31, 32, 33, 100), conv=(1, 17, 32))
MICRO_B = 96
HYPERS = OrderedDict((("default", dict(weight_decay=1e-6, policy_weight=1.0, value_weight=1.0)),
                      ("wd0", dict(weight_decay=0.0, policy_weight=1.0, value_weight=1.0)),
                      ("weighted", dict(weight_decay=1e-3, policy_weight=0.7, value_weight=1.9))))
BETA1, BETA2, EPS = 0.9, 0.999, 1e-8   # Adam::default()
N_FLOOR_SEEDS, MARGIN, GATE_FRAGILE_CAP = 8, 8.0, 2
LR, EPOCH_STEPS = 1e-3, 6
MUTATIONS = ("gate_ge", "tsum_one", "kl_keeps_t0", "wd_when_zero", "wd_dropped", "bias_step_off_by_one")   # + the flush built round the oracle
F32_TINY = float(np.finfo(np.float32).tiny)
# what the CPU test asserts of the subnormal members on the oracle (weight_decay = 0, recorded batch, B = 32): (quantity, floor)
SUBNORMAL_FLOORS = {("mlp", "mlp_init_x2^-30"): dict(grad_subnormal=10000, grad_zero=10000),
                    ("mlp", "mlp_init_x2^-28"): dict(grad_subnormal=5000, grad_zero=10000),
                    ("mlp", "init_x2^-16"): dict(v6_subnormal=1000, grad_zero=10000),
                    ("conv", CONV_OWN[0]): dict(grad_subnormal=100)}


def mlp_blocks():
    out, o = OrderedDict(), 0
    for l, (k, n) in enumerate(zip(fc.MLP_DIMS[:-1], fc.MLP_DIMS[1:]), 1):
        out[f"W{l}"] = slice(o, o + k * n); o += k * n
        out[f"b{l}"] = slice(o, o + n); o += n
    assert o == MLP_NUM
    return out


BLOCKS = dict(mlp=mlp_blocks(), conv=cbl.BLOCKS)


def count_subnormal(a):
    a = np.abs(np.asarray(a, np.float32))
    return int(((a > 0) & (a < np.float32(F32_TINY))).sum())


def flush_subnormal(a):
    a = np.array(a, np.float32)
    a[np.abs(a) < np.float32(F32_TINY)] = 0.0
    return a


# ---- checkpoints ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def family(net):
    blob, trained, cblob, ctrained = fc.load_fixtures()
    if net == "mlp":
        fam = fc.mlp_family(blob, trained)
        for k in (-30, -28):
            fam[f"mlp_init_x2^{k}"] = np.ascontiguousarray(blob, np.float32) * fc._p2(k)
        w = np.array(blob, np.float32); W, b = fc.mlp_views(w)[0]; W[:] = 0; b[:] = 0
        fam["mlp_init_l1_zero"] = w
    else:
        fam = fc.conv_family(cblob, ctrained)
        fam[CONV_OWN[0]] = np.ascontiguousarray(cblob, np.float32) * fc._p2(CONV_SUBNORMAL_EXP)
        w = np.array(cblob, np.float32); cw, cb, _, _ = fc.conv_views(w); cw[:] = 0; cb[:] = 0
        fam["conv_init_conv_zero"] = w
    assert tuple(fam)[-len(MLP_OWN if net == "mlp" else CONV_OWN):] == (MLP_OWN if net == "mlp" else CONV_OWN)
    assert all(v.dtype == np.float32 and np.isfinite(v).all() for v in fam.values())
    for v in fam.values():
        v.setflags(write=False)
    return fam


def scan_conv_subnormal(oracle, ks=range(40, 131, 2)):
    """How CONV_SUBNORMAL_EXP was found: {(kind, k): (subnormal, zero)} of the oracle's first gradient for head W x 2^-k and whole blob x 2^-k."""
    cblob = fc.load_fixtures()[2]
    my, op, tpi, tv = batch("recorded", 32)
    out = OrderedDict()
    for kind in ("head", "blob"):
        for k in ks:
            w = cblob.copy()
            if kind == "head":
                fc.conv_views(w)[2][:] *= fc._p2(-k)
            else:
                w *= fc._p2(-k)
            g, _ = oracle.convtrain_gradients(w, oracle_hyper("wd0"), my, op, tpi, tv)
            out[(kind, k)] = (count_subnormal(g), int((g == 0).sum()))
    return out


# ---- batches --------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def recorded():
    g = np.load(GOLD)
    out = (g["my_bb"].reshape(-1), g["op_bb"].reshape(-1), g["target_pi"].reshape(-1, 9), g["target_v"].reshape(-1, 3))
    for a in out:
        a.setflags(write=False)
    return out


def batch(variant, B, step=0):
    """(my [B], op [B], tpi [B][9], tv [B][3]) of step `step`: recorded rows step * B .. (wrapping round the 384), with the variant applied.
    The edited rows are 0 and B - 1 (both ends of the batch; the last row sits in the ragged chunk of B = 31, 33, 100)."""
    assert variant in VARIANTS
    my, op, tpi, tv = recorded()
    i = (step * B + np.arange(B)) % my.size
    if variant == "duplicates":   # one position B times (the issue's case is B = 32), with its own target
        i = np.full(B, i[0])
    my, op, tpi, tv = my[i].copy(), op[i].copy(), tpi[i].copy(), tv[i].copy()
    rows = sorted({0, B - 1})
    for r in rows:
        if variant == "onehot":   # both heads
            j, k = int(np.argmax(tpi[r])), int(np.argmax(tv[r]))
            tpi[r] = 0; tpi[r, j] = 1; tv[r] = 0; tv[r, k] = 1
        elif variant == "zero_row":   # tsum = 0 in both heads
            tpi[r] = 0; tv[r] = 0
        elif variant == "tsum_half":
            tpi[r] *= np.float32(0.5); tv[r] *= np.float32(0.5)
        elif variant in ("subnormal_t", "tiny_t"):   # one entry of the policy target: passes t > 0, so the logarithm runs on it
            tpi[r, int(np.argmin(tpi[r]))] = np.float32(1e-42 if variant == "subnormal_t" else 1e-30)
    if variant == "empty_board":
        my[0] = 0; op[0] = 0
    return my, op, tpi, tv


def batches(variant, B, n_steps):
    bs = [batch(variant, B, s) for s in range(n_steps)]
    return tuple(np.stack([b[k] for b in bs]) for k in range(4))


def oracle_hyper(name):
    from tests.oracle_lib import default_train_hyper

    return default_train_hyper(**HYPERS[name])


# ---- the float64 model ----------------------------------------------------------------------------------------------------------------
_Acc = cbl._Acc   # chains along the last axis: float64, or float32 in a seeded random order


def _head(raw, tgt, weight, B, acc, mutation):
    """One head group: (kl [B], dz [B][k]). kl = sum t (log t - log p) over t > 0 (0 log 0 = 0); dz = weight / B * (softmax * tsum - t).
    The three sums over the head's entries are chains like any other (random order in the f32 mode)."""
    f32 = acc.f32
    ft = np.float32 if f32 else np.float64
    x = raw.astype(ft); t = tgt.astype(ft)
    sc = (np.float32(weight) * (np.float32(1) / np.float32(B))) if f32 else np.float64(np.float32(weight)) / B
    mx = x.max(axis=1, keepdims=True)
    lse = mx + np.log(acc.chain(np.exp(x - mx).astype(np.float64)).astype(ft))[:, None]
    logp = x - lse
    tsum = np.ones_like(mx) if mutation == "tsum_one" else acc.chain(t.astype(np.float64)).astype(ft)[:, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        if mutation == "kl_keeps_t0":
            term = t * (np.log(t) - logp)
        else:
            term = np.where(t > 0, t * (np.log(np.where(t > 0, t, 1)) - logp), ft(0))
        dz = sc * (np.exp(logp) * tsum - t)
        return acc.chain(term.astype(np.float64)), dz.astype(np.float64)


def _heads(raw, tpi, tv, hp, B, acc, mutation):
    klp, dzp = _head(raw[:, :9], tpi, hp["policy_weight"], B, acc, mutation)
    klv, dzv = _head(raw[:, 9:], tv, hp["value_weight"], B, acc, mutation)
    with np.errstate(invalid="ignore"):
        total = acc.chain(np.stack([klp, klv]))                                  # over the samples
        if acc.f32:
            losses = ((np.float32(1) / np.float32(B)) * total.astype(np.float32)).astype(np.float64)
        else:
            losses = total / B
    return losses, np.concatenate([dzp, dzv], axis=1)


def _gate(pre, mutation):
    return pre >= 0 if mutation == "gate_ge" else pre > 0


def _targets(B, tpi, tv):
    return (np.asarray(tpi, np.float32).reshape(B, 9).astype(np.float64), np.asarray(tv, np.float32).reshape(B, 3).astype(np.float64))


def mlp_step(blob, my, op, tpi, tv, hp, mode="f64", seed=0, mutation=None):
    """Gradient and losses of Connect4Net on one minibatch: dict(grads [30492], losses [2], raw [B][12], pre = [B][sum of hidden widths])."""
    acc = _Acc(mode, seed)
    my = np.ascontiguousarray(my, np.uint64).ravel(); op = np.ascontiguousarray(op, np.uint64).ravel()
    B = my.size
    tpi, tv = _targets(B, tpi, tv)
    layers = fc.mlp_views(np.ascontiguousarray(blob, np.float64))   # f32 parameters are exact in f64; a float64 chain's stay as they are
    A, pre = [fc.features_f64(my, op)], []
    for l, (W, b) in enumerate(layers):
        t = A[-1][:, None, :] * W[None, :, :]                                   # [B][O][K]
        z = acc.chain(t, start=np.broadcast_to(b[None, :], t.shape[:-1]))
        pre.append(z)
        A.append(np.maximum(z, 0.0) if l < 4 else z)
    raw = A[-1]
    losses, dz = _heads(raw, tpi, tv, hp, B, acc, mutation)
    g = [None] * 5
    for l in range(4, -1, -1):
        W, _ = layers[l]
        gW = acc.chain(dz.T[:, None, :] * A[l].T[None, :, :])                   # [O][K][B]
        gb = acc.chain(dz.T)
        g[l] = np.concatenate([gW.ravel(), gb])
        if l > 0:
            dA = acc.chain(dz[:, None, :] * W.T[None, :, :])                    # [B][K][O]
            dz = np.where(_gate(pre[l - 1], mutation), dA, 0.0)
    return dict(grads=np.concatenate(g), losses=losses, raw=raw, pre=np.concatenate(pre[:4], axis=1))


def conv_step(blob, my, op, tpi, tv, hp, mode="f64", seed=0, mutation=None):
    """The same for Connect4ConvNet: dict(grads [12412] in the blob's layout, losses [2], raw [B][12], pre [B][1008])."""
    acc = _Acc(mode, seed)
    my = np.ascontiguousarray(my, np.uint64).ravel(); op = np.ascontiguousarray(op, np.uint64).ravel()
    B = my.size
    tpi, tv = _targets(B, tpi, tv)
    cw, cb, hw, hb = fc.conv_views(np.ascontiguousarray(blob, np.float64))
    X = cbl.tap_bits(my, op)                                                    # [B][18][63]
    t = cw.reshape(16, 18)[None, :, None, :] * X.transpose(0, 2, 1)[:, None, :, :]   # [B][16][63][18]
    pre = acc.chain(t, start=np.broadcast_to(cb[None, :, None], t.shape[:-1])).reshape(B, fc.CONV_FLAT)
    act = np.maximum(pre, 0.0)
    t = hw[None, :, :] * act[:, None, :]                                        # [B][12][1008]
    raw = acc.chain(t, start=np.broadcast_to(hb[None, :], t.shape[:-1]))
    losses, dz = _heads(raw, tpi, tv, hp, B, acc, mutation)
    dWh = acc.chain(dz.T[:, None, :] * act.T[None, :, :])                       # [12][1008][B]
    dbh = acc.chain(dz.T)
    dY = np.where(_gate(pre, mutation), acc.chain(hw.T[None, :, :] * dz[:, None, :]), 0.0).reshape(B, 16, 63)
    ydc = dY.transpose(1, 0, 2)[:, None, :, :]                                  # [16][1][B][63]
    xdc = X.transpose(1, 0, 2)[None, :, :, :]                                   # [1][18][B][63]
    dWc = acc.chain((ydc * xdc).reshape(16, 18, B * 63))
    dbc = acc.chain(dY.transpose(1, 0, 2).reshape(16, B * 63))
    return dict(grads=np.concatenate([dWc.ravel(), dbc, dWh.ravel(), dbh]), losses=losses, raw=raw, pre=pre)


STEP = dict(mlp=mlp_step, conv=conv_step)


def adam_step(w, m, v, g, step, lr, hp, mode="f64", mutation=None):
    """torch::optim::Adam (amsgrad off) as oracle/train.hpp states it: g += wd p (only when wd != 0); m = b1 m + (1 - b1) g;
    v = b2 v + (1 - b2) g g; p -= (lr / (1 - b1^t)) m / (sqrt(v) / sqrt(1 - b2^t) + eps), the two bias corrections computed on the host
    in double and handed over as f32. Returns (w, m, v, step + 1)."""
    step += 1
    t = step + 1 if mutation == "bias_step_off_by_one" else step
    ft = np.float32 if mode == "f32" else np.float64
    b1, b2, eps, wd = (np.float64(np.float32(x)) for x in (BETA1, BETA2, EPS, hp["weight_decay"]))
    if mutation == "wd_when_zero" and wd == 0:
        wd = np.float64(np.float32(1e-6))
    if mutation == "wd_dropped":
        wd = np.float64(0)
    step_size = np.float64(np.float32(lr)) / (1.0 - b1 ** t)
    inv = 1.0 / np.sqrt(1.0 - b2 ** t)
    if mode == "f32":
        step_size, inv = np.float64(np.float32(step_size)), np.float64(np.float32(inv))
    w, m, v, g = (np.asarray(a, np.float64).astype(ft) for a in (w, m, v, g))
    b1, b2, eps, wd, step_size, inv, one = (ft(x) for x in (b1, b2, eps, wd, step_size, inv, 1.0))
    with np.errstate(under="ignore", over="ignore", invalid="ignore"):
        if wd != 0:
            g = g + wd * w
        m = b1 * m + (one - b1) * g
        v = b2 * v + ((one - b2) * g) * g
        w = w - step_size * (m / (np.sqrt(v) * inv + eps))
    return w.astype(np.float64), m.astype(np.float64), v.astype(np.float64), step


def run_steps(net, blob, bs, hp, lrs, mode="f64", seed=0, mutation=None):
    """len(lrs) optimiser steps from zero moments on the batches bs = (my, op, tpi, tv) [n][B]...: dict(weights, m, v, step, losses [n][2],
    grads = the last step's, grads0 / pre0 = the first step's gradient and pre-activations)."""
    w = np.ascontiguousarray(blob, np.float32).astype(np.float64)
    m, v, step = np.zeros_like(w), np.zeros_like(w), 0
    losses, first = [], None
    for s, lr in enumerate(lrs):
        r = STEP[net](w, bs[0][s], bs[1][s], bs[2][s], bs[3][s], hp, mode=mode, seed=seed * 100 + s, mutation=mutation)
        first = first or r
        losses.append(r["losses"])
        w, m, v, step = adam_step(w, m, v, r["grads"], step, lr, hp, mode=mode, mutation=mutation)
    return dict(weights=w, m=m, v=v, step=step, losses=np.stack(losses), grads=r["grads"], grads0=first["grads"], pre0=first["pre"])


# ---- bars -----------------------------------------------------------------------------------------------------------------------------
STATE_KEYS = ("grads", "weights", "m", "v")


def block_max(net, err):
    return OrderedDict((name, float(np.max(np.abs(err[sl]), initial=0.0))) for name, sl in BLOCKS[net].items())


@functools.lru_cache(maxsize=None)
def reference(net, member, variant, B, hyper, n_steps):
    """The float64 chain of one case and its floors: dict(f64 = run_steps(...), floor = {key: {block: float}}, loss_floor [n][2],
    gate_fragile = number of fragile units of the first step)."""
    blob = family(net)[member]
    bs, hp, lrs = batches(variant, B, n_steps), HYPERS[hyper], [LR] * n_steps
    f64 = run_steps(net, blob, bs, hp, lrs)
    floor = {k: OrderedDict.fromkeys(BLOCKS[net], 0.0) for k in STATE_KEYS}
    lfloor = np.zeros((n_steps, 2)); spread = np.zeros_like(f64["pre0"])
    for s in range(N_FLOOR_SEEDS):
        var = run_steps(net, blob, bs, hp, lrs, mode="f32", seed=1000 + s)
        for k in STATE_KEYS:
            for name, e in block_max(net, var[k] - f64[k]).items():
                floor[k][name] = max(floor[k][name], e)
        lfloor = np.maximum(lfloor, np.abs(var["losses"] - f64["losses"]))
        spread = np.maximum(spread, np.abs(var["pre0"] - f64["pre0"]))
    fragile = int(((spread > 0) & (np.abs(f64["pre0"]) <= spread)).sum())
    return dict(f64=f64, floor=floor, loss_floor=lfloor, gate_fragile=fragile)


def errors(net, ref, got):
    """{key: {block: max |got - f64|}} and the loss errors [n][2] of a state dict (weights, m, v, grads, losses) against reference()."""
    out = {k: block_max(net, np.asarray(got[k], np.float64) - ref["f64"][k]) for k in STATE_KEYS if k in got}
    return out, np.abs(np.asarray(got["losses"], np.float64) - ref["f64"]["losses"])


def check_bars(tag, net, ref, got):
    """Asserts max |got - f64| <= 8 x floor for every block of every state key in `got`, and for the losses. Returns the errors."""
    err, lerr = errors(net, ref, got)
    for k, blocks in err.items():
        for name, e in blocks.items():
            assert e <= MARGIN * ref["floor"][k][name], (tag, k, name, e, ref["floor"][k][name])
    assert (lerr <= MARGIN * ref["loss_floor"]).all(), (tag, "losses", lerr, ref["loss_floor"])
    return err, lerr


# ---- the oracle's steps, one by one -----------------------------------------------------------------------------------------------------
def oracle_gradients(oracle, net, w, hyper, b):
    hp = oracle_hyper(hyper) if isinstance(hyper, str) else hyper
    if net == "mlp":
        return oracle.train_gradients(w, hp, oracle.c4_features(b[0], b[1]), b[2], b[3])
    return oracle.convtrain_gradients(w, hp, b[0], b[1], b[2], b[3])


def oracle_steps(oracle, net, blob, bs, hyper, lrs, gradients=oracle_gradients, flush=False):
    """The oracle's steps from zero moments, gradients then train_adam: the list of dict(weights, m, v, step, grads, losses) after every
    step. flush = True is the mutation "subnormal g, m, v flushed to zero", built round oracle.train_adam."""
    hp = oracle_hyper(hyper)
    w = np.array(blob, np.float32); m, v, step = np.zeros_like(w), np.zeros_like(w), 0
    out = []
    for s, lr in enumerate(lrs):
        g, l = gradients(oracle, net, w, hyper, tuple(a[s] for a in bs))
        if flush:
            g = flush_subnormal(g)
        w, m, v, step = oracle.train_adam(w, hp, g, float(lr), m, v, step)
        if flush:
            m, v = flush_subnormal(m), flush_subnormal(v)
        out.append(dict(weights=w, m=m, v=v, step=step, grads=g, losses=l))
    return out


def final_state(history):
    """The last state of oracle_steps (or of a device run shaped like it) with the losses of every step stacked, as check_bars takes it."""
    return dict(history[-1], losses=np.stack([h["losses"] for h in history]))


# ---- the table of cases -----------------------------------------------------------------------------------------------------------------
class Case(tuple):
    """(net, member, variant, B, hyper, route, steps): `steps` optimiser steps at LR from zero moments; the float64 bars cover all of them."""
    __slots__ = ()
    net, member, variant, B, hyper, route, steps = (property(lambda self, i=i: self[i]) for i in range(7))

    @property
    def id(self):
        return "-".join(str(x) for x in self)

    @property
    def ref_key(self):
        return self.net, self.member, self.variant, self.B, self.hyper, self.steps


ROUTES = ("step", "dp", "epoch", "micro", "child")
EDGE_VARIANTS = ("zero_row", "subnormal_t")


def must_members(net):
    """The members every route runs with weight_decay = 0: trained, the subnormal ones, zero (and the gate-at-zero member)."""
    return ("trained",) + SUBNORMAL_MEMBERS[net] + ("zero", GATE_ZERO_MEMBERS[net])


def _cases():
    out = []
    hn = tuple(HYPERS)
    for net in NETS:
        bs = BATCH_SIZES[net]
        # step: every member once, variant / batch size / hyper-parameters cycling (`duplicates` at B = 32, the issue's case) ...
        for i, member in enumerate(family(net)):
            variant = VARIANTS[i % len(VARIANTS)]
            B = 32 if variant == "duplicates" else bs[i % len(bs)]
            if variant == "zero_row" and B == 1:   # the only row would be the zeroed one: dz = 0, every gradient, loss and moment exactly 0
                B = bs[(i + 1) % len(bs)]
            out.append(Case((net, member, variant, B, hn[i % 3], "step", 1)))
        # ... and, as on every route, the must-members with weight_decay = 0 on the two target edges (these cases are shared by the
        # step and the data-parallel route: one float64 reference each)
        for j, member in enumerate(must_members(net)):
            for route in ("step", "dp"):
                out.append(Case((net, member, EDGE_VARIANTS[j % 2], (33, 32)[j % 2] if net == "mlp" else (32, 17)[j % 2], "wd0", route, 1)))
        out.append(Case((net, "init", "recorded", 32, "weighted", "dp", 1)))
        # epoch: six steps through set_data + train_epoch at a batch the persistent kernel takes (<= 32), one above it for Connect4Net
        for j, member in enumerate(must_members(net)):
            out.append(Case((net, member, EDGE_VARIANTS[(j + 1) % 2], 32 if net == "mlp" or j % 2 == 0 else 17, "wd0", "epoch", EPOCH_STEPS)))
        out.append(Case((net, "init", "tsum_half", 33 if net == "mlp" else 17, "default", "epoch", EPOCH_STEPS)))
        # micro: 96 positions = 3 micro-batches, two steps, against tests/micro_batch_model.py's combination of the oracle's blocks
        for j, member in enumerate(must_members(net)):
            out.append(Case((net, member, EDGE_VARIANTS[j % 2], MICRO_B, "wd0", "micro", 2)))
        out.append(Case((net, "init", "onehot", MICRO_B, "weighted", "micro", 2)))
        # child: the persistent kernel's alternatives in a fresh process: three members, weight_decay = 0, the epoch route's cases
        for c in [c for c in out if c.net == net and c.route == "epoch" and c.member in ("trained", SUBNORMAL_MEMBERS[net][0], "zero")]:
            out.append(Case(c[:5] + ("child", EPOCH_STEPS)))
    return tuple(out)


CASES = _cases()
BARRED_ROUTES = ("step", "dp", "epoch", "child")   # micro mode is another definition of the gradient (the mean of per-32 means): no f64 bar


def cases(net=None, route=None):
    return [c for c in CASES if (net is None or c.net == net) and (route is None or c.route == route)]


def case_reference(c):
    return reference(*c.ref_key)


def case_batches(c):
    return batches(c.variant, c.B, c.steps)


# ---- the epoch route, shared by the GPU test, its child process and tools/learner_f32_family_profile.py ---------------------------------
def trainer_init(eng, c):
    (eng.trainer_init if c.net == "mlp" else eng.trainer_init_conv)(family(c.net)[c.member], **HYPERS[c.hyper])


def run_epoch(eng, c):
    """The case's steps on a synthesis_amd.Engine through train_set_data + train_epoch; the uploaded rows are shuffled and the permutation
    undoes it. Returns (trainer_state(), losses [steps][2])."""
    bs = case_batches(c)
    flat = [a.reshape((c.steps * c.B,) + a.shape[2:]) for a in bs]
    p = np.random.default_rng(c.B + c.steps).permutation(c.steps * c.B)
    perm = np.argsort(p).astype(np.int32)
    assert (perm.size == 1 or not np.array_equal(perm, np.arange(perm.size))) and all(np.array_equal(a[p][perm], a) for a in flat)
    trainer_init(eng, c)
    eng.train_set_data(*[a[p] for a in flat])
    losses = eng.train_epoch(perm, c.B, LR)
    return eng.trainer_state(), losses
