"""The model of the micro-batch learner step (SYN_TRAIN_BATCH_MICRO, include/synthesis_amd.h), built only from pieces the oracle pins:

    a minibatch of B = 32 nb samples, in the order given, is nb micro-batches of 32;
    g_j, l_j = the oracle's gradients / losses of micro-batch j as a minibatch of its own (tests/oracle_lib.py train_gradients for
               Connect4Net, convtrain_gradients for Connect4ConvNet: batch mean 1/32, the oracle's chains);
    acc = g_0, then acc = acc + g_j in ascending j (numpy float32 additions; nothing is added to g_0);
    G = acc * inv with inv = float32(1) / float32(nb) (one IEEE division, one multiplication); the two losses alike;
    Adam = oracle.train_adam on G.

Data: positions and targets of a short oracle self-play (a pool of a few hundred recorded positions; batches index into it), with one
all-zero policy target row and one one-hot row planted in the pool. Hyper-parameters are the non-default ones of the existing training
tests."""
import os

import numpy as np

BLOCK = 32
HYPER = dict(weight_decay=1e-3, policy_weight=0.7, value_weight=1.9)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ZERO_ROW, ONE_HOT_ROW = 3, 40   # pool rows with an all-zero / a one-hot policy target (micro-batches 0 and 1 of an identity batch)


def hyper():
    from tests.oracle_lib import default_train_hyper

    return default_train_hyper(**HYPER)


def blob_of(net):
    if net == "mlp":
        return np.load(os.path.join(ROOT, "tests", "golden", "c4net_blob_f32.npy"))
    from bench import make_conv_weights

    return make_conv_weights(20260101)


_POOL = {}


def pool(oracle):
    """dict(my, op, tpi, tv, X): the recorded positions of 24 oracle self-play games at 16 explores (computed once per process)."""
    if "p" not in _POOL:
        from tests.oracle_lib import parity_rollout_config

        r = oracle.c4_selfplay(parity_rollout_config(16), blob_of("mlp"), 77, 24, threads=4, nn_mode=oracle.ACC_FMA)
        keep = np.arange(63)[None, :] < r["plies"][:, None]
        my = np.ascontiguousarray(r["states_bb"][..., 0][keep]); op = np.ascontiguousarray(r["states_bb"][..., 1][keep])
        tpi = np.ascontiguousarray(r["pis"][keep]); tv = np.ascontiguousarray(r["vs"][keep])
        assert my.size >= 128
        tpi[ZERO_ROW] = 0.0
        tpi[ONE_HOT_ROW] = 0.0
        tpi[ONE_HOT_ROW, 4] = 1.0
        for a in (my, op, tpi, tv):
            a.setflags(write=False)
        _POOL["p"] = dict(my=my, op=op, tpi=tpi, tv=tv, X=oracle.c4_features(my, op))
    return _POOL["p"]


def batch_indices(oracle, n, seed):
    """n pool rows for a batch: the identity on the first 64 rows (so that the planted rows are in micro-batches 0 and 1), then draws."""
    size = pool(oracle)["my"].size
    idx = np.random.default_rng(seed).integers(0, size, size=n).astype(np.int32)
    idx[: min(n, 64)] = np.arange(min(n, 64))
    return idx


def block_gradients(oracle, net, blob, idx):
    """(g, losses) of the 32 samples pool[idx] as a minibatch of their own: the oracle's chained step."""
    p = pool(oracle)
    assert len(idx) == BLOCK
    if net == "mlp":
        return oracle.train_gradients(blob, hyper(), p["X"][idx], p["tpi"][idx], p["tv"][idx])
    return oracle.convtrain_gradients(blob, hyper(), p["my"][idx], p["op"][idx], p["tpi"][idx], p["tv"][idx])


def combine(parts):
    """acc = parts[0]; acc = acc + parts[j] ascending; acc * (1 / nb) — all in float32."""
    acc = np.array(parts[0], np.float32).copy()
    for g in parts[1:]:
        acc = acc + np.asarray(g, np.float32)
    inv = np.float32(1.0) / np.float32(len(parts))
    out = acc * inv
    assert out.dtype == np.float32
    return out


def gradients(oracle, net, blob, idx):
    """The model's (G, losses) of the minibatch pool[idx], len(idx) = 32 nb."""
    assert len(idx) % BLOCK == 0 and len(idx) >= BLOCK
    parts = [block_gradients(oracle, net, blob, idx[o:o + BLOCK]) for o in range(0, len(idx), BLOCK)]
    return combine([g for g, _ in parts]), combine([l for _, l in parts])


def chained_gradients(oracle, net, blob, idx):
    """The oracle's chained gradient of the same samples (one chain over all of them)."""
    p = pool(oracle)
    if net == "mlp":
        return oracle.train_gradients(blob, hyper(), p["X"][idx], p["tpi"][idx], p["tv"][idx])
    return oracle.convtrain_gradients(blob, hyper(), p["my"][idx], p["op"][idx], p["tpi"][idx], p["tv"][idx])


def steps(oracle, net, blob, idx_steps, lrs):
    """Whole optimiser steps from zero moments: dict(weights, m, v, step, losses[n][2], grads = the last step's G, history = the
    (weights, m, v) after every step)."""
    w = np.array(blob, np.float32).copy()
    m, v, step = np.zeros_like(w), np.zeros_like(w), 0
    losses, hist, G = [], [], None
    for idx, lr in zip(idx_steps, lrs):
        G, l = gradients(oracle, net, w, idx)
        w, m, v, step = oracle.train_adam(w, hyper(), G, float(lr), m, v, step)
        losses.append(l)
        hist.append((w.copy(), m.copy(), v.copy()))
    return dict(weights=w, m=m, v=v, step=step, losses=np.stack(losses), grads=G, history=hist)


# Connect4Net's parameter blocks (l_k.weight[O][I], l_k.bias[O], k = 1..5: study-connect4/src/policies.rs:20-24)
MLP_DIMS = (63, 128, 96, 64, 48, 12)


def mlp_param_blocks():
    out, o = [], 0
    for k, n in zip(MLP_DIMS[:-1], MLP_DIMS[1:]):
        out.append(slice(o, o + k * n)); o += k * n
        out.append(slice(o, o + n)); o += n
    assert o == 30492
    return out
