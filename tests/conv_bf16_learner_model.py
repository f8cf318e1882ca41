"""A float64 model of the bf16 Connect4ConvNet learner step with bf16-rounded operands, a small checkpoint / batch family, and the bars
the device's gradients are held to. TEST INFRASTRUCTURE ONLY; numpy, no GPU.

The model restates synthesis_amd/csrc/train_conv_mfma.cuh::conv_grad_step_bf16 (the four-workgroup epoch kernel's BF16 branches must
agree with it) and rounds exactly where the kernel does:

  conv    pre = cb + sum_taps bf16(cw) * bit            f32 conv bias as the start value; act = relu(pre), kept unrounded
  head    raw = hb + sum_i bf16(Wh) * bf16(act)
  H       log-softmax, KL and dz unrounded, sc = weight / B; a target entry <= 0 has no KL term; tsum multiplies the softmax
          (oracle/train.hpp)
  dWh     sum_b bf16(dz) * bf16(act)                    dbh = sum_b dz, unrounded
  dY      [act > 0] * sum_o bf16(Wh) * bf16(dz)
  dWc     sum_b sum_cells bf16(dY) * bit                dbc = sum bf16(dY)  (the all-ones tap of the matrix core: the ROUNDED dY)

`round` is bf16 round-to-nearest-even (synthesis_amd.weights.f32_to_bf16_bits), truncation (a mutation) or the identity; `accumulate`
is float64, or "f32": every chain summed in float32 in a seeded random order, act / raw / dz / dY rounded to f32 where the kernel keeps
them as f32 and the H phase in f32 — that variant exists only to measure the reference's own noise floor (bars()).

The bars (none is taken from a kernel's output), per gradient entry with n = 32 for dWh / dbh and 2,016 for dWc / dbc:
  derived    n * 2^-23 * sum|terms| + flips         2^-23: the matrix core may truncate when it aligns; flips = the bf16 ulps of the
                                                    fragile dY entries that feed the chain
  measured   max(8 * floor, derived)                floor = the largest |f32 random-order variant - float64 model| of the entry's
                                                    parameter block over 8 seeds
The exact-forward members (grid, grid_sharp) use the derived bar, every other member the measured one.
"""
import functools
import os
from collections import OrderedDict

import numpy as np

from synthesis_amd.weights import bf16_bits_to_f32, f32_to_bf16_bits
from tests.f16x2_checkpoints import CONV_C, CONV_FLAT, CONV_HW, CONV_OUT, CONV_W, GOLDEN, _bits, _p2, conv_views

NUM = CONV_W + CONV_C + CONV_OUT * CONV_FLAT + CONV_OUT
BLOCKS = OrderedDict((("conv_W", slice(0, CONV_W)), ("conv_b", slice(CONV_W, CONV_W + CONV_C)),
                      ("head_W", slice(CONV_W + CONV_C, NUM - CONV_OUT)), ("head_b", slice(NUM - CONV_OUT, NUM))))
CHAIN_N = dict(conv_W=2016, conv_b=2016, head_W=32, head_b=32)   # chain lengths of the derived bar (32 samples x 63 cells; 32 samples)
U23 = 2.0 ** -23
MEMBERS = ("init", "trained", "grid", "grid_sharp", "dead", "head_x2^-12", "conv_x2^6")
EXACT_FORWARD = ("grid", "grid_sharp")
BATCHES = (1, 2, 15, 16, 17, 31, 32)
WEIGHTED = (17, 32)                # the batch sizes run with policy_weight = 0.7, value_weight = 1.9
DEAD_CHANNELS = (1, 6, 11, 15)
N_FLOOR_SEEDS = 8
MUTATIONS = ("trunc", "dz_unrounded_dWh", "dY_unrounded_dbc", "act_rounded_before_gate", "drop_edge_tap", "pad_rows", "tsum_one")


# ---- rounding -------------------------------------------------------------------------------------------------------------------------
def round_bf16(x):
    return bf16_bits_to_f32(f32_to_bf16_bits(np.asarray(x, np.float64).astype(np.float32))).astype(np.float64).reshape(np.shape(x))


def trunc_bf16(x):
    u = np.asarray(x, np.float64).astype(np.float32).view(np.uint32) & np.uint32(0xFFFF0000)
    return u.view(np.float32).astype(np.float64).reshape(np.shape(x))


def identity(x):
    return np.asarray(x, np.float64)


ROUND = {"bf16": round_bf16, "trunc": trunc_bf16, "identity": identity}


def bf16_ulp(x):
    """The spacing of bf16 numbers at |x| (normal range; 0 for x = 0)."""
    _, e = np.frexp(np.abs(np.asarray(x, np.float64)))
    return np.where(np.asarray(x) != 0, np.ldexp(1.0, e - 8), 0.0)


def boundary_distance(x):
    """Distance of |x| to the nearest bf16 rounding boundary (the midpoint of two neighbouring bf16 numbers); inf for x = 0."""
    a = np.abs(np.asarray(x, np.float64))
    ulp = bf16_ulp(a)
    with np.errstate(divide="ignore", invalid="ignore"):
        lo = np.floor(a / ulp) * ulp
        return np.where(a != 0, np.abs(a - lo - 0.5 * ulp), np.inf)


# ---- the step -------------------------------------------------------------------------------------------------------------------------
def tap_bits(my, op):
    """[n][18 taps = plane * 9 + k1 * 3 + k2][63 cells = row * 9 + col]: the input of each tap at each cell (0 outside the board)."""
    x = np.stack([_bits(my), _bits(op)], axis=1).astype(np.float64)
    xp = np.pad(x, ((0, 0), (0, 0), (1, 1), (1, 1)))
    out = np.zeros((len(x), 18, 7, 9))
    for ci in range(2):
        for k1 in range(3):
            for k2 in range(3):
                out[:, ci * 9 + k1 * 3 + k2] = xp[:, ci, k1:k1 + 7, k2:k2 + 9]
    return out.reshape(len(x), 18, CONV_HW)


class _Acc:
    """Sums chains along the last axis: float64, or float32 in a seeded random order (one order per call)."""

    def __init__(self, mode, seed):
        assert mode in ("f64", "f32")
        self.f32 = mode == "f32"
        self.rs = np.random.RandomState(seed)

    def chain(self, terms, start=None):
        if not self.f32:
            s = terms.sum(axis=-1)
            return s if start is None else s + start
        t = terms.astype(np.float32)[..., self.rs.permutation(terms.shape[-1])]
        if start is not None:
            t = np.concatenate([np.broadcast_to(np.asarray(start, np.float32)[..., None], t.shape[:-1] + (1,)), t], axis=-1)
        return np.cumsum(t, axis=-1, dtype=np.float32)[..., -1].astype(np.float64)


def _heads(raw, tgt, weight, B, f32, tsum_one):
    """One head group (policy: 9 entries, outcome: 3): (kl [n], dz [n][k], p * tsum, lse) as oracle/train.hpp computes them."""
    ft = np.float32 if f32 else np.float64
    x = raw.astype(ft); t = tgt.astype(ft)
    sc = (np.float32(weight) * (np.float32(1) / np.float32(B))) if f32 else np.float64(np.float32(weight)) / B
    mx = x.max(axis=1, keepdims=True)
    lse = mx + np.log(np.exp(x - mx).sum(axis=1, keepdims=True, dtype=ft))
    logp = x - lse
    tsum = np.ones_like(mx) if tsum_one else t.sum(axis=1, keepdims=True, dtype=ft)
    with np.errstate(divide="ignore", invalid="ignore"):
        term = np.where(t > 0, t * (np.log(np.where(t > 0, t, 1)) - logp), ft(0))
    pt = np.exp(x - lse) * tsum
    dz = sc * (pt - t)
    return (term.sum(axis=1, dtype=ft).astype(np.float64), dz.astype(np.float64), np.float64(sc) * np.abs(pt).astype(np.float64),
            np.abs(lse).astype(np.float64) + np.abs(logp).astype(np.float64))


def conv_bf16_step(blob, my_bb, op_bb, tpi, tv, policy_weight=1.0, value_weight=1.0, round="bf16", accumulate="f64", seed=0,
                   mutation=None, exact_forward=False):
    """One learner step. Returns a dict: grads [12412] (the blob's layout) and losses [2] in float64; the intermediates act [B][1008],
    pre, raw [B][12], dz [B][12], dY [B][1008]; sumabs [12412] = sum|terms| of every gradient chain; flips [12412] = the bf16 ulps of the
    fragile dY entries feeding each chain; fragile = dict of boolean masks (act, gate, dz, dY)."""
    assert mutation is None or mutation in MUTATIONS
    R = ROUND["trunc" if mutation == "trunc" else round]
    acc = _Acc("f32" if accumulate == "f32" else "f64", seed)
    f32 = acc.f32
    my = np.ascontiguousarray(my_bb, np.uint64).ravel(); op = np.ascontiguousarray(op_bb, np.uint64).ravel()
    B = my.size
    tpi = np.asarray(tpi, np.float32).reshape(B, 9).astype(np.float64); tv = np.asarray(tv, np.float32).reshape(B, 3).astype(np.float64)
    if mutation == "pad_rows":   # rows >= B of the 32-sample tile treated as live: empty boards with a uniform target
        my = np.concatenate([my, np.zeros(32 - B, np.uint64)]); op = np.concatenate([op, np.zeros(32 - B, np.uint64)])
        tpi = np.concatenate([tpi, np.full((32 - B, 9), np.float64(np.float32(1 / 9)))])
        tv = np.concatenate([tv, np.full((32 - B, 3), np.float64(np.float32(1 / 3)))])
    n = my.size
    cw, cb, hw, hb = conv_views(np.ascontiguousarray(blob, np.float32).astype(np.float64))
    X = tap_bits(my, op)                                                       # [n][18][63]
    if mutation == "drop_edge_tap":   # the tap that reads the row below is lost for the cells of the top row
        X[:, [0 * 9 + 0 * 3 + 1, 1 * 9 + 0 * 3 + 1], 6 * 9:7 * 9] = 0.0
    rcw = R(cw.reshape(CONV_C, 18))
    # conv + ReLU
    t = rcw[None, :, None, :] * X.transpose(0, 2, 1)[:, None, :, :]            # [n][16][63][18]
    pre = acc.chain(t, start=np.broadcast_to(cb[None, :, None], t.shape[:-1]))
    pre_sumabs = np.abs(t).sum(axis=-1) + np.abs(cb)[None, :, None]
    act = np.maximum(pre, 0.0).reshape(n, CONV_FLAT)
    ract = R(act)
    gate = (ract if mutation == "act_rounded_before_gate" else act) > 0
    if mutation == "act_rounded_before_gate":
        act = ract
    rhw = R(hw)
    # head
    t = rhw[None, :, :] * ract[:, None, :]                                     # [n][12][1008]
    raw = acc.chain(t, start=np.broadcast_to(hb[None, :], t.shape[:-1]))
    raw_sumabs = np.abs(t).sum(axis=-1) + np.abs(hb)[None, :]
    # H
    one = mutation == "tsum_one"
    klp, dzp, ptp, lp = _heads(raw[:, :9], tpi, policy_weight, B, f32, one)
    klv, dzv, ptv, lv = _heads(raw[:, 9:], tv, value_weight, B, f32, one)
    dz = np.concatenate([dzp, dzv], axis=1)                                     # [n][12]
    kl = np.stack([klp, klv], axis=1)[:B]
    if f32:
        losses = (np.float32(1) / np.float32(B)) * np.cumsum(kl.astype(np.float32), axis=0, dtype=np.float32)[-1]
        losses = losses.astype(np.float64)
    else:
        losses = kl.sum(axis=0) / B
    loss_sumabs = np.abs(kl).sum(axis=0) / B
    # what an f32 H phase can move dz by: the exponent's argument carries the rounding of lse and of x - lse, the exponential, the
    # products and the subtraction a few more roundings
    pt = np.concatenate([ptp, ptv], axis=1); labs = np.concatenate([lp, lv], axis=1)
    tg = np.concatenate([tpi * np.float64(np.float32(policy_weight)), tv * np.float64(np.float32(value_weight))], axis=1) / B
    dz_unc = np.maximum(2.0 ** -20 * np.abs(dz), 2.0 ** -24 * ((2.0 * labs + 8.0) * pt + 4.0 * np.abs(dz) + 2.0 * tg))
    rdz = R(dz)
    # head gradients
    t = (dz if mutation == "dz_unrounded_dWh" else rdz).T[:, None, :] * ract.T[None, :, :]   # [12][1008][n]
    dWh = acc.chain(t); dWh_sumabs = np.abs(t).sum(axis=-1)
    dbh = acc.chain(dz.T); dbh_sumabs = np.abs(dz.T).sum(axis=-1)
    # activation gradients
    t = rhw.T[None, :, :] * rdz[:, None, :]                                    # [n][1008][12]
    dY = np.where(gate, acc.chain(t), 0.0)
    dY_sumabs = np.where(gate, np.abs(t).sum(axis=-1), 0.0)
    rdY = R(dY).reshape(n, CONV_C, CONV_HW)
    # conv gradients
    ydc = rdY.transpose(1, 0, 2)[:, None, :, :]                                # [16][1][n][63]
    xdc = X.transpose(1, 0, 2)[None, :, :, :]                                  # [1][18][n][63]
    t = (ydc * xdc).reshape(CONV_C, 18, n * CONV_HW)
    dWc = acc.chain(t); dWc_sumabs = np.abs(t).sum(axis=-1)
    yb = (dY.reshape(n, CONV_C, CONV_HW) if mutation == "dY_unrounded_dbc" else rdY).transpose(1, 0, 2).reshape(CONV_C, n * CONV_HW)
    dbc = acc.chain(yb); dbc_sumabs = np.abs(yb).sum(axis=-1)
    # fragile operands
    fr_dY = (boundary_distance(dY) <= 12 * U23 * dY_sumabs) & (dY != 0)
    fr_dz = boundary_distance(dz) <= dz_unc
    if exact_forward:
        fr_act = np.zeros_like(gate); fr_gate = np.zeros_like(gate)
    else:
        bound = (18 * U23 * pre_sumabs).reshape(n, CONV_FLAT)
        fr_act = (boundary_distance(act) <= bound) & (act != 0)
        fr_gate = (np.abs(pre.reshape(n, CONV_FLAT)) <= bound) & (pre.reshape(n, CONV_FLAT) != 0)
    fu = np.where(fr_dY, bf16_ulp(dY), 0.0).reshape(n, CONV_C, CONV_HW).transpose(1, 0, 2)[:, None, :, :]
    flips = np.zeros(NUM)
    flips[BLOCKS["conv_W"]] = (fu * xdc).reshape(CONV_C, 18, -1).sum(axis=-1).ravel()
    flips[BLOCKS["conv_b"]] = fu.reshape(CONV_C, -1).sum(axis=-1)
    return dict(grads=np.concatenate([dWc.ravel(), dbc, dWh.ravel(), dbh]), losses=losses,
                sumabs=np.concatenate([dWc_sumabs.ravel(), dbc_sumabs, dWh_sumabs.ravel(), dbh_sumabs]), loss_sumabs=loss_sumabs,
                flips=flips, act=act, pre=pre.reshape(n, CONV_FLAT), raw=raw, raw_sumabs=raw_sumabs, dz=dz, dY=dY,
                fragile=dict(act=fr_act, gate=fr_gate, dz=fr_dz, dY=fr_dY))


def derived_bar(model):
    """[12412]: n * 2^-23 * sum|terms| + flips."""
    bar = model["flips"].copy()
    for name, sl in BLOCKS.items():
        bar[sl] += CHAIN_N[name] * U23 * model["sumabs"][sl]
    return bar


def measured_bars(blob, my, op, tpi, tv, pw, vw, model=None, seeds=N_FLOOR_SEEDS):
    """The bars of one case at arbitrary weights: dict(model, floor {block: float}, effect {block: float}, degenerate {block: bool},
    loss_floor [2], bar [12412], loss_bar [2]). effect = max |model(round = bf16) - model(round = identity)| of the block; a block is
    degenerate when that effect is not above 20 x its largest derived term (f32 accumulation alone hides the rounding there, whatever the
    order): such a block is held to the derived bar, every other one to max(8 x floor, derived)."""
    model = model or conv_bf16_step(blob, my, op, tpi, tv, pw, vw)
    floor = dict.fromkeys(BLOCKS, 0.0); lfloor = np.zeros(2)
    for s in range(seeds):
        v = conv_bf16_step(blob, my, op, tpi, tv, pw, vw, accumulate="f32", seed=1000 + s)
        d = np.abs(v["grads"] - model["grads"])
        for name, sl in BLOCKS.items():
            floor[name] = max(floor[name], float(d[sl].max()))
        lfloor = np.maximum(lfloor, np.abs(v["losses"] - model["losses"]))
    ident = conv_bf16_step(blob, my, op, tpi, tv, pw, vw, round="identity")
    effect = block_maxima(model["grads"] - ident["grads"])
    bar = derived_bar(model)
    degenerate = {name: bool(effect[name] <= 20 * bar[sl].max()) for name, sl in BLOCKS.items()}
    for name, sl in BLOCKS.items():
        if not degenerate[name]:
            bar[sl] = np.maximum(bar[sl], 8.0 * floor[name])
    return dict(model=model, floor=floor, effect=effect, degenerate=degenerate, loss_floor=lfloor, bar=bar,
                loss_effect=np.abs(model["losses"] - ident["losses"]),
                loss_bar=np.maximum(8.0 * lfloor, 32 * U23 * model["loss_sumabs"]))


def bar_means_something(c):
    """3b's condition on a measured_bars() result: in every block that is not degenerate, 8 x floor <= 1/20 of the bf16 effect."""
    return all(c["degenerate"][name] or 8 * c["floor"][name] <= c["effect"][name] / 20 for name in BLOCKS)


# ---- checkpoints ----------------------------------------------------------------------------------------------------------------------
def _grid(seed, conv_steps, head_steps):
    """An exact-forward member: conv weights / biases multiples of 1/8 up to conv_steps / 8, head weights ODD multiples of 1/64 up to
    head_steps / 64 (odd: a product with an 8-bit dz then has many bits, so an exact sum sitting exactly on a bf16 rounding boundary is
    rare), head biases multiples of 2^-9: every activation is a multiple of 1/8 below 32 (a bf16 number), every head product a multiple
    of 2^-9, and every partial sum of a logit stays below 2^11 (test_conv_bf16_learner_model.py asserts it): at most 20 bits."""
    rs = np.random.RandomState(seed)
    w = np.zeros(NUM, np.float32)
    cw, cb, hw, hb = conv_views(w)
    cw[:] = rs.randint(-conv_steps, conv_steps + 1, cw.shape) / 8.0
    cb[:] = rs.randint(-conv_steps, conv_steps + 1, cb.shape) / 8.0
    hw[:] = (rs.randint(-head_steps, head_steps + 1, hw.shape) | 1) / 64.0
    hb[:] = rs.randint(-256, 257, hb.shape) / 512.0
    return w


# (seed, conv_steps, head_steps) of the exact-forward members (the first weight seeds with which every batch size finds a batch seed),
# and the batch seeds that are not 0 (find_batch_seeds; test_conv_bf16_learner_model.py asserts the conditions they were chosen for)
GRID_SEEDS = dict(grid=(15, 1, 63), grid_sharp=(14, 4, 127))
BATCH_SEEDS = {("grid", 17): 1, ("grid_sharp", 2): 1, ("grid_sharp", 15): 1, ("grid_sharp", 17): 4, ("grid_sharp", 31): 2,
               ("dead", 32): 1}   # find_batch_seeds()


@functools.lru_cache(maxsize=None)
def family():
    from bench import make_conv_weights

    init = make_conv_weights(20260101)
    fam = OrderedDict()
    fam["init"] = init.copy()
    fam["trained"] = np.load(os.path.join(GOLDEN, "c4conv_trained_f32.npy")).astype(np.float32)
    for name, args in GRID_SEEDS.items():
        fam[name] = _grid(*args)
    w = init.copy(); conv_views(w)[1][list(DEAD_CHANNELS)] = np.float32(-40)
    fam["dead"] = w
    w = init.copy(); conv_views(w)[2][:] *= _p2(-12)
    fam["head_x2^-12"] = w
    w = init.copy(); cw, cb, _, _ = conv_views(w); cw *= _p2(6); cb *= _p2(6)
    fam["conv_x2^6"] = w
    assert tuple(fam) == MEMBERS and all(v.dtype == np.float32 and v.size == NUM for v in fam.values())
    return fam


# ---- batches --------------------------------------------------------------------------------------------------------------------------
def mirror_bb(bb):
    """The board mirrored left to right (column c -> 8 - c; bit = row + 7 col)."""
    bb = np.asarray(bb, np.uint64)
    out = np.zeros_like(bb)
    for c in range(9):
        out |= ((bb >> np.uint64(7 * c)) & np.uint64(0x7F)) << np.uint64(7 * (8 - c))
    return out


@functools.lru_cache(maxsize=None)
def pool():
    """The 256 golden positions followed by the hand-made rows: (my, op, tpi, tv, names of the hand-made rows -> index)."""
    g = np.load(os.path.join(GOLDEN, "conv_train_torch_goldens.npz"))
    my = list(g["my_bb"].reshape(-1)); op = list(g["op_bb"].reshape(-1))
    tpi = list(g["target_pi"].reshape(-1, 9)); tv = list(g["target_v"].reshape(-1, 3))
    names = {}

    def add(name, m, o, p, v):
        names[name] = len(my)
        my.append(np.uint64(m)); op.append(np.uint64(o)); tpi.append(np.asarray(p, np.float32)); tv.append(np.asarray(v, np.float32))

    add("empty", 0, 0, [0.02, 0.04, 0.08, 0.16, 0.4, 0.16, 0.08, 0.04, 0.02], [0.25, 0.5, 0.25])
    # column 4 full (alternating stones), stones in all four corners incl. the top row (bits 6 and 62); the full column's move is
    # illegal (zero target entries, and two more), the outcome target is one-hot
    col = [28 + r for r in range(7)]
    m = sum(1 << b for b in col[0::2]) | (1 << 0) | (1 << 62)
    o = sum(1 << b for b in col[1::2]) | (1 << 6) | (1 << 56)
    add("full_column_corners", m, o, [0.3, 0.2, 0.0, 0.1, 0.0, 0.15, 0.0, 0.05, 0.2], [0.0, 1.0, 0.0])
    # (the mirrored pair — a golden position and its mirror image with the mirrored policy target — is made per batch: batch())
    # policy targets that do not sum to 1: by one ulp (mirror-averaged rows drift like that), and by a tenth
    p = np.asarray(tpi[5], np.float32).copy(); p[np.argmax(p)] = np.nextafter(p[np.argmax(p)], np.float32(2))
    add("ulp_drift", my[5], op[5], p, tv[5])
    add("short_sum", my[9], op[9], np.asarray(tpi[9], np.float32) * np.float32(0.9), tv[9])
    return (np.array(my, np.uint64), np.array(op, np.uint64), np.stack(tpi).astype(np.float32), np.stack(tv).astype(np.float32), names)


MIRROR_ROW = -1   # batch_indices' marker of "the mirror image of the row before"


def batch_indices(B, seed=0):
    """Pool rows of the batch of size B: B = 1 the empty board, B = 2 a golden position and its mirror image, larger batches the
    hand-made rows at the tile edges (rows 0, 1, 15 / 16 — a mirrored pair across the two 16-sample tiles where B allows —, B - 2,
    B - 1) and seeded golden positions elsewhere."""
    names = pool()[4]
    rs = np.random.RandomState(100 * B + seed)
    if B == 1:
        return np.array([names["empty"]])
    idx = rs.choice(256, B, replace=False)
    my, op = pool()[:2]
    lopsided = [k for k in rs.permutation(256) if mirror_bb(my[k]) != my[k] or mirror_bb(op[k]) != op[k]]
    if B == 2:
        return np.array([lopsided[0], MIRROR_ROW])
    idx[0] = names["empty"]; idx[1] = names["full_column_corners"]
    at = 16 if B >= 19 else 8
    idx[at - 1] = lopsided[0]; idx[at] = MIRROR_ROW
    idx[B - 2] = names["ulp_drift"]; idx[B - 1] = names["short_sum"]
    return idx


def batch(B, seed=0):
    my, op, tpi, tv, _ = pool()
    i = batch_indices(B, seed)
    my, op, tpi, tv = my[i], op[i], tpi[i].copy(), tv[i].copy()
    for r in np.flatnonzero(i == MIRROR_ROW):
        my[r] = mirror_bb(my[r - 1]); op[r] = mirror_bb(op[r - 1]); tpi[r] = tpi[r - 1][::-1]; tv[r] = tv[r - 1]
    return my, op, tpi, tv


def loss_weights(B):
    return (0.7, 1.9) if B in WEIGHTED else (1.0, 1.0)


# ---- the bars of the family's cases ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case(member, B):
    """The float64 model of (member, B) and its bars: dict(blob, batch, pw, vw, model, bar [12412], loss_bar [2] or None (exact-forward:
    the oracle's bits), floor, loss_floor)."""
    blob = family()[member]
    my, op, tpi, tv = batch(B, BATCH_SEEDS.get((member, B), 0))
    pw, vw = loss_weights(B)
    out = dict(blob=blob, batch=(my, op, tpi, tv), pw=pw, vw=vw)
    if member in EXACT_FORWARD:
        model = conv_bf16_step(blob, my, op, tpi, tv, pw, vw, exact_forward=True)
        out.update(model=model, bar=derived_bar(model), loss_bar=None, floor=None, loss_floor=None)
    else:
        out.update(measured_bars(blob, my, op, tpi, tv, pw, vw))
    return out


def find_batch_seeds(tries=40):
    """How BATCH_SEEDS was made: per case the first batch seed whose MODEL meets the case's conditions — exact-forward members: no
    fragile dz and fragile dY entries under 0.8 % of the nonzero ones; every other member: bar_means_something. Nothing here looks at a
    kernel. (B = 1 is the empty board whatever the seed.)"""
    out = {}
    for member in MEMBERS:
        for B in BATCHES:
            for seed in range(1 if B == 1 else tries):
                my, op, tpi, tv = batch(B, seed)
                pw, vw = loss_weights(B)
                if member in EXACT_FORWARD:
                    m = conv_bf16_step(family()[member], my, op, tpi, tv, pw, vw, exact_forward=True)
                    ok = not m["fragile"]["dz"].any() and m["fragile"]["dY"].sum() <= 0.008 * (m["dY"] != 0).sum()
                else:
                    ok = bar_means_something(measured_bars(family()[member], my, op, tpi, tv, pw, vw))
                if ok:
                    break
            else:
                raise AssertionError((member, B))
            if seed:
                out[(member, B)] = seed
    return out


def block_maxima(err):
    return {name: float(np.abs(err[sl]).max()) for name, sl in BLOCKS.items()}


def check_device(tag, c, grads, losses, oracle_grads=None, oracle_losses=None, exact_forward=False):
    """Asserts one device result against a case()-shaped dict and returns the observed maxima per block (and of the losses).
    Exact-forward cases also take the oracle's gradients and losses: the 12 dbh entries and the losses are its bits."""
    g = np.asarray(grads, np.float32)
    err = np.abs(g.astype(np.float64) - c["model"]["grads"])
    obs = block_maxima(err)
    obs["loss"] = float(np.abs(np.asarray(losses, np.float64) - c["model"]["losses"]).max())
    worst = {name: float((err[sl] / np.maximum(c["bar"][sl], 1e-300)).max()) for name, sl in BLOCKS.items()}
    if c["loss_bar"] is not None:
        worst["loss"] = float((np.abs(np.asarray(losses, np.float64) - c["model"]["losses"]) / np.maximum(c["loss_bar"], 1e-300)).max())
    print(f"{tag}: max |device - model| " + "  ".join(f"{k} {v:.3e} (" + (f"{worst[k]:.3f} of its bar" if k in worst else "held to the oracle's bits") + ")"
                                                      for k, v in obs.items()))
    assert np.isfinite(g).all(), tag
    if exact_forward:
        hbs = BLOCKS["head_b"]
        assert np.array_equal(g[hbs].view(np.uint32), np.asarray(oracle_grads, np.float32)[hbs].view(np.uint32)), (tag, "dbh bits")
        assert np.array_equal(np.asarray(losses, np.float32).view(np.uint32), np.asarray(oracle_losses, np.float32).view(np.uint32)), (tag, "loss bits")
        sel = np.ones(NUM, bool); sel[hbs] = False
        assert (err[sel] <= c["bar"][sel]).all(), (tag, worst)
    else:
        assert (err <= c["bar"]).all(), (tag, worst)
        assert (np.abs(np.asarray(losses, np.float64) - c["model"]["losses"]) <= c["loss_bar"]).all(), (tag, obs["loss"], c["loss_bar"])
    return obs


def exact_zero_entries(member):
    """Gradient entries that must be exact zeros for `member` (dead: the dead channels' dWc / dbc rows and dWh columns)."""
    z = np.zeros(NUM, bool)
    if member == "dead":
        zw, zb, zh, _ = conv_views(z)
        for ch in DEAD_CHANNELS:
            zw[ch] = True; zb[ch] = True; zh[:, ch * CONV_HW:(ch + 1) * CONV_HW] = True
    return z


def report():
    """The floors and bars of every case, as text (profiles/conv_bf16_learner_bars.txt is this plus the device maxima of a GPU run)."""
    lines = ["member B | per block: floor (largest |f32 random-order variant - float64 model| over 8 seeds), bf16 effect (largest |model(bf16) - "
             "model(identity)|), largest bar in the block; 'derived' = held to n * 2^-23 * sum|terms| + flips only"]
    for member in MEMBERS:
        for B in BATCHES:
            c = case(member, B)
            m = c["model"]
            cells = []
            for name, sl in BLOCKS.items():
                if c["floor"] is None:
                    cells.append(f"{name}: derived, bar <= {c['bar'][sl].max():.3e}")
                else:
                    kind = "derived" if c["degenerate"][name] else "measured"
                    cells.append(f"{name}: floor {c['floor'][name]:.3e} effect {c['effect'][name]:.3e} {kind}, bar <= {c['bar'][sl].max():.3e}")
            loss = "losses: the oracle's bits" if c["loss_bar"] is None else f"losses: floor {c['loss_floor'].max():.3e} bar {c['loss_bar'].max():.3e}"
            fr = m["fragile"]
            lines.append(f"{member} B={B} | " + " | ".join(cells) + f" | {loss} | fragile act {int(fr['act'].sum())} gate {int(fr['gate'].sum())} "
                         f"dz {int(fr['dz'].sum())} dY {int(fr['dY'].sum())} of {int((m['dY'] != 0).sum())}")
    return "\n".join(lines)


if __name__ == "__main__":
    print(report())
