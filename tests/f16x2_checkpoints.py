"""A family of stress checkpoints for the f16x2 network arithmetic (SYN_NET_ARITH_F16X2) and a plain float64 reference of both networks.
TEST INFRASTRUCTURE ONLY; no GPU, no files other than the four committed parameter fixtures.

The four fixtures keep the f16x2 plan (synthesis_amd/csrc/f16x2_tile.cuh build_f16x2_image, conv_f16x2_tile.cuh build_conv_f16x2_image)
in its comfortable middle. The members below push it to the branches a checkpoint drifting during training reaches: the activation
exponent capped at 24 (activations far below 2^15, `lo` halves in the f16 subnormals), the weight exponent capped at 40 or 0 for an
all-zero layer, negative activation and rescale exponents (the rescale multiplies by 2^-k), one outlier weight per layer (every other
weight's `lo` half becomes subnormal), dead layers, and the edges of the window |s + t| <= 60 outside which a load is refused.
Every scaling is by an exact power of two in f32.

mlp_f64 / conv_f64 are the two networks in numpy float64, written from the definitions in include/synthesis_amd.h (syn_load_weights,
syn_load_weights_conv) and the feature map of oracle.c4_features (tests/test_oracle_f16x2.py checks features_f64 against it): the
yardstick the bars of check_f64_bars are stated against. They share no code with the engine or with the oracle's restatements.
"""
import os
from collections import OrderedDict

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MLP_DIMS = (63, 128, 96, 64, 48, 12)
CONV_W, CONV_C, CONV_HW, CONV_FLAT, CONV_OUT = 288, 16, 63, 1008, 12

MLP_MEMBERS = ("init", "trained", "init_l2_x2^-20", "init_l2_x2^-8", "init_l2_x2^8", "init_l2_x2^12", "init_allW_x4", "trained_allW_x2",
               "init_outlier_1000", "trained_outlier_4096", "init_W3_zero", "init_b3_dead", "init_b1_plus300", "zero", "wide_random",
               "init_x2^-16", "init_x2^16", "init_l1_x2^-30")
CONV_MEMBERS = ("init", "trained", "init_conv_x2^-30", "init_conv_x2^-12", "init_conv_x2^12", "init_conv_x2^20", "init_headW_x2^-30",
                "init_headW_x2^-12", "init_headW_x2^12", "init_headW_x2^20", "trained_outliers_4096", "init_convW_zero",
                "init_convb_minus10", "init_convb_plus500", "zero")
REFUSED_MEMBERS = ("init_x2^-24", "init_x2^24", "inf", "nan", "3e38", "init_b5_1e32", "init_b2_inf")
PUBLISH_MEMBERS = (("mlp", "trained_allW_x2"), ("conv", "init_headW_x2^-12"))   # the members the learner's hand-off is run from


def load_fixtures():
    """(blob, trained, cblob, ctrained): the random-init and trained fixture of Connect4Net and Connect4ConvNet."""
    from bench import make_conv_weights

    return (np.load(os.path.join(GOLDEN, "c4net_blob_f32.npy")), np.load(os.path.join(GOLDEN, "c4net_trained_f32.npy")),
            make_conv_weights(20260101), np.load(os.path.join(GOLDEN, "c4conv_trained_f32.npy")))


def _p2(k):
    return np.float32(2.0) ** np.float32(k)


def mlp_views(blob):
    """[(W_l [out][in], b_l)] for l = 1..5 as views into `blob` (layout W_l, b_l for widths 63 -> 128 -> 96 -> 64 -> 48 -> 12)."""
    out, off = [], 0
    for k, o in zip(MLP_DIMS[:-1], MLP_DIMS[1:]):
        out.append((blob[off:off + k * o].reshape(o, k), blob[off + k * o:off + k * o + o]))
        off += k * o + o
    assert off == blob.size
    return out


def conv_views(blob):
    """(conv.weight [16][2][3][3], conv.bias [16], head.weight [12][1008], head.bias [12]) as views into `blob`."""
    assert blob.size == CONV_W + CONV_C + CONV_OUT * CONV_FLAT + CONV_OUT
    a, b, c = CONV_W, CONV_W + CONV_C, CONV_W + CONV_C + CONV_OUT * CONV_FLAT
    return blob[:a].reshape(16, 2, 3, 3), blob[a:b], blob[b:c].reshape(CONV_OUT, CONV_FLAT), blob[c:]


def mlp_family(blob, trained):
    blob = np.ascontiguousarray(blob, np.float32); trained = np.ascontiguousarray(trained, np.float32)
    fam = OrderedDict()
    fam["init"] = blob.copy()
    fam["trained"] = trained.copy()
    for k in (-20, -8, 8, 12):   # layer 2 (W and b) x 2^k
        w = blob.copy()
        W, b = mlp_views(w)[1]
        W *= _p2(k); b *= _p2(k)
        fam[f"init_l2_x2^{k}"] = w
    for name, src, f in (("init_allW_x4", blob, 4.0), ("trained_allW_x2", trained, 2.0)):
        w = src.copy()
        for W, _ in mlp_views(w):
            W *= np.float32(f)
        fam[name] = w
    for name, src, at, f in (("init_outlier_1000", blob, 0, 1000.0), ("trained_outlier_4096", trained, 1, 4096.0)):
        w = src.copy()
        for W, _ in mlp_views(w):
            W[at, at] = np.float32(f) * np.abs(W).max()
        fam[name] = w
    w = blob.copy(); mlp_views(w)[2][0][:] = 0
    fam["init_W3_zero"] = w
    w = blob.copy(); b3 = mlp_views(w)[2][1]; b3[:] = -np.abs(b3) - np.float32(5)   # every unit of layer 3 is dead
    fam["init_b3_dead"] = w
    w = blob.copy(); mlp_views(w)[0][1][:] += np.float32(300)
    fam["init_b1_plus300"] = w
    fam["zero"] = np.zeros_like(blob)
    rs = np.random.RandomState(5)
    w = np.zeros_like(blob)
    for W, b in mlp_views(w):
        W[:] = (3.0 * rs.standard_normal(W.shape) * 2.0 ** rs.uniform(-12, 0, W.shape) / np.sqrt(W.shape[1])).astype(np.float32)
        b[:] = (0.1 * rs.standard_normal(b.shape)).astype(np.float32)
    fam["wide_random"] = w
    for k in (-16, 16):   # the last whole-blob scalings a coarse grid found accepted (x 2^+-24 are refused: refused_family)
        fam[f"init_x2^{k}"] = blob * _p2(k)
    # layer 1 (W and b) x 2^-30, the one place where Connect4Net's weight exponent reaches its cap of 40 inside
    # the window (s[0] = 8; every later layer with t = 40 has s + t > 60 and is refused)
    w = blob.copy()
    W, b = mlp_views(w)[0]
    W *= _p2(-30); b *= _p2(-30)
    fam["init_l1_x2^-30"] = w
    assert tuple(fam) == MLP_MEMBERS and all(v.dtype == np.float32 and np.isfinite(v).all() for v in fam.values())
    return fam


def conv_family(cblob, ctrained):
    cblob = np.ascontiguousarray(cblob, np.float32); ctrained = np.ascontiguousarray(ctrained, np.float32)
    fam = OrderedDict()
    fam["init"] = cblob.copy()
    fam["trained"] = ctrained.copy()
    for k in (-30, -12, 12, 20):   # the conv layer (W and b) x 2^k
        w = cblob.copy()
        cw, cb, _, _ = conv_views(w)
        cw *= _p2(k); cb *= _p2(k)
        fam[f"init_conv_x2^{k}"] = w
    for k in (-30, -12, 12, 20):   # the head's W x 2^k
        w = cblob.copy()
        conv_views(w)[2][:] *= _p2(k)
        fam[f"init_headW_x2^{k}"] = w
    w = ctrained.copy()
    cw, _, hw, _ = conv_views(w)
    cw.reshape(-1)[5] = np.float32(4096) * np.abs(cw).max()
    hw.reshape(-1)[77] = np.float32(4096) * np.abs(hw).max()
    fam["trained_outliers_4096"] = w
    w = cblob.copy(); conv_views(w)[0][:] = 0
    fam["init_convW_zero"] = w
    w = cblob.copy(); conv_views(w)[1][:] = np.float32(-10)
    fam["init_convb_minus10"] = w
    w = cblob.copy(); conv_views(w)[1][:] += np.float32(500)
    fam["init_convb_plus500"] = w
    fam["zero"] = np.zeros_like(cblob)
    assert tuple(fam) == CONV_MEMBERS and all(v.dtype == np.float32 and np.isfinite(v).all() for v in fam.values())
    return fam


def refused_family(blob):
    """Connect4Net parameter sets without an f16x2 plan: outside the window on either side, and the non-finite / huge single weights the
    suite already refuses."""
    blob = np.ascontiguousarray(blob, np.float32)
    fam = OrderedDict()
    fam["init_x2^-24"] = blob * _p2(-24)
    fam["init_x2^24"] = blob * _p2(24)
    for name, at, v in (("inf", 7, np.inf), ("nan", 100, np.nan), ("3e38", 7, 3e38)):
        w = blob.copy(); w[at] = np.float32(v)
        fam[name] = w
    # two more: a bias that is finite in f32 but not at its layer's scale (2^24 for the init network's last layer; f32
    # evaluates this network finitely, the f16x2 accumulator would start at infinity), and a non-finite bias
    w = blob.copy(); mlp_views(w)[4][1][0] = np.float32(1e32)
    fam["init_b5_1e32"] = w
    w = blob.copy(); mlp_views(w)[1][1][3] = np.float32(np.inf)
    fam["init_b2_inf"] = w
    assert tuple(fam) == REFUSED_MEMBERS
    return fam


# ---- the float64 reference ------------------------------------------------------------------------------------------------------------
def _bits(bb):
    """[n][7 rows][9 cols] booleans of bitboards (bit = row + 7 col, row 0 = bottom)."""
    bb = np.ascontiguousarray(bb, np.uint64).ravel()
    sh = (np.arange(7)[:, None] + 7 * np.arange(9)[None, :]).astype(np.uint64)
    return ((bb[:, None, None] >> sh[None]) & np.uint64(1)).astype(bool)


def features_f64(my, op):
    """[n][63] (feature row * 9 + col): +1 mine, -1 theirs, +0.1 the lowest free cell of a column, -0.1 any other free cell; the 0.1 is
    the f32 number, as the reference computes its features in f32."""
    m, o = _bits(my), _bits(op)
    occ = m | o
    below = np.concatenate([np.ones_like(occ[:, :1]), occ[:, :-1]], axis=1)   # the cell under row 0 counts as occupied
    tenth = np.float64(np.float32(0.1))
    x = np.where(m, 1.0, np.where(o, -1.0, np.where(below, tenth, -tenth)))
    return x.reshape(len(x), 63)


def _softmax3(raw):
    z = raw[:, 9:12] - raw[:, 9:12].max(axis=1, keepdims=True)
    with np.errstate(invalid="ignore"):
        e = np.exp(z)
        return e / e.sum(axis=1, keepdims=True)


def mlp_f64(blob, my, op):
    """(raw [n][12], value [n][3] = stabilised softmax of raw[9:12]) of Connect4Net: x -> relu(x W_l^T + b_l) for l = 1..4, then W_5, b_5."""
    x = features_f64(my, op)
    layers = mlp_views(np.ascontiguousarray(blob, np.float32).astype(np.float64))
    for l, (W, b) in enumerate(layers):
        x = x @ W.T + b
        if l < 4:
            x = np.maximum(x, 0.0)
    return x, _softmax3(x)


def conv_f64(blob, my, op):
    """(raw [n][12], value [n][3]) of Connect4ConvNet: planes (mine, theirs) [2][7][9] -> Conv2d<2, 16, 3, pad 1> + ReLU -> flatten
    [channel][row][col] -> Linear<1008, 12>."""
    cw, cb, hw, hb = conv_views(np.ascontiguousarray(blob, np.float32).astype(np.float64))
    x = np.stack([_bits(my), _bits(op)], axis=1).astype(np.float64)          # [n][2][7][9]
    xp = np.pad(x, ((0, 0), (0, 0), (1, 1), (1, 1)))
    y = np.zeros((len(x), 16, 7, 9)) + cb[None, :, None, None]
    for ci in range(2):
        for k1 in range(3):
            for k2 in range(3):
                y += cw[None, :, ci, k1, k2, None, None] * xp[:, None, ci, k1:k1 + 7, k2:k2 + 9]
    y = np.maximum(y, 0.0).reshape(len(x), CONV_FLAT)
    raw = y @ hw.T + hb
    return raw, _softmax3(raw)


def same_bits(a, b):
    """Bit-for-bit equality of two f32 arrays; NaN positions are compared by isnan (a NaN's payload is not part of the definition)."""
    a = np.ascontiguousarray(a, np.float32); b = np.ascontiguousarray(b, np.float32)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb]))


# ---- the bars -------------------------------------------------------------------------------------------------------------------------
LOGIT_REL = 2e-6      # the trained fixtures' bar (tests/test_oracle_f16x2.py, tests/test_conv_f16x2_model.py), relative to the scale
F32_RATIO = 4.0       # ... and no further from f64 than four times the f32 arithmetic (floor 1e-7 of the scale)


def f64_errors(l16, v16, lfma, raw64, v64):
    """The figures the bars are stated on: scale = max(1, max |raw_f64|) over all 12 outputs, the largest logit errors of the f16x2 and
    f32 arithmetic against f64 and the largest outcome-probability error."""
    scale = max(1.0, float(np.abs(raw64).max()))
    with np.errstate(invalid="ignore", over="ignore"):
        e16 = float(np.abs(l16.astype(np.float64) - raw64[:, :9]).max())
        e32 = float(np.abs(lfma.astype(np.float64) - raw64[:, :9]).max())
        ev = float(np.abs(v16.astype(np.float64) - v64).max())
    return dict(scale=scale, logit_err=e16, f32_logit_err=e32, value_err=ev)


def check_f64_bars(name, l16, v16, lfma, raw64, v64):
    """Asserts the f64 bars on one member's outputs and returns the figures. NaN fails every comparison."""
    f = f64_errors(l16, v16, lfma, raw64, v64)
    scale = f["scale"]
    print(f"{name}: scale {scale:.4g}  f16x2 logit error {f['logit_err']:.3e} ({f['logit_err'] / scale:.2e} relative)  "
          f"f32 {f['f32_logit_err']:.3e}  value error {f['value_err']:.3e}")
    assert f["logit_err"] / scale < LOGIT_REL, (name, f)
    assert f["logit_err"] < F32_RATIO * max(f["f32_logit_err"], 1e-7 * scale), (name, f)
    if LOGIT_REL * scale < 1.0:   # softmax moves at most half the largest change of its inputs; above this the statement is vacuous
        assert f["value_err"] < LOGIT_REL * scale, (name, f)
    return f


def accept_edges(has_plan, blob, ks=range(-30, 31)):
    """For blob x 2^k over `ks`: {k: bool} from has_plan(blob_k), and the largest accepted / smallest refused |k| on each side."""
    ok = OrderedDict((k, bool(has_plan(blob * _p2(k)))) for k in ks)
    neg_ok = [k for k in ok if k <= 0 and ok[k]]; pos_ok = [k for k in ok if k >= 0 and ok[k]]
    neg_no = [k for k in ok if k < 0 and not ok[k]]; pos_no = [k for k in ok if k > 0 and not ok[k]]
    edges = dict(last_accepted_down=min(neg_ok) if neg_ok else None, first_refused_down=max(neg_no) if neg_no else None,
                 last_accepted_up=max(pos_ok) if pos_ok else None, first_refused_up=min(pos_no) if pos_no else None)
    return ok, edges
