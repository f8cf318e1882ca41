"""The head of syn_dataset_evaluate_arith and the agreement statistics, restated from the text of include/synthesis_amd.h and of
synthesis_amd.arena.dataset_agreement's docstring. TEST INFRASTRUCTURE ONLY; numpy and the oracle's det_expf / det_logf, no GPU, nothing
here comes from the product.

head (per row, per head group: x = 9 policy or 3 value raw outputs, t = the targets; every operation rounds to f32):
    mx  = the first maximum of x
    se  = 0.0f;  se = se + det_expf(x_k - mx)                       k ascending
    lse = mx + det_logf(se)
    kl  = 0.0f;  kl = kl + t_k * (det_logf(t_k) - (x_k - lse))      k ascending, only where t_k > 0
agreement (two [n][12] arrays of raw outputs, f64): plain loops over rows, one row at a time.
"""
import math

import numpy as np

F32 = np.float32


def _group(oracle, x, t):
    """kl [n] f32 of one head group; x [n][k], t [n][k] f32"""
    x = np.ascontiguousarray(x, F32); t = np.ascontiguousarray(t, F32)
    n, k = x.shape
    with np.errstate(all="ignore"):
        mx = x[:, 0].copy()
        for c in range(1, k):
            mx = np.where(x[:, c] > mx, x[:, c], mx).astype(F32)
        se = np.zeros(n, F32)
        for c in range(k):
            se = (se + oracle.det_expf((x[:, c] - mx).astype(F32))).astype(F32)
        lse = (mx + oracle.det_logf(se)).astype(F32)
        kl = np.zeros(n, F32)
        for c in range(k):
            logp = (x[:, c] - lse).astype(F32)
            pos = t[:, c] > 0
            lt = oracle.det_logf(np.where(pos, t[:, c], F32(1.0)).astype(F32))
            term = (t[:, c] * (lt - logp).astype(F32)).astype(F32)
            kl = np.where(pos, (kl + term).astype(F32), kl).astype(F32)
    return kl


def head(oracle, raw12, tpi, tv):
    """(kl_pi [n], kl_v [n]) in f32 from the raw outputs [n][12] and the targets [n][9], [n][3]"""
    raw = np.ascontiguousarray(raw12, F32).reshape(-1, 12)
    n = raw.shape[0]
    return (_group(oracle, raw[:, :9], np.asarray(tpi, F32).reshape(n, 9)), _group(oracle, raw[:, 9:], np.asarray(tv, F32).reshape(n, 3)))


def row_kl(oracle, raw12, tpi, tv):
    """[n][2] as syn_dataset_evaluate_arith's row_kl"""
    p, v = head(oracle, raw12, tpi, tv)
    return np.stack([p, v], axis=1).astype(F32)


# ---- agreement ------------------------------------------------------------------------------------------------------------------------
def _argmax(x, allowed):
    best, bv = len(x), None
    for c in range(len(x)):
        if allowed[c] and (best == len(x) or x[c] > bv):
            best, bv = c, x[c]
    return best


def _kl(a, b, allowed):
    ia = [c for c in range(len(a)) if allowed[c]]
    if not ia:
        return 0.0
    ma, mb = max(a[c] for c in ia), max(b[c] for c in ia)
    za = math.log(sum(math.exp(a[c] - ma) for c in ia)); zb = math.log(sum(math.exp(b[c] - mb) for c in ia))
    out = 0.0
    for c in ia:
        la, lb = a[c] - ma - za, b[c] - mb - zb
        out += math.exp(la) * (la - lb)
    return out


def dataset_agreement(rows_a, rows_b, my_bb, op_bb):
    a = np.asarray(rows_a, F32).reshape(-1, 12).astype(np.float64); b = np.asarray(rows_b, F32).reshape(-1, 12).astype(np.float64)
    n = a.shape[0]
    if n == 0:
        return dict(rows=0, max_abs_diff=0.0, mean_abs_diff=0.0, pi_argmax_differs=0.0, v_argmax_differs=0.0, mean_kl_pi=0.0, mean_kl_v=0.0)
    my = np.asarray(my_bb, np.uint64).ravel(); op = np.asarray(op_bb, np.uint64).ravel()
    mx, sm, pd, vd, kp, kv = 0.0, 0.0, 0, 0, 0.0, 0.0
    for i in range(n):
        occ = int(my[i]) | int(op[i])
        legal = [((occ >> (6 + 7 * c)) & 1) == 0 for c in range(9)]
        d = [abs(float(a[i, k]) - float(b[i, k])) for k in range(12)]
        mx = max(mx, max(d)); sm += sum(d)
        pd += _argmax(a[i, :9], legal) != _argmax(b[i, :9], legal)
        vd += _argmax(a[i, 9:], [True] * 3) != _argmax(b[i, 9:], [True] * 3)
        kp += _kl(a[i, :9], b[i, :9], legal); kv += _kl(a[i, 9:], b[i, 9:], [True] * 3)
    return dict(rows=n, max_abs_diff=mx, mean_abs_diff=sm / (12 * n), pi_argmax_differs=pd / n, v_argmax_differs=vd / n, mean_kl_pi=kp / n,
                mean_kl_v=kv / n)
