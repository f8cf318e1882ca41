"""Held-out evaluation restated in numpy from the text of include/synthesis_amd.h ("Held-out evaluation"). TEST INFRASTRUCTURE ONLY; no
GPU, nothing here comes from the product.

    arg-max, first maximum wins:  best = the first (legal) entry; a later entry replaces it only when it compares greater
    legal column c:               bit 6 + 7 c of my | op is clear; no legal column -> 9 (never a hit)
    block j = rows [32 j, 32 j + 32) of the range; loss_j = (1.0f / rows_j) * (0.0f + kl_0 + kl_1 + ...) in f32, row order
    chunk c = blocks [256 c, 256 c + 256): S_c = 0.0 + rows_j * loss_j in ascending j (f64); sum = 0.0 + S_c in ascending c; mean = sum / n
    held out:  (sm(sm(key ^ HOLDOUT_TAG, gid >> 32), gid & 0xFFFFFFFF) >> 32) < threshold     (sm: tests/sampler_model.py)
"""
import numpy as np

from tests.sampler_model import M64, sm

BLOCK = 32
CHUNK_BLOCKS = 256
HOLDOUT_TAG = 0x401D0075E7C0FFEE


def argmax_first(x):
    best, bv = 0, x[0]
    for c in range(1, len(x)):
        if x[c] > bv:
            best, bv = c, x[c]
    return best


def argmax_legal(x, occ):
    best, bv = 9, None
    for c in range(9):
        if (int(occ) >> (6 + 7 * c)) & 1:
            continue
        if best == 9 or x[c] > bv:
            best, bv = c, x[c]
    return best


def row_hits(row_logits, my, op, tpi, tv):
    """(pi_hit [n], v_hit [n]) as uint32 0 / 1 from the twelve logits of every row"""
    lg = np.asarray(row_logits, np.float32).reshape(-1, 12)
    n = lg.shape[0]
    my = np.asarray(my, np.uint64).ravel(); op = np.asarray(op, np.uint64).ravel()
    tpi = np.asarray(tpi, np.float32).reshape(n, 9); tv = np.asarray(tv, np.float32).reshape(n, 3)
    ph = np.zeros(n, np.uint32); vh = np.zeros(n, np.uint32)
    for i in range(n):
        ph[i] = argmax_legal(lg[i, :9], int(my[i]) | int(op[i])) == argmax_first(tpi[i])
        vh[i] = argmax_first(lg[i, 9:]) == argmax_first(tv[i])
    return ph, vh


def block_rows(n):
    nb = (n + BLOCK - 1) // BLOCK
    return np.array([min(BLOCK, n - BLOCK * j) for j in range(nb)], np.int64)


def block_losses(row_kl):
    """[n_blocks][2] f32 from the per-row KL values [n][2]: the one-thread chain of the learner's loss words"""
    kl = np.asarray(row_kl, np.float32).reshape(-1, 2)
    rows = block_rows(kl.shape[0])
    out = np.zeros((rows.size, 2), np.float32)
    with np.errstate(all="ignore"):
        for j, r in enumerate(rows):
            bm = np.float32(1.0) / np.float32(r)
            acc = np.zeros(2, np.float32)
            for b in range(r):
                acc = (acc + kl[BLOCK * j + b]).astype(np.float32)
            out[j] = (bm * acc).astype(np.float32)
    return out


def reduce_sum(rows, losses):
    """The f64 sum of rows_j * loss_j in the header's order; losses [n_blocks] f32"""
    rows = np.asarray(rows, np.int64); losses = np.asarray(losses, np.float32)
    total = np.float64(0.0)
    with np.errstate(all="ignore"):
        for c0 in range(0, rows.size, CHUNK_BLOCKS):
            s = np.float64(0.0)
            for j in range(c0, min(c0 + CHUNK_BLOCKS, rows.size)):
                s = s + np.float64(rows[j]) * np.float64(losses[j])
            total = total + s
    return total


def totals(n, blk_losses, pi_hit, v_hit):
    """dict(mean_pi, mean_v, sum_pi, sum_v, rows, blocks, pi_hits, v_hits) of n rows from the block losses [n_blocks][2] and the per-row hits"""
    if n == 0:
        return dict(mean_pi=0.0, mean_v=0.0, sum_pi=0.0, sum_v=0.0, rows=0, blocks=0, pi_hits=0, v_hits=0)
    rows = block_rows(n)
    bl = np.asarray(blk_losses, np.float32).reshape(rows.size, 2)
    sp, sv = reduce_sum(rows, bl[:, 0]), reduce_sum(rows, bl[:, 1])
    with np.errstate(all="ignore"):
        return dict(mean_pi=float(sp / np.float64(n)), mean_v=float(sv / np.float64(n)), sum_pi=float(sp), sum_v=float(sv), rows=int(n),
                    blocks=int(rows.size), pi_hits=int(np.sum(pi_hit, dtype=np.uint64)), v_hits=int(np.sum(v_hit, dtype=np.uint64)))


def f64_bits(x):
    return np.asarray([x], np.float64).view(np.uint64)[0]


# ---- holding games out ---------------------------------------------------------------------------------------------------------------
def holdout_hash(key, gid):
    """the 32-bit value compared with the threshold, per game id (int64 array, taken as its 64-bit pattern)"""
    g = np.asarray(gid, np.int64).astype(np.uint64)
    k0 = np.uint64((int(key) & M64) ^ HOLDOUT_TAG)
    return (sm(sm(k0, g >> np.uint64(32)), g & np.uint64(0xFFFFFFFF)) >> np.uint64(32)).astype(np.uint64)


def holdout_flags(key, gid, threshold):
    return holdout_hash(key, gid) < np.uint64(int(threshold))


def holdout_threshold(fraction):
    return int(np.floor(float(fraction) * 4294967296.0))


def is_seen(my, op, train_my, train_op):
    """which (my, op) rows are among the rows of (train_my, train_op), the latter sorted ascending by (my, op): one binary search each"""
    keys = list(zip((int(x) for x in train_my), (int(x) for x in train_op)))
    assert keys == sorted(keys)
    import bisect

    out = np.zeros(len(my), bool)
    for i, k in enumerate(zip((int(x) for x in my), (int(x) for x in op))):
        p = bisect.bisect_left(keys, k)
        out[i] = p < len(keys) and keys[p] == k
    return out


def unseen_first(D, seen):
    """the rows of the de-duplicated dict D (my_bb, op_bb, pis, vs) stably partitioned: unseen first, then seen; returns (D', n_unseen)"""
    order = np.concatenate([np.flatnonzero(~seen), np.flatnonzero(seen)])
    return {k: np.ascontiguousarray(np.asarray(D[k])[order]) for k in ("my_bb", "op_bb", "pis", "vs")}, int((~seen).sum())
