"""The device-side epoch sampler restated in numpy from the text of include/synthesis_amd.h ("Device-side epoch sampler"): unsigned
64-bit arithmetic with wrap-around, then np.argsort. Nothing here comes from the product.

    finalise(z):  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;  z = (z ^ (z >> 27)) * 0x94D049BB133111EB;  z ^ (z >> 31)
    sm(seed, idx) = finalise(seed + (idx + 1) * 0x9E3779B97F4A7C15), idx + 1 in 32 bits
    K_e = sm(key ^ SAMPLER_TAG, e);  k_i = sm(K_e, i);  perm_e = argsort(k);  flip_e[i] = k_i & 1
"""
import numpy as np

M64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15
SAMPLER_TAG = 0x5AD3C0DE5EED1E55


def finalise(z):
    """z: np.uint64 array (or scalar array); wraps modulo 2^64"""
    z = np.asarray(z, np.uint64)
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def sm(seed, idx):
    """seed: uint64 (scalar or array), idx: uint32 values (scalar or array); idx + 1 wraps in 32 bits"""
    with np.errstate(over="ignore"):
        nxt = (np.asarray(idx, np.uint64) + np.uint64(1)) & np.uint64(0xFFFFFFFF)
        return finalise(np.asarray(seed, np.uint64) + nxt * np.uint64(GOLDEN))


def epoch_key(key, epoch):
    return sm(np.uint64((int(key) & M64) ^ SAMPLER_TAG), np.uint64(int(epoch) & 0xFFFFFFFF))


def sort_keys(key, epoch, n):
    """k_i for i in [0, n)"""
    return sm(epoch_key(key, epoch), np.arange(int(n), dtype=np.uint64))


def sampler(key, epoch, n):
    """(perm [n] int32: the rows in ascending order of k_i, flip [n] uint8 by row: k_i & 1)"""
    k = sort_keys(key, epoch, n)
    return np.argsort(k, kind="stable").astype(np.int32), (k & np.uint64(1)).astype(np.uint8)


def chi_square(counts):
    """Pearson's statistic of `counts` against the uniform distribution over its cells"""
    c = np.asarray(counts, np.float64)
    e = c.sum() / c.size
    return float(((c - e) ** 2 / e).sum())
