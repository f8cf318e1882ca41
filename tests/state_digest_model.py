"""The state digest restated in numpy from the text of include/synthesis_amd.h ("State digests") on top of tests/sampler_model.py's
finalise and sm. Nothing here comes from the product.

    T = 0xD16E57000000AA00 + what
    a_i = finalise(T + (i + 1) * GOLDEN);  h_i = sm(a_i, w_i);  S = sum of h_i mod 2^64 (0 for no words)
    digest = sm(sm(S ^ T, hi32(L)), lo32(L))
A component's words: its arrays concatenated, each read as it lies in memory (a 64-bit value = its low word, then its high word).
"""
import numpy as np

from tests.sampler_model import GOLDEN, M64, finalise, sm

TAG = 0xD16E57000000AA00
TRAINER, NETWORK, REPLAY, TRAIN_DATA, EVAL_DATA = 1, 2, 3, 4, 5


def words(*arrays):
    """the uint32 words of the arrays, in the order given"""
    parts = []
    for a in arrays:
        a = np.ascontiguousarray(a)
        assert a.dtype.itemsize in (4, 8) and a.dtype.byteorder in ("=", "<", "|")
        parts.append(np.frombuffer(a.tobytes(), dtype="<u4"))
    return np.concatenate(parts) if parts else np.zeros(0, np.uint32)


def digest_of_words(what, w):
    w = np.asarray(w, np.uint32)
    L = int(w.size)
    T = np.uint64((TAG + int(what)) & M64)
    with np.errstate(over="ignore"):
        i = np.arange(1, L + 1, dtype=np.uint64)
        a = finalise(T + i * np.uint64(GOLDEN))
        S = np.uint64(int(sm(a, w).sum(dtype=np.uint64)) & M64) if L else np.uint64(0)
        return int(sm(sm(S ^ T, np.uint64(L >> 32)), np.uint64(L & 0xFFFFFFFF)))


def digest(what, *arrays):
    return digest_of_words(what, words(*arrays))


def trainer(w, m, v, step):
    return digest(TRAINER, np.asarray(w, np.float32), np.asarray(m, np.float32), np.asarray(v, np.float32), np.array([int(step)], np.int64))


def network(blob):
    return digest(NETWORK, np.asarray(blob, np.float32))


def replay(my, op, gid, pi, v):
    return digest(REPLAY, np.asarray(my, np.uint64), np.asarray(op, np.uint64), np.asarray(gid, np.int64), np.asarray(pi, np.float32),
                  np.asarray(v, np.float32))


def dataset(what, my, op, pi, v):
    return digest(what, np.asarray(my, np.uint64), np.asarray(op, np.uint64), np.asarray(pi, np.float32), np.asarray(v, np.float32))


def random_rows(rng, n, with_gid=True):
    """n rows whose words are anything at all: random bit patterns as f32 (NaN payloads, infinities, denormals among them), negative
    zeros, quiet and signalling NaNs put in by hand, boards with bit 63 set and game ids above 2^32 and below zero."""
    my = rng.integers(0, 1 << 64, n, dtype=np.uint64)
    op = rng.integers(0, 1 << 64, n, dtype=np.uint64)
    gid = rng.integers(-(1 << 40), 1 << 40, n, dtype=np.int64)
    pi = rng.integers(0, 1 << 32, (n, 9), dtype=np.uint32).view(np.float32)
    v = rng.integers(0, 1 << 32, (n, 3), dtype=np.uint32).view(np.float32)
    if n:
        gid[0] = (1 << 32) + 5
        gid[-1] = (7 << 32) | 0xFFFFFFFF
        pi.view(np.uint32)[0, :3] = (0x80000000, 0x7FC00001, 0xFF800123)   # -0.0, a quiet NaN with a payload, a negative signalling NaN
        v.view(np.uint32)[-1, :2] = (0x80000000, 0x7F800001)
    out = dict(my=my, op=op, pi=pi, v=v)
    if with_gid:
        out["gid"] = gid
    return out
