"""State digests on the host: the definition of include/synthesis_amd.h "State digests" (syn_state_digest) in numpy, so that state a
run keeps in host memory (the replay="host" loop's buffer) is reported with the same words as state the engine keeps on the device.

A component is a sequence of 32-bit words w_0 .. w_{L-1}: its arrays concatenated, each read as it lies in memory (a 64-bit value is
its low word followed by its high word). With T = 0xD16E57000000AA00 + what and all arithmetic unsigned 64-bit with wrap-around:

    finalise(z):  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;  z = (z ^ (z >> 27)) * 0x94D049BB133111EB;  z ^ (z >> 31)
    sm(seed, idx) = finalise(seed + ((idx + 1) mod 2^32) * GOLDEN),   GOLDEN = 0x9E3779B97F4A7C15
    a_i = finalise(T + (i + 1) * GOLDEN);   h_i = sm(a_i, w_i);   S = sum h_i mod 2^64;   digest = sm(sm(S ^ T, hi32(L)), lo32(L))
"""
import sys

import numpy as np

COMPONENTS = {"trainer": 1, "network": 2, "replay": 3, "train_data": 4, "eval_data": 5}   # SYN_DIGEST_*
DIGEST_TAG = 0xD16E57000000AA00
GOLDEN = 0x9E3779B97F4A7C15
_M64 = (1 << 64) - 1
_CHUNK = 1 << 20   # words per pass: bounds the temporaries at a few tens of MB whatever the buffer's size


def _finalise(z):
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def _sm(seed, idx):
    return _finalise(seed + ((idx + np.uint64(1)) & np.uint64(0xFFFFFFFF)) * np.uint64(GOLDEN))


def words_of(array):
    """`array` as the uint32 words it occupies in memory (C order, little-endian: low word of a 64-bit value first)"""
    a = np.ascontiguousarray(array)
    if a.dtype.itemsize % 4 != 0:
        raise ValueError(f"a digest is over 32-bit words: dtype {a.dtype} has {a.dtype.itemsize} bytes per item")
    if sys.byteorder != "little" and a.dtype.itemsize > 4:
        raise NotImplementedError("word order of 64-bit values on a big-endian host")
    return a.reshape(-1).view(np.uint32)


def component_tag(what):
    if isinstance(what, str):
        if what not in COMPONENTS:
            raise ValueError(f"what must be one of {sorted(COMPONENTS)}, got {what!r}")
        what = COMPONENTS[what]
    return (DIGEST_TAG + int(what)) & _M64


def digest_words(what, *arrays):
    """The digest (an int) of component `what` (a name of COMPONENTS or its number) whose word sequence is `arrays` concatenated in
    the order given — e.g. digest_words("replay", my, op, gid, pi, v), digest_words("trainer", w, m, v, np.int64(step))."""
    tag = np.uint64(component_tag(what))
    total, at = np.uint64(0), 0
    with np.errstate(over="ignore"):
        for array in arrays:
            w = words_of(array)
            for lo in range(0, w.size, _CHUNK):
                part = w[lo:lo + _CHUNK].astype(np.uint64)
                i = np.arange(at + lo + 1, at + lo + 1 + part.size, dtype=np.uint64)
                total = total + _sm(_finalise(tag + i * np.uint64(GOLDEN)), part).sum(dtype=np.uint64)
            at += w.size
        out = _sm(_sm(np.uint64(total) ^ tag, np.uint64(at >> 32)), np.uint64(at & 0xFFFFFFFF))
    return int(out)


def trainer_digest(weights, m, v, step):
    """SYN_DIGEST_TRAINER of a trainer_state(): w, m, v as f32 words, then the step count's low and high word"""
    f = [np.ascontiguousarray(a, dtype=np.float32) for a in (weights, m, v)]
    return digest_words("trainer", f[0], f[1], f[2], np.array([int(step)], np.int64))


def replay_digest(my, op, gid, pi, v):
    """SYN_DIGEST_REPLAY of a buffer's five arrays (Engine.replay_read() / the host loop's R)"""
    return digest_words("replay", np.ascontiguousarray(my, np.uint64), np.ascontiguousarray(op, np.uint64),
                        np.ascontiguousarray(gid, np.int64), np.ascontiguousarray(pi, np.float32), np.ascontiguousarray(v, np.float32))


def dataset_digest(what, my, op, pi, v):
    """SYN_DIGEST_TRAIN_DATA / SYN_DIGEST_EVAL_DATA of a data set's four arrays"""
    return digest_words(what, np.ascontiguousarray(my, np.uint64), np.ascontiguousarray(op, np.uint64),
                        np.ascontiguousarray(pi, np.float32), np.ascontiguousarray(v, np.float32))


def hex16(digest):
    """a digest as the 16-digit hex string the loop's records carry"""
    return f"{int(digest) & _M64:016x}"
