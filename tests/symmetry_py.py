"""The mirror symmetry of the 9x7 board and the symmetric replay de-duplication, restated in numpy (DESIGN.md "Mirror-symmetric
de-duplication"). This is the specification the device code is held to; nothing here calls the code under test.

    bit index of a bitboard      row + 7 * col, col in 0..8, row in 0..6 (synthesis_amd/match.py, csrc/device_common.cuh)
    mirror(bb)                   bit (row, col) -> (row, 8 - col); bit 63 is not part of the board and stays
    reverse(pi)[c]               pi[8 - c]
    canonical orientation        a record is FLIPPED when (mirror(my), mirror(op)) < (my, op) as pairs of unsigned 64-bit numbers, my
                                 first; its canonical form is then (mirror(my), mirror(op), reverse(pi), v), otherwise itself
    self-symmetric state         mirror(my) == my and mirror(op) == op
"""
import numpy as np

COL = np.uint64(0x7F)


def mirror(bb):
    """Column groups c and 8 - c exchanged, one column at a time (the device code uses four delta-swaps: not the same algorithm)."""
    bb = np.ascontiguousarray(bb, dtype=np.uint64)
    out = bb & np.uint64(1 << 63)
    for c in range(9):
        out = out | (((bb >> np.uint64(7 * c)) & COL) << np.uint64(7 * (8 - c)))
    return out


def reverse(pi):
    return np.ascontiguousarray(np.asarray(pi, dtype=np.float32).reshape(-1, 9)[:, ::-1])


def flipped(my, op):
    my, op = np.ascontiguousarray(my, dtype=np.uint64), np.ascontiguousarray(op, dtype=np.uint64)
    mm, mo = mirror(my), mirror(op)
    return (mm < my) | ((mm == my) & (mo < op))


def self_symmetric(my, op):
    my, op = np.ascontiguousarray(my, dtype=np.uint64), np.ascontiguousarray(op, dtype=np.uint64)
    return (mirror(my) == my) & (mirror(op) == op)


def canonicalise(my, op, pi):
    """-> (my, op, pi, flip) with every record in its canonical orientation"""
    my, op = np.ascontiguousarray(my, dtype=np.uint64).ravel(), np.ascontiguousarray(op, dtype=np.uint64).ravel()
    pi = np.ascontiguousarray(pi, dtype=np.float32).reshape(my.size, 9)
    f = flipped(my, op)
    return np.where(f, mirror(my), my), np.where(f, mirror(op), op), np.where(f[:, None], reverse(pi), pi), f


def expand(D):
    """Rows [U, U + M) behind the U canonical rows of a plain de-duplication `D` (dict my_bb, op_bb, pis, vs, num): the mirror
    images of the classes that are not self-symmetric, in class order. Returns the dict with `canonical` = U."""
    e = ~self_symmetric(D["my_bb"], D["op_bb"])
    return dict(my_bb=np.concatenate([D["my_bb"], mirror(D["my_bb"][e])]), op_bb=np.concatenate([D["op_bb"], mirror(D["op_bb"][e])]),
                pis=np.concatenate([D["pis"].reshape(-1, 9), reverse(D["pis"][e])]), vs=np.concatenate([D["vs"], D["vs"][e]]),
                num=np.concatenate([D["num"], D["num"][e]]), canonical=int(D["num"].size))


def symmetric_deduplicate(plain_deduplicate, my, op, pi, v):
    """The symmetric de-duplication of n records in buffer order, given a plain one (unique states in ascending (my, op) order,
    targets summed in buffer order and divided by the count): canonicalise, de-duplicate, expand."""
    cmy, cop, cpi, _ = canonicalise(my, op, pi)
    return expand(plain_deduplicate(cmy, cop, cpi, np.ascontiguousarray(v, dtype=np.float32).reshape(-1, 3)))

