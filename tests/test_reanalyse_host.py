"""The selection of a reanalysis (include/synthesis_amd.h "Reanalyse") as the learner restates it in numpy — learner.reanalyse_flags,
learner.searchable_positions — and LearningLoop's validation of its reanalyse* arguments. No GPU."""
import numpy as np
import pytest

from synthesis_amd.learner import LearningLoop, reanalyse_flags, searchable_positions

FULL = 1 << 32
INT64_MAX = (1 << 63) - 1


def play_random(rng, n_moves):
    """A legal position after up to n_moves random moves (stones alternate, gravity holds): (my, op), my = the side to move"""
    heights = [0] * 9
    bb = [0, 0]
    for k in range(n_moves):
        free = [c for c in range(9) if heights[c] < 7]
        if not free:
            break
        c = free[rng.integers(len(free))]
        bb[k & 1] |= 1 << (heights[c] + 7 * c)
        heights[c] += 1
    k = sum(heights)
    return bb[k & 1], bb[(k & 1) ^ 1]


@pytest.fixture(scope="module")
def synthetic_rows():
    """200,000 rows (gid, my, op): legal positions of random games, ~21 plies each, in buffer order"""
    rng = np.random.default_rng(20261020)
    n = 200_000
    gid = np.sort(rng.integers(0, 10_000, n)).astype(np.int64)
    my, op = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
    # a few thousand distinct positions, drawn with repetition (openings recur across games, as in a real buffer)
    pool = [play_random(rng, int(rng.integers(0, 12))) for _ in range(4000)]
    pick = rng.integers(0, len(pool), n)
    my[:] = np.array([pool[i][0] for i in pick], np.uint64)
    op[:] = np.array([pool[i][1] for i in pick], np.uint64)
    return gid, my, op


def test_selected_fraction_is_the_threshold(synthetic_rows):
    """Over 200,000 rows the selected fraction lies within 5 sigma of threshold / 2^32 (among the searchable rows: the hash is drawn per
    (gid, my, op), and every row here is eligible)."""
    gid, my, op = synthetic_rows
    ok = searchable_positions(my, op)
    n = int(ok.sum())
    assert n > 190_000   # positions of at most 11 plies: four in a row is rare
    for frac in (1 / 16, 0.37, 0.5):
        thr = int(np.floor(frac * 4294967296.0))
        p = thr / FULL
        sel = reanalyse_flags(0xC0FFEE, thr, INT64_MAX, gid, my, op)
        assert not sel[~ok].any()
        # identical (gid, my, op) triples share their fate: count distinct triples, the independent draws
        _, first = np.unique(np.stack([gid.astype(np.uint64), my, op], axis=1)[ok], axis=0, return_index=True)
        draws = sel[ok][first]
        sigma = np.sqrt(p * (1 - p) / draws.size)
        assert draws.size > 100_000
        assert abs(draws.mean() - p) < 5 * sigma, (frac, draws.mean(), p, sigma)
    # another key selects another set
    a = reanalyse_flags(1, FULL // 2, INT64_MAX, gid, my, op)
    b = reanalyse_flags(2, FULL // 2, INT64_MAX, gid, my, op)
    assert 0.2 < (a & b).sum() / a.sum() < 0.8


def test_flags_do_not_depend_on_the_row_index(synthetic_rows):
    gid, my, op = (a[:50_000] for a in synthetic_rows)
    perm = np.random.default_rng(5).permutation(gid.size)
    sel = reanalyse_flags(77, FULL // 3, 6000, gid, my, op)
    assert np.array_equal(reanalyse_flags(77, FULL // 3, 6000, gid[perm], my[perm], op[perm]), sel[perm])
    # ... nor on what precedes a row: a keep-window's shift leaves every surviving row's flag alone
    assert np.array_equal(reanalyse_flags(77, FULL // 3, 6000, gid[12_345:], my[12_345:], op[12_345:]), sel[12_345:])


def test_before_gid_and_the_extreme_thresholds(synthetic_rows):
    gid, my, op = (a[:50_000] for a in synthetic_rows)
    ok = searchable_positions(my, op)
    assert not reanalyse_flags(9, 0, INT64_MAX, gid, my, op).any()
    assert np.array_equal(reanalyse_flags(9, FULL, INT64_MAX, gid, my, op), ok)
    assert np.array_equal(reanalyse_flags(9, FULL, None, gid, my, op), ok)
    cut = int(gid[gid.size // 2])
    assert np.array_equal(reanalyse_flags(9, FULL, cut, gid, my, op), ok & (gid < cut))
    half = reanalyse_flags(9, FULL // 2, INT64_MAX, gid, my, op)
    assert np.array_equal(reanalyse_flags(9, FULL // 2, cut, gid, my, op), half & (gid < cut))
    assert not reanalyse_flags(9, FULL, int(gid.min()), gid, my, op).any()
    # negative game ids are ordinary ids (the bound is signed, the hash takes the 64-bit pattern)
    neg = gid - 20_000
    assert np.array_equal(reanalyse_flags(9, FULL, -15_000, neg, my, op), ok & (neg < -15_000))


def test_searchable_predicate_agrees_with_the_oracle(oracle):
    """searchable_positions == the column-shape rule (disjoint, inside the 63 cells, no holes, a free column) and neither side won
    (the oracle's Connect4::won), on legal positions of every length — finished games and full boards among them — and on broken ones."""
    rng = np.random.default_rng(11)
    boards = [play_random(rng, int(rng.integers(0, 64))) for _ in range(3000)]
    for _ in range(1500):   # illegal: random bits, overlaps, floating stones, bit 63
        my, op = play_random(rng, int(rng.integers(0, 40)))
        kind = rng.integers(4)
        if kind == 0:
            my |= 1 << int(rng.integers(63))
            op |= 1 << int(rng.integers(63))
        elif kind == 1:
            op |= my & -my if my else 1
        elif kind == 2:
            my |= 1 << 63
        else:
            my, op = int(rng.integers(0, 1 << 63)), int(rng.integers(0, 1 << 63))
        boards.append((my, op))

    def shape_ok(my, op):
        if my & op or (my | op) >> 63:
            return False
        occ = my | op
        cols = [(occ >> (7 * c)) & 0x7F for c in range(9)]
        return all(col in (0, 1, 3, 7, 15, 31, 63, 127) for col in cols) and any(col != 127 for col in cols)

    want = np.array([shape_ok(my, op) and not oracle.c4_won(my) and not oracle.c4_won(op) for my, op in boards])
    got = searchable_positions(np.array([b[0] for b in boards], np.uint64), np.array([b[1] for b in boards], np.uint64))
    assert np.array_equal(got, want)
    n_legal = 3000
    assert 0 < want[:n_legal].sum() < n_legal          # finished games are among the legal positions
    assert want[n_legal:].sum() < 0.5 * (len(boards) - n_legal)
    won = np.array([oracle.c4_won(my) or oracle.c4_won(op) for my, op in boards[:n_legal]])
    assert won.sum() > 100 and not got[:n_legal][won].any()


@pytest.mark.parametrize("kw", [dict(reanalyse=-0.1), dict(reanalyse=1.5), dict(reanalyse="half"), dict(reanalyse=True),
                                dict(reanalyse=float("nan")), dict(reanalyse=0.5, reanalyse_explores=-1),
                                dict(reanalyse=0.5, reanalyse_explores=2.5), dict(reanalyse=0.5, reanalyse_value_mix=1.01),
                                dict(reanalyse=0.5, reanalyse_value_mix=-0.5), dict(reanalyse=0.5, reanalyse_value_mix=float("nan")),
                                dict(reanalyse=0.5, reanalyse_value_mix=None)])
def test_learning_loop_refuses_bad_reanalyse_arguments(kw):
    """The arguments are validated before the engine is touched (engine=None would fail on its first use)."""
    with pytest.raises(ValueError, match="reanalyse"):
        LearningLoop(None, "mlp", np.zeros(1, np.float32), **kw)
