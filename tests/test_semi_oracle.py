"""The semi-global oracle (tests/_semi_oracle.py) pinned independently of itself: on exhaustive tiny
pairs its score is the best GLOBAL score of the query against any substring of the subject (the
empty one included), its j_end the smallest end of such a substring, and its CIGAR replays to its
score and end cell; then the hand-made cases the GPU tests reuse, each shown to have the property it
is named for.  No GPU."""
import itertools

import numpy as np
import pytest

from tests import _align_oracle as AO
from tests import _semi_oracle as SO

# asymmetric on purpose: subst[query letter][subject letter]
SUB2 = np.array([[3, -2], [-1, 2]], np.int32)
SUB3 = np.array([[3, -2, -1], [-1, 2, -3], [-2, 0, 4]], np.int32)
GAPS = [(-2, -2), (-4, -1), (0, 0), (-3, 0)]


def _seqs(nletters, lo, hi):
    for n in range(lo, hi + 1):
        for t in itertools.product(range(nletters), repeat=n):
            yield np.array((0,) + t, np.int32)


def _best_substring(q, s, sub, go, ge):
    """(best global score over substrings s[a+1 .. b], the smallest b that attains it)."""
    R, C = len(q) - 1, len(s) - 1
    best = np.full(C + 1, -(1 << 30), np.int64)
    for a in range(C + 1):
        H, _, _ = AO.matrices(q, np.concatenate(([0], s[a + 1:])), sub, go, ge, False)
        best[a:] = np.maximum(best[a:], H[R, :])  # H[R, b - a]: the query against s[a+1 .. b]
    return int(best.max()), int(np.argmax(best))


# two letters to the full size in one linear and one affine model; three letters, smaller, in all four
@pytest.mark.parametrize("sub,maxr,maxc,go,ge", [(SUB2, 5, 7) + g for g in GAPS[:2]] + [(SUB3, 3, 4) + g for g in GAPS],
                         ids=lambda v: None if isinstance(v, np.ndarray) else str(v))
def test_exhaustive_tiny_pairs(sub, maxr, maxc, go, ge):
    n = sub.shape[0]
    subjects = list(_seqs(n, 0, maxc))
    for q in _seqs(n, 1, maxr):
        R = len(q) - 1
        for s in subjects:
            want, wantj = _best_substring(q, s, sub, go, ge)
            score, i0, j0, ie, je, cig = SO.align(q, s, sub, go, ge)
            assert (score, ie, je) == (want, R, wantj), (q, s)
            assert SO.score(q, s, sub, go, ge) == (score, ie, je)
            assert i0 == 0 and 0 <= j0 <= je
            assert AO.rescore(cig, q, s, 0, j0, sub, go, ge) == (score, R, je), (q, s, cig)
            runs = AO.runs(cig)
            assert runs and runs[0][1] != "D", (q, s, cig)  # the walk stopped on entering row 0: no D there


def test_empty_sides():
    q = np.array([0, 1, 0, 1], np.int32)
    e = np.array([0], np.int32)
    assert SO.align(q, e, SUB2, -4, -1) == (-6, 0, 0, 3, 0, "3I")
    assert SO.align(e, q, SUB2, -4, -1) == (0, 0, 0, 0, 0, "")


# -- hand-made cases, shared with the GPU tests ------------------------------------------------
SUB5 = (np.full((5, 5), -1, np.int32) + 3 * np.eye(5, dtype=np.int32)).astype(np.int32)  # +2 / -1
SUB5_HARSH = (np.full((5, 5), -10, np.int32) + 12 * np.eye(5, dtype=np.int32)).astype(np.int32)  # +2 / -10


def _h(letters):
    return np.array([0] + list(letters), np.int32)


def planted_once():
    rng = np.random.default_rng(7)
    q = rng.integers(0, 4, 12)
    return _h(q), _h([4] * 9 + list(q) + [4] * 6)


def planted_twice():
    rng = np.random.default_rng(8)
    q = rng.integers(0, 4, 10)
    return _h(q), _h([4] * 5 + list(q) + [4] * 7 + list(q) + [4] * 3)


def all_mismatch():
    return _h([0, 1, 2, 3, 0, 1]), _h([4] * 20)


@pytest.mark.parametrize("go,ge", [(-3, -1), (-2, -2)])
def test_planted_once(go, ge):
    q, s = planted_once()
    assert SO.align(q, s, SUB5, go, ge) == (24, 0, 9, 12, 21, "12=")


@pytest.mark.parametrize("go,ge", [(-3, -1), (-2, -2)])
def test_planted_twice_takes_the_first_copy(go, ge):
    q, s = planted_twice()
    H, _, _ = SO.matrices(q, s, SUB5, go, ge)
    assert int((H[10] == H[10].max()).sum()) == 2  # two maximal cells in row R
    assert SO.align(q, s, SUB5, go, ge) == (20, 0, 5, 10, 15, "10=")


def test_mismatch_below_the_gap_cost_ends_in_column_0():
    q, s = all_mismatch()
    assert SO.align(q, s, SUB5_HARSH, -1, -1) == (-6, 0, 0, 6, 0, "6I")
    assert SO.align(q, s, SUB5_HARSH, -2, -1) == (-7, 0, 0, 6, 0, "6I")


@pytest.mark.parametrize("go,ge", [(-3, -1), (-2, -2)])
def test_all_mismatch_is_negative_where_local_says_zero(go, ge):
    q, s = all_mismatch()
    score, i0, j0, ie, je, cig = SO.align(q, s, SUB5, go, ge)
    assert score == -6 and cig == "6X" and (i0, j0, ie, je) == (0, 0, 6, 6)
    assert AO.align(q, s, SUB5, go, ge, True)[0] == 0
