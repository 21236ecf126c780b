"""tests/_overlap_oracle.py pinned independently of the kernels (no GPU): on sequences of at most 7
letters over 2 and 4 letters and three gap models its score is the brute-force maximum of the global
oracle's score (oracle/score_oracle.c) over every pair of cells that an overlap alignment may join; it
agrees with tests/_semi_oracle.py where the optimum is a containment and is never below it or below 0;
every CIGAR replays to its score and cells; and hand-written cases fix the tie rule."""
import itertools

import numpy as np

import oracle
from tests import _overlap_oracle as oo
from tests import _semi_oracle as so

GAPS3 = [(-3, -1), (-2, -2), (0, 0)]
TABLES = {2: np.array([[2, -3], [-3, 2]], np.int32), 4: (np.where(np.eye(4, dtype=bool), 3, -2)).astype(np.int32)}


def _hdr(a):
    return np.concatenate([[0], np.asarray(a, np.int64)]).astype(np.int32)


def _global(y, x, sub, go, ge):
    """The global score of two letter strings without header; an empty side is one gap or nothing."""
    if len(y) == 0 or len(x) == 0:
        n = len(y) + len(x)
        return 0 if n == 0 else go + (n - 1) * ge
    return oracle.score_ag(_hdr(y), _hdr(x), sub, go, ge, local=False)[0]


def _brute(y, x, sub, go, ge):
    R, C = len(y), len(x)
    best = None
    for i0, j0 in itertools.product(range(R + 1), range(C + 1)):
        if i0 != 0 and j0 != 0:
            continue
        for i1, j1 in itertools.product(range(i0, R + 1), range(j0, C + 1)):
            if i1 != R and j1 != C:
                continue
            v = _global(y[i0:i1], x[j0:j1], sub, go, ge)
            best = v if best is None else max(best, v)
    return best


def _cases():
    rng = np.random.default_rng(5)
    out = []
    for n in range(36):
        alpha = (2, 4)[n % 2]
        R, C = int(rng.integers(0, 8)), int(rng.integers(0, 8))
        y, x = rng.integers(0, alpha, R), rng.integers(0, alpha, C)
        if n % 3 == 0 and R >= 2 and C >= 2:  # a planted dovetail: Y's tail is X's head
            k = min(R, C) - 1
            x[:k] = y[R - k:]
        out.append((alpha, y, x))
    return out


def test_score_is_the_brute_force_maximum():
    for alpha, y, x in _cases():
        sub = TABLES[alpha]
        for go, ge in GAPS3:
            got = oo.score(_hdr(y), _hdr(x), sub, go, ge)
            assert got[0] == _brute(y, x, sub, go, ge), (y, x, go, ge, got)
            assert got[1] == len(y) or got[2] == len(x)


def test_relations_to_the_semi_global_oracle():
    contained = 0
    for alpha, y, x in _cases():
        sub = TABLES[alpha]
        for go, ge in GAPS3:
            Y, X = _hdr(y), _hdr(x)
            res = oo.align(Y, X, sub, go, ge)
            y_in_x = so.score(Y, X, sub, go, ge)[0]
            x_in_y = so.score(X, Y, sub.T.copy(), go, ge)[0]
            assert res[0] >= 0 and res[0] >= y_in_x and res[0] >= x_in_y
            # the optimum a containment: Y wholly inside X, or X wholly inside Y
            if res[1] == 0 and res[3] == len(y):
                assert res[0] == y_in_x
                contained += 1
            if res[2] == 0 and res[4] == len(x):
                assert res[0] == x_in_y
                contained += 1
            assert oo.replay(Y, X, sub, go, ge, res) == res[0]
            assert res[1] == 0 or res[2] == 0
            # the int64 fill agrees
            assert oo.align(Y, X, sub, go, ge, wide=True) == res
    assert contained >= 20


def test_tie_rule_on_hand_written_cases():
    sub = np.where(np.eye(4, dtype=bool), 2, -3).astype(np.int32)
    A, B = [0, 1, 0, 0], [2, 3, 3, 2]
    # Y = A + B, X = B + A, a constant match score: Y's tail B on X's head (row R, column |B|) and X's
    # tail A on Y's head (row |A|, column C) both score 8; row R wins
    Y, X = _hdr(A + B), _hdr(B + A)
    assert oo.align(Y, X, sub, -5, -1) == (8, 4, 0, 8, 4, "4=")
    # identical sequences end at the corner (R, C)
    assert oo.align(Y, Y, sub, -5, -1) == (16, 0, 0, 8, 8, "8=")
    # an unrelated pair: 0 at (R, 0), an empty CIGAR
    assert oo.align(_hdr([0, 0, 0]), _hdr([1, 1, 1, 1]), sub, -5, -1) == (0, 3, 0, 3, 0, "")
    # empty sides
    assert oo.align(_hdr([]), _hdr([1, 1]), sub, -5, -1) == (0, 0, 0, 0, 0, "")
    assert oo.align(_hdr([1, 1]), _hdr([]), sub, -5, -1) == (0, 2, 0, 2, 0, "")
    # a maximum on column C only: X's tail on Y's head, the smallest row that attains it
    assert oo.align(_hdr([2, 3, 0, 0]), _hdr([1, 1, 2, 3]), sub, -5, -1) == (4, 0, 2, 2, 4, "2=")
    # two equal maxima on row R: the smaller column
    assert oo.align(_hdr([2, 3]), _hdr([2, 3, 1, 2, 3, 1]), sub, -5, -1) == (4, 0, 0, 2, 2, "2=")
