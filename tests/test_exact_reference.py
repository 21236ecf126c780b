"""tests/_exact.py against the oracles the rest of the suite compares with (oracle.score_ag, plain and
tiled, and tests/_align_oracle.py), on the CPU.  The oracles stand in for minus infinity with -2^29, as
the kernels do; _exact does not.  They must agree wherever a test expects an answer -- the six modes on
small shapes, and every input of tests/test_gpu_value_ranges.py on the accepted side of a guard -- and
the recorded cases at the bottom show where they stop agreeing: global alignments past
B + |go| < 2^29, which gsa_score.hip's score_ranges now rejects."""
import numpy as np
import pytest

import oracle
from tests import _align_oracle as ao
from tests import _exact
from tests import test_gpu_value_ranges as vr
from tests._data import random_pair, related_pair
from tests.test_gpu_score import MODES
from tests.test_score_oracle import py_score

SMALL = [(0, 0), (0, 5), (6, 0), (1, 1), (17, 23), (40, 31)]


def _against_oracles(Y, X, sub, go, ge, local, what):
    """The three oracles' scores and end cells equal _exact's; the align oracle's CIGAR spans its cells
    and scores what it reports."""
    want = vr.exact(Y, X, sub, go, ge, local)
    assert oracle.score_ag(Y, X, sub, go, ge, local) == want, what
    assert oracle.score_ag(Y, X, sub, go, ge, local, mt=True, blocksz=64, nthreads=2) == want, what
    score, i0, j0, i1, j1, cigar = ao.align(Y, X, sub, go, ge, local)
    assert (score, i1, j1) == want, what
    assert _exact.rescore(cigar, Y, X, sub, go, ge, i0, j0, i1, j1) == score, what
    if not local:
        assert (i0, j0) == (0, 0), what


@pytest.mark.parametrize("go,ge,local", MODES)
def test_six_modes_on_small_shapes(golden, go, ge, local):
    for R, C in SMALL:
        Y, X = random_pair(R, C, 100 * R + C + 7)
        _against_oracles(Y, X, golden.blosum62, go, ge, local, (R, C))
        assert py_score(Y, X, golden.blosum62, go, ge, local) == vr.exact(Y, X, golden.blosum62, go, ge, local), (R, C)
    Y, X = related_pair(60, 5)
    _against_oracles(Y, X, golden.blosum62, go, ge, local, "related")
    Y, X = random_pair(300, 257, 11)  # several tiles of the tiled oracle
    _against_oracles(Y, X, golden.blosum62, go, ge, local, (300, 257))


def test_linear_global_is_the_reference_cost(golden):
    """go == ge, global: the NW-LG cost of oracle.fill_full, which is pinned to the reference's answers."""
    n = 0
    for _, Y, X in golden.pairs("pair_debug.txt")[:40]:
        if (len(Y) - 1) * (len(X) - 1) <= 300000:
            assert _exact.score(Y, X, golden.blosum62, -11, -11, False)[0] == oracle.fill_full(Y, X, golden.blosum62, -11)[1]
            n += 1
    assert n >= 5


_TAGS = ["gaps", "gaps-past", "gaps-batch", "int16-top", "int16-over", "int16-bottom", "int16-under", "sw", "key-score",
         "key-column", "trace"]
_CASES = {}


@pytest.mark.parametrize("tag", _TAGS)
def test_value_range_inputs(tag):
    """Every table / gap / shape combination tests/test_gpu_value_ranges.py expects an answer for."""
    if not _CASES:
        for c in vr.accepted_cases():
            _CASES.setdefault(c[0], []).append(c[1:])
        assert sorted(_CASES) == sorted(_TAGS)
    for n, (Y, X, sub, go, ge, local) in enumerate(_CASES[tag]):
        _against_oracles(Y, X, sub, go, ge, local, (tag, n, len(Y) - 1, len(X) - 1, go, ge, local))


def test_rescore_refuses_a_wrong_cigar(golden):
    sub = golden.blosum62
    Y = np.array([0, 3, 4, 5, 6], np.int32)
    X = np.array([0, 3, 9, 6], np.int32)
    n = int(round(np.sqrt(np.asarray(sub).size)))
    S = np.asarray(sub).reshape(n, n)
    assert _exact.rescore("1=1X1I1=", Y, X, sub, -11, -1, 0, 0, 4, 3) == int(S[3, 3] + S[4, 9] + S[6, 6]) - 11
    assert _exact.rescore("1=2I1D1=", Y, X, sub, -11, -1, 0, 0, 4, 3) == int(S[3, 3] + S[6, 6]) - 11 - 1 - 11
    assert _exact.rescore("1X", Y, X, sub, -5, -2, 1, 1, 2, 2) == int(S[4, 9])
    assert _exact.rescore("", Y, X, sub, -5, -2, 0, 0, 0, 0) == 0
    for bad, cells in [("1=1X1I", (0, 0, 4, 3)),       # ends at (3, 2)
                       ("1=1X1I1=", (0, 0, 4, 4)),     # the reported end is another cell
                       ("1=1X1I1=", (1, 0, 4, 3)),     # the reported start is another cell
                       ("2=1I1=", (0, 0, 4, 3)),       # '=' on 4, 9
                       ("1=1X1I1X", (0, 0, 4, 3)),     # 'X' on 6, 6
                       ("1=1X1I1=5D", (0, 0, 4, 8)),   # leaves the matrix
                       ("1=0X1I1=", (0, 0, 4, 3)),
                       ("1=1Y", (0, 0, 2, 2))]:
        with pytest.raises(ValueError):
            _exact.rescore(bad, Y, X, sub, -11, -1, *cells)


# R, C, go, ge, the exact score, what the int32 recurrence with -2^29 for minus infinity gives
RECORDED = [(300, 10, -2000010, -2000000, -579999935, -538870873),
            (10, 300, -2000010, -2000000, -579999940, -538870881),
            (400, 8, -3000000, -1400000, -550399956, -538270884),
            (300, 10, -2000000, -2000000, -579999890, -538870873),
            (300, 300, -1500010, -1500000, 1066, 1066)]


@pytest.mark.parametrize("R,C,go,ge,right,sentinel", RECORDED)
def test_recorded_sentinel_cases(R, C, go, ge, right, sentinel):
    """Global alignments the library accepted while its bound was B < 2^30 (all five have B below it),
    on the 20-letter table of values in -4 .. 11 and random_pair(R, C, 7 R + C).  In the first four the
    true H + go of a row's or column's first gap falls below -2^29 + ge, the sentinel wins, and both
    oracles return a value a little under -2^29; the fifth has no gap on its best path.  The exact
    values are _exact's, and a literal Gotoh on Python ints with float('-inf') (py_score) agrees.  The
    oracles are left as they are and asserted to differ: they are exact within the range the library
    accepts (test_value_range_inputs), and B + |go| >= 2^29 for all five: the bound is sufficient, not
    necessary, and a pair like the fifth is the price."""
    t = vr.table20()
    Y, X = random_pair(R, C, 7 * R + C)
    assert vr.bound(R, C, 11, go, ge, 0) < vr.LOCAL_LIMIT
    assert vr.bound(R, C, 11, go, ge, 1) >= vr.GLOBAL_LIMIT  # rejected now, the fifth with them
    assert _exact.score(Y, X, t, go, ge, False) == (right, R, C)
    assert py_score(Y, X, t, go, ge, False) == (right, R, C)
    assert oracle.score_ag(Y, X, t, go, ge, False) == (sentinel, R, C)
    assert oracle.score_ag(Y, X, t, go, ge, False, mt=True, blocksz=64, nthreads=2) == (sentinel, R, C)
    assert int(ao.matrices(Y, X, t, go, ge, False)[0][R, C]) == sentinel  # (its walk loses its way there)
