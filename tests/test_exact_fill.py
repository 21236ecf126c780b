"""tests/_exact.py's reference for the NW-LG fill family, and the oracle (oracle/nw_oracle.c, int32 C)
held against it on every input tests/test_gpu_fill_value_ranges.py expects an answer for.  fill_lg is
pinned by a plain triple loop, homopolymer_lg by fill_lg, headers_lg by its own definition; the two
65k pairs of the GPU file are covered by the closed form alone."""
import numpy as np
import pytest

import oracle
from tests import _exact
from tests import test_gpu_fill_value_ranges as V


def triple_loop(Y, X, sub, g):
    R, C = len(Y) - 1, len(X) - 1
    H = [[0] * (C + 1) for _ in range(R + 1)]
    for j in range(C + 1):
        H[0][j] = j * g
    for i in range(1, R + 1):
        H[i][0] = i * g
        for j in range(1, C + 1):
            H[i][j] = max(H[i - 1][j - 1] + int(sub[Y[i]][X[j]]), H[i - 1][j] + g, H[i][j - 1] + g)
    return np.array(H, dtype=np.int64)


@pytest.mark.parametrize("g", [-11, 0, 5, -8000])
@pytest.mark.parametrize("R,C", [(0, 0), (0, 5), (4, 0), (1, 1), (7, 13), (40, 23)])
def test_fill_lg_is_the_recurrence(R, C, g):
    t = V.table(20)
    t[2, 9], t[9, 2] = 16767, -30000
    Y, X = V.random_pair(R, C, 20, 3 * R + C)
    assert np.array_equal(_exact.fill_lg(Y, X, t, g), triple_loop(Y, X, t, g))
    Y, X = V.related_pair(R, C, 20, 5 * R + C)
    assert np.array_equal(_exact.fill_lg(Y, X, t, g), triple_loop(Y, X, t, g))


def test_fill_lg_reads_rows_as_seqy_letters():
    """One entry off the diagonal of the table: only (seqY letter 1, seqX letter 2) scores."""
    t = np.zeros((3, 3), np.int64)
    t[1, 2] = 9
    H = _exact.fill_lg([0, 1], [0, 2], t, -1)
    assert H.tolist() == [[0, -1], [-1, 9]]
    assert _exact.fill_lg([0, 2], [0, 1], t, -1).tolist() == [[0, -1], [-1, 0]]


@pytest.mark.parametrize("R,C,tBy,tBx", [(1, 1, 4, 4), (9, 14, 4, 4), (8, 8, 4, 2), (0, 3, 4, 4), (5, 0, 2, 4)])
def test_headers_lg_layout(R, C, tBy, tBx):
    """Tile-major, element 0 the corner, the padding letter 0: word by word from the padded matrix."""
    t = V.table(4)
    Y, X = V.random_pair(R, C, 4, 11 * R + C)
    hrow, hcol = _exact.headers_lg(Y, X, t, -3, tBy, tBx)
    trows, tcols = max(1, -(-R // tBy)), max(1, -(-C // tBx))
    Yp = np.concatenate([Y, np.zeros(trows * tBy - R, np.int64)])
    Xp = np.concatenate([X, np.zeros(tcols * tBx - C, np.int64)])
    H = triple_loop(Yp, Xp, t, -3)
    assert hrow.shape == (trows * tcols * (1 + tBx),) and hcol.shape == (trows * tcols * (1 + tBy),)
    for iT in range(trows):
        for jT in range(tcols):
            k = iT * tcols + jT
            assert hrow[k * (1 + tBx):(k + 1) * (1 + tBx)].tolist() == H[iT * tBy, jT * tBx:(jT + 1) * tBx + 1].tolist()
            assert hcol[k * (1 + tBy):(k + 1) * (1 + tBy)].tolist() == H[iT * tBy:(iT + 1) * tBy + 1, jT * tBx].tolist()


@pytest.mark.parametrize("v,g", [(16767, -8000), (0, 0), (5, 0), (0, -3), (11, -11)])
@pytest.mark.parametrize("R,C", [(1, 1), (9, 14), (14, 9), (16, 16)])
def test_homopolymer_closed_form(R, C, v, g):
    hp = _exact.homopolymer_lg(R, C, v, g)
    zeros = lambda n: np.zeros(n + 1, np.int64)
    H = _exact.fill_lg(zeros(R), zeros(C), [[v]], g)
    assert np.array_equal(hp.rows(0, R + 1), H) and hp.cost() == H[R, C]
    assert np.array_equal(hp.rows(3, 3), H[3:3]) and np.array_equal(hp.rows(1, 2), H[1:2])
    for tBy, tBx in ((4, 4), (8, 2)):
        hrow, hcol = hp.headers(tBy, tBx)
        want_r, want_c = _exact.headers_lg(zeros(R), zeros(C), [[v]], g, tBy, tBx)
        assert np.array_equal(hrow, want_r) and np.array_equal(hcol, want_c)


def test_the_65k_pairs_are_where_the_gpu_file_says():
    """Inside, past and rectangular: the shifted value 32767 min(i, j) against 2^31, the true H far from it."""
    q = V.ACC_V - 2 * V.ACC_G
    assert q == 32767 and q * V.ACC_INSIDE < 2 ** 31 <= q * V.ACC_PAST
    for R, C in [(V.ACC_INSIDE,) * 2, (V.ACC_PAST,) * 2, V.ACC_RECT]:
        hp = _exact.homopolymer_lg(R, C, V.ACC_V, V.ACC_G)
        assert 0 < hp.cost() < 2 ** 31 and hp.at(R, 0) == R * V.ACC_G > -2 ** 31 and hp.at(0, C) > -2 ** 31


def test_cases_reach_their_edges():
    """Every edge case has its extreme exactly where it says, the maximum's run on the optimal path (the
    cost falls by more than half the run's worth when the entry is an ordinary one), the minimum's letter
    pair in many cells."""
    names = [c.name for c in V.all_cases()]
    assert len(set(names)) == len(names) and set(V.BATCH_CASES) | set(V.CHECK_CASES) <= set(names)
    for c in V.edge_cases():
        kind, edge = ("max", c.qmax) if c.plant else ("min", c.qmin)
        assert c.name.startswith("%s%d-" % (kind, edge))
        Y, X = c.pair()
        if kind == "max":
            a, b = V.MAX_PAIR
            run = min(V.RUN, min(c.shape[:2]) // 2)
            base = c.sub.copy()
            base[a, b] = 11
            gain = _exact.fill_lg(Y, X, c.sub, c.g)[-1, -1] - _exact.fill_lg(Y, X, base, c.g)[-1, -1]
            assert gain > (run // 2) * (int(c.sub[a, b]) - 11), (c, gain)
        else:
            a, b = V.MIN_PAIR
            assert ((Y[1:, None] == a) & (X[None, 1:] == b)).sum() >= 100, c


_INPUTS = list(V.answered_inputs())


@pytest.mark.parametrize("k", range(len(_INPUTS)), ids=lambda k: "%s-%dx%d" % (_INPUTS[k][0].name, len(_INPUTS[k][1]) - 1,
                                                                               len(_INPUTS[k][2]) - 1))
def test_oracle_equals_exact(k):
    """oracle.fill_full, fill_full_mt and sparse_headers word for word against fill_lg and headers_lg; for
    g <= 0 the score reference's global linear score is the fill's last cell."""
    c, Y, X, tBx = _INPUTS[k]
    Yp, Xp, trows, tcols = _exact.pad_to_tiles(Y, X, V.TBY, tBx)
    Hp = _exact.fill_lg(Yp, Xp, c.sub, c.g)
    H = Hp[:len(Y), :len(X)]
    assert np.abs(Hp).max() < 2 ** 31
    if len(Y) * len(X) <= 1 << 20:  # the padding changes nothing inside
        assert np.array_equal(_exact.fill_lg(Y, X, c.sub, c.g), H)
    S, cost = oracle.fill_full(Y, X, c.sub, c.g)
    assert np.array_equal(S, H) and cost == H[-1, -1]
    S, cost = oracle.fill_full_mt(Y, X, c.sub, c.g)
    assert np.array_equal(S, H) and cost == H[-1, -1]
    hrow, hcol = _exact.headers_of(Hp, trows, tcols, V.TBY, tBx)
    ohr, ohc, otr, otc, ocost = oracle.sparse_headers(Y, X, c.sub, c.g, V.TBY, tBx)
    assert (otr, otc, ocost) == (trows, tcols, H[-1, -1])
    assert np.array_equal(ohr, hrow) and np.array_equal(ohc, hcol)
    if c.g <= 0:
        assert _exact.score(Y, X, c.sub, c.g, c.g, False)[0] == H[-1, -1]
