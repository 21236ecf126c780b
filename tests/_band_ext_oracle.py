"""Oracle of the banded extension alignment (gsa_score_band_ext_dev, gsa_align_pair_band_ext_dev;
DESIGN.md 2.2r): a plain restatement of the semantics in include/gsa.h over the matrices of
tests/_band_oracle.py, which are the global banded call's.

  values:    tests/_band_oracle.matrices -- H(0, 0) = 0, row 0 E only, column 0 F only, Gotoh inside,
             minus infinity outside lo <= j - i <= hi
  validity:  lo <= 0 <= hi; the band need not hold (R, C)
  score:     the maximum of H over the cells of the band (never negative)
  end cell:  the first maximal cell in row-major order
  walk:      from the end cell in state H, by the rules of tests/_band_oracle.align (diagonal, then F,
             then E; a gap extended only when strictly better than opening), until (0, 0)

Nothing here knows of strips, lanes, codes or trimming: `align` fills the whole (R + 1) x (C + 1)
rectangle."""
import numpy as np

from tests import _band_oracle as bo


def valid(lo, hi):
    """The band holds (0, 0)."""
    return lo <= 0 <= hi


def clamp(R, C, lo, hi):
    return max(lo, -R), min(hi, C)


def trim(R, C, lo, hi):
    """(R', C'): the rows and columns the (clamped) band reaches."""
    lo, hi = clamp(R, C, lo, hi)
    return min(R, C - lo), min(C, R + hi)


def maxima(H, lo, hi):
    """(best, cells): the largest H of the band and all cells that hold it, in row-major order."""
    R, C = H.shape[0] - 1, H.shape[1] - 1
    d = np.arange(C + 1)[None, :] - np.arange(R + 1)[:, None]
    inband = (d >= lo) & (d <= hi)
    best = int(H[inband].max())
    cells = [(int(i), int(j)) for i, j in np.argwhere(inband & (H == best))]
    return best, cells


def align(query, subject, subst, go, ge, lo, hi, wide=False, want_cells=False):
    """(score, i_start, j_start, i_end, j_end, cigar); with want_cells also the list of all maximal
    cells in row-major order (the first is the end cell)."""
    y, x = bo._c32(query), bo._c32(subject)
    sub = bo._c32(subst)
    n = int(round(np.sqrt(sub.size)))
    sub = sub.reshape(n, n)
    assert valid(lo, hi), (lo, hi)
    H, E, F = bo.matrices(y, x, sub, go, ge, lo, hi, wide)
    best, cells = maxima(H, lo, hi)
    assert best >= 0
    ie, je = cells[0]
    i, j, state = ie, je, "H"
    ops = []
    while True:
        assert lo <= j - i <= hi, (i, j)
        if state == "H":
            h = int(H[i, j])
            if i == 0 and j == 0:
                break
            if i > 0 and j > 0 and h == int(H[i - 1, j - 1]) + int(sub[y[i], x[j]]):
                ops.append("=" if y[i] == x[j] else "X")
                i, j = i - 1, j - 1
            elif i > 0 and h == int(F[i, j]):
                state = "F"
            else:
                assert j > 0 and h == int(E[i, j]), (i, j, h)
                state = "E"
        elif state == "F":
            ops.append("I")
            state = "F" if int(F[i - 1, j]) + ge > int(H[i - 1, j]) + go else "H"
            i -= 1
        else:
            ops.append("D")
            state = "E" if int(E[i, j - 1]) + ge > int(H[i, j - 1]) + go else "H"
            j -= 1
    res = (best, 0, 0, ie, je, bo._fold(ops[::-1]))
    return res + (cells,) if want_cells else res


def score(query, subject, subst, go, ge, lo, hi, wide=False):
    """(score, i_end, j_end)."""
    r = align(query, subject, subst, go, ge, lo, hi, wide)
    return r[0], r[3], r[4]


def certificate(R, C, lo, hi, subst, go, ge, S):
    """proved_optimal of include/gsa.h, for the band clamped to the whole pair."""
    lo, hi = clamp(R, C, lo, hi)
    pmax = max(0, int(np.max(subst)))
    if hi < C and S <= pmax * min(R, C - hi - 1) + go + hi * ge:
        return 0
    if lo > -R:
        a = 1 - lo
        if S <= pmax * min(C, R - a) + go + (a - 1) * ge:
            return 0
    return 1
