"""An exact reference for the score and alignment calls: NumPy int64, no compiled part, and a minus
infinity that no sum of table values and gap costs can reach.  Written from the semantics stated in
include/gsa.h and in the header of oracle/score_oracle.c, not from any implementation:

  E[i][j] = max(E[i][j-1] + ge, H[i][j-1] + go)      a gap consuming subject letters
  F[i][j] = max(F[i-1][j] + ge, H[i-1][j] + go)      a gap consuming query letters
  H[i][j] = max(H[i-1][j-1] + s(Y[i], X[j]), E[i][j], F[i][j]  [, 0 if local])

with go <= ge <= 0, so a gap of L letters costs go + (L - 1) ge.  Global: H[0][0] = 0, H[0][j] and
H[i][0] one gap from the corner, E[i][0] and F[0][j] minus infinity; the score is H[R][C] at (R, C).
Local: H = 0 on both borders, the score is the largest H (the border's zeros included), its end cell
the first one holding it in row-major order, (0, 0) for a score of 0.

Sequences carry their header element in front, as every entry point takes them: R = len(Y) - 1.

The sweep goes by anti-diagonals d = i + j, every array indexed by the row i: the three cells a cell
reads are on the diagonals d - 1 (rows i and i - 1) and d - 2 (row i - 1)."""
import re

import numpy as np

NINF = -(1 << 62)  # sums here stay within 2^45 or so: nothing climbs back from this


def _table(sub):
    sub = np.asarray(sub, dtype=np.int64)
    n = int(round(np.sqrt(sub.size)))
    return sub.reshape(n, n)


def score(Y, X, sub, go, ge, local):
    """(score, i_end, j_end) as Python ints."""
    assert go <= ge <= 0, (go, ge)
    Y, X, S = np.asarray(Y, dtype=np.int64), np.asarray(X, dtype=np.int64), _table(sub)
    R, C = len(Y) - 1, len(X) - 1
    go, ge = int(go), int(ge)

    def border(k):
        return 0 if (local or k == 0) else go + (k - 1) * ge

    if R == 0 or C == 0:
        return (0, 0, 0) if local else (border(R + C), R, C)
    h2 = np.full(R + 1, NINF, np.int64)  # H of diagonal d - 2
    h1 = np.full(R + 1, NINF, np.int64)  # H, E, F of diagonal d - 1
    e1 = np.full(R + 1, NINF, np.int64)
    f1 = np.full(R + 1, NINF, np.int64)
    h2[0] = 0                    # d = 0
    h1[0] = border(1)            # d = 1: the cells (0, 1) and (1, 0)
    h1[1] = border(1)
    best, bi, bj = 0, 0, 0
    for d in range(2, R + C + 1):
        lo, hi = max(1, d - C), min(R, d - 1)  # the rows of the diagonal's inner cells
        h0 = np.full(R + 1, NINF, np.int64)
        e0 = np.full(R + 1, NINF, np.int64)
        f0 = np.full(R + 1, NINF, np.int64)
        rows = slice(lo, hi + 1)
        up = slice(lo - 1, hi)
        e = np.maximum(e1[rows] + ge, h1[rows] + go)    # from (i, j - 1)
        f = np.maximum(f1[up] + ge, h1[up] + go)        # from (i - 1, j)
        s = S[Y[lo:hi + 1], X[d - hi:d - lo + 1][::-1]]
        h = np.maximum(np.maximum(h2[up] + s, e), f)
        if local:
            h = np.maximum(h, 0)
            m = int(h.max())
            if m > 0 and m >= best:
                i = lo + int(np.argmax(h))  # the smallest row on this diagonal holding m
                if m > best or (i, d - i) < (bi, bj):
                    best, bi, bj = m, i, d - i
        h0[rows], e0[rows], f0[rows] = h, e, f
        if d <= C:
            h0[0] = border(d)
        if d <= R:
            h0[d] = border(d)
        h2, h1, e1, f1 = h1, h0, e0, f0
    if local:
        return best, bi, bj
    return int(h1[R]), R, C


def runs(cigar):
    """[(count, op)] of a CIGAR string; ValueError for anything else."""
    if not re.fullmatch(r"(\d+[=XID])*", cigar):
        raise ValueError("not a CIGAR: %r" % (cigar,))
    return [(int(c), op) for c, op in re.findall(r"(\d+)([=XID])", cigar)]


def rescore(cigar, Y, X, sub, go, ge, i0, j0, i1, j1):
    """The score of the path `cigar` describes from the cell (i0, j0) to the cell (i1, j1): the aligned
    letters are Y[i0+1 .. i1] and X[j0+1 .. j1].  '=' / 'X' are diagonal moves on equal / different
    letters, 'I' consumes a query letter, 'D' a subject letter; consecutive gap letters of one kind are
    one gap.  ValueError when the lengths do not span the two cells, when a count is 0, when an '='
    sits on different letters or an 'X' on equal ones.  Knows no tie-break rule."""
    Y, X, S = np.asarray(Y, dtype=np.int64), np.asarray(X, dtype=np.int64), _table(sub)
    i, j, total, last = int(i0), int(j0), 0, None
    for count, op in runs(cigar):
        if count < 1:
            raise ValueError("empty run in %r" % (cigar,))
        if op in "=X":
            if i + count > len(Y) - 1 or j + count > len(X) - 1:
                raise ValueError("%r leaves the matrix at (%d, %d)" % (cigar, i, j))
            a, b = Y[i + 1:i + count + 1], X[j + 1:j + count + 1]
            bad = np.flatnonzero((a == b) != (op == "="))
            if bad.size:
                k = int(bad[0]) + 1
                raise ValueError("'%s' at (%d, %d) on letters %d, %d" % (op, i + k, j + k, a[k - 1], b[k - 1]))
            total += int(S[a, b].sum())
            i, j = i + count, j + count
        else:
            total += count * int(ge) if op == last else int(go) + (count - 1) * int(ge)
            if op == "I":
                i += count
            else:
                j += count
        last = op
    if (i, j) != (int(i1), int(j1)):
        raise ValueError("%r from (%d, %d) ends at (%d, %d), not (%d, %d)" % (cigar, i0, j0, i, j, i1, j1))
    if i > len(Y) - 1 or j > len(X) - 1:
        raise ValueError("%r leaves the matrix" % (cigar,))
    return total
