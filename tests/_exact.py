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
reads are on the diagonals d - 1 (rows i and i - 1) and d - 2 (row i - 1).

The NW-LG fill family (fill_lg, headers_lg, homopolymer_lg) has its own reference further down: the
whole matrix of the one-gap-cost recurrence, its tile headers, and a closed form for pairs too long
to fill."""
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


def fill_lg(Y, X, sub, g):
    """The (R + 1) x (C + 1) int64 matrix of the NW-LG fill, from the recurrence include/gsa.h states
    (UpdateScore): H[0][j] = j g, H[i][0] = i g, H[i][j] = max(H[i-1][j-1] + s(Y[i], X[j]),
    H[i-1][j] + g, H[i][j-1] + g), s = sub[Y letter][X letter], for g of any sign.
    A row at a time: with t[j] the best of the two moves out of row i - 1 (t[0] = i g), H[i][j] is the
    largest t[k] + (j - k) g over k <= j, a running maximum of t[k] - k g."""
    Y, X, S = np.asarray(Y, dtype=np.int64), np.asarray(X, dtype=np.int64), _table(sub)
    R, C, g = len(Y) - 1, len(X) - 1, int(g)
    jg = np.arange(C + 1, dtype=np.int64) * g
    H = np.empty((R + 1, C + 1), np.int64)
    H[0] = jg
    t = np.empty(C + 1, np.int64)
    for i in range(1, R + 1):
        up = H[i - 1]
        t[0] = i * g
        np.maximum(up[:-1] + S[Y[i], X[1:]], up[1:] + g, out=t[1:])
        H[i] = np.maximum.accumulate(t - jg) + jg
    return H


def pad_to_tiles(Y, X, tBy, tBx):
    """Both sequences padded with letter 0 to whole tiles (at least one): the pair whose matrix the
    sparse representation samples."""
    Y, X = np.asarray(Y, dtype=np.int64), np.asarray(X, dtype=np.int64)
    trows, tcols = max(1, -(-(len(Y) - 1) // tBy)), max(1, -(-(len(X) - 1) // tBx))
    Yp, Xp = np.zeros(trows * tBy + 1, np.int64), np.zeros(tcols * tBx + 1, np.int64)
    Yp[:len(Y)], Xp[:len(X)] = Y, X
    return Yp, Xp, trows, tcols


def headers_of(H, trows, tcols, tBy, tBx):
    """(tileHrowMat, tileHcolMat) of include/gsa.h out of the padded pair's matrix H: tile-major,
    k = tcols iT + jT, 1 + tBx resp. 1 + tBy values per tile, element 0 the tile's corner:
    hrow[k][e] = H[iT tBy][jT tBx + e], hcol[k][e] = H[iT tBy + e][jT tBx]."""
    rows = H[np.arange(trows) * tBy]                                      # trows x (Cp + 1)
    hrow = rows[:, np.arange(tcols)[:, None] * tBx + np.arange(tBx + 1)]  # trows x tcols x (1 + tBx)
    cols = H[:, np.arange(tcols) * tBx]                                   # (Rp + 1) x tcols
    hcol = cols[np.arange(trows)[:, None] * tBy + np.arange(tBy + 1)]     # trows x (1 + tBy) x tcols
    return hrow.reshape(-1), hcol.transpose(0, 2, 1).reshape(-1)


def headers_lg(Y, X, sub, g, tBy, tBx):
    """(tileHrowMat, tileHcolMat), int64, from fill_lg of the pair padded with letter 0."""
    Yp, Xp, trows, tcols = pad_to_tiles(Y, X, tBy, tBx)
    return headers_of(fill_lg(Yp, Xp, sub, g), trows, tcols, tBy, tBx)


class homopolymer_lg:
    """The fill of two runs of letter 0, R and C letters, with s(0, 0) = v >= 0 and g <= 0, in closed
    form: H[i][j] = v min(i, j) + g |i - j| (the diagonal as far as it goes, then one gap; no path does
    better since a diagonal step gains v >= 0 >= 2 g over two gap steps).  The padding letter is 0 too,
    so the form holds over the padded region.  Only rows, columns and headers are ever built."""

    def __init__(self, R, C, v, g):
        assert v >= 0 and g <= 0, (v, g)
        self.R, self.C, self.v, self.g = int(R), int(C), int(v), int(g)

    def at(self, i, j):
        """H at the (broadcast) int64 indices i, j."""
        i, j = np.asarray(i, dtype=np.int64), np.asarray(j, dtype=np.int64)
        return self.v * np.minimum(i, j) + self.g * np.abs(i - j)

    def cost(self):
        return int(self.at(self.R, self.C))

    def rows(self, i0, i1):
        """Rows i0 .. i1 - 1 of the unpadded matrix, (i1 - i0) x (C + 1)."""
        return self.at(np.arange(i0, i1)[:, None], np.arange(self.C + 1)[None, :])

    def headers(self, tBy, tBx):
        """(tileHrowMat, tileHcolMat), int64, laid out as headers_of lays them out."""
        trows, tcols = max(1, -(-self.R // tBy)), max(1, -(-self.C // tBx))
        iT, jT = np.arange(trows)[:, None, None], np.arange(tcols)[None, :, None]
        hrow = self.at(iT * tBy, jT * tBx + np.arange(tBx + 1)[None, None, :])
        hcol = self.at(iT * tBy + np.arange(tBy + 1)[None, None, :], jT * tBx)
        return hrow.reshape(-1), hcol.reshape(-1)


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
