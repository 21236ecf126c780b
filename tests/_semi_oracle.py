"""Oracle of the semi-global database search (gsa_score_db_multi_semi_dev, gsa_align_db_multi_semi_dev;
DESIGN.md 2.2h): a plain restatement of the semantics in include/gsa.h, in the manner of
tests/_align_oracle.py.  The whole query is aligned; the subject's head and tail are free.

  row 0:     H(0, j) = 0, E(0, j) = F(0, j) = minus infinity, j = 0 ... C
  column 0:  H(i, 0) = F(i, 0) = go + (i - 1) ge, E(i, 0) = minus infinity, i >= 1
  inside:    the Gotoh recurrences, no zero floor
  score:     max over j = 0 ... C of H(R, j); end cell (R, the smallest such j)
  walk:      from the end cell in state H, by the rules of tests/_align_oracle.py (diagonal, then F,
             then E; a gap extended only when strictly better than opening), until i = 0.

The matrices come from a few lines of C compiled once per session; the walk is Python.  Nothing here
knows of the kernels' keys or codes.  NEG is finite, as in oracle/score_oracle.c; the library takes
pairs within B < 2^18 only, far inside the range where that is exact."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np

NEG = -(1 << 29)

_SRC = r"""
#include <stdint.h>
#define NEG (-(1 << 29))
static int32_t maxi(int32_t a, int32_t b) { return a >= b ? a : b; }
/* H, E, F: (R + 1) x (C + 1), row-major; y, x with the header element in front */
void fill_semi(const int32_t* y, int64_t R, const int32_t* x, int64_t C, const int32_t* subst, int32_t n,
               int32_t go, int32_t ge, int32_t* H, int32_t* E, int32_t* F)
{
    const int64_t W = C + 1;
    for (int64_t j = 0; j <= C; j++)
    {
        H[j] = 0;
        E[j] = NEG;
        F[j] = NEG;
    }
    for (int64_t i = 1; i <= R; i++)
    {
        H[i * W] = (int32_t)(go + (i - 1) * ge);
        F[i * W] = H[i * W];
        E[i * W] = NEG;
        for (int64_t j = 1; j <= C; j++)
        {
            const int32_t e = maxi(E[i * W + j - 1] + ge, H[i * W + j - 1] + go);
            const int32_t f = maxi(F[(i - 1) * W + j] + ge, H[(i - 1) * W + j] + go);
            E[i * W + j] = e;
            F[i * W + j] = f;
            H[i * W + j] = maxi(maxi(H[(i - 1) * W + j - 1] + subst[(int64_t)y[i] * n + x[j]], e), f);
        }
    }
}
"""

_LIB = None


def _lib():
    global _LIB
    if _LIB is None:
        d = tempfile.mkdtemp(prefix="semi_oracle_")
        src, so = os.path.join(d, "fill_semi.c"), os.path.join(d, "fill_semi.so")
        with open(src, "w") as f:
            f.write(_SRC)
        subprocess.check_call([os.environ.get("CC", "cc"), "-O2", "-shared", "-fPIC", "-o", so, src])
        _LIB = ctypes.CDLL(so)
        vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
        _LIB.fill_semi.restype = None
        _LIB.fill_semi.argtypes = [vp, i64, vp, i64, vp, i32, i32, i32, vp, vp, vp]
    return _LIB


def _c32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def matrices(query, subject, subst, go, ge):
    """(H, E, F), each (R + 1) x (C + 1) int32; `query` and `subject` with the header element in front."""
    y, x, sub = _c32(query), _c32(subject), _c32(subst)
    n = int(round(np.sqrt(sub.size)))
    R, C = len(y) - 1, len(x) - 1
    H, E, F = (np.empty((R + 1, C + 1), np.int32) for _ in range(3))
    _lib().fill_semi(y.ctypes.data, R, x.ctypes.data, C, sub.ctypes.data, n, go, ge, H.ctypes.data, E.ctypes.data,
                     F.ctypes.data)
    return H, E, F


def score(query, subject, subst, go, ge):
    """(score, i_end, j_end): the best of row R at its smallest column; an empty query: (0, 0, 0)."""
    H, _, _ = matrices(query, subject, subst, go, ge)
    R = H.shape[0] - 1
    return int(H[R].max()), R, int(np.argmax(H[R]))


def _fold(ops):
    out, k = [], 0
    while k < len(ops):
        m = k
        while m < len(ops) and ops[m] == ops[k]:
            m += 1
        out.append("%d%s" % (m - k, ops[k]))
        k = m
    return "".join(out)


def align(query, subject, subst, go, ge):
    """(score, i_start, j_start, i_end, j_end, cigar); i_start is 0."""
    y, x = _c32(query), _c32(subject)
    sub = _c32(subst)
    n = int(round(np.sqrt(sub.size)))
    sub = sub.reshape(n, n)
    H, E, F = matrices(y, x, sub, go, ge)
    R = len(y) - 1
    best, i_end, j_end = int(H[R].max()), R, int(np.argmax(H[R]))
    i, j, state = i_end, j_end, "H"
    ops = []
    while i > 0:
        if state == "H":
            h = int(H[i, j])
            if j > 0 and h == int(H[i - 1, j - 1]) + int(sub[y[i], x[j]]):
                ops.append("=" if y[i] == x[j] else "X")
                i, j = i - 1, j - 1
            elif h == int(F[i, j]):
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
    return best, 0, j, i_end, j_end, _fold(ops[::-1])
