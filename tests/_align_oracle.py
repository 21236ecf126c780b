"""Alignment oracle of the database search's traceback (gsa_align_db_dev): a plain
restatement of the semantics in include/gsa.h, written from the recurrences of oracle/score_oracle.c.
It fills the full H / E / F matrices (a few lines of C, compiled once per session with the host
compiler -- a per-cell Python loop is too slow for the GPU cases) and walks them with the stated rule:

  state H at (i, j): local and H == 0: stop; else H == H[i-1][j-1] + s: diagonal; else H == F[i][j]:
                     state F; else state E.  Global stops at (0, 0).
  state F at (i, j): a vertical move to (i-1, j); extended (stay in F) iff
                     F[i-1][j] + ge > H[i-1][j] + go, strictly; else opened (back to H).
  state E:           the same along the row.

CIGAR: forward order, run-length encoded: '=' / 'X' diagonal on equal / different letters, 'I' vertical
(a query letter only), 'D' horizontal (a subject letter only).  Nothing here knows the kernel's codes.

NEG is finite, as in oracle/score_oracle.c, and the same range holds: global pairs within
B + |go| < 2^29, the range the library accepts (tests/test_exact_reference.py)."""
import ctypes
import os
import re
import subprocess
import tempfile

import numpy as np

NEG = -(1 << 29)

_SRC = r"""
#include <stdint.h>
#define NEG (-(1 << 29))
static int32_t maxi(int32_t a, int32_t b) { return a >= b ? a : b; }
/* H, E, F: (R + 1) x (C + 1), row-major; y, x with the header element in front */
void fill_hef(const int32_t* y, int64_t R, const int32_t* x, int64_t C, const int32_t* subst, int32_t n,
              int32_t go, int32_t ge, int32_t local, int32_t* H, int32_t* E, int32_t* F)
{
    const int64_t W = C + 1;
    for (int64_t j = 0; j <= C; j++)
    {
        H[j] = (local || j == 0) ? 0 : (int32_t)(go + (j - 1) * ge);
        E[j] = (local || j == 0) ? NEG : H[j];
        F[j] = NEG;
    }
    for (int64_t i = 1; i <= R; i++)
    {
        H[i * W] = local ? 0 : (int32_t)(go + (i - 1) * ge);
        F[i * W] = local ? NEG : H[i * W];
        E[i * W] = NEG;
        for (int64_t j = 1; j <= C; j++)
        {
            const int32_t e = maxi(E[i * W + j - 1] + ge, H[i * W + j - 1] + go);
            const int32_t f = maxi(F[(i - 1) * W + j] + ge, H[(i - 1) * W + j] + go);
            int32_t h = maxi(maxi(H[(i - 1) * W + j - 1] + subst[(int64_t)y[i] * n + x[j]], e), f);
            if (local) h = maxi(h, 0);
            E[i * W + j] = e;
            F[i * W + j] = f;
            H[i * W + j] = h;
        }
    }
}
"""

_LIB = None


def _lib():
    global _LIB
    if _LIB is None:
        d = tempfile.mkdtemp(prefix="align_oracle_")
        src, so = os.path.join(d, "fill_hef.c"), os.path.join(d, "fill_hef.so")
        with open(src, "w") as f:
            f.write(_SRC)
        subprocess.check_call([os.environ.get("CC", "cc"), "-O2", "-shared", "-fPIC", "-o", so, src])
        _LIB = ctypes.CDLL(so)
        vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
        _LIB.fill_hef.restype = None
        _LIB.fill_hef.argtypes = [vp, i64, vp, i64, vp, i32, i32, i32, i32, vp, vp, vp]
    return _LIB


def _c32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def matrices(query, subject, subst, go, ge, local):
    """(H, E, F), each (R + 1) x (C + 1) int32; `query` and `subject` with the header element in front."""
    y, x, sub = _c32(query), _c32(subject), _c32(subst)
    n = int(round(np.sqrt(sub.size)))
    R, C = len(y) - 1, len(x) - 1
    H, E, F = (np.empty((R + 1, C + 1), np.int32) for _ in range(3))
    _lib().fill_hef(y.ctypes.data, R, x.ctypes.data, C, sub.ctypes.data, n, go, ge, int(bool(local)), H.ctypes.data,
                    E.ctypes.data, F.ctypes.data)
    return H, E, F


def _fold(ops):
    out, k = [], 0
    while k < len(ops):
        m = k
        while m < len(ops) and ops[m] == ops[k]:
            m += 1
        out.append("%d%s" % (m - k, ops[k]))
        k = m
    return "".join(out)


def align(query, subject, subst, go, ge, local, want_path=False):
    """(score, i_start, j_start, i_end, j_end, cigar); with want_path also the list of (i, j, state)
    the walk visited, from the end cell backwards, and the matrices."""
    y, x = _c32(query), _c32(subject)
    sub = _c32(subst)
    n = int(round(np.sqrt(sub.size)))
    sub = sub.reshape(n, n)
    R, C = len(y) - 1, len(x) - 1
    H, E, F = matrices(y, x, sub, go, ge, local)
    if local:
        score = int(H.max())
        # the first maximal cell in row-major order; a score of 0: the cell (0, 0)
        i_end, j_end = (int(v) for v in np.unravel_index(int(np.argmax(H)), H.shape)) if score > 0 else (0, 0)
    else:
        score, i_end, j_end = int(H[R, C]), R, C
    i, j, state = i_end, j_end, "H"
    ops, path = [], []
    while True:
        path.append((i, j, state))
        if state == "H":
            h = int(H[i, j])
            if local and h == 0:
                break
            if not local and i == 0 and j == 0:
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
    res = (score, i, j, i_end, j_end, _fold(ops[::-1]))
    return res + (path, (H, E, F)) if want_path else res


def runs(cigar):
    """[(count, op)] of a CIGAR string."""
    assert re.fullmatch(r"(\d+[=XID])*", cigar), cigar
    return [(int(c), op) for c, op in re.findall(r"(\d+)([=XID])", cigar)]


def rescore(cigar, query, subject, i_start, j_start, subst, go, ge):
    """Replay a CIGAR from (i_start, j_start): (score, i_end, j_end).  Every '=' must sit on equal
    letters and every 'X' on different ones; adjacent runs must differ; a run of L gap letters costs
    go + (L - 1) ge."""
    y, x = _c32(query), _c32(subject)
    sub = _c32(subst)
    n = int(round(np.sqrt(sub.size)))
    sub = sub.reshape(n, n)
    i, j, score, last = i_start, j_start, 0, None
    for count, op in runs(cigar):
        assert count > 0 and op != last, cigar
        last = op
        if op in "=X":
            for _ in range(count):
                i, j = i + 1, j + 1
                assert (y[i] == x[j]) == (op == "="), (i, j, op)
                score += int(sub[y[i], x[j]])
        else:
            score += go + (count - 1) * ge
            if op == "I":
                i += count
            else:
                j += count
    return score, i, j
