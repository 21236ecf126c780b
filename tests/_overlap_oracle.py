"""Oracle of the long pairs' overlap (dovetail) mode (gsa_score_overlap_dev, gsa_align_pair_overlap_dev;
DESIGN.md 2.2m): a plain restatement of the semantics in include/gsa.h, in the manner of
tests/_semi_oracle.py.  A suffix of either sequence against a prefix of the other, or either within the
other: all four overhangs are free.

  row 0:      H(0, j) = 0, E = F = minus infinity, j = 0 ... C
  column 0:   H(i, 0) = 0, E = F = minus infinity, i = 0 ... R
  inside:     the Gotoh recurrences, no zero floor
  score:      the largest H among row R (j = 0 ... C) and column C (i = 0 ... R)
  end cell:   (R, the smallest j that attains it) if row R attains it, else (the smallest such i, C)
  walk:       from the end cell in state H, by the rules of tests/_align_oracle.py (diagonal, then F,
              then E; a gap extended only when strictly better than opening), until i = 0 or j = 0.

The matrices come from a few lines of C compiled once per session; the end-cell rule and the walk are
Python.  Nothing here knows of the kernels' keys, masks or codes.  Two fills: int32 cells with a finite
NEG as oracle/score_oracle.c has (exact far beyond the pairs the library takes), and int64 cells with
minus infinity at -2^62 for the inputs at the value-range guards: there |H| <= B < 2^31 (exact_for
asserts it), so no sum overflows and nothing that comes from minus infinity reaches a true value."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np

NEG = -(1 << 29)
NEG64 = -(1 << 62)

_SRC = r"""
#include <stdint.h>
#define FILL(NAME, T, NEGV)                                                                            \
    void NAME(const int32_t* y, int64_t R, const int32_t* x, int64_t C, const T* subst, int32_t n,    \
              T go, T ge, T* H, T* E, T* F)                                                            \
    {                                                                                                  \
        const int64_t W = C + 1;                                                                       \
        for (int64_t j = 0; j <= C; j++)                                                               \
        {                                                                                              \
            H[j] = 0;                                                                                  \
            E[j] = NEGV;                                                                               \
            F[j] = NEGV;                                                                               \
        }                                                                                              \
        for (int64_t i = 1; i <= R; i++)                                                               \
        {                                                                                              \
            H[i * W] = 0;                                                                              \
            E[i * W] = NEGV;                                                                           \
            F[i * W] = NEGV;                                                                           \
            for (int64_t j = 1; j <= C; j++)                                                           \
            {                                                                                          \
                const T e1 = E[i * W + j - 1] + ge, e2 = H[i * W + j - 1] + go;                       \
                const T f1 = F[(i - 1) * W + j] + ge, f2 = H[(i - 1) * W + j] + go;                   \
                const T e = e1 >= e2 ? e1 : e2, f = f1 >= f2 ? f1 : f2;                                \
                const T d = H[(i - 1) * W + j - 1] + subst[(int64_t)y[i] * n + x[j]];                  \
                const T m = e >= f ? e : f;                                                            \
                E[i * W + j] = e;                                                                      \
                F[i * W + j] = f;                                                                      \
                H[i * W + j] = d >= m ? d : m;                                                         \
            }                                                                                          \
        }                                                                                              \
    }
FILL(fill_overlap, int32_t, (-(1 << 29)))
FILL(fill_overlap64, int64_t, (-((int64_t)1 << 62)))
"""

_LIB = None


def _lib():
    global _LIB
    if _LIB is None:
        d = tempfile.mkdtemp(prefix="overlap_oracle_")
        src, so = os.path.join(d, "fill_overlap.c"), os.path.join(d, "fill_overlap.so")
        with open(src, "w") as f:
            f.write(_SRC)
        subprocess.check_call([os.environ.get("CC", "cc"), "-O2", "-shared", "-fPIC", "-o", so, src])
        _LIB = ctypes.CDLL(so)
        vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
        _LIB.fill_overlap.restype = None
        _LIB.fill_overlap.argtypes = [vp, i64, vp, i64, vp, i32, i32, i32, vp, vp, vp]
        _LIB.fill_overlap64.restype = None
        _LIB.fill_overlap64.argtypes = [vp, i64, vp, i64, vp, i32, i64, i64, vp, vp, vp]
    return _LIB


def _c32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def _table(subst, dtype):
    sub = np.ascontiguousarray(subst, dtype=dtype)
    n = int(round(np.sqrt(sub.size)))
    return sub.reshape(n, n), n


def matrices(seqY, seqX, subst, go, ge, wide=False):
    """(H, E, F), each (R + 1) x (C + 1); the sequences with the header element in front.  wide: int64."""
    y, x = _c32(seqY), _c32(seqX)
    dt = np.int64 if wide else np.int32
    sub, n = _table(subst, dt)
    R, C = len(y) - 1, len(x) - 1
    H, E, F = (np.empty((R + 1, C + 1), dt) for _ in range(3))
    fn = _lib().fill_overlap64 if wide else _lib().fill_overlap
    fn(y.ctypes.data, R, x.ctypes.data, C, sub.ctypes.data, n, go, ge, H.ctypes.data, E.ctypes.data, F.ctypes.data)
    return H, E, F


def end_cell(H):
    """(score, i_end, j_end) by the header's rule."""
    R, C = H.shape[0] - 1, H.shape[1] - 1
    best = max(int(H[R].max()), int(H[:, C].max()))
    if int(H[R].max()) == best:
        return best, R, int(np.argmax(H[R]))
    return best, int(np.argmax(H[:, C])), C


def score(seqY, seqX, subst, go, ge, wide=False):
    """(score, i_end, j_end)."""
    return end_cell(matrices(seqY, seqX, subst, go, ge, wide)[0])


def _fold(ops):
    out, k = [], 0
    while k < len(ops):
        m = k
        while m < len(ops) and ops[m] == ops[k]:
            m += 1
        out.append("%d%s" % (m - k, ops[k]))
        k = m
    return "".join(out)


def align(seqY, seqX, subst, go, ge, wide=False):
    """(score, i_start, j_start, i_end, j_end, cigar)."""
    y, x = _c32(seqY), _c32(seqX)
    sub, _ = _table(subst, np.int64)
    H, E, F = matrices(y, x, sub, go, ge, wide)
    best, i_end, j_end = end_cell(H)
    i, j, state, ops = i_end, j_end, "H", []
    while i > 0 and j > 0:
        if state == "H":
            h = int(H[i, j])
            if h == int(H[i - 1, j - 1]) + int(sub[y[i], x[j]]):
                ops.append("=" if y[i] == x[j] else "X")
                i, j = i - 1, j - 1
            elif h == int(F[i, j]):
                state = "F"
            else:
                assert h == int(E[i, j]), (i, j, h)
                state = "E"
        elif state == "F":
            ops.append("I")
            state = "F" if int(F[i - 1, j]) + ge > int(H[i - 1, j]) + go else "H"
            i -= 1
        else:
            ops.append("D")
            state = "E" if int(E[i, j - 1]) + ge > int(H[i, j - 1]) + go else "H"
            j -= 1
    return best, i, j, i_end, j_end, _fold(ops[::-1])


def value_bound(R, C, sub, go, ge):
    """B = smax min(R, C) + |go| + (R + C) |ge| of the header."""
    smax = max(1, int(np.abs(np.asarray(sub, np.int64)).max()))
    return smax * min(R, C) + (-go) + (R + C) * (-ge)


def span(R, C, sub, go, ge):
    smax = max(1, int(np.abs(np.asarray(sub, np.int64)).max()))
    return (R + C) * (-ge) + (ge - go) + smax


def exact_for(R, C, sub, go, ge):
    """The int64 fill is exact: no |H| exceeds B, so with B < 2^31 every sum of true values stays far
    inside int64 and nothing that comes from -2^62 reaches -B."""
    B = value_bound(R, C, sub, go, ge)
    assert B < (1 << 31) and -B + go + ge > NEG64 // 2
    return B


def align64(seqY, seqX, subst, go, ge):
    exact_for(len(seqY) - 1, len(seqX) - 1, subst, go, ge)
    return align(seqY, seqX, subst, go, ge, wide=True)


def replay(seqY, seqX, subst, go, ge, res):
    """The score of the alignment `res` = (score, i_start, j_start, i_end, j_end, cigar) says, letter by
    letter; asserts that the CIGAR leads from the start cell to the end cell and names matches rightly."""
    y, x = _c32(seqY), _c32(seqX)
    sub, _ = _table(subst, np.int64)
    _, i, j, i_end, j_end, cigar = res
    total, num, prev = 0, "", ""
    for ch in cigar:
        if ch.isdigit():
            num += ch
            continue
        n = int(num)
        num = ""
        assert n > 0 and ch != prev
        prev = ch
        if ch in "=X":
            for _ in range(n):
                i, j = i + 1, j + 1
                assert (y[i] == x[j]) == (ch == "=")
                total += int(sub[y[i], x[j]])
        else:
            total += go + (n - 1) * ge
            if ch == "I":
                i += n
            else:
                assert ch == "D"
                j += n
    assert (i, j) == (i_end, j_end)
    return total
