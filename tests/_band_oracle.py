"""Oracle of the banded alignment of one long pair (gsa_score_band_dev, gsa_align_pair_band_dev;
DESIGN.md 2.2p): a plain restatement of the semantics in include/gsa.h, in the manner of
tests/_semi_oracle.py.  Global alignment; only the cells with lo <= j - i <= hi exist.

  outside the band:  H = E = F = minus infinity, border cells included
  (0, 0):            H = 0
  row 0:             H(0, j) = E(0, j) = go + (j - 1) ge, F = minus infinity
  column 0:          H(i, 0) = F(i, 0) = go + (i - 1) ge, E = minus infinity
  inside:            the Gotoh recurrences
  score:             H(R, C); end cell (R, C), start cell (0, 0)
  walk:              from (R, C) in state H, by the rules of tests/_align_oracle.py (diagonal, then F,
                     then E; a gap extended only when strictly better than opening; row 0 is E only,
                     column 0 F only), until (0, 0)

The matrices come from a few lines of C compiled once per session; the walk is Python.  Nothing here
knows of strips, lanes or codes.  NEG is finite: -2^29 in the int32 matrices, exact within
B + |go| < 2^29; the int64 variant (NEG = -2^60) is the reference at and beyond the guards."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np

NEG = -(1 << 29)
NEG64 = -(1 << 60)

_SRC = r"""
#include <stdint.h>
#define FILL(NAME, T, NEGV)                                                                              \
    static T maxi_##NAME(T a, T b) { return a >= b ? a : b; }                                           \
    /* H, E, F: (R + 1) x (C + 1), row-major; y, x with the header element in front */                 \
    void NAME(const int32_t* y, int64_t R, const int32_t* x, int64_t C, const int32_t* subst, int32_t n, \
              int32_t go, int32_t ge, int64_t lo, int64_t hi, T* H, T* E, T* F)                        \
    {                                                                                                    \
        const int64_t W = C + 1;                                                                         \
        for (int64_t i = 0; i <= R; i++)                                                                 \
            for (int64_t j = 0; j <= C; j++)                                                             \
            {                                                                                            \
                const int64_t at = i * W + j;                                                            \
                T h = NEGV, e = NEGV, f = NEGV;                                                          \
                if (j - i >= lo && j - i <= hi)                                                          \
                {                                                                                        \
                    if (i == 0 && j == 0)                                                                \
                        h = 0;                                                                           \
                    else if (i == 0)                                                                     \
                        h = e = (T)go + (T)(j - 1) * ge;                                                 \
                    else if (j == 0)                                                                     \
                        h = f = (T)go + (T)(i - 1) * ge;                                                 \
                    else                                                                                 \
                    {                                                                                    \
                        e = maxi_##NAME(E[at - 1] + ge, H[at - 1] + go);                                 \
                        f = maxi_##NAME(F[at - W] + ge, H[at - W] + go);                                 \
                        h = maxi_##NAME(maxi_##NAME(H[at - W - 1] + subst[(int64_t)y[i] * n + x[j]], e), f); \
                    }                                                                                    \
                }                                                                                        \
                H[at] = h;                                                                               \
                E[at] = e;                                                                               \
                F[at] = f;                                                                               \
            }                                                                                            \
    }
FILL(fill_band, int32_t, (-(1 << 29)))
FILL(fill_band64, int64_t, (-((int64_t)1 << 60)))
"""

_LIB = None


def _lib():
    global _LIB
    if _LIB is None:
        d = tempfile.mkdtemp(prefix="band_oracle_")
        src, so = os.path.join(d, "fill_band.c"), os.path.join(d, "fill_band.so")
        with open(src, "w") as f:
            f.write(_SRC)
        subprocess.check_call([os.environ.get("CC", "cc"), "-O2", "-shared", "-fPIC", "-o", so, src])
        _LIB = ctypes.CDLL(so)
        vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
        for name in ("fill_band", "fill_band64"):
            fn = getattr(_LIB, name)
            fn.restype = None
            fn.argtypes = [vp, i64, vp, i64, vp, i32, i32, i32, i64, i64, vp, vp, vp]
    return _LIB


def _c32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def valid(R, C, lo, hi):
    """The band holds (0, 0) and (R, C)."""
    return lo <= hi and lo <= min(0, C - R) and hi >= max(0, C - R)


def clamp(R, C, lo, hi):
    return max(lo, -R), min(hi, C)


def matrices(query, subject, subst, go, ge, lo, hi, wide=False):
    """(H, E, F), each (R + 1) x (C + 1), int32 or (wide) int64; the sequences with the header element
    in front."""
    y, x, sub = _c32(query), _c32(subject), _c32(subst)
    n = int(round(np.sqrt(sub.size)))
    R, C = len(y) - 1, len(x) - 1
    H, E, F = (np.empty((R + 1, C + 1), np.int64 if wide else np.int32) for _ in range(3))
    fn = _lib().fill_band64 if wide else _lib().fill_band
    fn(y.ctypes.data, R, x.ctypes.data, C, sub.ctypes.data, n, go, ge, lo, hi, H.ctypes.data, E.ctypes.data,
       F.ctypes.data)
    return H, E, F


def score(query, subject, subst, go, ge, lo, hi, wide=False):
    """H(R, C) of the banded problem."""
    assert valid(len(query) - 1, len(subject) - 1, lo, hi)
    H, _, _ = matrices(query, subject, subst, go, ge, lo, hi, wide)
    return int(H[-1, -1])


def _fold(ops):
    out, k = [], 0
    while k < len(ops):
        m = k
        while m < len(ops) and ops[m] == ops[k]:
            m += 1
        out.append("%d%s" % (m - k, ops[k]))
        k = m
    return "".join(out)


def align(query, subject, subst, go, ge, lo, hi, wide=False, want_path=False):
    """(score, i_start, j_start, i_end, j_end, cigar); with want_path also the cells (i, j) the walk
    visited, from the end cell backwards."""
    y, x = _c32(query), _c32(subject)
    sub = _c32(subst)
    n = int(round(np.sqrt(sub.size)))
    sub = sub.reshape(n, n)
    R, C = len(y) - 1, len(x) - 1
    assert valid(R, C, lo, hi), (R, C, lo, hi)
    H, E, F = matrices(y, x, sub, go, ge, lo, hi, wide)
    i, j, state = R, C, "H"
    ops, path = [], []
    while True:
        path.append((i, j))
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
    res = (int(H[R, C]), 0, 0, R, C, _fold(ops[::-1]))
    return res + (path,) if want_path else res


def certificate(R, C, lo, hi, subst, go, ge, S):
    """proved_optimal of include/gsa.h, for the clamped band."""
    lo, hi = clamp(R, C, lo, hi)
    pmax = max(0, int(np.max(subst)))
    D = C - R
    if hi < C and S <= pmax * (C - hi - 1) + 2 * go + hi * ge + (hi - D) * ge:
        return 0
    if lo > -R:
        a = 1 - lo
        if S <= pmax * (R - a) + 2 * go + (a - 1) * ge + (a + D - 1) * ge:
            return 0
    return 1
