"""What the tests of the long pairs' semi-global mode share (gsa_score_semi_dev, gsa_align_pair_semi_dev;
DESIGN.md 2.2k): the gap models, pairs on the device, the oracle's alignment with its path, the window
and the plan of chunks computed independently of the library, and an int64 reference for the inputs at
the value-range guards.

The reference for every ordinary case is tests/_semi_oracle.py.  The int64 reference restates the
header's semantics (include/gsa.h, "Long pairs, semi-global mode") with 64-bit cells and minus infinity
at -2^62: with |H| <= B < 2^31 for every accepted or just-refused input of the tests, no sum overflows
and no term that comes from minus infinity can reach a true value, so it is exact there
(exact_for asserts the bound)."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np

from tests import _semi_oracle as so

# the issue's gap models: affine, linear, affine, and zero costs
GAPS = [(-11, -1), (-4, -4), (-5, -2), (0, 0), (-7, 0)]
FIELDS = ("score", "i_start", "j_start", "i_end", "j_end", "cigar")


def rows_per_lane(go, ge, k=None):
    """K of the score kernel: GSA_SCORE_K when forced, else 4 for linear gaps and 2 for affine ones."""
    return k if k in (2, 4) else (4 if go == ge else 2)


def strip_rows(go, ge, k=None):
    return 256 * rows_per_lane(go, ge, k)


def hdr(a):
    return np.concatenate([[0], np.asarray(a)]).astype(np.int32)


class Pair:
    """A pair and the table on the device."""

    def __init__(self, Y, X, sub):
        import torch
        dev = torch.device("cuda:0")
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)
        self.Y, self.X = np.asarray(Y, np.int32), np.asarray(X, np.int32)
        self.R, self.C = len(self.Y) - 1, len(self.X) - 1
        self.substsz = int(round(np.sqrt(np.asarray(sub).size)))
        self.subm = np.asarray(sub).reshape(self.substsz, self.substsz)
        self.y, self.x, self.sub = up(self.Y), up(self.X), up(self.subm.ravel())
        torch.cuda.synchronize(dev)

    def args(self):
        return (self.y.data_ptr(), self.y.numel(), self.x.data_ptr(), self.x.numel(), self.sub.data_ptr(), self.substsz)

    def score(self, engine, go, ge):
        r = engine.score_semi_dev(*self.args(), go, ge)
        return r["score"], r["i_end"], r["j_end"]

    def align(self, engine, go, ge, limit=0):
        r = engine.align_pair_semi_dev(*self.args(), go, ge, scratch_limit=limit)
        return r, engine.last_align_pair_semi_info()


def path_of(res):
    """The cells of an alignment, last cell first, from its start cell and CIGAR."""
    _, i, j, _, _, cigar = res
    cells = [(i, j)]
    num = ""
    for ch in cigar:
        if ch.isdigit():
            num += ch
            continue
        for _ in range(int(num)):
            i += 0 if ch == "D" else 1
            j += 0 if ch == "I" else 1
            cells.append((i, j))
        num = ""
    return cells[::-1]


_REF = {}


def want(key, p, go, ge, align=so.align):
    """The reference's alignment and its path, computed once per (pair, gap model)."""
    k = (key, go, ge)
    if k not in _REF:
        res = align(p.Y, p.X, p.subm, go, ge)
        assert (res[1], res[3]) == (0, p.R)
        _REF[k] = (tuple(res), path_of(res))
    return _REF[k]


def window(R, j_end, S, sub, ge):
    """jW by the header's formula."""
    if ge == 0:
        return 0
    pmax = max(0, int(np.asarray(sub).max()))
    dmax = (pmax * R - S) // -ge
    return max(0, j_end - R - dmax - 1)


def plan(path, tr, R, j_end, jW, limit):
    """(chunks, strips filled, peak code bytes) of the bottom-up plan along the reference's path: a
    chunk takes the strips that fit from the lowest one not yet filled, over the columns jW + 1 ... the
    column where the path first reaches the upper boundary of the chunk below; a path on column 0
    needs no more codes; every strip up to strip 0 is filled otherwise."""
    if j_end == 0:
        return 0, 0, 0
    strips = -(-R // tr)
    hi, J, chunks, filled, peak = strips - 1, j_end, 0, 0, 0
    while True:
        sb = (J - jW) * tr // 2
        n = min(limit // sb, hi + 1)
        assert n >= 1
        chunks, filled, peak = chunks + 1, filled + n, max(peak, n * sb)
        lo = hi + 1 - n
        at = [j for i, j in path if i == lo * tr]
        if lo == 0 or at[0] == 0:
            return chunks, filled, peak
        hi, J = lo - 1, at[0]


def t6(r):
    return tuple(r[f] for f in FIELDS)


def check(engine, p, key, go, ge, limit=0, k=None, align=so.align):
    """Both calls against the reference: the score call's three fields; the alignment call's six
    fields, status 0, and everything its info says, computed here along the reference's path."""
    w, path = want(key, p, go, ge, align)
    assert p.score(engine, go, ge) == (w[0], w[3], w[4]), (key, go, ge, p.R, p.C, w)
    r, info = p.align(engine, go, ge, limit)
    print(key, (go, ge), limit, r["status"], t6(r)[:5], r["cigar"][:32], info)  # (shown with pytest -s)
    assert r["status"] == 0, (key, r, info)
    assert t6(r) == w, (key, go, ge, p.R, p.C, t6(r), w)
    tr = strip_rows(go, ge, k)
    jW = window(p.R, w[4], w[0], p.subm, ge)
    chunks, filled, peak = plan(path, tr, p.R, w[4], jW, limit if limit else 2 << 30)
    assert info["strip_rows"] == tr and info["strips"] == -(-p.R // tr), info
    assert info["j_window"] == (jW if w[4] > 0 else 0), (info, jW)
    assert (info["chunks"], info["strips_filled"], info["code_bytes"]) == (chunks, filled, peak), (info, chunks, filled, peak)
    if not limit and w[4] > 0:
        assert info["chunks"] == 1 and info["strips_filled"] == info["strips"], info
    return r, info


# -- the int64 reference ------------------------------------------------------------------------------

NEG64 = -(1 << 62)

_SRC = r"""
#include <stdint.h>
#define NEG (-((int64_t)1 << 62))
static int64_t maxi(int64_t a, int64_t b) { return a >= b ? a : b; }
/* H, E, F: (R + 1) x (C + 1) int64, row-major; y, x with the header element in front; subst int64 */
void fill_semi64(const int32_t* y, int64_t R, const int32_t* x, int64_t C, const int64_t* subst, int32_t n,
                 int64_t go, int64_t ge, int64_t* H, int64_t* E, int64_t* F)
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
        H[i * W] = go + (i - 1) * ge;
        F[i * W] = H[i * W];
        E[i * W] = NEG;
        for (int64_t j = 1; j <= C; j++)
        {
            const int64_t e = maxi(E[i * W + j - 1] + ge, H[i * W + j - 1] + go);
            const int64_t f = maxi(F[(i - 1) * W + j] + ge, H[(i - 1) * W + j] + go);
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
        d = tempfile.mkdtemp(prefix="semi_ref64_")
        src, lib = os.path.join(d, "fill_semi64.c"), os.path.join(d, "fill_semi64.so")
        with open(src, "w") as f:
            f.write(_SRC)
        subprocess.check_call([os.environ.get("CC", "cc"), "-O2", "-shared", "-fPIC", "-o", lib, src])
        _LIB = ctypes.CDLL(lib)
        vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
        _LIB.fill_semi64.restype = None
        _LIB.fill_semi64.argtypes = [vp, i64, vp, i64, vp, i32, i64, i64, vp, vp, vp]
    return _LIB


def value_bound(R, C, sub, go, ge):
    """B = smax min(R, C) + |go| + (R + C) |ge| of the header."""
    smax = max(1, int(np.abs(np.asarray(sub, np.int64)).max()))
    return smax * min(R, C) + (-go) + (R + C) * (-ge)


def span(R, C, sub, go, ge):
    smax = max(1, int(np.abs(np.asarray(sub, np.int64)).max()))
    return (R + C) * (-ge) + (ge - go) + smax


def exact_for(R, C, sub, go, ge):
    """The int64 reference is exact: no |H| exceeds B, so with B < 2^31 every sum of true values stays
    far inside int64 and nothing that comes from -2^62 (at most -2^62 + (R + C) 0) reaches -B."""
    B = value_bound(R, C, sub, go, ge)
    assert B < (1 << 31) and -B + go + ge > NEG64 // 2
    return B


def matrices64(query, subject, subst, go, ge):
    y = np.ascontiguousarray(query, np.int32)
    x = np.ascontiguousarray(subject, np.int32)
    sub = np.ascontiguousarray(subst, np.int64)
    n = int(round(np.sqrt(sub.size)))
    R, C = len(y) - 1, len(x) - 1
    H, E, F = (np.empty((R + 1, C + 1), np.int64) for _ in range(3))
    _lib().fill_semi64(y.ctypes.data, R, x.ctypes.data, C, sub.ctypes.data, n, go, ge, H.ctypes.data, E.ctypes.data,
                       F.ctypes.data)
    return H, E, F


def align64(query, subject, subst, go, ge):
    """(score, 0, j_start, R, j_end, cigar) by the header's rules, on the int64 matrices."""
    y = np.ascontiguousarray(query, np.int32)
    x = np.ascontiguousarray(subject, np.int32)
    sub = np.asarray(subst, np.int64)
    n = int(round(np.sqrt(sub.size)))
    sub = sub.reshape(n, n)
    exact_for(len(y) - 1, len(x) - 1, sub, go, ge)
    H, E, F = matrices64(y, x, sub, go, ge)
    R = len(y) - 1
    best, j_end = int(H[R].max()), int(np.argmax(H[R]))
    i, j, state, ops = R, j_end, "H", []
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
    return best, 0, j, R, j_end, so._fold(ops[::-1])
