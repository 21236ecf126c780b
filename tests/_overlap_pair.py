"""What the GPU tests of the long pairs' overlap mode share (gsa_score_overlap_dev,
gsa_align_pair_overlap_dev): the gap models, pairs on the device, the oracle's alignment
with its path, and the plan of chunks computed here, independently of the library, along that path.
The reference is tests/_overlap_oracle.py; its int64 fill (align64) serves the inputs at the value-range
guards."""
import numpy as np

from tests import _overlap_oracle as oo

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
        r = engine.score_overlap_dev(*self.args(), go, ge)
        return r["score"], r["i_end"], r["j_end"]

    def align(self, engine, go, ge, limit=0):
        r = engine.align_pair_overlap_dev(*self.args(), go, ge, scratch_limit=limit)
        return r, engine.last_align_pair_overlap_info()


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


def want(key, p, go, ge, align=oo.align):
    """The reference's alignment and its path, computed once per (pair, gap model)."""
    k = (key, go, ge)
    if k not in _REF:
        res = tuple(align(p.Y, p.X, p.subm, go, ge))
        assert res[0] >= 0 and (res[1] == 0 or res[2] == 0) and (res[3] == p.R or res[4] == p.C)
        assert (res[3], res[4]) == path_of(res)[0]
        _REF[k] = (res, path_of(res))
    return _REF[k]


def plan(path, tr, i_end, j_end, limit):
    """(strips, chunks, strips filled, peak code bytes) of the bottom-up plan along the reference's path:
    the strips of the rows 1 ... i_end; a chunk takes the strips that fit from the lowest one not yet
    filled, over the columns 1 ... the column where the path first reaches the upper boundary of the
    chunk below; a path that ends on column 0 at or below that boundary needs no more codes.  An end
    cell on a border needs none at all."""
    strips = -(-i_end // tr)
    if i_end == 0 or j_end == 0:
        return strips, 0, 0, 0
    hi, J, chunks, filled, peak = strips - 1, j_end, 0, 0, 0
    while True:
        sb = J * tr // 2
        n = min(limit // sb, hi + 1)
        assert n >= 1
        chunks, filled, peak = chunks + 1, filled + n, max(peak, n * sb)
        lo = hi + 1 - n
        at = [j for i, j in path if i == lo * tr]  # the path's cells on the chunk's upper boundary, lowest first
        if lo == 0 or not at or at[0] == 0:
            return strips, chunks, filled, peak
        hi, J = lo - 1, at[0]


def t6(r):
    return tuple(r[f] for f in FIELDS)


def check(engine, p, key, go, ge, limit=0, k=None, align=oo.align):
    """Both calls against the reference: the score call's three fields; the alignment call's six
    fields, status 0, and everything its info says, computed here along the reference's path."""
    w, path = want(key, p, go, ge, align)
    got = p.score(engine, go, ge)
    print(key, (go, ge), "score", got, "want", (w[0], w[3], w[4]))  # (shown with pytest -s)
    assert got == (w[0], w[3], w[4]), (key, go, ge, p.R, p.C, got, w[:5])
    r, info = p.align(engine, go, ge, limit)
    print(key, (go, ge), limit, r["status"], t6(r)[:5], r["cigar"][:32], info)
    assert r["status"] == 0, (key, r, info)
    assert t6(r) == w, (key, go, ge, p.R, p.C, t6(r)[:5], w[:5])
    tr = strip_rows(go, ge, k)
    strips, chunks, filled, peak = plan(path, tr, w[3], w[4], limit if limit else 2 << 30)
    assert info["strip_rows"] == tr and info["strips"] == strips, (info, tr, strips)
    assert (info["chunks"], info["strips_filled"], info["code_bytes"]) == (chunks, filled, peak), (info, chunks, filled, peak)
    assert info["score_ms"] > 0 and (info["fill_ms"] > 0) == (chunks > 0) and (info["walk_ms"] > 0) == (chunks > 0), info
    return r, info
