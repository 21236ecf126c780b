"""What the tests of the batched semi-global calls share (gsa_score_semi_batch_dev,
gsa_align_batch_semi_dev): lists of pairs on the device with one table, the reference per
pair (tests/_semi_oracle.py through tests/_semi_pair.py, computed once per pair and gap model), the
batch's round plan restated in Python along the reference's paths, and the lists the two test files use.
A strip is TR rows: 1024 in both gap models, 512 with GSA_SCORE_K=2."""
import numpy as np

from gpuseqalign_amd import formats as F
from tests import _semi_oracle as so
from tests import _semi_pair as sp
from tests._semi_pair import Pair, hdr, t6

DEFAULT_LIMIT = 8 << 30


def seq(n, seed, alphabet=20):
    return F.synthetic_seq(n, seed, alphabet)


def related(R, C, seed):
    """A query of R letters, a mutated stretch of the subject (C letters) from its middle, cut or padded
    with random letters."""
    x = seq(C, seed)
    at = max(0, (C - R) // 2)
    mut = F.mutate_seq(hdr(x[1 + at:1 + at + R]), seed + 1)[1:]
    mut = np.concatenate([mut, seq(R, seed + 2)[1:]])[:R]
    return hdr(mut), x


def plant(R, a, n, seed, inserted):
    """A query of R letters and a subject that holds it between two flanks of 150 letters: with the
    query's rows a ... a + n - 1 removed (a vertical gap there), or with n letters inserted behind row
    a - 1 (a horizontal gap on row a - 1).  The gap's letters are a letter the rest does not use."""
    y = seq(R, seed, 19)
    if not inserted:
        y = y.copy()
        y[a:a + n] = 19
        core = np.concatenate([y[1:a], y[a + n:]])
    else:
        core = np.concatenate([y[1:a], np.full(n, 19), y[a:]])
    return y, hdr(np.concatenate([seq(150, seed + 1, 19)[1:], core, seq(150, seed + 2, 19)[1:]]))


class Batch:
    """A list of (key, Pair) over one table; two entries may be one Pair, or share a subject buffer."""

    def __init__(self, name, sub):
        self.name, self.sub, self.items = name, sub, []

    def add(self, key, Y, X):
        p = Pair(Y, X, self.sub)
        self.items.append((key, p))
        return p

    def again(self, k):
        self.items.append(self.items[k])

    def add_sharing_subject(self, key, Y, other):
        """A second query against `other`'s subject buffer."""
        p = Pair(Y, other.X, self.sub)
        p.x = other.x
        self.items.append((key, p))
        return p

    def __len__(self):
        return len(self.items)

    def pair(self, k):
        return self.items[k][1]

    def ptrs(self, order=None):
        order = range(len(self.items)) if order is None else order
        out = []
        for k in order:
            p = self.items[k][1]
            out.append((p.y.data_ptr(), p.y.numel(), p.x.data_ptr(), p.x.numel()))
        return out

    def table(self):
        p = self.items[0][1]
        return p.sub.data_ptr(), p.substsz

    def want(self, k, go, ge, align=so.align):
        key, p = self.items[k]
        return sp.want((self.name, key), p, go, ge, align)

    def score(self, engine, go, ge, order=None):
        r = engine.score_semi_batch_dev(self.ptrs(order), *self.table(), go, ge)
        return [(x["score"], x["i_end"], x["j_end"]) for x in r]

    def align(self, engine, go, ge, mwg=0, limit=0, order=None):
        r = engine.align_batch_semi_dev(self.ptrs(order), *self.table(), go, ge, mwg, limit)
        return r, engine.last_align_batch_semi_info()


def plan_rounds(tr, limit, items):
    """(rounds, strips filled, peak code bytes) of gsa_align_batch_semi_dev's rounds, restated: `items` is
    one (R, j_end, jW, path) per traced pair, in list order.  Active pairs by remaining code bytes
    descending, ties by index; each gets its lowest unfilled strip and as many above as still fit, for the
    columns jW + 1 ... j where the reference's path first reaches the upper boundary of its chunk below; a
    path on column 0 there, or a chunk that holds strip 0, ends the pair."""
    st = [[-(-R // tr) - 1, j_end, jW] for R, j_end, jW, _ in items]
    rounds = filled = peak = 0
    while any(s[0] >= 0 for s in st):
        act = [p for p, s in enumerate(st) if s[0] >= 0]
        act.sort(key=lambda p: (-(st[p][0] + 1) * (st[p][1] - st[p][2]) * (tr // 2), p))
        used, took = 0, []
        for p in act:
            hi, J, jW = st[p]
            sb = (J - jW) * (tr // 2)
            if sb > limit - used:
                continue
            n = min((limit - used) // sb, hi + 1)
            took.append((p, hi + 1 - n))
            used += n * sb
            filled += n
        assert took, "a round fills no strip"
        rounds, peak = rounds + 1, max(peak, used)
        for p, lo in took:
            at = [j for i, j in items[p][3] if i == lo * tr]
            if lo == 0 or at[0] == 0:
                st[p][0] = -1
            else:
                st[p][0], st[p][1] = lo - 1, at[0]
    return rounds, filled, peak


def check_batch(engine, b, go, ge, tr, mwg=0, limit=0, single=True, reverse=True, align=so.align):
    """Both batched calls on the whole list against the reference, the single-pair calls and the list
    reversed; then everything the info says, restated here along the reference's paths."""
    n = len(b)
    want = [b.want(k, go, ge, align) for k in range(n)]
    sc = b.score(engine, go, ge)
    res, info = b.align(engine, go, ge, mwg, limit)
    print(b.name, (go, ge), tr, mwg, limit, info)  # (shown with pytest -s)
    for k in range(n):
        w = want[k][0]
        assert sc[k] == (w[0], w[3], w[4]), (b.items[k][0], go, ge, sc[k], w)
        assert res[k]["status"] == 0, (b.items[k][0], res[k])
        assert t6(res[k]) == w, (b.items[k][0], go, ge, t6(res[k]), w)
    if single:
        for k in range(n):
            p = b.pair(k)
            assert p.score(engine, go, ge) == sc[k], b.items[k][0]
            one = engine.align_pair_semi_dev(*p.args(), go, ge)
            assert (one["status"], t6(one)) == (0, t6(res[k])), b.items[k][0]
    if reverse:
        order = list(range(n))[::-1]
        assert b.score(engine, go, ge, order) == sc[::-1]
        rev, _ = b.align(engine, go, ge, mwg, limit, order)
        assert [(r["status"], t6(r)) for r in rev] == [(r["status"], t6(r)) for r in res][::-1]
    # the info: what ran, along the reference's paths
    traced = [k for k in range(n) if b.pair(k).R > 0 and b.pair(k).C > 0 and want[k][0][4] > 0]
    items = []
    for k in traced:
        p, (w, path) = b.pair(k), want[k]
        items.append((p.R, w[4], sp.window(p.R, w[4], w[0], p.subm, ge), path))
    assert info["batch_pairs"] == len(traced) and info["host_pairs"] == n - len(traced), info
    assert info["strip_rows"] == (tr if any(b.pair(k).R > 0 and b.pair(k).C > 0 for k in range(n)) else 0), info
    assert info["strips"] == sum(-(-it[0] // tr) for it in items), info
    assert info["window_cols"] == sum(it[1] - it[2] for it in items), info
    gran = 0
    for k in range(n):
        p = b.pair(k)
        if p.R > 0 and p.C > 0:
            gran += 16 * (-(-p.R // tr)) * ((p.C + 16) & ~15)
    assert info["gran_bytes"] == gran, (info, gran)
    rounds, filled, peak = plan_rounds(tr, limit if limit else DEFAULT_LIMIT, items)
    assert (info["rounds"], info["strips_filled"], info["code_bytes"]) == (rounds, filled, peak), (info, rounds, filled, peak)
    return res, info, items


# -- the lists ------------------------------------------------------------------------------------------

_LISTS = {}


def lowest_pair_of(sub):
    """Two different letters whose table value is the table's smallest."""
    m = np.asarray(sub).reshape(int(round(np.sqrt(np.asarray(sub).size))), -1)[:20, :20]
    a, b = np.unravel_index(int(np.argmin(m)), m.shape)
    assert a != b and m[a, b] < 0 and m[b, a] == m[a, b]
    return int(a), int(b)


def edge_list(tr, sub):
    """The issue's edges in one list (see tests/test_gpu_align_batch_semi.py)."""
    if ("edge", tr) in _LISTS:
        return _LISTS[("edge", tr)]
    b = Batch("edge%d" % tr, sub)
    shapes = [(R, C) for R in (1, 3, 4, 5, 255, 256, 257, tr - 1, tr, tr + 1, 2 * tr + 1) for C in (1, 65, 300)]
    shapes += [(R, C) for C in (15, 16, 17, 63, 64, 65, 511, 512, 513, 1023, 1024, 1025) for R in (9, tr + 1)]
    for R, C in shapes:
        b.add(("rc", R, C), *related(R, C, 3 * R + C))
    b.again(7)                                                       # the same pair twice
    first = b.add("shared0", *related(500, 900, 71))
    b.add_sharing_subject("shared1", related(300, 900, 72)[0], first)  # two queries, one subject buffer
    b.add("R0", hdr([]), seq(40, 73))
    b.add("C0", seq(40, 74), hdr([]))
    lo, other = lowest_pair_of(sub)
    b.add("allI", hdr(np.full(40, lo)), hdr(np.full(30, other)))     # every cell negative: ends on column 0
    x = np.full(30, other)
    x[9] = lo
    b.add("neg", hdr(np.full(30, lo)), hdr(x))                       # one match among inserts: a negative score
    xs = seq(700, 75)
    q = np.concatenate([F.mutate_seq(hdr(xs[372:698]), 76)[1:], xs[698:701]])[-300:]
    b.add("endC", hdr(q), xs)                                        # the query ends with the subject's last letters
    for n in (1, 30):
        for inserted in (False, True):
            a = tr + 1 if inserted else tr + 1 - (n + 1) // 2        # the gap lies across rows TR / TR + 1
            b.add(("plant", n, inserted), *plant(tr + 300, a, n, 31 * tr + n, inserted))
    _LISTS[("edge", tr)] = b
    return b
