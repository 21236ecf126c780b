"""What the tests of the batched overlap calls share (gsa_score_overlap_batch_dev,
gsa_align_batch_overlap_dev): lists of pairs on the device with one table, the reference
per pair (tests/_overlap_oracle.py through tests/_overlap_pair.py's want and path_of, computed once per
pair and gap model), the batch's round plan restated in Python along the reference's paths, and the edge
list the two test files use.  A strip is TR rows: 1024 in both gap models, 512 with GSA_SCORE_K=2."""
import numpy as np

from gpuseqalign_amd import formats as F
from tests import _overlap_oracle as oo
from tests import _overlap_pair as op
from tests._overlap_pair import Pair, hdr, t6

DEFAULT_LIMIT = 8 << 30
STRICT = [(-11, -1), (-4, -4), (-5, -2)]  # the gap models under which a planted layout is the only optimum
ID20 = np.where(np.eye(20, dtype=bool), 5, -4)


def seq(n, seed, alphabet=20):
    return F.synthetic_seq(n, seed, alphabet)


def part(n, seed, lo, hi):
    """n letters of lo ... hi - 1, no header."""
    return seq(n, seed, hi - lo)[1:] + lo


def dovetail(R, C, ov, seed):
    """Y's last ov letters, mutated, are X's first letters: the path starts on column 0 and ends on row R."""
    core = seq(ov, seed)
    mut = F.mutate_seq(core, seed + 1)[1:]
    y = np.concatenate([seq(max(R - ov, 0), seed + 2)[1:], core[1:]])[-R:]
    x = np.concatenate([mut, seq(C, seed + 3)[1:]])[:C]
    return hdr(y), hdr(x)


def mirror(R, C, ov, seed):
    """X's last letters are Y's first ov letters, mutated: the path starts on row 0 and ends on column C."""
    x, y = dovetail(C, R, ov, seed)
    return y, x


def related(R, C, seed):
    """A dovetail, its mirror, or the shorter sequence, mutated, inside the longer one, by seed % 3."""
    kind = seed % 3
    if kind == 0:
        return dovetail(R, C, max(1, 2 * min(R, C) // 3), seed)
    if kind == 1:
        return mirror(R, C, max(1, 2 * min(R, C) // 3), seed)
    if R <= C:
        x = seq(C, seed)
        at = (C - R) // 2
        y = np.concatenate([F.mutate_seq(hdr(x[1 + at:1 + at + R]), seed + 1)[1:], seq(R, seed + 2)[1:]])[:R]
        return hdr(y), x
    x, y = related(C, R, seed)
    return y, x


def end_on_column_c(R, C, e):
    """Y = core + junk, X = junk + core over disjoint alphabets (table ID20): the core's e letters end on
    (e, C) and nothing else scores."""
    core = part(e, 11 + e, 0, 12)
    return hdr(np.concatenate([core, part(R - e, 12 + e, 16, 20)])), hdr(np.concatenate([part(C - e, 13 + e, 12, 16), core]))


def start_on_column_0(R, s, tail=30):
    """Y = junk + core, X = core + junk (table ID20): the path starts on (s, 0) and ends on row R."""
    core = part(R - s, 21 + s, 0, 12)
    return hdr(np.concatenate([part(s, 22 + s, 16, 20), core])), hdr(np.concatenate([core, part(tail, 23 + s, 12, 16)]))


def plant(R, a, n, seed, inserted):
    """Y of R letters and an X that holds it between two flanks of 150 letters: with Y's rows a ... a + n
    - 1 removed (a vertical gap there), or with n letters inserted behind row a - 1 (a horizontal gap on
    row a - 1).  The gap's letters are a letter the rest does not use."""
    y = seq(R, seed, 19)
    if not inserted:
        y = y.copy()
        y[a:a + n] = 19
        core = np.concatenate([y[1:a], y[a + n:]])
    else:
        core = np.concatenate([y[1:a], np.full(n, 19), y[a:]])
    return y, hdr(np.concatenate([seq(150, seed + 1, 19)[1:], core, seq(150, seed + 2, 19)[1:]]))


class Batch:
    """A list of (key, Pair) over one table; two entries may be one Pair, or share a seqX buffer."""

    def __init__(self, name, sub):
        self.name, self.sub, self.items = name, sub, []

    def add(self, key, Y, X):
        p = Pair(Y, X, self.sub)
        self.items.append((key, p))
        return p

    def again(self, k):
        self.items.append(self.items[k])

    def add_sharing_x(self, key, Y, other):
        """A second seqY against `other`'s seqX buffer."""
        p = Pair(Y, other.X, self.sub)
        p.x = other.x
        self.items.append((key, p))
        return p

    def __len__(self):
        return len(self.items)

    def pair(self, k):
        return self.items[k][1]

    def index(self, key):
        return [k for k, _ in self.items].index(key)

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

    def want(self, k, go, ge, align=oo.align):
        key, p = self.items[k]
        return op.want(("batch", self.name, key), p, go, ge, align)  # (a key of its own in the shared cache)

    def score(self, engine, go, ge, order=None):
        r = engine.score_overlap_batch_dev(self.ptrs(order), *self.table(), go, ge)
        return [(x["score"], x["i_end"], x["j_end"]) for x in r]

    def align(self, engine, go, ge, mwg=0, limit=0, order=None):
        r = engine.align_batch_overlap_dev(self.ptrs(order), *self.table(), go, ge, mwg, limit)
        return r, engine.last_align_batch_overlap_info()


def plan_rounds(tr, limit, items):
    """(rounds, strips filled, peak code bytes) of gsa_align_batch_overlap_dev's rounds, restated: `items`
    is one (i_end, j_end, path) per traced pair, in list order.  A pair starts at (i_end's strip, j_end).
    Active pairs by remaining code bytes descending, ties by index; each gets its lowest unfilled strip and
    as many above as still fit, for the columns 1 ... j where the reference's path first reaches the upper
    boundary of its chunk below; a chunk that holds strip 0, or a path that ended on column 0 at or below
    that boundary, ends the pair."""
    st = [[-(-i_end // tr) - 1, j_end] for i_end, j_end, _ in items]
    rounds = filled = peak = 0
    while any(s[0] >= 0 for s in st):
        act = [p for p, s in enumerate(st) if s[0] >= 0]
        act.sort(key=lambda p: (-(st[p][0] + 1) * st[p][1] * (tr // 2), p))
        used, took = 0, []
        for p in act:
            hi, J = st[p]
            sb = J * (tr // 2)
            if sb > limit - used:
                continue
            n = min((limit - used) // sb, hi + 1)
            took.append((p, hi + 1 - n))
            used += n * sb
            filled += n
        assert took, "a round fills no strip"
        rounds, peak = rounds + 1, max(peak, used)
        for p, lo in took:
            at = [j for i, j in items[p][2] if i == lo * tr]  # the path's cells on the boundary, lowest first
            if lo == 0 or not at or at[0] == 0:
                st[p][0] = -1
            else:
                st[p][0], st[p][1] = lo - 1, at[0]
    return rounds, filled, peak


def check_batch(engine, b, go, ge, tr, mwg=0, limit=0, single=True, reverse=True, align=oo.align):
    """Both batched calls on the whole list against the reference, the single-pair calls and the list
    reversed; then everything the info says, restated here along the reference's paths."""
    n = len(b)
    want = [b.want(k, go, ge, align) for k in range(n)]
    sc = b.score(engine, go, ge)
    res, info = b.align(engine, go, ge, mwg, limit)
    print(b.name, (go, ge), tr, mwg, limit, info)  # (shown with pytest -s)
    for k in range(n):
        w = want[k][0]
        assert sc[k] == (w[0], w[3], w[4]), (b.items[k][0], go, ge, sc[k], w[:5])
        assert res[k]["status"] == 0, (b.items[k][0], res[k])
        assert t6(res[k]) == w, (b.items[k][0], go, ge, t6(res[k])[:5], w[:5])
    if single:
        for k in range(n):
            p = b.pair(k)
            assert p.score(engine, go, ge) == sc[k], b.items[k][0]
            one = engine.align_pair_overlap_dev(*p.args(), go, ge)
            assert (one["status"], t6(one)) == (0, t6(res[k])), b.items[k][0]
    if reverse:
        order = list(range(n))[::-1]
        assert b.score(engine, go, ge, order) == sc[::-1]
        rev, _ = b.align(engine, go, ge, mwg, limit, order)
        assert [(r["status"], t6(r)) for r in rev] == [(r["status"], t6(r)) for r in res][::-1]
    # the info: what ran, along the reference's paths
    traced = [k for k in range(n) if want[k][0][3] > 0 and want[k][0][4] > 0]
    items = [(want[k][0][3], want[k][0][4], want[k][1]) for k in traced]
    dev = [k for k in range(n) if b.pair(k).R > 0 and b.pair(k).C > 0]
    assert info["batch_pairs"] == len(traced) and info["host_pairs"] == n - len(traced), info
    assert info["strip_rows"] == (tr if dev else 0), info
    assert info["strips"] == sum(-(-it[0] // tr) for it in items), info
    gran = sum(16 * (-(-b.pair(k).R // tr)) * ((b.pair(k).C + 16) & ~15) for k in dev)
    assert info["gran_bytes"] == gran, (info, gran)
    rounds, filled, peak = plan_rounds(tr, limit if limit else DEFAULT_LIMIT, items)
    assert (info["rounds"], info["strips_filled"], info["code_bytes"]) == (rounds, filled, peak), (info, rounds, filled, peak)
    assert (info["score_ms"] > 0) == bool(dev) and (info["fill_ms"] > 0) == (rounds > 0) == (info["walk_ms"] > 0), info
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
    """The issue's edges in one list (see tests/test_gpu_align_batch_overlap.py)."""
    if ("edge", tr) in _LISTS:
        return _LISTS[("edge", tr)]
    b = Batch("edge%d" % tr, sub)
    shapes = [(R, C) for R in (1, 3, 4, 5, 255, 256, 257, tr - 1, tr, tr + 1, 2 * tr + 1) for C in (1, 65, 300)]
    shapes += [(R, C) for C in (1, 2, 15, 16, 17, 47, 63, 64, 65, 79, 80, 1023, 1024, 1025) for R in (9, tr + 1)]
    for R, C in shapes:
        b.add(("rc", R, C), *related(R, C, 3 * R + C))
    b.again(7)                                                       # the same pair twice
    first = b.add("shared0", *related(500, 900, 71))
    b.add_sharing_x("shared1", related(300, 900, 72)[0], first)      # two pairs on one seqX buffer
    b.add("R0", hdr([]), seq(40, 73))
    b.add("C0", seq(40, 74), hdr([]))
    lo, other = lowest_pair_of(sub)
    b.add("zero", hdr(np.full(40, lo)), hdr(np.full(30, other)))     # nothing scores: 0 at (R, 0), a host pair
    x = seq(1400, 34)
    y = F.mutate_seq(hdr(x[301:901]), 35)
    b.add("yinx", y, x)                                              # both containments
    b.add("xiny", x, y)
    core = seq(200, 31)[1:]
    b.add("corner", hdr(core), hdr(np.concatenate([seq(90, 32)[1:], core])))  # the end at (R, C)
    for n in (1, 30):
        for inserted in (False, True):
            a = tr + 1 if inserted else tr + 1 - (n + 1) // 2        # the gap lies across rows TR / TR + 1
            b.add(("plant", n, inserted), *plant(tr + 300, a, n, 31 * tr + n, inserted))
    _LISTS[("edge", tr)] = b
    return b


def bleed_list(tr):
    """Column buffers side by side (table ID20).  A pair with R = 1, whose one ticket stores TR rows of
    column C, directly before and after pairs whose only maximum lies on column C at rows 1 ... 4, and the
    corner pair (its maximum at row R of column C); then a pair whose maximum lies on column C in the last
    wave of its first ticket of three, between pairs with R = TR + 1 and 2 TR + 1."""
    if ("bleed", tr) in _LISTS:
        return _LISTS[("bleed", tr)]
    b = Batch("bleed%d" % tr, ID20)
    one = lambda n: b.add(("R1", n), hdr(part(1, 80 + n, 0, 12)), hdr(part(50, 90 + n, 0, 20)))
    one(0)
    for e in (1, 2, 3, 4):
        b.add(("colC", e), *end_on_column_c(tr + 40, 300, e))
        one(e)
    core = part(200, 31, 0, 12)
    b.add("corner", hdr(core), hdr(np.concatenate([part(90, 32, 12, 16), core])))
    one(5)
    b.add(("rows", tr + 1), *related(tr + 1, 200, 3 * tr + 5))
    b.add(("lastwave", tr - 3), *end_on_column_c(2 * tr + 50, tr + 60, tr - 3))
    b.add(("rows", 2 * tr + 1), *related(2 * tr + 1, 120, 3 * tr + 7))
    _LISTS[("bleed", tr)] = b
    return b


UNIT = np.array([3, 7, 11, 2, 16])


def tie_list():
    """Two equal maxima on row R (columns 58 and 63), on column C (rows 12 and 13) and on both ((80, 40)
    and (40, 80): row R wins), each between neighbours with larger scores (table ID20)."""
    if "tie" in _LISTS:
        return _LISTS["tie"]
    b = Batch("tie", ID20)
    big = lambda n: b.add(("big", n), *start_on_column_0(400 + n, 100 + n))
    big(0)
    junk = part(80, 5, 17, 20)
    b.add("row", hdr(np.tile(UNIT, 8)), hdr(np.concatenate([junk[:18], np.tile(UNIT, 9), junk[18:]])))
    big(1)
    b.add("col", hdr(np.concatenate([part(4, 41, 12, 16), np.full(9, 5), part(40, 42, 16, 20)])), hdr(np.full(8, 5)))
    big(2)
    A, B = part(40, 51, 0, 10), part(40, 52, 10, 20)
    b.add("both", hdr(np.concatenate([A, B])), hdr(np.concatenate([B, A])))
    big(3)
    _LISTS["tie"] = b
    return b
