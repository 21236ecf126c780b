"""The score and alignment calls at their value-range guards (gsa_score.hip score_ranges and the routes
behind it; DESIGN.md 2.2, "Value-range guards"): every guard from both sides, with gap costs and table
values as large as the guard lets through.  Every expectation is tests/_exact.py's -- int64 with a true
minus infinity -- never the oracle's, which shares its finite sentinel with the kernels.  Every case
names the kernel it reached: gsa_last_launch's kind for the calls that leave a launch record
(score_dev, score_batch_dev, score_db_dev), the call's own info struct for the multi and align calls,
which leave that record untouched by contract (lane_queries / other_queries, lane_hits / unsupported).

The inputs are built by plain functions at the top, without a GPU: tests/test_exact_reference.py runs
the oracles over the same ones, on the accepted side of every guard.

The guards, as include/gsa.h states them, with smax the largest |table value| and
B = smax min(R, C) + |go| + (R + C) |ge|:
  global  B + |go| < 2^29, else errorInvalidValue        local  B < 2^30, else errorInvalidValue
  trace   B < 2^26, else status 1                         lane key  local: smax min(R, C) < 2^18, C <= 8191
  K-rows / strip score kernels: every s - go - ge in [-32767, 32767], local: smax min(R, C) < 2^26"""
import numpy as np
import pytest

import gpuseqalign_amd as gsa
from gpuseqalign_amd import formats as F
from tests import _exact
from tests._data import random_pair

pytestmark = pytest.mark.gpu

LANES = 16   # lanes per subject
K_LANE = 24  # query rows a lane holds; the GPU tests read it from gsa_last_launch and compare
GLOBAL_LIMIT, LOCAL_LIMIT, TRACE_LIMIT = 1 << 29, 1 << 30, 1 << 26
KEY_SCORES, KEY_COLS = 1 << 18, 8191

_EXACT = {}


def exact(Y, X, sub, go, ge, local):
    """_exact.score, computed once per input and shared by every test of the session."""
    sub = np.ascontiguousarray(sub, dtype=np.int32)
    k = (np.asarray(Y, np.int32).tobytes(), np.asarray(X, np.int32).tobytes(), sub.tobytes(), go, ge, bool(local))
    if k not in _EXACT:
        _EXACT[k] = _exact.score(Y, X, sub, go, ge, local)
    return _EXACT[k]


def seq(n, seed):
    return F.synthetic_seq(n, seed, 20)


def table20():
    """20 letters, values in -4 .. 11, not symmetric."""
    t = np.random.default_rng(2029).integers(-4, 12, (20, 20)).astype(np.int32)
    assert np.abs(t).max() == 11 and not np.array_equal(t, t.T)
    return t


def diag_table(v):
    t = np.full((20, 20), -v, np.int32)
    np.fill_diagonal(t, v)
    return t


def bound(R, C, smax, go, ge, extra_go):
    """B + extra_go |go|."""
    return smax * min(R, C) + (1 + extra_go) * (-go) + (R + C) * (-ge)


def gaps_at(limit, R, C, smax, affine, extra_go, past=False):
    """(go, ge) of the largest magnitude with B + extra_go |go| < limit, go = ge - 10 (affine) or ge;
    past: |ge| one larger, which is at or over the limit.  Inside is within 1 % of the limit."""
    d = 10 if affine else 0
    m = (limit - 1 - smax * min(R, C) - (1 + extra_go) * d) // (R + C + 1 + extra_go) + (1 if past else 0)
    go, ge = -(m + d), -m
    b = bound(R, C, smax, go, ge, extra_go)
    assert b >= limit if past else 0.99 * limit < b < limit, (b, limit)
    return go, ge


# -- the inputs ------------------------------------------------------------------------------------

SCAN_SHAPES = [(300, 10), (10, 300), (130, 130), (700, 9)]
DB_LENS = [1, 40, 17, 2, 33, 39, 8, 25, 40]


def scan_pair(R, C):
    return random_pair(R, C, 7 * R + C)


def db_subjects():
    return [seq(c, 9000 + i) for i, c in enumerate(DB_LENS)]


def db_queries(R):
    """Two different queries of R letters: the multi call rebuilds the profile between them."""
    return [seq(R, 500 + R), seq(R, 700 + R)]


def sweep_rows(k):
    s = LANES * k
    return [s - 1, s + 1, 2 * s + 1]


def global_gap_cases(k, limit=GLOBAL_LIMIT, extra_go=1):
    """(Y, X, table, go, ge) of every pair of the large-gap tests, just inside `limit`."""
    t = table20()
    for affine in (True, False):
        for R, C in SCAN_SHAPES:
            Y, X = scan_pair(R, C)
            yield (Y, X, t) + gaps_at(limit, R, C, 11, affine, extra_go)
        for R in sweep_rows(k):
            g = gaps_at(limit, R, max(DB_LENS), 11, affine, extra_go)
            for Y in db_queries(R):
                for X in db_subjects():
                    yield (Y, X, t) + g


BATCH_SHAPES = SCAN_SHAPES[:3]


def batch_gaps(affine, past=False):
    """One (go, ge) for the three pairs of a batch: the smallest of their own, so the tightest pair is
    just inside the bound (or, past, the only one over it)."""
    return min((gaps_at(GLOBAL_LIMIT, R, C, 11, affine, 1, past=past) for R, C in BATCH_SHAPES), key=lambda g: -g[1])


EDGE_PAIR = (1100, 70)
EDGE_TABLES = {"top": (32755, True), "over": (32756, False), "bottom": (-32779, True), "under": (-32780, False)}
SMALL_SHAPES = [(64, 65), (200, 130), (65, 100), (300, 257)]


def edge_table(value):
    """table20 with one entry at the int16 profile's edge under -11 / -1: s - go - ge = value + 12."""
    t = table20()
    t[3, 7] = value
    return t


def edge_pairs():
    """The 1100 x 70 pair among short ordinary ones (index 2)."""
    small = [random_pair(R, C, 3 * R + C) for R, C in SMALL_SHAPES]
    return small[:2] + [random_pair(*EDGE_PAIR, 77)] + small[2:]


def sw_edge_pair(n):
    y = seq(n, 2600 + n)
    return y, y.copy()


def key_score_pool(k, over):
    """(queries, subjects, table, v): a query of 16 k + 1 letters, a subject identical to it (index 5)
    among 8 random short ones, and a second random query; diagonal v, every other entry -v, with
    v (16 k + 1) just under 2^18, or just over."""
    R = LANES * k + 1
    v = KEY_SCORES // R + (1 if over else 0)
    assert (v * R >= KEY_SCORES) == bool(over) and (v - 1) * R < KEY_SCORES
    q = seq(R, 41)
    lens = [60, 1, 33, 7, 52, None, 18, 45, 29]
    subjects = [q.copy() if c is None else seq(c, 4100 + i) for i, c in enumerate(lens)]
    return [q, seq(R, 43)], subjects, diag_table(v), v


SPACER = 22


def match_table():
    """Match +5 among letters 0 .. 19, everything else -4; the spacer letter matches nothing."""
    t = np.full((24, 24), -4, np.int32)
    np.fill_diagonal(t[:20, :20], 5)
    return t


def key_column_pool():
    """(queries, subjects, table): a 30-letter query, and subjects of spacer letters with the query's
    letters planted: 8190 letters, at columns 1 .. 30; 8191, ending at column 8191; 8191, at both places
    (a tie in row 30: the first wins); 8192, ending at column 8192; 8190, ending at column 8190."""
    q = seq(30, 9)

    def subject(n, ends):
        x = np.full(n + 1, SPACER, np.int32)
        x[0] = 0
        for e in ends:
            x[e - 29:e + 1] = q[1:]
        return x

    subjects = [subject(8190, [30]), subject(8191, [8191]), subject(8191, [30, 8191]), subject(8192, [8192]),
                subject(8190, [8190])]
    return [q, seq(30, 10)], subjects, match_table()


TRACE_LENS = [30, 150, 300]


def trace_pool(k):
    R = LANES * k + 1
    return [seq(R, 61), seq(R, 62)], [seq(c, 6100 + i) for i, c in enumerate(TRACE_LENS)], table20()


def accepted_cases(k=K_LANE):
    """(tag, Y, X, table, go, ge, local) of every input the tests below expect an answer for."""
    for local in (False, True):
        for c in global_gap_cases(k):
            yield ("gaps",) + c + (local,)
    t = table20()
    for affine in (True, False):  # local: past the global bound too
        for R, C in SCAN_SHAPES:
            yield ("gaps-past", *scan_pair(R, C), t, *gaps_at(GLOBAL_LIMIT, R, C, 11, affine, 1, past=True), True)
        for R in sweep_rows(k):
            g = gaps_at(GLOBAL_LIMIT, R, max(DB_LENS), 11, affine, 1, past=True)
            for Y in db_queries(R):
                for X in db_subjects():
                    yield ("gaps-past", Y, X, t, *g, True)
        for R, C in BATCH_SHAPES:
            for g, local in [(batch_gaps(affine), False), (batch_gaps(affine), True), (batch_gaps(affine, True), True)]:
                yield ("gaps-batch", *scan_pair(R, C), t, *g, local)
    for name, (value, _) in EDGE_TABLES.items():
        for Y, X in edge_pairs():
            for local in (False, True):
                yield ("int16-" + name, Y, X, edge_table(value), -11, -1, local)
    for n in (2048, 2049):
        yield ("sw", *sw_edge_pair(n), diag_table(32755), -11, -1, True)
    for over in (False, True):
        queries, subjects, t, _ = key_score_pool(k, over)
        for go, ge in [(-11, -1), (-11, -11)]:
            for Y in queries:
                for X in subjects:
                    yield ("key-score", Y, X, t, go, ge, True)
    queries, subjects, t = key_column_pool()
    for go, ge in [(-11, -1), (-11, -11)]:
        for Y in queries:
            for X in subjects:
                yield ("key-column", Y, X, t, go, ge, True)
    queries, subjects, t = trace_pool(k)
    R = len(queries[0]) - 1
    for affine in (True, False):
        for past in (False, True):
            g = gaps_at(TRACE_LIMIT, R, max(TRACE_LENS), 11, affine, 0, past=past)
            for Y in queries:
                for X in subjects:
                    yield ("trace", Y, X, t, *g, False)


# -- on the device ---------------------------------------------------------------------------------

class _Pool:
    """Queries in one device buffer, subjects in another, the table."""

    def __init__(self, queries, subjects, sub):
        import torch
        dev = torch.device("cuda:0")
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)
        self.queries, self.subjects, self.subm = queries, subjects, np.ascontiguousarray(sub, dtype=np.int32)
        self.sub = up(self.subm.ravel())
        self.substsz = int(round(np.sqrt(self.subm.size)))
        self.q = up(np.concatenate(queries))
        self.db = up(np.concatenate(subjects))
        self.qoff = np.concatenate([[0], np.cumsum([len(x) for x in queries])]).astype(np.int64)
        self.off = np.concatenate([[0], np.cumsum([len(x) for x in subjects])]).astype(np.int64)
        torch.cuda.synchronize(dev)

    def _q(self, q):
        return self.q.data_ptr() + 4 * int(self.qoff[q]), len(self.queries[q])

    def score_dev(self, engine, q, s, go, ge, local):
        return engine.score_dev(*self._q(q), self.db.data_ptr() + 4 * int(self.off[s]), len(self.subjects[s]),
                                self.sub.data_ptr(), self.substsz, go, ge, local)

    def score_batch(self, engine, go, ge, local):
        """Query q against subject q, for every q."""
        ptrs = [self._q(q) + (self.db.data_ptr() + 4 * int(self.off[q]), len(self.subjects[q]))
                for q in range(len(self.queries))]
        return engine.score_batch_dev(ptrs, self.sub.data_ptr(), self.substsz, go, ge, local)

    def score_db(self, engine, q, go, ge, local):
        return engine.score_db_dev(*self._q(q), self.db.data_ptr(), self.off, self.sub.data_ptr(), self.substsz, go, ge,
                                   local)

    def score_multi(self, engine, go, ge, local):
        before = engine.last_launch()
        r = engine.score_db_multi_dev(self.q.data_ptr(), self.qoff, self.db.data_ptr(), self.off, self.sub.data_ptr(),
                                      self.substsz, go, ge, local, top=len(self.subjects))
        assert engine.last_launch() == before  # the call's own info says what ran
        return r, engine.last_score_db_multi_info()

    def align_db(self, engine, q, hits, go, ge, local):
        before = engine.last_launch()
        r = engine.align_db_dev(*self._q(q), self.db.data_ptr(), self.off, hits, self.sub.data_ptr(), self.substsz, go, ge,
                                local)
        assert engine.last_launch() == before
        return r, engine.last_align_db_info()

    def align_multi(self, engine, hq, hs, go, ge, local):
        before = engine.last_launch()
        r = engine.align_db_multi_dev(self.q.data_ptr(), self.qoff, self.db.data_ptr(), self.off, hq, hs,
                                      self.sub.data_ptr(), self.substsz, go, ge, local)
        assert engine.last_launch() == before
        return r, engine.last_align_db_multi_info()

    def want(self, q, s, go, ge, local):
        return exact(self.queries[q], self.subjects[s], self.subm, go, ge, local)

    def check_scores(self, res, q, go, ge, local):
        assert len(res) == len(self.subjects)
        for s, r in enumerate(res):
            assert _t(r) == self.want(q, s, go, ge, local), (q, s, go, ge, local, _t(r))

    def check_multi(self, r, go, ge, local):
        nq, n = len(self.queries), len(self.subjects)
        want = np.array([[self.want(q, s, go, ge, local) for s in range(n)] for q in range(nq)], dtype=np.int64)
        assert np.array_equal(r["scores"], want[:, :, 0]), (go, ge, local)
        for q in range(nq):
            order = sorted(range(n), key=lambda s: (-int(want[q, s, 0]), s))
            got = r["hits"][q]
            assert got["subject"].tolist() == order, (q, go, ge, local)
            for f, c in (("score", 0), ("i_end", 1), ("j_end", 2)):
                assert got[f].tolist() == want[q, order, c].tolist(), (q, f, go, ge, local)

    def check_aligned(self, res, hq, hs, go, ge, local, status1=()):
        """Scores and end cells exact for every hit; status 0 and a CIGAR that spans the reported cells
        and scores what the call reports, except for the hits named in status1 (score and end cell only)."""
        assert len(res) == len(hs)
        for h, (q, s, r) in enumerate(zip(hq, hs, res)):
            assert _t(r) == self.want(q, s, go, ge, local), (q, s, go, ge, local, r)
            if h in status1:
                assert r["status"] == 1 and r["cigar"] == "", (q, s, r)
                continue
            assert r["status"] == 0, (q, s, r)
            if not local:
                assert (r["i_start"], r["j_start"]) == (0, 0), (q, s, r)
            got = _exact.rescore(r["cigar"], self.queries[q], self.subjects[s], self.subm, go, ge, r["i_start"],
                                 r["j_start"], r["i_end"], r["j_end"])
            assert got == r["score"], (q, s, go, ge, local, got, r)


def _t(r):
    return (r["score"], r["i_end"], r["j_end"])


def _kind(engine):
    return engine.last_launch()["kind"]


def _ran_lanes(engine, n):
    ll = engine.last_launch()
    assert ll["kind"] == "score_lanes" and ll["npairs"] == n, ll


def _rejected(call):
    with pytest.raises(gsa.NwError) as ei:
        call()
    assert ei.value.stat == gsa.NwStat.errorInvalidValue


_NORMAL = {}


def _normal_call_is_right(engine, golden):
    """An ordinary call after a rejected one: the rejection left nothing behind."""
    if not _NORMAL:
        _NORMAL["p"] = _Pool([seq(130, 3)], [seq(c, 30 + c) for c in (70, 1, 200)], golden.blosum62)
    p = _NORMAL["p"]
    for local in (False, True):
        p.check_scores(p.score_db(engine, 0, -11, -1, local), 0, -11, -1, local)
        _ran_lanes(engine, 3)
        assert _t(p.score_dev(engine, 0, 2, -11, -1, local)) == p.want(0, 2, -11, -1, local)
        assert _kind(engine) == "score_krow"


@pytest.fixture(scope="module")
def kq(engine, golden):
    p = _Pool([seq(5, 1)], [seq(7, 2)], golden.blosum62)
    p.score_db(engine, 0, -11, -1, False)
    _ran_lanes(engine, 1)
    k = engine.last_launch()["k"]
    assert k == K_LANE, "tests/test_exact_reference.py builds its inputs with K_LANE"
    return k


# -- 1. global (and local) alignments at the largest gap costs -------------------------------------

@pytest.mark.parametrize("affine", [True, False], ids=["affine", "linear"])
def test_gap_costs_at_the_global_bound_row_scan(engine, golden, affine):
    """gsa_score_dev just inside B + |go| < 2^29: the span (R + C) |ge| is over 2^28, so the row scan
    runs (a 64-row tile boundary at 130 and 700 rows).  One step further a global pair is rejected
    before any launch and a local one still exact (H >= 0 keeps the sentinel out)."""
    t = table20()
    for R, C in SCAN_SHAPES:
        p = _Pool([scan_pair(R, C)[0]], [scan_pair(R, C)[1]], t)
        go, ge = gaps_at(GLOBAL_LIMIT, R, C, 11, affine, 1)
        for local in (False, True):
            assert _t(p.score_dev(engine, 0, 0, go, ge, local)) == p.want(0, 0, go, ge, local), (R, C, go, ge, local)
            assert _kind(engine) == "score_scan"
        go, ge = gaps_at(GLOBAL_LIMIT, R, C, 11, affine, 1, past=True)
        _rejected(lambda: p.score_dev(engine, 0, 0, go, ge, False))
        assert _t(p.score_dev(engine, 0, 0, go, ge, True)) == p.want(0, 0, go, ge, True), (R, C, go, ge)
        assert _kind(engine) == "score_scan"
    _normal_call_is_right(engine, golden)


@pytest.mark.parametrize("affine", [True, False], ids=["affine", "linear"])
def test_gap_costs_at_the_global_bound_batch(engine, golden, affine):
    """gsa_score_batch_dev with three such pairs: each runs alone on the row scan."""
    shapes = BATCH_SHAPES
    pairs = [scan_pair(R, C) for R, C in shapes]
    p = _Pool([y for y, _ in pairs], [x for _, x in pairs], table20())
    inside, past = batch_gaps(affine), batch_gaps(affine, past=True)
    assert max(bound(R, C, 11, *inside, 1) for R, C in shapes) < GLOBAL_LIMIT <= max(bound(R, C, 11, *past, 1) for R, C in shapes)
    for local in (False, True):
        res = p.score_batch(engine, *inside, local)
        assert _kind(engine) == "score_scan"
        for q, r in enumerate(res):
            assert _t(r) == p.want(q, q, *inside, local), (q, inside, local)
    _rejected(lambda: p.score_batch(engine, *past, False))
    res = p.score_batch(engine, *past, True)
    assert _kind(engine) == "score_scan"
    for q, r in enumerate(res):
        assert _t(r) == p.want(q, q, *past, True), (q, past)
    _normal_call_is_right(engine, golden)


@pytest.mark.parametrize("affine", [True, False], ids=["affine", "linear"])
@pytest.mark.parametrize("sweep", [0, 1, 2], ids=["16k-1", "16k+1", "32k+1"])
def test_gap_costs_at_the_global_bound_lanes(engine, golden, kq, sweep, affine):
    """gsa_score_db_dev and gsa_score_db_multi_dev on the lane kernels, the query on either side of a
    sweep boundary and over two, against 9 subjects of 1 .. 40 letters; two queries in the multi call."""
    R = sweep_rows(kq)[sweep]
    p = _Pool(db_queries(R), db_subjects(), table20())
    go, ge = gaps_at(GLOBAL_LIMIT, R, max(DB_LENS), 11, affine, 1)
    gp = gaps_at(GLOBAL_LIMIT, R, max(DB_LENS), 11, affine, 1, past=True)
    for local, g in [(False, (go, ge)), (True, (go, ge)), (True, gp)]:
        p.check_scores(p.score_db(engine, 0, *g, local), 0, *g, local)
        _ran_lanes(engine, len(DB_LENS))
        r, info = p.score_multi(engine, *g, local)
        assert (info["lane_queries"], info["other_queries"], info["lane_pairs"]) == (2, 0, 2 * len(DB_LENS)), info
        assert info["profile_builds"] >= 2, info
        p.check_multi(r, *g, local)
    _rejected(lambda: p.score_db(engine, 0, *gp, False))
    _rejected(lambda: p.score_multi(engine, *gp, False))
    _normal_call_is_right(engine, golden)


# -- 2. the int16 profile of the K-rows and strip score kernels -------------------------------------

@pytest.mark.parametrize("local", [False, True], ids=["global", "local"])
@pytest.mark.parametrize("kernel,k", [("krow", "2"), ("krow", "4"), ("strip", None)])
def test_int16_profile_edges(engine, knobs, kernel, k, local):
    """s - go - ge of 32767 and of -32767 run on the kernel; 32768 and -32768 make it raise its flag,
    and the row scan answers.  1100 x 70: more than one ticket at 2 and at 4 rows per lane.  Single, and
    in a batch among short pairs (the flag is the table's: every pair of that batch runs alone)."""
    if kernel == "strip":
        knobs("GSA_SCORE_KERNEL", "strip")
    else:
        knobs("GSA_SCORE_K", k)
    pairs = edge_pairs()
    for name, (value, runs) in EDGE_TABLES.items():
        t = edge_table(value)
        assert (-32767 <= value + 12 <= 32767) == runs
        p = _Pool([y for y, _ in pairs], [x for _, x in pairs], t)
        assert _t(p.score_dev(engine, 2, 2, -11, -1, local)) == p.want(2, 2, -11, -1, local), (name, local)
        ll = engine.last_launch()
        assert ll["kind"] == ("score_scan" if not runs else "score_" + kernel), (name, ll)
        if runs and kernel == "krow":
            assert ll["k"] == int(k) and ll["tickets"] >= 2, ll
        res = p.score_batch(engine, -11, -1, local)
        ll = engine.last_launch()
        assert ll["kind"] == ("score_scan" if not runs else "score_" + kernel), (name, ll)
        if runs and kernel == "krow":
            assert ll["npairs"] == len(pairs) and ll["k"] == int(k), ll
        for q, r in enumerate(res):
            assert _t(r) == p.want(q, q, -11, -1, local), (name, q, local)


# -- 3. local scores at 2^26 ------------------------------------------------------------------------

@pytest.mark.parametrize("kernel", ["krow", "strip"])
def test_local_score_at_2_to_26(engine, knobs, kernel):
    """Diagonal 32755, everything else -32755, -11 / -1, an identical pair: 2048 letters score
    67 082 240, under 2^26, on the score kernel; 2049 letters 67 114 995, over it, on the row scan."""
    if kernel == "strip":
        knobs("GSA_SCORE_KERNEL", "strip")
    t = diag_table(32755)
    for n, kind in [(2048, "score_" + kernel), (2049, "score_scan")]:
        y, x = sw_edge_pair(n)
        p = _Pool([y], [x], t)
        want = p.want(0, 0, -11, -1, True)
        assert want == (32755 * n, n, n) and (want[0] < 1 << 26) == (n == 2048)
        assert _t(p.score_dev(engine, 0, 0, -11, -1, True)) == want, n
        assert _kind(engine) == kind, n


# -- 4. the lane kernels' key: score bits ------------------------------------------------------------

@pytest.mark.parametrize("go,ge", [(-11, -1), (-11, -11)])
@pytest.mark.parametrize("over", [False, True], ids=["under", "over"])
def test_lane_key_score_bits(engine, kq, over, go, ge):
    """A local score of v (16 k + 1) just under 2^18 stays on the lane kernels in all four database
    calls; with v + 1 the pairs whose bound reaches 2^18 take the other path (status 1 in the align
    calls), and every result is the same kind of exact."""
    queries, subjects, t, v = key_score_pool(kq, over)
    R, n = len(queries[0]) - 1, len(subjects)
    p = _Pool(queries, subjects, t)
    assert p.want(0, 5, go, ge, True) == (v * R, R, R)
    p.check_scores(p.score_db(engine, 0, go, ge, True), 0, go, ge, True)
    _ran_lanes(engine, n - 1 if over else n)
    r, info = p.score_multi(engine, go, ge, True)
    assert (info["lane_queries"], info["other_queries"]) == ((0, 2) if over else (2, 0)), info
    p.check_multi(r, go, ge, True)
    res, info = p.align_db(engine, 0, list(range(n)), go, ge, True)
    assert (info["lane_hits"], info["unsupported"]) == ((n - 1, 1) if over else (n, 0)), info
    p.check_aligned(res, [0] * n, list(range(n)), go, ge, True, status1=[5] if over else [])
    hq, hs = [0] * n + [1] * n, list(range(n)) * 2
    res, info = p.align_multi(engine, hq, hs, go, ge, True)
    assert (info["lane_hits"], info["unsupported"]) == ((2 * n - 2, 2) if over else (2 * n, 0)), info
    p.check_aligned(res, hq, hs, go, ge, True, status1=[5, n + 5] if over else [])


# -- 5. the lane kernels' key: column bits -----------------------------------------------------------

@pytest.mark.parametrize("go,ge", [(-11, -1), (-11, -11)])
def test_lane_key_column_bits(engine, knobs, go, ge):
    """Subjects of 8190, 8191 and 8192 letters with GSA_DB_MAXC=8191: the best local segment in the
    first columns, ending in column 8191 (the key's column field is then 0), at both places in one row
    (the first is reported), and ending in column 8192, which the lane kernels do not take."""
    knobs("GSA_DB_MAXC", str(KEY_COLS))
    queries, subjects, t = key_column_pool()
    p = _Pool(queries, subjects, t)
    assert [len(x) - 1 for x in subjects] == [8190, 8191, 8191, 8192, 8190]
    assert [p.want(0, s, go, ge, True) for s in range(5)] == [(150, 30, 30), (150, 30, 8191), (150, 30, 30),
                                                              (150, 30, 8192), (150, 30, 8190)]
    for q in (0, 1):
        p.check_scores(p.score_db(engine, q, go, ge, True), q, go, ge, True)
        _ran_lanes(engine, 4)
    r, info = p.score_multi(engine, go, ge, True)
    assert (info["lane_queries"], info["other_queries"], info["lane_pairs"]) == (2, 0, 8), info
    p.check_multi(r, go, ge, True)
    res, info = p.align_db(engine, 0, [0, 1, 2, 3, 4], go, ge, True)
    assert (info["lane_hits"], info["unsupported"]) == (4, 1), info
    p.check_aligned(res, [0] * 5, [0, 1, 2, 3, 4], go, ge, True, status1=[3])
    assert [r["cigar"] for r in res] == ["30=", "30=", "30=", "", "30="]
    hq, hs = [0] * 5 + [1] * 5, [0, 1, 2, 3, 4] * 2
    res, info = p.align_multi(engine, hq, hs, go, ge, True)
    assert (info["lane_hits"], info["unsupported"]) == (8, 2), info
    p.check_aligned(res, hq, hs, go, ge, True, status1=[3, 8])


# -- 6. the trace fills' values ----------------------------------------------------------------------

@pytest.mark.parametrize("affine", [True, False], ids=["affine", "linear"])
def test_trace_values_at_2_to_26(engine, kq, affine):
    """Global alignments of a 16 k + 1 letter query with B just under 2^26 for the longest subject are
    traced on the device; one step further that hit alone (B >= 2^26) comes back with status 1 and its
    score intact.  The fills keep 4 x value + source, with -2^27 for minus infinity."""
    queries, subjects, t = trace_pool(kq)
    R, n = len(queries[0]) - 1, len(subjects)
    p = _Pool(queries, subjects, t)
    for past in (False, True):
        go, ge = gaps_at(TRACE_LIMIT, R, max(TRACE_LENS), 11, affine, 0, past=past)
        assert [bound(R, c, 11, go, ge, 0) >= TRACE_LIMIT for c in TRACE_LENS] == [False, False, past]
        res, info = p.align_db(engine, 0, list(range(n)), go, ge, False)
        assert (info["lane_hits"], info["unsupported"]) == ((n - 1, 1) if past else (n, 0)), info
        p.check_aligned(res, [0] * n, list(range(n)), go, ge, False, status1=[2] if past else [])
        assert [(r["i_end"], r["j_end"]) for r in res] == [(R, c) for c in TRACE_LENS]
        hq, hs = [0] * n + [1] * n, list(range(n)) * 2
        res, info = p.align_multi(engine, hq, hs, go, ge, False)
        assert (info["lane_hits"], info["unsupported"]) == ((2 * n - 2, 2) if past else (2 * n, 0)), info
        p.check_aligned(res, hq, hs, go, ge, False, status1=[2, n + 2] if past else [])
