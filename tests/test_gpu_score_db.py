"""Database search (gsa_score_db_dev: one query against many short subjects, every subject on 16
lanes of a wave of the lane kernel, nw_lanes.hip) against oracle.score_ag per subject.  Every case
that expects the lane kernel asserts gsa_last_launch: kind score_lanes and npairs = the subjects it
took.  A lane holds k = last_launch()["k"] query rows; one sweep covers 16 k rows, a longer query
takes several sweeps over a boundary row."""
import numpy as np
import pytest

import gpuseqalign_amd as gsa
from gpuseqalign_amd import formats as F
from tests.test_gpu_score import MODES

pytestmark = pytest.mark.gpu

LANES_PER_SUBJECT = 16
_REF = {}


def _ref(key, Y, X, sub, go, ge, local):
    """oracle.score_ag, computed once per (pair, table, mode) and shared by the cases."""
    import oracle
    k = (key, go, ge, local)
    if k not in _REF:
        _REF[k] = oracle.score_ag(Y, X, sub, go, ge, local)
    return _REF[k]


def _seq(n, seed, alphabet=20):
    return F.synthetic_seq(n, seed, alphabet)


class _Db:
    """Query, the subjects in one buffer and the table on the device."""

    def __init__(self, query, subjects, sub):
        import torch
        dev = torch.device("cuda:0")
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)
        self.query, self.subjects, self.subm = query, subjects, sub
        self.sub = up(np.asarray(sub).ravel())
        self.substsz = int(round(np.sqrt(np.asarray(sub).size)))
        self.q = up(query)
        self.db = up(np.concatenate(subjects))
        self.off = np.concatenate([[0], np.cumsum([len(x) for x in subjects])]).astype(np.int64)
        torch.cuda.synchronize(dev)

    def run(self, engine, go, ge, local, off=None):
        return engine.score_db_dev(self.q.data_ptr(), self.q.numel(), self.db.data_ptr(),
                                   self.off if off is None else off, self.sub.data_ptr(), self.substsz, go, ge, local)

    def check(self, res, key, go, ge, local):
        assert len(res) == len(self.subjects)
        for s, (X, r) in enumerate(zip(self.subjects, res)):
            want = _ref((key, s), self.query, X, self.subm, go, ge, local)
            assert _t(r) == want, (key, s, len(self.query) - 1, len(X) - 1, _t(r), want)


def _t(r):
    return (r["score"], r["i_end"], r["j_end"])


def _ran_lanes(engine, n):
    ll = engine.last_launch()
    assert ll["kind"] == "score_lanes" and ll["npairs"] == n, ll
    assert ll["tickets"] == -(-n // (64 // LANES_PER_SUBJECT)) and ll["ns"] == 4, ll
    return ll


def _mixed_subjects(n, seed):
    """Lengths 1..300 mixed; a subject of one letter beside one of 300, and one with no letters."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(1, 301, n)
    lens[0] = 300
    if n > 1:
        lens[1] = 1
    if n > 2:
        lens[n // 2] = 0
    return [_seq(int(c), seed * 1000 + i) for i, c in enumerate(lens)]


@pytest.fixture(scope="module")
def kq(engine, golden):
    d = _Db(_seq(5, 1), [_seq(7, 2)], golden.blosum62)
    d.run(engine, -11, -1, False)
    return _ran_lanes(engine, 1)["k"]


_WAVE = {}


@pytest.mark.parametrize("nsubj", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("go,ge,local", MODES)
def test_wave_edges(engine, golden, go, ge, local, nsubj):
    if nsubj not in _WAVE:
        _WAVE[nsubj] = _Db(_seq(200, 77), _mixed_subjects(nsubj, nsubj), golden.blosum62)
    d = _WAVE[nsubj]
    res = d.run(engine, go, ge, local)
    _ran_lanes(engine, sum(len(x) > 1 for x in d.subjects))
    d.check(res, ("wave", nsubj), go, ge, local)


def _many(n, seed, lo, hi):
    rng = np.random.default_rng(seed)
    return [_seq(int(c), seed * 1000 + i) for i, c in enumerate(rng.integers(lo, hi + 1, n))]


_STRIP = {}


@pytest.mark.parametrize("go,ge,local", MODES)
def test_strip_edges(engine, golden, kq, go, ge, local):
    """The global result cell and the local maximum on the first and last register row of a lane, on
    either side of the hand-off between two lanes, and (16 k - 1 ... 2 x 16 k + 1) of a sweep."""
    sweep = LANES_PER_SUBJECT * kq
    for R in [1, kq - 1, kq, kq + 1, 2 * kq + 1, 300, sweep - 1, sweep, sweep + 1, 2 * sweep + 1]:
        if R not in _STRIP:
            _STRIP[R] = _Db(_seq(R, 500 + R), _many(70, R, 1, 120), golden.blosum62)
        d = _STRIP[R]
        res = d.run(engine, go, ge, local)
        _ran_lanes(engine, 70)
        d.check(res, ("strip", R), go, ge, local)


def _local_matrix(Y, X, sub, go, ge):
    """H of the local affine recurrence (oracle/score_oracle.c), a plain fill."""
    R, C = len(Y) - 1, len(X) - 1
    neg = -(1 << 29)
    H = np.zeros((R + 1, C + 1), np.int64)
    Fc = np.full(C + 1, neg, np.int64)
    for i in range(1, R + 1):
        E = neg
        for j in range(1, C + 1):
            E = max(E + ge, H[i, j - 1] + go)
            Fc[j] = max(Fc[j] + ge, H[i - 1, j] + go)
            H[i, j] = max(H[i - 1, j - 1] + sub[Y[i], X[j]], E, Fc[j], 0)
    return H


@pytest.mark.parametrize("go,ge", [(-11, -11), (-11, -1), (-5, -2)])
def test_ties(engine, golden, kq, go, ge):
    """Two maxima in one row, two in one column (the copies on different lanes, and in different
    sweeps), an all-mismatch pair: the first cell in row-major order.  Match +5, everything else -4;
    the spacer letter matches nothing."""
    n = int(round(np.sqrt(golden.blosum62.size)))
    sub = np.full((n, n), -4, np.int32)
    np.fill_diagonal(sub[:20, :20], 5)
    seg = _seq(30, 9)[1:]
    sp = lambda k: np.full(k, 22, np.int32)
    hdr = lambda a: np.concatenate([[0], a]).astype(np.int32)
    sweep = LANES_PER_SUBJECT * kq
    cases = [
        (hdr(seg), hdr(np.concatenate([seg, sp(7), seg])), (150, 30, 30)),
        (hdr(np.concatenate([seg, sp(2 * kq), seg])), hdr(seg), (150, 30, 30)),
        (hdr(np.concatenate([sp(3), seg, sp(sweep), seg])), hdr(np.concatenate([sp(5), seg])), (150, 33, 35)),
        (hdr(np.full(40, 3, np.int32)), hdr(np.full(50, 7, np.int32)), (0, 0, 0)),
    ]
    for Y, X, want in cases[:3]:
        H = _local_matrix(Y, X, sub, go, ge)
        assert H.max() == want[0] and (H == H.max()).sum() >= 2, "the planted pair has one maximal cell only"
        i, j = np.argwhere(H == H.max())[0]
        assert (int(i), int(j)) == want[1:]
    for c, (Y, X, want) in enumerate(cases):
        subjects = _many(5, 40 + c, 1, 90) + [X] + _many(3, 50 + c, 1, 90)
        d = _Db(Y, subjects, sub)
        res = d.run(engine, go, ge, True)
        _ran_lanes(engine, len(subjects))
        assert _t(res[5]) == want, (c, _t(res[5]))
        d.check(res, ("ties", c), go, ge, True)


def test_nothing_right_of_the_last_column_scores(engine, golden):
    """Waves whose longest subject is 10 x the shortest, local affine.  Letter 0 -- the header element
    of the next subject in the buffer, what a read past a subject's end finds -- scores +15 against
    every query letter, and no subject holds it."""
    n = int(round(np.sqrt(golden.blosum62.size)))
    sub = np.array(golden.blosum62, dtype=np.int32).reshape(n, n).copy()
    sub[:, 0] = 15
    lens = [300, 30, 30, 30, 290, 29, 31, 30, 300, 30]
    subjects = []
    for i, c in enumerate(lens):
        x = _seq(c, 900 + i, 19)
        x[1:] += 1  # letters 1..19
        subjects.append(x)
    q = _seq(100, 5, 19)
    q[1:] += 1
    d = _Db(q, subjects, sub)
    res = d.run(engine, -11, -1, True)
    _ran_lanes(engine, len(lens))
    d.check(res, "pad", -11, -1, True)


@pytest.mark.parametrize("go,ge,local", [(-11, -1, True), (-11, -11, False), (-11, -1, False)])
def test_back_to_back_calls(engine, golden, knobs, go, ge, local):
    """Long subjects, then short ones, on one context and a query of two sweeps: stale boundary rows
    or task state would show in the second call."""
    knobs("GSA_DB_MAXC", "1000")  # the long ones on the lane kernel too, whatever the default
    q = _seq(500, 31)
    long_ = _Db(q, _many(40, 7, 600, 900), golden.blosum62)
    short = _Db(q, _many(90, 8, 1, 60), golden.blosum62)
    r1 = long_.run(engine, go, ge, local)
    _ran_lanes(engine, 40)
    r2 = short.run(engine, go, ge, local)
    _ran_lanes(engine, 90)
    long_.check(r1, "b2b-long", go, ge, local)
    short.check(r2, "b2b-short", go, ge, local)


@pytest.mark.parametrize("go,ge,local", [(-11, -1, True), (-11, -11, True), (-11, -1, False)])
def test_routing(engine, golden, knobs, go, ge, local):
    lens = [100, 200] * 15 + [128, 129, 100]
    d = _Db(_seq(150, 3), [_seq(c, 70 + i) for i, c in enumerate(lens)], golden.blosum62)
    knobs("GSA_DB_MAXC", "128")
    ra = d.run(engine, go, ge, local)
    _ran_lanes(engine, sum(c <= 128 for c in lens))
    d.check(ra, "route", go, ge, local)
    knobs("GSA_DB_LANES", "0")
    rb = d.run(engine, go, ge, local)
    ll = engine.last_launch()
    assert ll["kind"] == "score_krow" and ll["npairs"] == len(lens), ll
    d.check(rb, "route", go, ge, local)
    assert [_t(r) for r in ra] == [_t(r) for r in rb]


@pytest.mark.parametrize("go,ge,local", MODES)
def test_tables(engine, golden, go, ge, local):
    """An asymmetric table (row = query letter), and one with values outside int8."""
    rng = np.random.default_rng(11)
    asym = rng.integers(-6, 12, size=(20, 20)).astype(np.int32)
    assert not np.array_equal(asym, asym.T)
    wide = np.full((20, 20), -200, np.int32)
    np.fill_diagonal(wide, 300)
    for name, sub in [("asym", asym), ("wide", wide)]:
        d = _Db(_seq(90, 13), _many(20, 21, 1, 150), sub)
        res = d.run(engine, go, ge, local)
        _ran_lanes(engine, 20)
        d.check(res, ("tab", name), go, ge, local)


def test_large_local_scores_take_the_other_path(engine, golden):
    """A local score bound of 2^18 or more (30000 x 100) does not fit a row's best key."""
    sub = np.full((20, 20), -30000, np.int32)
    np.fill_diagonal(sub, 30000)
    d = _Db(_seq(100, 13), _many(6, 22, 90, 150), sub)
    res = d.run(engine, -11, -1, True)
    assert engine.last_launch()["kind"] != "score_lanes"
    d.check(res, "big", -11, -1, True)
    res = d.run(engine, -11, -1, False)  # global: no key
    _ran_lanes(engine, 6)
    d.check(res, "big", -11, -1, False)


def test_host_form(engine, golden):
    q = _seq(120, 4)
    subjects = _many(12, 5, 0, 200)
    for go, ge, local in [(-11, -1, True), (-11, -11, False)]:
        a = engine.score_db(q, subjects, golden.blosum62, go, ge, local)
        b = engine.score_batch([(q, x) for x in subjects], golden.blosum62, go, ge, local)
        assert [_t(r) for r in a] == [_t(r) for r in b]


def test_invalid_input(engine, golden):
    d = _Db(_seq(60, 4), _many(9, 6, 1, 80), golden.blosum62)

    def good():
        res = d.run(engine, -11, -1, False)
        _ran_lanes(engine, 9)
        d.check(res, "inv", -11, -1, False)

    def bad(go, ge, off=None):
        with pytest.raises(gsa.NwError) as ei:
            d.run(engine, go, ge, False, off=off)
        assert ei.value.stat == gsa.NwStat.errorInvalidValue
        good()

    equal, dec = d.off.copy(), d.off.copy()
    equal[4] = equal[3]
    dec[4] = dec[3] - 1
    bad(-11, -1, equal)
    bad(-11, -1, dec)
    bad(-11, -1, d.off[:1])  # nsubj = 0
    bad(-1, -11)
