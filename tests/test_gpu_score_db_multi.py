"""Many queries against one database in one call (gsa_score_db_multi_dev; nw_lanes_multi.hip, DESIGN.md
2.2f): every (query, subject) result exactly what oracle.score_ag gives (small cases) or what
score_db_dev gives for that query alone (larger ones; it is pinned to the oracle in
tests/test_gpu_score_db.py), the hits a host sort of the scores by (-score, subject), and
last_score_db_multi_info() for what ran.  No tolerances anywhere."""
import numpy as np
import pytest

import gpuseqalign_amd as gsa
from gpuseqalign_amd import formats as F
from tests import _align_oracle as ao
from tests.test_gpu_score import MODES

pytestmark = pytest.mark.gpu

SWEEP = 384  # query rows of one sweep (16 lanes x 24 rows)
_REF = {}


def _seq(n, seed, alphabet=20):
    return F.synthetic_seq(n, seed, alphabet)


def _oracle_rows(key, queries, subjects, sub, go, ge, local):
    """oracle.score_ag for every pair, [nq, nsubj, 3], computed once per (key, mode)."""
    import oracle
    k = (key, go, ge, local)
    if k not in _REF:
        _REF[k] = np.array([[oracle.score_ag(Y, X, sub, go, ge, local) for X in subjects] for Y in queries],
                           dtype=np.int64).reshape(len(queries), len(subjects), 3)
    return _REF[k]


class _Multi:
    """The queries in one buffer, the subjects in another, the table: on the device."""

    def __init__(self, queries, subjects, sub):
        import torch
        dev = torch.device("cuda:0")
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)
        self.queries, self.subjects, self.subm = queries, subjects, sub
        self.sub = up(np.asarray(sub).ravel())
        self.substsz = int(round(np.sqrt(np.asarray(sub).size)))
        self.q = up(np.concatenate(queries))
        self.db = up(np.concatenate(subjects))
        self.qoff = np.concatenate([[0], np.cumsum([len(x) for x in queries])]).astype(np.int64)
        self.off = np.concatenate([[0], np.cumsum([len(x) for x in subjects])]).astype(np.int64)
        torch.cuda.synchronize(dev)

    def run(self, engine, go, ge, local, qoff=None, off=None, **kw):
        """(result dict, info) of one multi call; top defaults to all subjects."""
        kw.setdefault("top", len(self.subjects))
        r = engine.score_db_multi_dev(self.q.data_ptr(), self.qoff if qoff is None else qoff, self.db.data_ptr(),
                                      self.off if off is None else off, self.sub.data_ptr(), self.substsz, go, ge, local,
                                      **kw)
        return r, engine.last_score_db_multi_info()

    def single(self, engine, go, ge, local):
        """score_db_dev per query: [nq, nsubj, 3]."""
        rows = []
        for k in range(len(self.queries)):
            res = engine.score_db_dev(self.q.data_ptr() + 4 * int(self.qoff[k]), len(self.queries[k]), self.db.data_ptr(),
                                      self.off, self.sub.data_ptr(), self.substsz, go, ge, local)
            rows.append([(r["score"], r["i_end"], r["j_end"]) for r in res])
        return np.array(rows, dtype=np.int64).reshape(len(self.queries), len(self.subjects), 3)


def _check_ranked(r, want, top=None):
    """scores and hits of a result against want[nq, nsubj, 3]: the ranking is the host's sort."""
    nq, n, _ = want.shape
    ntop = n if top is None else min(top, n)
    if r["scores"] is not None:
        assert r["scores"].shape == (nq, n) and r["scores"].dtype == np.int32
        assert np.array_equal(r["scores"], want[:, :, 0])
    if r["hits"] is not None:
        assert r["hits"].shape == (nq, ntop)
        for q in range(nq):
            order = sorted(range(n), key=lambda s: (-int(want[q, s, 0]), s))[:ntop]
            got = r["hits"][q]
            assert got["subject"].tolist() == order, (q, got["subject"].tolist(), order)
            for f, c in (("score", 0), ("i_end", 1), ("j_end", 2)):
                assert got[f].tolist() == want[q, order, c].tolist(), (q, f)


def _mixed_subjects(n, seed):
    """Lengths 1..300 mixed; a subject of one letter beside one of 300, and one with no letters."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(1, 301, n)
    lens[0], lens[1], lens[n // 2] = 300, 1, 0
    return [_seq(int(c), seed * 1000 + i) for i, c in enumerate(lens)]


# -- 1. query switching ----------------------------------------------------------------------------

_SWITCH = {}


@pytest.mark.parametrize("go,ge,local", MODES)
def test_one_workgroup_runs_every_query_over_the_same_lds(engine, golden, go, ge, local):
    """Queries on every edge of a lane's rows and of a sweep, one, two and three sweeps: with one
    workgroup the profile is built once per query, and every grid gives the same results."""
    if not _SWITCH:
        lens = [1, 23, 24, 25, 200, SWEEP - 1, SWEEP, SWEEP + 1, 2 * SWEEP + 1]
        _SWITCH["m"] = _Multi([_seq(R, 300 + R) for R in lens], _mixed_subjects(70, 7), golden.blosum62)
    m = _SWITCH["m"]
    want = _oracle_rows("switch", m.queries, m.subjects, m.subm, go, ge, local)
    r1, i1 = m.run(engine, go, ge, local, max_workgroups=1)
    assert i1["workgroups"] == 1 and i1["lane_queries"] == len(m.queries) and i1["other_queries"] == 0, i1
    assert i1["profile_builds"] == i1["lane_queries"], i1
    assert i1["launches"] == 3, i1  # the sweep classes
    assert i1["lane_pairs"] == len(m.queries) * 69, i1
    _check_ranked(r1, want)
    for wg in (2, 0):
        r, info = m.run(engine, go, ge, local, max_workgroups=wg)
        assert info["lane_queries"] == len(m.queries) and info["profile_builds"] >= info["launches"], info
        if wg:
            assert info["workgroups"] <= wg, info
        assert np.array_equal(r["scores"], r1["scores"]) and np.array_equal(r["hits"], r1["hits"]), wg


# -- 2. edges of the task and unit grid ------------------------------------------------------------

_GRID = {}


def _grid_pool(golden):
    if not _GRID:
        rng = np.random.default_rng(5)
        queries = [_seq(int(c), 4000 + i) for i, c in enumerate(rng.integers(1, 121, 33))]
        queries[1] = _seq(0, 1)          # an empty query among real ones
        queries[3] = queries[0].copy()   # two identical queries
        subjects = [_seq(int(c), 5000 + i) for i, c in enumerate(rng.integers(1, 151, 130))]
        _GRID["pool"] = (queries, subjects)
    return _GRID["pool"]


@pytest.mark.parametrize("nq", [1, 2, 5, 33])
@pytest.mark.parametrize("go,ge,local", [(-11, -1, True), (-11, -11, False)])
def test_task_and_unit_edges(engine, golden, go, ge, local, nq):
    queries, subjects = _grid_pool(golden)
    want = _oracle_rows("grid", queries, subjects, golden.blosum62, go, ge, local)
    unit = 4 * gsa.score_db_multi_unit()  # subjects of a unit
    for nsubj in sorted({1, 3, 4, 5, 65, 130, unit - 4, unit, unit + 4}):
        assert 1 <= nsubj <= len(subjects)
        key = (nq, nsubj)
        if key not in _GRID:
            _GRID[key] = _Multi(queries[:nq], subjects[:nsubj], golden.blosum62)
        r, info = _GRID[key].run(engine, go, ge, local)
        lane_q = sum(len(q) > 1 for q in queries[:nq])
        assert info["lane_queries"] == lane_q and info["lane_pairs"] == lane_q * nsubj, (key, info)
        tasks = -(-nsubj // 4)
        assert info["units"] == lane_q * -(-tasks // gsa.score_db_multi_unit()), (key, info)
        _check_ranked(r, want[:nq, :nsubj])
        if nq >= 5:
            assert np.array_equal(r["scores"][0], r["scores"][3])


# -- 3. stale profile ------------------------------------------------------------------------------

def test_short_query_after_a_long_one_sees_none_of_its_rows(engine, golden):
    """One workgroup runs a query of 383 letters, then one of 5 in the same LDS.  Letter 0 -- the
    header element of the next query in the buffer, what a read past a query's end finds -- scores
    +15 against every subject letter, and no sequence holds it."""
    n = int(round(np.sqrt(golden.blosum62.size)))
    sub = np.array(golden.blosum62, dtype=np.int32).reshape(n, n).copy()
    sub[0, :] = 15

    def letters(c, seed):
        x = _seq(c, seed, 19)
        x[1:] += 1  # letters 1..19
        return x

    m = _Multi([letters(SWEEP - 1, 1), letters(5, 2), letters(5, 3)], [letters(c, 10 + c) for c in (300, 30, 7, 120, 5, 64)], sub)
    for go, ge, local in [(-11, -1, True), (-11, -11, True), (-11, -1, False)]:
        want = _oracle_rows("stale", m.queries, m.subjects, sub, go, ge, local)
        r, info = m.run(engine, go, ge, local, max_workgroups=1)
        assert info["profile_builds"] == 3 and info["workgroups"] == 1, info
        _check_ranked(r, want)


# -- 4. ranking ------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def planted(engine):
    """Match +5, everything else -4.  Subjects 3, 9 and 17 are copies of subject 0 (equal scores
    against every query), and five subjects of letters no query holds score 0 in local mode."""
    sub = np.full((20, 20), -4, np.int32)
    np.fill_diagonal(sub, 5)
    subjects = [_seq(int(c), 600 + i, 10) for i, c in enumerate(np.random.default_rng(3).integers(20, 90, 22))]
    for k in (3, 9, 17):
        subjects[k] = subjects[0].copy()
    for k in (2, 5, 11, 12, 21):
        subjects[k] = subjects[k] + np.where(np.arange(len(subjects[k])) > 0, 10, 0).astype(np.int32)
    m = _Multi([_seq(R, 700 + R, 10) for R in (40, 3, 150)], subjects, sub)
    return m, {mode: m.single(engine, *mode) for mode in [(-11, -1, True), (-5, -5, False)]}


@pytest.mark.parametrize("top", [1, 3, 22, 27])
def test_ranking(engine, planted, top):
    m, refs = planted
    for (go, ge, local), want in refs.items():
        assert (want[:, 3] == want[:, 0]).all() and (want[:, 17] == want[:, 0]).all()
        if local:
            assert (want[:, [2, 5, 11, 12, 21], 0] == 0).all()
        r, _ = m.run(engine, go, ge, local, top=top)
        _check_ranked(r, want, top)
        only_hits, _ = m.run(engine, go, ge, local, top=top, want_scores=False)
        assert only_hits["scores"] is None and np.array_equal(only_hits["hits"], r["hits"])
    only_scores, info = m.run(engine, -11, -1, True, top=0)
    assert only_scores["hits"] is None and info["select_ms"] >= 0.0
    assert np.array_equal(only_scores["scores"], refs[(-11, -1, True)][:, :, 0])


# -- 5. chunks -------------------------------------------------------------------------------------

def test_chunks(engine, golden):
    queries = [_seq(int(c), 800 + i) for i, c in enumerate([50, 120, 7, 90, 33, 200, 61])]
    m = _Multi(queries, _mixed_subjects(20, 9), golden.blosum62)
    row = 16 * len(m.subjects)
    for go, ge, local in [(-11, -1, True), (-11, -11, False)]:
        whole, iw = m.run(engine, go, ge, local)
        assert iw["launches"] == 1 and iw["result_bytes"] == 7 * row, iw
        limit = 2 * row + row // 2  # two rows at a time: 4 chunks
        r, info = m.run(engine, go, ge, local, scratch_limit=limit)
        assert info["launches"] == 4 and info["result_bytes"] == 2 * row <= limit, info
        assert info["lane_queries"] == 7 and info["units"] == iw["units"] and info["lane_pairs"] == iw["lane_pairs"], info
        assert np.array_equal(r["scores"], whole["scores"]) and np.array_equal(r["hits"], whole["hits"])
        _check_ranked(r, _oracle_rows("chunks", m.queries, m.subjects, m.subm, go, ge, local))
        one, i1 = m.run(engine, go, ge, local, scratch_limit=row)
        assert i1["launches"] == 7 and i1["result_bytes"] == row, i1
        assert np.array_equal(one["hits"], whole["hits"])
    with pytest.raises(gsa.NwError) as ei:
        m.run(engine, -11, -1, True, scratch_limit=row - 1)
    assert ei.value.stat == gsa.NwStat.errorInvalidValue


# -- 6. routing ------------------------------------------------------------------------------------

@pytest.mark.parametrize("go,ge,local", [(-11, -1, True), (-11, -11, True), (-11, -1, False)])
def test_routing_knobs(engine, golden, knobs, go, ge, local):
    lens = [100, 200] * 15 + [128, 129, 100]
    m = _Multi([_seq(R, 30 + R) for R in (150, 40, 400)], [_seq(c, 70 + i) for i, c in enumerate(lens)], golden.blosum62)
    want = m.single(engine, go, ge, local)
    r0, i0 = m.run(engine, go, ge, local)
    assert i0["lane_pairs"] == 3 * len(lens) and i0["lane_queries"] == 3, i0
    _check_ranked(r0, want)
    knobs("GSA_DB_MAXC", "128")
    ra, ia = m.run(engine, go, ge, local)
    assert ia["lane_pairs"] == i0["lane_pairs"] - 3 * sum(c > 128 for c in lens) and ia["lane_queries"] == 3, ia
    _check_ranked(ra, want)
    knobs("GSA_DB_LANES", "0")
    rb, ib = m.run(engine, go, ge, local)
    assert ib["lane_queries"] == 0 and ib["other_queries"] == 3 and ib["launches"] == 0 and ib["lane_pairs"] == 0, ib
    _check_ranked(rb, want)
    assert np.array_equal(ra["hits"], rb["hits"]) and np.array_equal(ra["hits"], r0["hits"])


def test_query_past_the_local_key_bound_goes_whole_through_the_other_path(engine, golden):
    """30000 x min(100, C) does not fit a row's best key (2^18); 30000 x 5 does."""
    sub = np.full((20, 20), -30000, np.int32)
    np.fill_diagonal(sub, 30000)
    subjects = [_seq(int(c), 2200 + i) for i, c in enumerate([90, 150, 120, 101, 97, 133])]
    m = _Multi([_seq(5, 13), _seq(100, 14), _seq(8, 15)], subjects, sub)
    r, info = m.run(engine, -11, -1, True)
    assert info["other_queries"] == 1 and info["lane_queries"] == 2 and info["lane_pairs"] == 12, info
    _check_ranked(r, _oracle_rows("big", m.queries, m.subjects, sub, -11, -1, True))
    r, info = m.run(engine, -11, -1, False)  # global: no key
    assert info["other_queries"] == 0 and info["lane_queries"] == 3, info
    _check_ranked(r, _oracle_rows("big", m.queries, m.subjects, sub, -11, -1, False))


@pytest.mark.parametrize("go,ge,local", MODES)
def test_tables(engine, golden, go, ge, local):
    """An asymmetric table (row = query letter), and one with values outside int8."""
    rng = np.random.default_rng(11)
    asym = rng.integers(-6, 12, size=(20, 20)).astype(np.int32)
    assert not np.array_equal(asym, asym.T)
    wide = np.full((20, 20), -200, np.int32)
    np.fill_diagonal(wide, 300)
    for name, sub in [("asym", asym), ("wide", wide)]:
        if name not in _GRID:
            subjects = [_seq(int(c), 2100 + i) for i, c in enumerate(rng.integers(1, 151, 20))]
            _GRID[name] = _Multi([_seq(90, 13), _seq(17, 14), _seq(130, 15)], subjects, sub)
        m = _GRID[name]
        r, info = m.run(engine, go, ge, local)
        assert info["lane_queries"] == 3 and info["lane_pairs"] == 60, info
        _check_ranked(r, _oracle_rows(("tab", name), m.queries, m.subjects, sub, go, ge, local))


# -- 7. neighbours ---------------------------------------------------------------------------------

def test_neighbours_keep_their_record_and_their_results(engine, golden, knobs):
    sub = golden.blosum62
    queries = [_seq(R, 900 + R) for R in (60, 500, 130)]
    subjects = [_seq(int(c), 950 + i) for i, c in enumerate([80, 200, 33, 150, 7, 260, 90, 121, 64])]
    m = _Multi(queries, subjects, sub)
    knobs("GSA_DB_MAXC", "250")  # subject 5 takes the batched path inside the multi call
    first = m.single(engine, -11, -1, True)
    before = engine.last_launch()
    assert before["kind"] == "score_lanes" and before["npairs"] == 8, before
    r, info = m.run(engine, -11, -1, True)
    assert info["lane_pairs"] == 3 * 8, info
    assert engine.last_launch() == before
    _check_ranked(r, first)
    # score_db_dev and align_db_dev share context buffers with the multi call: right after it
    again = m.single(engine, -11, -1, True)
    assert np.array_equal(again, first)
    assert np.array_equal(first, _oracle_rows("nb", queries, subjects, sub, -11, -1, True))
    hits = [int(s) for s in r["hits"][1]["subject"][:3]]
    al = engine.align_db_dev(m.q.data_ptr() + 4 * int(m.qoff[1]), len(queries[1]), m.db.data_ptr(), m.off, hits,
                             m.sub.data_ptr(), m.substsz, -11, -1, True)
    for h, a in zip(hits, al):
        want = ao.align(queries[1], subjects[h], sub, -11, -1, True)
        assert tuple(a[f] for f in ("score", "i_start", "j_start", "i_end", "j_end", "cigar")) == want, h


def test_mem_stats_count_the_new_buffers(golden):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    queries = [_seq(100, 40 + i) for i in range(16)]
    subjects = [_seq(150, 60 + i) for i in range(512)]
    with gsa.Engine(0) as e:
        m = _Multi(queries, subjects, golden.blosum62)
        e.reset_mem_stats()
        r, info = m.run(e, -11, -1, True, top=5)
        pairs = len(queries) * len(subjects)
        assert info["result_bytes"] == 16 * pairs, info
        # the matrix, the ranking's keys in and out, the compacted scores
        assert e.mem_stats()["glmem_peak_allocs"] >= (16 + 16 + 4) * pairs
        assert r["hits"].shape == (16, 5)


# -- 8. host forms ---------------------------------------------------------------------------------

def test_host_forms(engine, golden):
    queries = [_seq(R, 1100 + R) for R in (120, 0, 45)]
    subjects = [_seq(int(c), 1200 + i) for i, c in enumerate(np.random.default_rng(8).integers(0, 200, 40))]
    m = _Multi(queries, subjects, golden.blosum62)
    for go, ge, local in [(-11, -1, True), (-11, -11, False)]:
        dev, _ = m.run(engine, go, ge, local, top=4)
        host = engine.score_db_multi(queries, subjects, golden.blosum62, go, ge, local, top=4)
        assert np.array_equal(host["scores"], dev["scores"]) and np.array_equal(host["hits"], dev["hits"])
        multi = engine.search_db_multi(queries, subjects, golden.blosum62, go, ge, local, top=4)
        loop = [engine.search_db(q, subjects, golden.blosum62, go, ge, local, top=4) for q in queries]
        strip = lambda rows: [[(s, {k: v for k, v in d.items() if k != "kernel_ms"}) for s, d in row] for row in rows]
        assert strip(multi) == strip(loop)
        assert [len(row) for row in multi] == [4, 4, 4]


# -- 9. invalid input ------------------------------------------------------------------------------

def test_invalid_input(engine, golden):
    m = _Multi([_seq(60, 4), _seq(20, 5), _seq(33, 6)], [_seq(int(c), 1300 + c) for c in (5, 80, 41, 17, 66)], golden.blosum62)
    want = _oracle_rows("inv", m.queries, m.subjects, m.subm, -11, -1, False)
    before = engine.last_launch()

    def bad(go=-11, ge=-1, **kw):
        with pytest.raises(gsa.NwError) as ei:
            m.run(engine, go, ge, False, **kw)
        assert ei.value.stat == gsa.NwStat.errorInvalidValue, kw
        assert engine.last_launch() == before

    for table in ("qoff", "off"):
        src = getattr(m, table)
        equal, dec, neg = src.copy(), src.copy(), src.copy()
        equal[2] = equal[1]
        dec[2] = dec[1] - 1
        neg[0] = -1
        for off in (equal, dec, neg, src[:1]):  # the last: nq / nsubj = 0
            bad(**{table: off})
    bad(go=-1, ge=-11)
    bad(ge=1, go=-11)
    bad(top=-1)
    bad(max_workgroups=-1)
    bad(scratch_limit=-1)
    bad(top=0, want_scores=False)   # both outputs null
    # hits null with top > 0 and scores null: straight through the C entry point
    import ctypes
    i64p = ctypes.POINTER(ctypes.c_int64)
    st = gsa.lib().gsa_score_db_multi_dev(engine._h, m.q.data_ptr(), m.qoff.ctypes.data_as(i64p), 3, m.db.data_ptr(),
                                          m.off.ctypes.data_as(i64p), 5, m.sub.data_ptr(), m.substsz, -11, -1, 0, 3, 0, 0,
                                          None, None, None, None, None)
    assert st == gsa.NwStat.errorInvalidValue
    for name in ("queries", "db", "subst"):  # a null device pointer
        ptr = {"queries": m.q.data_ptr(), "db": m.db.data_ptr(), "subst": m.sub.data_ptr()}
        ptr[name] = None
        with pytest.raises(gsa.NwError) as ei:
            engine.score_db_multi_dev(ptr["queries"], m.qoff, ptr["db"], m.off, ptr["subst"], m.substsz, -11, -1, False)
        assert ei.value.stat == gsa.NwStat.errorInvalidValue, name
    for substsz in (0, 33):
        with pytest.raises(gsa.NwError) as ei:
            engine.score_db_multi_dev(m.q.data_ptr(), m.qoff, m.db.data_ptr(), m.off, m.sub.data_ptr(), substsz, -11, -1, False)
        assert ei.value.stat == gsa.NwStat.errorInvalidValue, substsz
    r, _ = m.run(engine, -11, -1, False)
    _check_ranked(r, want)
