"""Semi-global database search, scores and ranking (gsa_score_db_multi_semi_dev; nw_lanes_semi.hip,
DESIGN.md 2.2h): every (query, subject) result -- score and end cell (R, smallest column of row R
that attains the score) -- exactly what tests/_semi_oracle.py gives, in a linear and an affine gap
model; the hits a host sort of the scores by (-score, subject); last_score_db_semi_info() for what
ran; every refusal.  No tolerances anywhere."""
import ctypes

import numpy as np
import pytest

import gpuseqalign_amd as gsa
from tests import _semi_oracle as so
from tests import test_semi_oracle as hand
from tests.test_gpu_score_db_multi import _check_ranked, _mixed_subjects, _Multi, _seq

pytestmark = pytest.mark.gpu

SWEEP = 384  # query rows of one sweep (16 lanes x 24 rows)
GAPS = [(-11, -1), (-4, -4)]  # affine, linear
_REF = {}
_POOL = {}


def _want(key, m, go, ge):
    """The oracle's (score, i_end, j_end) of every pair, [nq, nsubj, 3], computed once per (key, gaps)."""
    k = (key, go, ge)
    if k not in _REF:
        _REF[k] = np.array([[so.score(Y, X, m.subm, go, ge) for X in m.subjects] for Y in m.queries],
                           dtype=np.int64).reshape(len(m.queries), len(m.subjects), 3)
    return _REF[k]


def _run(engine, m, go, ge, qoff=None, off=None, **kw):
    """(result dict, info) of one semi-global call; top defaults to all subjects."""
    kw.setdefault("top", len(m.subjects))
    r = engine.score_db_semi_dev(m.q.data_ptr(), m.qoff if qoff is None else qoff, m.db.data_ptr(),
                                 m.off if off is None else off, m.sub.data_ptr(), m.substsz, go, ge, **kw)
    return r, engine.last_score_db_semi_info()


# -- 1. every position of the result row, every sweep edge -----------------------------------------

@pytest.mark.parametrize("go,ge", GAPS + [(0, 0), (-3, 0)])
def test_row_positions_and_sweep_edges(engine, golden, go, ge):
    """Queries whose last row sits on every edge of a lane's rows and of a sweep, one to three sweeps,
    against subjects of 1 ... 300 letters (1 beside 300, C < R, no letters): with one workgroup the
    profile is built once per query, and every grid gives the same results."""
    if "rows" not in _POOL:
        lens = [1, 2, 23, 24, 25, 47, 48, 49, SWEEP - 1, SWEEP, SWEEP + 1, 2 * SWEEP + 1]
        _POOL["rows"] = _Multi([_seq(R, 300 + R) for R in lens], _mixed_subjects(70, 7), golden.blosum62)
    m = _POOL["rows"]
    want = _want("rows", m, go, ge)
    assert (want[:, :, 0] > 0).any() and ((want[:, :, 0] < 0).any() or go == 0)
    r1, i1 = _run(engine, m, go, ge, max_workgroups=1)
    assert i1["workgroups"] == 1 and i1["lane_queries"] == len(m.queries) and i1["other_queries"] == 0, i1
    assert i1["profile_builds"] == i1["lane_queries"], i1
    assert i1["launches"] == 3, i1  # the sweep classes
    assert i1["lane_pairs"] == len(m.queries) * 69, i1
    _check_ranked(r1, want)
    if (go, ge) in GAPS:
        for wg in (2, 0):
            r, info = _run(engine, m, go, ge, max_workgroups=wg)
            assert info["lane_queries"] == len(m.queries) and info["profile_builds"] >= info["launches"], info
            if wg:
                assert info["workgroups"] <= wg, info
            assert np.array_equal(r["scores"], r1["scores"]) and np.array_equal(r["hits"], r1["hits"]), wg


# -- 2. edges of the task and unit grid ------------------------------------------------------------

def _grid_pool():
    if "grid" not in _POOL:
        rng = np.random.default_rng(5)
        queries = [_seq(int(c), 4000 + i) for i, c in enumerate(rng.integers(1, 121, 33))]
        queries[1] = _seq(0, 1)          # an empty query among real ones
        queries[3] = queries[0].copy()   # two identical queries
        subjects = [_seq(int(c), 5000 + i) for i, c in enumerate(rng.integers(1, 151, 130))]
        _POOL["grid"] = (queries, subjects)
    return _POOL["grid"]


@pytest.mark.parametrize("nq", [1, 2, 5, 33])
@pytest.mark.parametrize("go,ge", GAPS)
def test_task_and_unit_edges(engine, golden, go, ge, nq):
    queries, subjects = _grid_pool()
    if "gridm" not in _POOL:
        _POOL["gridm"] = _Multi(queries, subjects, golden.blosum62)
    want = _want("grid", _POOL["gridm"], go, ge)
    assert want[1, :, :].tolist() == [[0, 0, 0]] * len(subjects)  # the empty query: score 0 at (0, 0)
    unit = 4 * gsa.score_db_multi_unit()  # subjects of a unit
    for nsubj in sorted({1, 3, 4, 5, 65, 130, unit - 4, unit, unit + 4}):
        assert 1 <= nsubj <= len(subjects)
        key = ("grid", nq, nsubj)
        if key not in _POOL:
            _POOL[key] = _Multi(queries[:nq], subjects[:nsubj], golden.blosum62)
        r, info = _run(engine, _POOL[key], go, ge)
        lane_q = sum(len(q) > 1 for q in queries[:nq])
        assert info["lane_queries"] == lane_q and info["lane_pairs"] == lane_q * nsubj, (key, info)
        tasks = -(-nsubj // 4)
        assert info["units"] == lane_q * -(-tasks // gsa.score_db_multi_unit()), (key, info)
        assert info["other_queries"] == 0, info
        _check_ranked(r, want[:nq, :nsubj])
        if nq >= 5:
            assert np.array_equal(r["scores"][0], r["scores"][3])


# -- 3. the hand-made cases ------------------------------------------------------------------------

@pytest.mark.parametrize("go,ge", [(-3, -1), (-2, -2)])
def test_hand_made_cases(engine, go, ge):
    """Two maximal cells in row R (the first one's column), a query planted between flanks, and an
    all-mismatch subject whose score is negative; then, under a table whose mismatch is below the gap
    cost, j_end = 0.  Each is first shown by the oracle to have the property it is named for."""
    q1, s1 = hand.planted_once()
    q2, s2 = hand.planted_twice()
    q3, s3 = hand.all_mismatch()
    if "hand" not in _POOL:
        _POOL["hand"] = _Multi([q1, q2, q3], [s1, s2, s3], hand.SUB5)
        _POOL["harsh"] = _Multi([q3, q1], [s3, s1, s3[:3]], hand.SUB5_HARSH)
    m = _POOL["hand"]
    want = _want("hand", m, go, ge)
    H = so.matrices(q2, s2, hand.SUB5, go, ge)[0]
    assert int((H[-1] == H[-1].max()).sum()) == 2 and want[1, 1].tolist() == [20, 10, 15]
    assert want[0, 0].tolist() == [24, 12, 21]
    assert want[2, 2].tolist() == [-6, 6, 6]
    r, info = _run(engine, m, go, ge)
    assert info["lane_pairs"] == 9, info
    _check_ranked(r, want)
    m = _POOL["harsh"]
    for g in ((-1, -1), (-2, -1)):
        want = _want("harsh", m, *g)
        assert want[0, 0].tolist() == [g[0] + 5 * g[1], 6, 0] and want[0, 2, 2] == 0  # j_end = 0
        r, _ = _run(engine, m, *g)
        _check_ranked(r, want)


# -- 4. stale profile, short subjects beside long ones ------------------------------------------------

def test_short_query_after_a_long_one_and_short_subjects_beside_long_ones(engine, golden):
    """One workgroup runs a query of 383 letters, then ones of 5 in the same LDS.  Letter 0 -- the header
    element of the next sequence in a buffer, what a read past a sequence's end finds -- scores +15
    against everything, in either role, and no sequence holds it.  Subjects of 1, 2 and 7 letters share
    a wave with one of 300."""
    n = int(round(np.sqrt(golden.blosum62.size)))
    sub = np.array(golden.blosum62, dtype=np.int32).reshape(n, n).copy()
    sub[0, :] = 15
    sub[:, 0] = 15

    def letters(c, seed):
        x = _seq(c, seed, 19)
        x[1:] += 1  # letters 1..19
        return x

    m = _Multi([letters(SWEEP - 1, 1), letters(5, 2), letters(5, 3)], [letters(c, 10 + c) for c in (300, 1, 2, 7)], sub)
    for go, ge in GAPS:
        want = _want("stale", m, go, ge)
        r, info = _run(engine, m, go, ge, max_workgroups=1)
        assert info["profile_builds"] == 3 and info["workgroups"] == 1 and info["units"] == 3, info
        _check_ranked(r, want)


# -- 5. ranking ------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def planted():
    """Match +5, everything else -4.  Subjects 3, 9 and 17 are copies of subject 0 (equal scores
    against every query), and five subjects of letters no query holds score below zero."""
    sub = np.full((20, 20), -4, np.int32)
    np.fill_diagonal(sub, 5)
    subjects = [_seq(int(c), 600 + i, 10) for i, c in enumerate(np.random.default_rng(3).integers(20, 90, 22))]
    for k in (3, 9, 17):
        subjects[k] = subjects[0].copy()
    for k in (2, 5, 11, 12, 21):
        subjects[k] = subjects[k] + np.where(np.arange(len(subjects[k])) > 0, 10, 0).astype(np.int32)
    return _Multi([_seq(R, 700 + R, 10) for R in (40, 3, 150)], subjects, sub)


@pytest.mark.parametrize("top", [1, 3, 22, 27])
def test_ranking_with_ties_and_negative_scores(engine, planted, top):
    m = planted
    for go, ge in [(-11, -1), (-5, -5)]:
        want = _want("planted", m, go, ge)
        assert (want[:, 3] == want[:, 0]).all() and (want[:, 17] == want[:, 0]).all()
        assert (want[:, [2, 5, 11, 12, 21], 0] < 0).all()
        r, _ = _run(engine, m, go, ge, top=top)
        _check_ranked(r, want, top)
        only_hits, _ = _run(engine, m, go, ge, top=top, want_scores=False)
        assert only_hits["scores"] is None and np.array_equal(only_hits["hits"], r["hits"])
    only_scores, info = _run(engine, m, -11, -1, top=0)
    assert only_scores["hits"] is None and info["select_ms"] >= 0.0
    assert np.array_equal(only_scores["scores"], _want("planted", m, -11, -1)[:, :, 0])


# -- 6. chunks -------------------------------------------------------------------------------------

def test_chunks(engine, golden):
    queries = [_seq(int(c), 800 + i) for i, c in enumerate([50, 120, 7, 90, 33, 200, 61])]
    m = _Multi(queries, _mixed_subjects(20, 9), golden.blosum62)
    row = 16 * len(m.subjects)
    for go, ge in GAPS:
        whole, iw = _run(engine, m, go, ge)
        assert iw["launches"] == 1 and iw["result_bytes"] == 7 * row, iw
        limit = 2 * row + row // 2  # two rows at a time: 4 chunks
        r, info = _run(engine, m, go, ge, scratch_limit=limit)
        assert info["launches"] == 4 and info["result_bytes"] == 2 * row <= limit, info
        assert info["lane_queries"] == 7 and info["units"] == iw["units"] and info["lane_pairs"] == iw["lane_pairs"], info
        assert np.array_equal(r["scores"], whole["scores"]) and np.array_equal(r["hits"], whole["hits"])
        _check_ranked(r, _want("chunks", m, go, ge))
        one, i1 = _run(engine, m, go, ge, scratch_limit=row)
        assert i1["launches"] == 7 and i1["result_bytes"] == row, i1
        assert np.array_equal(one["hits"], whole["hits"])
    with pytest.raises(gsa.NwError) as ei:
        _run(engine, m, -11, -1, scratch_limit=row - 1)
    assert ei.value.stat == gsa.NwStat.errorInvalidValue


# -- 7. tables -------------------------------------------------------------------------------------

@pytest.mark.parametrize("go,ge", GAPS)
def test_tables(engine, go, ge):
    """An asymmetric table (row = query letter), and one with values outside int8."""
    rng = np.random.default_rng(11)
    asym = rng.integers(-6, 12, size=(20, 20)).astype(np.int32)
    assert not np.array_equal(asym, asym.T)
    wide = np.full((20, 20), -200, np.int32)
    np.fill_diagonal(wide, 300)
    for name, sub in [("asym", asym), ("wide", wide)]:
        if name not in _POOL:
            subjects = [_seq(int(c), 2100 + i) for i, c in enumerate(rng.integers(1, 151, 20))]
            _POOL[name] = _Multi([_seq(90, 13), _seq(17, 14), _seq(130, 15)], subjects, sub)
        m = _POOL[name]
        r, info = _run(engine, m, go, ge)
        assert info["lane_queries"] == 3 and info["lane_pairs"] == 60, info
        _check_ranked(r, _want(name, m, go, ge))


# -- 8. refusals -----------------------------------------------------------------------------------

def _record(engine):
    """gsa_last_launch's record, after a tiny score_db_dev call if nothing has been recorded yet."""
    try:
        return engine.last_launch()
    except gsa.NwError:
        tiny = _Multi([_seq(5, 1)], [_seq(6, 2)], np.eye(20, dtype=np.int32))
        tiny.single(engine, -1, -1, False)
        return engine.last_launch()


def _refused(engine, m, go, ge, **kw):
    before = _record(engine)
    with pytest.raises(gsa.NwError) as ei:
        _run(engine, m, go, ge, **kw)
    assert ei.value.stat == gsa.NwStat.errorInvalidValue, kw
    assert engine.last_launch() == before


def test_no_second_path_a_pair_runs_on_the_lanes_or_the_call_is_refused(engine, golden, knobs):
    """A subject of 8192 letters; a query whose profile cannot fit LDS; both with an empty partner
    only are fine.  GSA_DB_MAXC and GSA_DB_LANES do not apply."""
    short = [_seq(40, 1), _seq(7, 2)]
    ok = _Multi(short, [_seq(8191, 3), _seq(12, 4)], golden.blosum62)
    r, info = _run(engine, ok, -11, -1)
    assert info["lane_pairs"] == 4 and info["other_queries"] == 0, info
    _check_ranked(r, _want("c8191", ok, -11, -1))
    _refused(engine, _Multi(short, [_seq(8192, 3), _seq(12, 4)], golden.blosum62), -11, -1)
    # no query has letters: the long subject meets no letters on the other side
    r, info = _run(engine, _Multi([_seq(0, 1), _seq(0, 2)], [_seq(8192, 3), _seq(12, 4)], golden.blosum62), -11, -1)
    assert info["lane_pairs"] == 0 and info["launches"] == 0 and (r["scores"] == 0).all(), info
    # 25 letters x (5 x 384 + 4) rows x 4 bytes do not fit 160 KiB; 4 sweeps do
    n = int(round(np.sqrt(golden.blosum62.size)))
    assert n * (5 * SWEEP + 4) * 4 > 160 * 1024 >= n * (4 * SWEEP + 4) * 4
    subjects = [_seq(30, 5), _seq(0, 6), _seq(9, 7)]
    fits = _Multi([_seq(4 * SWEEP, 8), _seq(3, 9)], subjects, golden.blosum62)
    r, info = _run(engine, fits, -4, -4)
    assert info["launches"] == 2 and info["lane_pairs"] == 4, info
    _check_ranked(r, _want("fits", fits, -4, -4))
    _refused(engine, _Multi([_seq(4 * SWEEP + 1, 8), _seq(3, 9)], subjects, golden.blosum62), -4, -4)
    r, info = _run(engine, _Multi([_seq(4 * SWEEP + 1, 8), _seq(3, 9)], [_seq(0, 6)], golden.blosum62), -4, -1)
    assert r["scores"].tolist() == [[-4 - 4 * SWEEP], [-6]] and info["launches"] == 0, info
    assert r["hits"][0][0].tolist() == (0, -4 - 4 * SWEEP, 4 * SWEEP + 1, 0)
    # the knobs of the old modes change nothing here
    want = _want("c8191", ok, -11, -1)
    knobs("GSA_DB_MAXC", "10")
    knobs("GSA_DB_LANES", "0")
    r, info = _run(engine, ok, -11, -1)
    assert info["lane_pairs"] == 4 and info["other_queries"] == 0, info
    _check_ranked(r, want)


def test_value_bound_from_both_sides(engine):
    """B = smax min(R, C) + |go| + (R + C) |ge|: 2^18 - 1 runs and is exact, 2^18 is refused."""
    q = _seq(4, 1, 4)
    subjects = [np.concatenate([q[:2], [(q[1] + 1) % 4], q[1:]]).astype(np.int32), _seq(5, 3, 4), _seq(2, 4, 4)]
    assert len(subjects[0]) - 1 == 6  # the query itself behind two letters: 4 smax

    def table(s):
        sub = np.full((4, 4), -s, np.int32)
        np.fill_diagonal(sub, s)
        return sub

    s, go, ge = 65533, -1, -1
    assert 4 * s + 1 + 10 * 1 == (1 << 18) - 1
    m = _Multi([q, _seq(3, 5, 4)], subjects, table(s))
    r, info = _run(engine, m, go, ge)
    assert info["lane_pairs"] == 6, info
    want = _want("bound", m, go, ge)
    assert want[0, 0].tolist() == [4 * s, 4, 6]
    _check_ranked(r, want)
    _refused(engine, _Multi([q, _seq(3, 5, 4)], subjects, table(s + 1)), go, ge)
    _refused(engine, m, go - 1, ge)       # |go| one larger
    _refused(engine, m, -2, -2)           # |ge| one larger: + 1 + 10
    # one more subject letter: (R + C) |ge| one larger
    _refused(engine, _Multi([q, _seq(3, 5, 4)], subjects + [_seq(7, 6, 4)], table(s)), go, ge)


def test_inherited_rejections(engine, golden):
    m = _Multi([_seq(60, 4), _seq(20, 5), _seq(33, 6)], [_seq(int(c), 1300 + c) for c in (5, 80, 41, 17, 66)], golden.blosum62)
    want = _want("inv", m, -11, -1)
    for table in ("qoff", "off"):
        src = getattr(m, table)
        equal, dec, neg = src.copy(), src.copy(), src.copy()
        equal[2] = equal[1]
        dec[2] = dec[1] - 1
        neg[0] = -1
        for off in (equal, dec, neg, src[:1]):  # the last: nq / nsubj = 0
            _refused(engine, m, -11, -1, **{table: off})
    _refused(engine, m, -1, -11)
    _refused(engine, m, -11, 1)
    _refused(engine, m, -11, -1, top=-1)
    _refused(engine, m, -11, -1, max_workgroups=-1)
    _refused(engine, m, -11, -1, scratch_limit=-1)
    _refused(engine, m, -11, -1, top=0, want_scores=False)   # both outputs null
    # hits null with top > 0 and scores null: straight through the C entry point
    i64p = ctypes.POINTER(ctypes.c_int64)
    st = gsa.lib().gsa_score_db_multi_semi_dev(engine._h, m.q.data_ptr(), m.qoff.ctypes.data_as(i64p), 3, m.db.data_ptr(),
                                               m.off.ctypes.data_as(i64p), 5, m.sub.data_ptr(), m.substsz, -11, -1, 3, 0, 0,
                                               None, None, None, None, None)
    assert st == gsa.NwStat.errorInvalidValue
    for name in ("queries", "db", "subst"):  # a null device pointer
        ptr = {"queries": m.q.data_ptr(), "db": m.db.data_ptr(), "subst": m.sub.data_ptr()}
        ptr[name] = None
        with pytest.raises(gsa.NwError) as ei:
            engine.score_db_semi_dev(ptr["queries"], m.qoff, ptr["db"], m.off, ptr["subst"], m.substsz, -11, -1)
        assert ei.value.stat == gsa.NwStat.errorInvalidValue, name
    for substsz in (0, 33):
        with pytest.raises(gsa.NwError) as ei:
            engine.score_db_semi_dev(m.q.data_ptr(), m.qoff, m.db.data_ptr(), m.off, m.sub.data_ptr(), substsz, -11, -1)
        assert ei.value.stat == gsa.NwStat.errorInvalidValue, substsz
    r, _ = _run(engine, m, -11, -1)
    _check_ranked(r, want)


# -- 9. neighbours ---------------------------------------------------------------------------------

def test_neighbours_keep_their_record_and_their_results(engine, golden):
    """score_db_multi_dev in both old modes right before and right after, over a query of two sweeps:
    the calls share context buffers.  gsa_last_launch is left alone."""
    queries = [_seq(R, 900 + R) for R in (60, 500, 130)]
    subjects = [_seq(int(c), 950 + i) for i, c in enumerate([80, 200, 33, 150, 7, 260, 90, 121, 64])]
    m = _Multi(queries, subjects, golden.blosum62)

    def around():
        out = []
        for local in (True, False):
            r, _ = m.run(engine, -11, -1, local, top=3)
            out += [r["scores"].copy(), r["hits"].copy()]
        return out

    m.single(engine, -11, -1, True)  # a launch record to be left alone
    before = engine.last_launch()
    assert before["kind"] == "score_lanes", before
    first = around()
    r, info = _run(engine, m, -11, -1, top=3)
    assert engine.last_launch() == before
    assert info["launches"] == 2 and info["lane_pairs"] == 27, info
    _check_ranked(r, _want("nb", m, -11, -1), 3)
    again = around()
    assert all(np.array_equal(a, b) for a, b in zip(first, again))
    r2, _ = _run(engine, m, -11, -1, top=3)
    assert np.array_equal(r["scores"], r2["scores"]) and np.array_equal(r["hits"], r2["hits"])


def test_mem_stats_count_the_buffers(golden):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    queries = [_seq(100, 40 + i) for i in range(16)]
    subjects = [_seq(150, 60 + i) for i in range(512)]
    with gsa.Engine(0) as e:
        m = _Multi(queries, subjects, golden.blosum62)
        e.reset_mem_stats()
        r, info = _run(e, m, -11, -1, top=5)
        pairs = len(queries) * len(subjects)
        assert info["result_bytes"] == 16 * pairs, info
        # the matrix, the ranking's keys in and out, the compacted scores
        stats = e.mem_stats()
        assert stats["glmem_peak_allocs"] >= (16 + 16 + 4) * pairs
        assert r["hits"].shape == (16, 5)
        # the old mode on the same context reuses the slots: nothing new is held
        m.run(e, -11, -1, False, top=5)
        assert e.mem_stats()["glmem_peak_allocs"] == stats["glmem_peak_allocs"]


# -- 10. host form ---------------------------------------------------------------------------------

def test_host_form(engine, golden):
    queries = [_seq(R, 1100 + R) for R in (120, 0, 45)]
    subjects = [_seq(int(c), 1200 + i) for i, c in enumerate(np.random.default_rng(8).integers(0, 200, 40))]
    m = _Multi(queries, subjects, golden.blosum62)
    for go, ge in GAPS:
        dev, _ = _run(engine, m, go, ge, top=4)
        host = engine.score_db_semi(queries, subjects, golden.blosum62, go, ge, top=4)
        assert np.array_equal(host["scores"], dev["scores"]) and np.array_equal(host["hits"], dev["hits"])
        _check_ranked(host, _want("host", m, go, ge), 4)
