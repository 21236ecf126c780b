"""Overlap (dovetail) database search, scores and ranking (gsa_score_db_multi_overlap_dev;
nw_lanes_overlap.hip): every (query, subject) result -- score and end cell, (R, smallest j)
if row R attains the score, else (smallest i, C) -- exactly what tests/_overlap_oracle.py gives; the hits a
host sort of the scores by (-score, subject); last_score_db_overlap_info() for what ran; every refusal
beside the largest input that runs.  The tests count from the oracle how their cases end, so that a seed
that no longer ends on column C fails here and not silently.  No tolerances anywhere."""
import ctypes

import numpy as np
import pytest

import gpuseqalign_amd as gsa
from tests import _overlap_oracle as oo
from tests.test_gpu_score_db_multi import _check_ranked, _Multi, _seq

pytestmark = pytest.mark.gpu

K = 24
SWEEP = 16 * K  # query rows of one sweep (16 lanes x 24 rows)
GAPS = [(-11, -1), (-4, -4)]  # affine, linear
GRID_GAPS = [(-11, -1), (-11, -11), (-3, 0), (0, 0)]
GRID_ROWS = [1, 2, 23, 24, 25, 47, 48, 49, SWEEP - 1, SWEEP, SWEEP + 1, 2 * SWEEP + 1]
_REF = {}
_POOL = {}


def _hdr(letters):
    return np.concatenate([[0], np.asarray(letters, np.int64)]).astype(np.int32)


def _table(n, match, mismatch, dead=()):
    """match on the diagonal, mismatch elsewhere; a dead letter mismatches itself too."""
    sub = np.full((n, n), mismatch, np.int32)
    np.fill_diagonal(sub, match)
    for d in dead:
        sub[d, d] = mismatch
    return sub


SUB4 = _table(4, 5, -4)
# letters 0 ... 3 as in SUB4; 4 (the queries' filler) and 5 (the subjects') match nothing, themselves included
SUB6 = _table(6, 5, -4, dead=(4, 5))


def _want(key, queries, subjects, sub, go, ge):
    """The oracle's (score, i_end, j_end) of every pair, [nq, nsubj, 3], computed once per (key, gaps)."""
    k = (key, go, ge)
    if k not in _REF:
        _REF[k] = np.array([[oo.score(Y, X, sub, go, ge) for X in subjects] for Y in queries],
                           dtype=np.int64).reshape(len(queries), len(subjects), 3)
    return _REF[k]


def _wantm(key, m, go, ge):
    return _want(key, m.queries, m.subjects, m.subm, go, ge)


def _run(engine, m, go, ge, qoff=None, off=None, **kw):
    """(result dict, info) of one overlap call; top defaults to all subjects."""
    kw.setdefault("top", len(m.subjects))
    r = engine.score_db_overlap_dev(m.q.data_ptr(), m.qoff if qoff is None else qoff, m.db.data_ptr(),
                                    m.off if off is None else off, m.sub.data_ptr(), m.substsz, go, ge, **kw)
    return r, engine.last_score_db_overlap_info()


def ends(want, queries, subjects):
    """How the pairs of want[nq, nsubj, 3] end: {"row": on row R left of column C, "col": on column C above
    row R, "corner", "zero"} as boolean [nq, nsubj]."""
    R = np.array([len(q) - 1 for q in queries])[:, None]
    C = np.array([len(x) - 1 for x in subjects])[None, :]
    score, i, j = want[:, :, 0], want[:, :, 1], want[:, :, 2]
    zero = score == 0
    return {"zero": zero, "corner": ~zero & (i == R) & (j == C), "row": ~zero & (i == R) & (j < C),
            "col": ~zero & (i < R) & (j == C)}


# -- 1. the row grid: every position of the last row in a lane and a sweep, every way to end ---------------

def grid_inputs():
    """Uniform random letters over 4: queries on every edge of a lane's rows and of a sweep, one to three
    sweeps; subjects of 1 ... 69 and 300 letters."""
    queries = [_seq(R, 300 + R, 4) for R in GRID_ROWS]
    subjects = [_seq(c, 7000 + c, 4) for c in list(range(1, 70)) + [300]]
    return queries, subjects


def grid_counts(want, queries, subjects):
    e = ends(want, queries, subjects)
    early = sum(int((e["col"][q] & (want[q, :, 1] <= SWEEP)).sum()) for q, R in enumerate(GRID_ROWS) if R > SWEEP)
    return {k: int(v.sum()) for k, v in e.items()}, early


@pytest.mark.parametrize("go,ge", GRID_GAPS)
def test_row_grid_and_how_its_pairs_end(engine, go, ge):
    queries, subjects = grid_inputs()
    if "grid" not in _POOL:
        _POOL["grid"] = _Multi(queries, subjects, SUB4)
    m = _POOL["grid"]
    want = _want("grid", queries, subjects, SUB4, go, ge)
    n, early = grid_counts(want, queries, subjects)
    print("gaps", (go, ge), "ends", n, "column ends in an earlier sweep", early)
    assert sum(n.values()) == len(queries) * len(subjects)
    if go < 0:
        assert n["col"] >= 100 and n["row"] >= 100 and early >= 10, (n, early)
    r1, i1 = _run(engine, m, go, ge, max_workgroups=1)
    assert i1["workgroups"] == 1 and i1["lane_queries"] == len(queries) and i1["other_queries"] == 0, i1
    assert i1["profile_builds"] == i1["lane_queries"], i1
    assert i1["launches"] == 3, i1  # the sweep classes
    assert i1["lane_pairs"] == len(queries) * len(subjects), i1
    _check_ranked(r1, want)
    for wg in (2, 0):
        r, info = _run(engine, m, go, ge, max_workgroups=wg)
        assert info["lane_queries"] == len(queries) and info["profile_builds"] >= info["launches"], info
        if wg:
            assert info["workgroups"] <= wg, info
        assert np.array_equal(r["scores"], r1["scores"]) and np.array_equal(r["hits"], r1["hits"]), wg


def test_a_sample_of_the_grid_agrees_with_the_long_pairs_call(engine):
    """About 20 pairs of the grid through Engine.score_overlap_dev, the K-rows kernel's overlap instances."""
    queries, subjects = grid_inputs()
    if "grid" not in _POOL:
        _POOL["grid"] = _Multi(queries, subjects, SUB4)
    m = _POOL["grid"]
    rng = np.random.default_rng(17)
    pairs = {(int(q), int(s)) for q, s in zip(rng.integers(0, len(queries), 24), rng.integers(0, len(subjects), 24))}
    pairs |= {(len(queries) - 1, len(subjects) - 1), (0, 0)}
    assert len(pairs) >= 20
    for go, ge in GAPS:
        r, _ = _run(engine, m, go, ge, top=0)
        want = _want("grid", queries, subjects, SUB4, go, ge)
        hits, _ = _run(engine, m, go, ge, want_scores=False)
        for q, s in sorted(pairs):
            one = engine.score_overlap_dev(m.q.data_ptr() + 4 * int(m.qoff[q]), len(queries[q]),
                                           m.db.data_ptr() + 4 * int(m.off[s]), len(subjects[s]), m.sub.data_ptr(),
                                           m.substsz, go, ge)
            row = hits["hits"][q]
            hit = row[list(row["subject"]).index(s)]
            assert (one["score"], one["i_end"], one["j_end"]) == (int(hit["score"]), int(hit["i_end"]), int(hit["j_end"])), (q, s)
            assert one["score"] == r["scores"][q, s] == want[q, s, 0]


# -- 2. the hand-made cases --------------------------------------------------------------------------

def _core(n, seed):
    return _seq(n, seed, 4)[1:]


def planted_cases():
    """(name, query, subject, expected (score, i_end, j_end)) under SUB6 and gaps of at least 4 per letter:
    the four arrangements with their ends on the rows and columns named, and the tie rules."""
    Q, S = 4, 5  # fillers
    out = []
    for L in (15, 16, 17):  # the query's suffix on the subject's prefix: row R, j_end = L
        c = _core(L, 100 + L)
        out.append(("suffix-prefix-%d" % L, _hdr([Q] * 30 + list(c)), _hdr(list(c) + [S] * 9), (5 * L, 30 + L, L)))
    for L in (K, K + 1, SWEEP, SWEEP + 1):  # the subject's suffix on the query's prefix: column C, i_end = L
        c = _core(L, 200 + L)
        out.append(("prefix-suffix-%d" % L, _hdr(list(c) + [Q] * 40), _hdr([S] * 11 + list(c)), (5 * L, L, 11 + L)))
    for b, R in ((3, 12), (5, 11), (8, 9)):  # the query inside the subject: row R, j_end = b + R
        c = _core(R, 300 + R)
        out.append(("query-inside-%d" % (b + R), _hdr(c), _hdr([S] * b + list(c) + [S] * 7), (5 * R, R, b + R)))
    for a, C in ((4, 20), (5, 20), (350, 34), (350, 35)):  # the subject inside the query: column C, i_end = a + C
        c = _core(C, 400 + a + C)
        out.append(("subject-inside-%d" % (a + C), _hdr([Q] * a + list(c) + [Q] * 30), _hdr(c), (5 * C, a + C, C)))
    u, v = _core(6, 501), _core(6, 502)
    # row R and column C attain 30 at different cells: row R's
    out.append(("row-beats-column", _hdr(list(v) + [Q] + list(u)), _hdr(list(u) + [S] + list(v)), (30, 13, 6)))
    out.append(("two-on-column", _hdr(list(v) + [Q] + list(v) + [Q]), _hdr(v), (30, 6, 6)))
    out.append(("two-on-row", _hdr(u), _hdr(list(u) + [S] + list(u) + [S]), (30, 6, 6)))
    out.append(("corner-alone", _hdr(u), _hdr(u), (30, 6, 6)))
    out.append(("all-mismatch", _hdr([Q] * 9), _hdr([S] * 13), (0, 9, 0)))
    return out


def check_planted_by_the_oracle(go, ge):
    """Each case is first shown by the oracle to have the property it is named for."""
    for name, q, x, want in planted_cases():
        H = oo.matrices(q, x, SUB6, go, ge)[0]
        assert oo.end_cell(H) == want, (name, oo.end_cell(H), want)
        row, col, best = H[-1], H[:, -1], want[0]
        if name == "row-beats-column":
            assert int(row.max()) == int(col.max()) == best and int(np.argmax(col)) == 6 and int(np.argmax(row)) == 6
            assert H[-1, -1] < best
        if name == "two-on-column":
            assert np.flatnonzero(col == best).tolist() == [6, 13] and int(row.max()) < best
        if name == "two-on-row":
            assert np.flatnonzero(row == best).tolist() == [6, 13] and int(col.max()) < best
        if name == "corner-alone":
            assert int((row == best).sum()) == 1 and int((col == best).sum()) == 1 and H[-1, -1] == best


@pytest.mark.parametrize("go,ge", [(-11, -1), (-5, -5)])
def test_hand_made_cases(engine, go, ge):
    check_planted_by_the_oracle(go, ge)
    cases = planted_cases()
    if "hand" not in _POOL:
        _POOL["hand"] = _Multi([c[1] for c in cases], [c[2] for c in cases], SUB6)
    m = _POOL["hand"]
    want = _wantm("hand", m, go, ge)
    for k, c in enumerate(cases):
        assert tuple(want[k, k]) == c[3], c[0]
    assert sorted({int(want[k, k, 1]) for k, c in enumerate(cases) if c[0].startswith(("prefix-suffix", "subject-inside"))}) \
        == [K, K + 1, SWEEP, SWEEP + 1]
    assert sorted({int(want[k, k, 2]) for k, c in enumerate(cases) if c[0].startswith(("suffix-prefix", "query-inside"))}) \
        == [15, 16, 17]
    r, info = _run(engine, m, go, ge)
    assert info["lane_pairs"] == len(cases) ** 2, info
    _check_ranked(r, want)  # all pairs, the planted ones on the diagonal


# -- 3. one wave, unequal subjects -------------------------------------------------------------------

WAVES = [[1, 2, 7, 300], [300, 1, 1, 7], [300, 1, 1, 1], [300, 300, 300, 300, 1], [2, 300, 300, 7, 1, 1],
         [9, 1, 1, 1, 1, 1, 300]]


def _groups_of_the_one_letter_subjects(lens):
    return {s % 4 for s, c in enumerate(sorted(lens, reverse=True)) if c == 1}


@pytest.mark.parametrize("lens", WAVES, ids=lambda v: "-".join(map(str, v)))
def test_unequal_subjects_in_one_wave(engine, lens):
    """Subjects of 1, 2 and 7 letters share a wave with one of 300: the step at which a lane stands on
    column C differs per 16-lane group, and for C < 16 it falls before the higher lanes have started.  The
    call orders the subjects longest first, ties by index, four to a wave: the counts and ties here put a
    1-letter subject into each of the four groups in turn."""
    assert set().union(*map(_groups_of_the_one_letter_subjects, WAVES)) == {0, 1, 2, 3}
    assert _groups_of_the_one_letter_subjects(WAVES[0]) == {3} and sorted(WAVES[0]) == [1, 2, 7, 300]
    queries = [_seq(R, 40 + R, 4) for R in (1, 5, 30, SWEEP + 16)]
    subjects = [_seq(c, 900 + 10 * k + c, 4) for k, c in enumerate(lens)]
    m = _Multi(queries, subjects, SUB4)
    for go, ge in GAPS + [(-3, 0)]:
        want = _want(("wave", tuple(lens)), queries, subjects, SUB4, go, ge)
        r, info = _run(engine, m, go, ge, max_workgroups=1)
        assert info["lane_pairs"] == len(queries) * len(lens), info
        _check_ranked(r, want)


# -- 4. stale profile, a table that rewards reading past a sequence's end -------------------------------

def test_short_queries_after_a_long_one_under_a_hostile_table(engine, golden):
    """One workgroup runs a query of 383 letters, then ones of 5 in the same LDS.  Letter 0 -- the header
    element of the next sequence in a buffer, what a read past a sequence's end finds -- scores +15, the
    table's maximum, against everything in either role, and no sequence holds it."""
    n = int(round(np.sqrt(golden.blosum62.size)))
    sub = np.array(golden.blosum62, dtype=np.int32).reshape(n, n).copy()
    sub[0, :] = 15
    sub[:, 0] = 15
    assert sub.max() == 15

    def letters(c, seed):
        x = _seq(c, seed, 19)
        x[1:] += 1  # letters 1..19
        return x

    m = _Multi([letters(SWEEP - 1, 1), letters(5, 2), letters(5, 3)], [letters(c, 10 + c) for c in (300, 1, 2, 7)], sub)
    for go, ge in GAPS:
        want = _wantm("stale", m, go, ge)
        r, info = _run(engine, m, go, ge, max_workgroups=1)
        assert info["profile_builds"] == 3 and info["workgroups"] == 1 and info["units"] == 3, info
        _check_ranked(r, want)


# -- 5. edges of the task and unit grid ------------------------------------------------------------

def _sched_pool():
    if "sched" not in _POOL:
        rng = np.random.default_rng(5)
        queries = [_seq(int(c), 4000 + i) for i, c in enumerate(rng.integers(1, 121, 33))]
        queries[1] = _seq(0, 1)          # an empty query among real ones
        queries[3] = queries[0].copy()   # two identical queries
        n = 4 * gsa.score_db_multi_unit() + 4
        subjects = [_seq(int(c), 5000 + i) for i, c in enumerate(rng.integers(1, 151, max(130, n)))]
        subjects[2] = _seq(0, 2)         # subjects without letters
        subjects[70] = _seq(0, 3)
        _POOL["sched"] = (queries, subjects)
    return _POOL["sched"]


@pytest.mark.parametrize("nq", [1, 2, 5, 33])
@pytest.mark.parametrize("go,ge", GAPS)
def test_task_and_unit_edges(engine, golden, go, ge, nq):
    queries, subjects = _sched_pool()
    want = _want("sched", queries, subjects, golden.blosum62, go, ge)
    assert want[1, :, :].tolist() == [[0, 0, 0]] * len(subjects)  # the empty query: score 0 at (R, 0) = (0, 0)
    assert want[0, 2].tolist() == [0, len(queries[0]) - 1, 0]     # the empty subject: score 0 at (R, 0)
    unit = 4 * gsa.score_db_multi_unit()  # subjects of a unit
    for nsubj in sorted({1, 3, 4, 5, 65, 130, unit - 4, unit, unit + 4}):
        assert 1 <= nsubj <= len(subjects)
        key = ("sched", nq, nsubj)
        if key not in _POOL:
            _POOL[key] = _Multi(queries[:nq], subjects[:nsubj], golden.blosum62)
        r, info = _run(engine, _POOL[key], go, ge)
        lane_q = sum(len(q) > 1 for q in queries[:nq])
        lane_s = sum(len(x) > 1 for x in subjects[:nsubj])
        assert info["lane_queries"] == lane_q and info["lane_pairs"] == lane_q * lane_s, (key, info)
        tasks = -(-lane_s // 4)
        assert info["units"] == lane_q * -(-tasks // gsa.score_db_multi_unit()), (key, info)
        assert info["other_queries"] == 0, info
        _check_ranked(r, want[:nq, :nsubj])
        if nq >= 5:
            assert np.array_equal(r["scores"][0], r["scores"][3])


# -- 6. ranking ------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def planted():
    """Match +5, everything else -4.  Subjects 3, 9 and 17 are copies of subject 0 (equal scores against
    every query), and five subjects of letters no query holds score 0: ties at both ends of the order."""
    sub = _table(20, 5, -4)
    subjects = [_seq(int(c), 600 + i, 10) for i, c in enumerate(np.random.default_rng(3).integers(20, 90, 22))]
    for k in (3, 9, 17):
        subjects[k] = subjects[0].copy()
    for k in (2, 5, 11, 12, 21):
        subjects[k] = subjects[k] + np.where(np.arange(len(subjects[k])) > 0, 10, 0).astype(np.int32)
    return _Multi([_seq(R, 700 + R, 10) for R in (40, 3, 150)], subjects, sub)


@pytest.mark.parametrize("top", [1, 3, 22, 27])
def test_ranking_with_ties(engine, planted, top):
    m = planted
    for go, ge in [(-11, -1), (-5, -5)]:
        want = _wantm("planted", m, go, ge)
        assert (want[:, 3] == want[:, 0]).all() and (want[:, 17] == want[:, 0]).all()
        assert (want[:, [2, 5, 11, 12, 21], 0] == 0).all() and (want[:, :, 0] >= 0).all()
        r, _ = _run(engine, m, go, ge, top=top)
        _check_ranked(r, want, top)
        only_hits, _ = _run(engine, m, go, ge, top=top, want_scores=False)
        assert only_hits["scores"] is None and np.array_equal(only_hits["hits"], r["hits"])
    only_scores, info = _run(engine, m, -11, -1, top=0)
    assert only_scores["hits"] is None and info["select_ms"] >= 0.0
    assert np.array_equal(only_scores["scores"], _wantm("planted", m, -11, -1)[:, :, 0])


# -- 7. chunks -------------------------------------------------------------------------------------

def test_chunks(engine, golden):
    queries = [_seq(int(c), 800 + i) for i, c in enumerate([50, 120, 7, 90, 33, 200, 61])]
    subjects = [_seq(int(c), 9000 + i) for i, c in enumerate(np.random.default_rng(9).integers(1, 301, 20))]
    m = _Multi(queries, subjects, golden.blosum62)
    row = 16 * len(m.subjects)
    for go, ge in GAPS:
        whole, iw = _run(engine, m, go, ge)
        assert iw["launches"] == 1 and iw["result_bytes"] == 7 * row, iw
        limit = 2 * row + row // 2  # two rows at a time: 4 chunks
        r, info = _run(engine, m, go, ge, scratch_limit=limit)
        assert info["launches"] == 4 and info["result_bytes"] == 2 * row <= limit, info
        assert info["lane_queries"] == 7 and info["units"] == iw["units"] and info["lane_pairs"] == iw["lane_pairs"], info
        assert np.array_equal(r["scores"], whole["scores"]) and np.array_equal(r["hits"], whole["hits"])
        _check_ranked(r, _wantm("chunks", m, go, ge))
        one, i1 = _run(engine, m, go, ge, scratch_limit=row)
        assert i1["launches"] == 7 and i1["result_bytes"] == row, i1
        assert np.array_equal(one["hits"], whole["hits"])
    with pytest.raises(gsa.NwError) as ei:
        _run(engine, m, -11, -1, scratch_limit=row - 1)
    assert ei.value.stat == gsa.NwStat.errorInvalidValue


# -- 8. refusals, each beside the largest input that runs -----------------------------------------------

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


def test_subject_of_8192_letters_beside_8191(engine, golden, knobs):
    short = [_seq(40, 1), _seq(7, 2)]
    ok = _Multi(short, [_seq(8191, 3), _seq(12, 4)], golden.blosum62)
    r, info = _run(engine, ok, -11, -1)
    assert info["lane_pairs"] == 4 and info["other_queries"] == 0, info
    _check_ranked(r, _wantm("c8191", ok, -11, -1))
    _refused(engine, _Multi(short, [_seq(8192, 3), _seq(12, 4)], golden.blosum62), -11, -1)
    # no query has letters: the long subject meets no letters on the other side
    r, info = _run(engine, _Multi([_seq(0, 1), _seq(0, 2)], [_seq(8192, 3), _seq(12, 4)], golden.blosum62), -11, -1)
    assert info["lane_pairs"] == 0 and info["launches"] == 0 and (r["scores"] == 0).all(), info
    # the knobs of the old modes change nothing here
    knobs("GSA_DB_MAXC", "10")
    knobs("GSA_DB_LANES", "0")
    r, info = _run(engine, ok, -11, -1)
    assert info["lane_pairs"] == 4 and info["other_queries"] == 0, info
    _check_ranked(r, _wantm("c8191", ok, -11, -1))


def test_query_of_8192_letters_beside_8191_under_a_table_the_lds_test_lets_through(engine):
    """4 letters x (22 x 384 + 4) rows x 4 bytes fit 160 KiB for 8191 and for 8192 letters alike: the
    row index's 13 bits refuse the longer one."""
    sweeps = -(-8192 // SWEEP)
    assert sweeps == -(-8191 // SWEEP) and 4 * (sweeps * SWEEP + 4) * 4 <= 160 * 1024
    subjects = [_seq(12, 4, 4), _seq(0, 5, 4), _seq(40, 6, 4)]
    # a copy of the long query's head as a subject: a column-C end far up an early sweep
    long_q = _seq(8191, 7, 4)
    subjects.append(long_q[:31].copy())
    ok = _Multi([long_q, _seq(3, 8, 4)], subjects, SUB4)
    r, info = _run(engine, ok, -4, -4)
    assert info["launches"] == 2 and info["lane_pairs"] == 6, info
    want = _wantm("r8191", ok, -4, -4)
    assert want[0, 3].tolist() == [150, 30, 30]
    _check_ranked(r, want)
    _refused(engine, _Multi([_seq(8192, 7, 4), _seq(3, 8, 4)], subjects, SUB4), -4, -4)
    r, info = _run(engine, _Multi([_seq(8192, 7, 4)], [_seq(0, 5, 4)], SUB4), -4, -4)  # an empty partner only
    assert r["scores"].tolist() == [[0]] and info["launches"] == 0 and r["hits"][0][0].tolist() == (0, 0, 8192, 0)


def test_profile_one_sweep_past_the_lds(engine, golden):
    # 25 letters x (5 x 384 + 4) rows x 4 bytes do not fit 160 KiB; 4 sweeps do
    n = int(round(np.sqrt(golden.blosum62.size)))
    assert n * (5 * SWEEP + 4) * 4 > 160 * 1024 >= n * (4 * SWEEP + 4) * 4
    subjects = [_seq(30, 5), _seq(0, 6), _seq(9, 7)]
    fits = _Multi([_seq(4 * SWEEP, 8), _seq(3, 9)], subjects, golden.blosum62)
    r, info = _run(engine, fits, -4, -4)
    assert info["launches"] == 2 and info["lane_pairs"] == 4, info
    _check_ranked(r, _wantm("fits", fits, -4, -4))
    _refused(engine, _Multi([_seq(4 * SWEEP + 1, 8), _seq(3, 9)], subjects, golden.blosum62), -4, -4)
    r, info = _run(engine, _Multi([_seq(4 * SWEEP + 1, 8), _seq(3, 9)], [_seq(0, 6)], golden.blosum62), -4, -1)
    assert r["scores"].tolist() == [[0], [0]] and info["launches"] == 0, info


def test_value_bound_from_both_sides(engine):
    """B = smax min(R, C) + |go| + (R + C) |ge|: 2^18 - 1 runs and is exact, 2^18 is refused."""
    q = _seq(4, 1, 4)
    subjects = [np.concatenate([q[:2], [(q[1] + 1) % 4], q[1:]]).astype(np.int32), _seq(5, 3, 4), _seq(2, 4, 4)]
    assert len(subjects[0]) - 1 == 6  # the query itself behind two letters: 4 smax

    def table(s):
        return _table(4, s, -s)

    s, go, ge = 65533, -1, -1
    assert 4 * s + 1 + 10 * 1 == (1 << 18) - 1 == oo.value_bound(4, 6, table(s), go, ge)
    m = _Multi([q, _seq(3, 5, 4)], subjects, table(s))
    r, info = _run(engine, m, go, ge)
    assert info["lane_pairs"] == 6, info
    want = _wantm("bound", m, go, ge)
    assert want[0, 0].tolist() == [4 * s, 4, 6]
    _check_ranked(r, want)
    _refused(engine, _Multi([q, _seq(3, 5, 4)], subjects, table(s + 1)), go, ge)
    _refused(engine, m, go - 1, ge)       # |go| one larger
    _refused(engine, m, -2, -2)           # |ge| one larger: + 1 + 10
    # one more subject letter: (R + C) |ge| one larger
    _refused(engine, _Multi([q, _seq(3, 5, 4)], subjects + [_seq(7, 6, 4)], table(s)), go, ge)


def test_inherited_rejections(engine, golden):
    m = _Multi([_seq(60, 4), _seq(20, 5), _seq(33, 6)], [_seq(int(c), 1300 + c) for c in (5, 80, 41, 17, 66)], golden.blosum62)
    want = _wantm("inv", m, -11, -1)
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
    i64p = ctypes.POINTER(ctypes.c_int64)
    st = gsa.lib().gsa_score_db_multi_overlap_dev(engine._h, m.q.data_ptr(), m.qoff.ctypes.data_as(i64p), 3, m.db.data_ptr(),
                                                  m.off.ctypes.data_as(i64p), 5, m.sub.data_ptr(), m.substsz, -11, -1, 3, 0,
                                                  0, None, None, None, None, None)
    assert st == gsa.NwStat.errorInvalidValue
    for name in ("queries", "db", "subst"):  # a null device pointer
        ptr = {"queries": m.q.data_ptr(), "db": m.db.data_ptr(), "subst": m.sub.data_ptr()}
        ptr[name] = None
        with pytest.raises(gsa.NwError) as ei:
            engine.score_db_overlap_dev(ptr["queries"], m.qoff, ptr["db"], m.off, ptr["subst"], m.substsz, -11, -1)
        assert ei.value.stat == gsa.NwStat.errorInvalidValue, name
    for substsz in (0, 33):
        with pytest.raises(gsa.NwError) as ei:
            engine.score_db_overlap_dev(m.q.data_ptr(), m.qoff, m.db.data_ptr(), m.off, m.sub.data_ptr(), substsz, -11, -1)
        assert ei.value.stat == gsa.NwStat.errorInvalidValue, substsz
    r, _ = _run(engine, m, -11, -1)
    _check_ranked(r, want)


# -- 9. neighbours ---------------------------------------------------------------------------------

def test_neighbours_keep_their_record_and_their_results(engine, golden):
    """score_db_semi_dev and score_db_multi_dev in both old modes right before and right after, over a
    query of two sweeps: the calls share context buffers.  gsa_last_launch is left alone."""
    queries = [_seq(R, 900 + R) for R in (60, 500, 130)]
    subjects = [_seq(int(c), 950 + i) for i, c in enumerate([80, 200, 33, 150, 7, 260, 90, 121, 64])]
    m = _Multi(queries, subjects, golden.blosum62)

    def around():
        out = []
        for local in (True, False):
            r, _ = m.run(engine, -11, -1, local, top=3)
            out += [r["scores"].copy(), r["hits"].copy()]
        r = engine.score_db_semi_dev(m.q.data_ptr(), m.qoff, m.db.data_ptr(), m.off, m.sub.data_ptr(), m.substsz, -11, -1,
                                     top=3)
        return out + [r["scores"].copy(), r["hits"].copy()]

    m.single(engine, -11, -1, True)  # a launch record to be left alone
    before = engine.last_launch()
    assert before["kind"] == "score_lanes", before
    first = around()
    r, info = _run(engine, m, -11, -1, top=3)
    assert engine.last_launch() == before
    assert info["launches"] == 2 and info["lane_pairs"] == 27, info
    _check_ranked(r, _wantm("nb", m, -11, -1), 3)
    again = around()
    assert all(np.array_equal(a, b) for a, b in zip(first, again))
    r2, _ = _run(engine, m, -11, -1, top=3)
    assert np.array_equal(r["scores"], r2["scores"]) and np.array_equal(r["hits"], r2["hits"])


def test_mem_stats_hold_nothing_more_afterwards(golden):
    """The semi-global call first, then the overlap call on the same context and inputs: the same slots,
    nothing new held."""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    queries = [_seq(100, 40 + i) for i in range(16)]
    subjects = [_seq(150, 60 + i) for i in range(512)]
    with gsa.Engine(0) as e:
        m = _Multi(queries, subjects, golden.blosum62)
        e.reset_mem_stats()
        e.score_db_semi_dev(m.q.data_ptr(), m.qoff, m.db.data_ptr(), m.off, m.sub.data_ptr(), m.substsz, -11, -1, top=5)
        stats = e.mem_stats()
        r, info = _run(e, m, -11, -1, top=5)
        pairs = len(queries) * len(subjects)
        assert info["result_bytes"] == 16 * pairs and r["hits"].shape == (16, 5), info
        assert stats["glmem_peak_allocs"] >= (16 + 16 + 4) * pairs
        assert e.mem_stats()["glmem_peak_allocs"] == stats["glmem_peak_allocs"]


# -- 10. host form ---------------------------------------------------------------------------------

def test_host_form(engine, golden):
    queries = [_seq(R, 1100 + R) for R in (120, 0, 45)]
    subjects = [_seq(int(c), 1200 + i) for i, c in enumerate(np.random.default_rng(8).integers(0, 200, 40))]
    m = _Multi(queries, subjects, golden.blosum62)
    for go, ge in GAPS:
        dev, _ = _run(engine, m, go, ge, top=4)
        host = engine.score_db_overlap(queries, subjects, golden.blosum62, go, ge, top=4)
        assert np.array_equal(host["scores"], dev["scores"]) and np.array_equal(host["hits"], dev["hits"])
        _check_ranked(host, _wantm("host", m, go, ge), 4)
