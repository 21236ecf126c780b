"""Overlap (dovetail) database search, the alignments (gsa_align_db_multi_overlap_dev;
nw_lanes_overlap_trace.hip): every result exactly what tests/_overlap_oracle.py gives on
all six fields (score, start cell, end cell, CIGAR), status 0, the CIGAR replayed letter by letter to the
score, and the counts of gsa_align_db_multi_info, so that no case passes through another route.  A task
is 4 hits of one query, a unit align_db_multi_unit() tasks, a sweep 384 query rows.  Each case is first
shown by the oracle to have the property it is named for.  No tolerances anywhere."""
import ctypes

import numpy as np
import pytest

import gpuseqalign_amd as gsa
from tests import _overlap_oracle as oo
from tests.test_gpu_align_db import FIELDS, PLANTS, _gap_run
from tests.test_gpu_align_db_multi import EMPTY, _counts, _expect, _hit_list, _same
from tests.test_gpu_score_db_multi import _mixed_subjects, _Multi, _seq
from tests.test_gpu_score_db_overlap import SUB4, SUB6, _hdr, _record, _table

pytestmark = pytest.mark.gpu

K = 24
SWEEP = 16 * K
GAPS = [(-11, -1), (-5, -2), (-4, -4)]  # two affine models, one linear
Q, S = 4, 5  # SUB6's fillers: the queries', the subjects'; they match nothing
_REF = {}
_POOL = {}


def _t(r):
    return tuple(r[f] for f in FIELDS)


def _ref(key, m, q, s, go, ge):
    """The oracle's alignment of (query q, subject s) of pool `key`, computed once per gap model."""
    k = (key, q, s, go, ge)
    if k not in _REF:
        _REF[k] = oo.align(m.queries[q], m.subjects[s], m.subm, go, ge)
    return _REF[k]


def _ov(engine, m, hq, hs, go, ge, **kw):
    res = engine.align_db_overlap_dev(m.q.data_ptr(), m.qoff, m.db.data_ptr(), m.off, hq, hs, m.sub.data_ptr(), m.substsz,
                                      go, ge, **kw)
    return res, engine.last_align_db_overlap_info()


def _check(m, res, hq, hs, key, go, ge):
    assert len(res) == len(hq)
    for q, s, r in zip(hq, hs, res):
        want = _ref(key, m, q, s, go, ge)
        assert r["status"] == 0, (key, q, s, r)
        assert _t(r) == want, (key, q, s, len(m.queries[q]) - 1, len(m.subjects[s]) - 1, _t(r), want)
        assert oo.replay(m.queries[q], m.subjects[s], m.subm, go, ge, _t(r)) == r["score"], (key, q, s)
        R, C = len(m.queries[q]) - 1, len(m.subjects[s]) - 1
        assert r["i_end"] == R or r["j_end"] == C or R == 0 or C == 0
        assert r["i_start"] == 0 or r["j_start"] == 0 or r["score"] == 0  # the walk stops on a border
        if r["score"] == 0:
            assert r["cigar"] == "" and (r["i_start"], r["j_start"]) == (r["i_end"], r["j_end"]) == (R, 0)


def _code_bytes(R, C):
    return -(-R // SWEEP) * SWEEP * (C + 1) // 2


def _score_hits(engine, m, go, ge):
    return engine.score_db_overlap_dev(m.q.data_ptr(), m.qoff, m.db.data_ptr(), m.off, m.sub.data_ptr(), m.substsz, go, ge,
                                       top=len(m.subjects))["hits"]


def _same_end_as_the_score_call(engine, m, hq, hs, res, go, ge):
    sc = _score_hits(engine, m, go, ge)
    for q, s, r in zip(hq, hs, res):
        hit = sc[q][list(sc[q]["subject"]).index(s)]
        assert (r["score"], r["i_end"], r["j_end"]) == (int(hit["score"]), int(hit["i_end"]), int(hit["j_end"])), (q, s)


# -- 1. task and unit edges ------------------------------------------------------------------------

def _grid_pool(golden):
    if "grid" not in _POOL:
        rng = np.random.default_rng(5)
        queries = [_seq(int(c), 4000 + i) for i, c in enumerate(rng.integers(1, 121, 33))]
        _POOL["grid"] = _Multi(queries, _mixed_subjects(70, 7), golden.blosum62)
        lens = [len(x) - 1 for x in _POOL["grid"].subjects]
        assert lens[0] == 300 and lens[1] == 1 and lens[EMPTY] == 0
    return _POOL["grid"]


@pytest.mark.parametrize("nq", [1, 5, 33])
@pytest.mark.parametrize("go,ge", [(-11, -1), (-4, -4)])
def test_task_and_unit_edges(engine, golden, go, ge, nq):
    """Hits per query on every edge of a task and of a unit; a query without hits between two with some,
    a repeated pair, one subject hit by many queries, the subject with no letters."""
    m = _grid_pool(golden)
    for shift in (range(8) if nq <= 2 else (0, 3)):
        hq, hs = _hit_list(nq, shift)
        res, info = _ov(engine, m, hq, hs, go, ge)
        _counts(info, _expect(m, hq, hs))
        _check(m, res, hq, hs, "grid", go, ge)


# -- 2. row, lane and sweep edges in one call --------------------------------------------------------

@pytest.mark.parametrize("go,ge", GAPS)
def test_row_lane_and_sweep_edges_in_one_call(engine, go, ge):
    """The last query row on the first and last register row of a lane, on either side of the hand-off
    between two lanes and of the boundary between two sweeps, one, two and three sweeps, 5 hits each: one
    call, under one workgroup and under all.  Score and end cell are the score call's."""
    if "rows" not in _POOL:
        lens = [1, K - 1, K, K + 1, SWEEP - 1, SWEEP, SWEEP + 1, 2 * SWEEP + 1]
        subjects = [_seq(int(c), 7000 + i, 4) for i, c in enumerate(np.random.default_rng(12).integers(1, 301, 12))]
        _POOL["rows"] = _Multi([_seq(R, 500 + R, 4) for R in lens], subjects, SUB4)
    m = _POOL["rows"]
    rng = np.random.default_rng(3)
    hq = [q for k in range(5) for q in range(8)]
    hs = [int(s) for s in rng.integers(0, 12, 40)]
    want = [_ref("rows", m, q, s, go, ge) for q, s in zip(hq, hs)]
    on_col = [w for q, w in zip(hq, want) if w[0] > 0 and w[3] < len(m.queries[q]) - 1]
    on_row = [w for q, s, w in zip(hq, hs, want) if w[0] > 0 and w[4] < len(m.subjects[s]) - 1]
    assert len(on_col) >= 5 and len(on_row) >= 5, (len(on_col), len(on_row))
    res, info = _ov(engine, m, hq, hs, go, ge, max_workgroups=1)
    _counts(info, _expect(m, hq, hs))
    assert info["launches"] == 3 and info["lane_hits"] == 40 and info["workgroups"] == 1, info
    assert info["profile_builds"] == info["lane_queries"] == 8, info
    _check(m, res, hq, hs, "rows", go, ge)
    res0, info = _ov(engine, m, hq, hs, go, ge)
    _counts(info, _expect(m, hq, hs))
    assert _same(res, res0)
    _same_end_as_the_score_call(engine, m, hq, hs, res, go, ge)


# -- 3. the four arrangements with gaps across the hand-offs ---------------------------------------------

FRONT = SWEEP  # filler in front of a query: a multiple of 24 and of 384, so the hand-offs stay hand-offs


def _plant4(R, a, b, seed, inserted):
    """A query over 4 letters, and a subject that is the query with rows a..b removed, or with b - a + 1
    other letters inserted behind row a - 1 (letters only, no header)."""
    q = _seq(R, seed, 4)[1:]
    if not inserted:
        return q, np.concatenate([q[:a - 1], q[b:]])
    block = _seq(b - a + 1, seed + 100, 4)[1:]
    return q, np.concatenate([q[:a - 1], block, q[a - 1:]])


def arrangements(inserted):
    """(queries, subjects, [(q, s, arrangement, rows of filler in front of the query's image, a, b, edge)])."""
    queries, subjects, pairs = [], [], []
    for R, a, b, edge, seed in PLANTS:
        q, x = _plant4(R, a, b, seed, inserted)
        for name, qq, xx, front in [
                ("suffix-prefix", [Q] * FRONT + list(q), list(x) + [S] * 9, FRONT),
                ("prefix-suffix", list(q) + [Q] * 40, [S] * 11 + list(x), 0),
                ("query-inside", list(q), [S] * 11 + list(x) + [S] * 9, 0),
                ("subject-inside", [Q] * FRONT + list(q) + [Q] * 40, list(x), FRONT)]:
            queries.append(_hdr(qq))
            subjects.append(_hdr(xx))
            pairs.append((len(queries) - 1, len(subjects) - 1, name, front, a, b, edge))
    return queries, subjects, pairs


@pytest.mark.parametrize("inserted", [False, True], ids=["removed", "inserted"])
@pytest.mark.parametrize("go,ge", [(-11, -1), (-5, -2)])
def test_four_arrangements_with_gaps_across_hand_offs(engine, go, ge, inserted):
    """Gaps of 1 and 30 letters across the DPP hand-off (rows 24 / 25 of the planted part) and across the
    boundary array between two sweeps (rows 384 / 385), in each of the four arrangements: the query's
    suffix on the subject's prefix (the walk ends on column 0), the subject's suffix on the query's prefix
    (it ends on row 0, from column C), the query inside the subject and the subject inside the query."""
    key = ("arr", inserted)
    if key not in _POOL:
        queries, subjects, pairs = arrangements(inserted)
        _POOL[key] = (_Multi(queries, subjects, SUB6), pairs)
    m, pairs = _POOL[key]
    for q, s, name, front, a, b, edge in pairs:
        want = _ref(key, m, q, s, go, ge)
        R, C = len(m.queries[q]) - 1, len(m.subjects[s]) - 1
        count, row, col = _gap_run(want[5], want[1], want[2], "D" if inserted else "I")
        assert count == b - a + 1, "the oracle's alignment does not hold the planted block: %s" % want[5]
        if edge is not None:
            first = (col - (11 if name in ("prefix-suffix", "query-inside") else 0)) if inserted else row - front
            assert first <= edge < first + count - 1, (name, first, count, edge)
        if name == "suffix-prefix":
            assert (want[1], want[2]) == (front, 0) and want[3] == R and want[4] < C, want[:5]
        if name == "prefix-suffix":
            assert (want[1], want[2]) == (0, 11) and want[3] < R and want[4] == C, want[:5]
        if name == "query-inside":
            assert (want[1], want[2]) == (0, 11) and want[3] == R and want[4] == C - 9, want[:5]
        if name == "subject-inside":
            assert (want[1], want[2]) == (front, 0) and want[3] == R - 40 and want[4] == C, want[:5]
    hq = [p[0] for p in pairs]
    hs = [p[1] for p in pairs]
    res, info = _ov(engine, m, hq, hs, go, ge, max_workgroups=1)
    _counts(info, _expect(m, hq, hs))
    assert info["workgroups"] == 1 and info["profile_builds"] == len(pairs), info
    _check(m, res, hq, hs, key, go, ge)
    _same_end_as_the_score_call(engine, m, hq, hs, res, go, ge)


# -- 4. where walks end, ends in an earlier sweep, score 0, homopolymers -----------------------------------

def border_cases():
    core = lambda n, seed: list(_seq(n, seed, 4)[1:])
    c30, c50 = core(30, 71), core(50, 72)
    homo = [[1] * n for n in (8, 30, 3)]
    mixed = [1] * 5 + [2] + [1] * 5
    queries = [[Q] * 7 + c30,            # 0: its suffix on subject 0's prefix: the walk ends on column 0
               c30 + [Q] * 7,            # 1: subject 1's suffix on its prefix: the walk ends on row 0
               c30,                      # 2: subject 2 itself: the walk ends at (0, 0)
               c50 + [Q] * (2 * SWEEP),  # 3: three sweeps, subject 3 ends on column C in the first
               [Q] * 9,                  # 4: matches nothing
               homo[0], homo[2], [Q] * 400 + c50 + [Q] * 300]  # 7: subject 8 ends on column C in the second sweep
    subjects = [c30 + [S] * 5, [S] * 6 + c30, c30, [S] * 4 + c50, [S] * 13, homo[1], mixed, homo[2], c50]
    return [_hdr(q) for q in queries], [_hdr(x) for x in subjects]


@pytest.mark.parametrize("go,ge", GAPS)
def test_where_walks_end_and_where_alignments_end(engine, go, ge):
    if "border" not in _POOL:
        _POOL["border"] = _Multi(*border_cases(), SUB6)
    m = _POOL["border"]
    assert _ref("border", m, 0, 0, go, ge) == (150, 7, 0, 37, 30, "30=")      # column 0, i_start > 0
    assert _ref("border", m, 1, 1, go, ge) == (150, 0, 6, 30, 36, "30=")      # row 0, j_start > 0, column C
    assert _ref("border", m, 2, 2, go, ge) == (150, 0, 0, 30, 30, "30=")      # (0, 0)
    assert _ref("border", m, 3, 3, go, ge) == (250, 0, 4, 50, 54, "50=")      # column C in the first of three sweeps
    assert _ref("border", m, 7, 8, go, ge) == (250, 400, 0, 450, 50, "50=")   # column C in the second of two
    assert _ref("border", m, 4, 4, go, ge) == (0, 9, 0, 9, 0, "")             # score 0
    hq = [0, 1, 2, 3, 7, 4, 5, 5, 5, 6, 6, 6, 4, 0, 3, 7]
    hs = [0, 1, 2, 3, 8, 4, 5, 6, 7, 5, 6, 7, 0, 4, 2, 3]
    res, info = _ov(engine, m, hq, hs, go, ge)
    _counts(info, _expect(m, hq, hs))
    _check(m, res, hq, hs, "border", go, ge)
    _same_end_as_the_score_call(engine, m, hq, hs, res, go, ge)


# -- 5. chunks -------------------------------------------------------------------------------------

def test_chunking_and_the_limit_below_the_largest_hit(engine, golden):
    """A limit that forces at least three chunks gives the default run's results; the limit at the largest
    hit's own need runs, the limit below it is refused: this mode has no status 1."""
    m = _grid_pool(golden)
    hq, hs = _hit_list(5, 3)
    first = hs.index(0)  # the 300-letter subject once only: codes depend on C alone within a sweep class
    hs = [2 if s == 0 and h != first else s for h, s in enumerate(hs)]
    go, ge = -11, -1
    need = [_code_bytes(len(m.queries[q]) - 1, len(m.subjects[s]) - 1) if len(m.subjects[s]) > 1 else 0 for q, s in zip(hq, hs)]
    total, largest = sum(need), max(need)
    limit = total // 3
    assert limit >= largest and 2 * limit < total
    base, ib = _ov(engine, m, hq, hs, go, ge)
    _counts(ib, _expect(m, hq, hs))
    assert ib["code_bytes"] == total
    res, info = _ov(engine, m, hq, hs, go, ge, scratch_limit=limit)
    assert info["chunks"] >= 3 and 0 < info["code_bytes"] <= limit, (info, limit)
    assert info["lane_hits"] == ib["lane_hits"] and info["unsupported"] == 0 and info["tasks"] >= ib["tasks"], info
    assert info["launches"] == info["chunks"], info  # one sweep class
    assert _same(res, base)
    _check(m, res, hq, hs, "grid", go, ge)
    res, info = _ov(engine, m, hq, hs, go, ge, scratch_limit=largest)
    assert info["lane_hits"] == ib["lane_hits"] and _same(res, base), info
    assert sum(n == largest for n in need) == 1
    before = _record(engine)
    with pytest.raises(gsa.NwError) as ei:
        _ov(engine, m, hq, hs, go, ge, scratch_limit=largest - 1)
    assert ei.value.stat == gsa.NwStat.errorInvalidValue and engine.last_launch() == before


# -- 6. buffer, tables, refusals -----------------------------------------------------------------------

def _raw(engine, m, hq, hs, go, ge, cap, limit=0, wgs=0, nhits=None, nq=None, nsubj=None, null=(), qoff=None, off=None):
    """gsa_align_db_multi_overlap_dev through the raw ABI: (status, results, buffer, cigar_need, info)."""
    i64p, i32p = ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int32)
    qo = np.ascontiguousarray(m.qoff if qoff is None else qoff, dtype=np.int64)
    of = np.ascontiguousarray(m.off if off is None else off, dtype=np.int64)
    q = np.ascontiguousarray(hq, dtype=np.int32)
    s = np.ascontiguousarray(hs, dtype=np.int32)
    n = len(q) if nhits is None else nhits
    res = (gsa.AlignDbResult * max(len(q), 1))()
    buf = ctypes.create_string_buffer(max(cap, 1))
    need, info, ms = ctypes.c_int64(-1), gsa.AlignDbMultiInfo(), ctypes.c_float(0.0)
    arg = lambda name, v: None if name in null else v
    st = gsa.lib().gsa_align_db_multi_overlap_dev(
        engine._h, arg("queries", m.q.data_ptr()), arg("q_off", qo.ctypes.data_as(i64p)), len(qo) - 1 if nq is None else nq,
        arg("db", m.db.data_ptr()), arg("db_off", of.ctypes.data_as(i64p)), len(of) - 1 if nsubj is None else nsubj,
        arg("hit_query", q.ctypes.data_as(i32p)), arg("hit_subject", s.ctypes.data_as(i32p)), n, arg("subst", m.sub.data_ptr()),
        m.substsz, go, ge, wgs, limit, arg("out", res), arg("cigar", buf), cap, ctypes.byref(need),
        ctypes.byref(info), ctypes.byref(ms), None)
    return st, res, buf, need.value, info


def _tuples(res, buf):
    return [(r.score, r.i_start, r.j_start, r.i_end, r.j_end, buf.raw[r.cigar_off:r.cigar_off + r.cigar_len].decode())
            for r in res]


def test_cigar_buffer(engine, golden):
    """cigar_cap too small for the last two hits: those have status 2, the earlier ones are intact, and
    *cigar_need is the total of the full run."""
    m = _grid_pool(golden)
    hq, hs = [0, 3, 1, 3, 2, 0], [0, 5, 12, 7, 9, 12]
    go, ge = -11, -1
    st, full, buf, need, _ = _raw(engine, m, hq, hs, go, ge, 1 << 16)
    assert st == 0 and 0 < need <= 1 << 16
    strings = [buf.raw[r.cigar_off:r.cigar_off + r.cigar_len].decode() for r in full]
    for q, s, r, c in zip(hq, hs, full, strings):
        want = _ref("grid", m, q, s, go, ge)
        assert r.status == 0 and c == want[5] and buf.raw[r.cigar_off + r.cigar_len] == 0
    assert need == sum(len(c) + 1 for c in strings)
    assert [r.cigar_off for r in full] == list(np.cumsum([0] + [len(c) + 1 for c in strings[:-1]]))  # hit order
    cap = int(full[-2].cigar_off) + 1  # the fifth string needs more than its terminator
    assert len(strings[-2]) > 0 and len(strings[-1]) > 0
    st, res, buf2, need2, info = _raw(engine, m, hq, hs, go, ge, cap)
    assert st == 0 and need2 == need and info.lane_hits == len(hq) and info.chunks == 1 and info.unsupported == 0
    assert [r.status for r in res] == [0, 0, 0, 0, 2, 2]
    for r, f, c in zip(res[:4], full[:4], strings[:4]):
        assert (r.cigar_off, r.cigar_len) == (f.cigar_off, f.cigar_len)
        assert buf2.raw[r.cigar_off:r.cigar_off + r.cigar_len + 1] == c.encode() + b"\0"
    for r, f in zip(res, full):
        assert (r.score, r.i_start, r.j_start, r.i_end, r.j_end) == (f.score, f.i_start, f.j_start, f.i_end, f.j_end)


def test_tables(engine):
    """An asymmetric table (row = query letter), one with values outside int8, a 4-letter alphabet."""
    rng = np.random.default_rng(11)
    asym = rng.integers(-6, 12, size=(20, 20)).astype(np.int32)
    assert not np.array_equal(asym, asym.T)
    wide = _table(20, 300, -200)
    dna = _table(4, 2, -3)
    hq = [q for s in range(5) for q in range(3)]
    hs = [int(s) for s in np.random.default_rng(4).integers(0, 10, 15)]
    for name, sub, alphabet, (go, ge) in [("asym", asym, 20, (-11, -1)), ("wide", wide, 20, (-5, -2)),
                                          ("dna", dna, 4, (-5, -2)), ("dna", dna, 4, (-4, -4))]:
        if name not in _POOL:
            subjects = [_seq(int(c), 2100 + i, alphabet) for i, c in enumerate(np.random.default_rng(21).integers(1, 151, 10))]
            _POOL[name] = _Multi([_seq(90, 13, alphabet), _seq(17, 14, alphabet), _seq(130, 15, alphabet)], subjects, sub)
        m = _POOL[name]
        assert m.substsz == len(sub)
        res, info = _ov(engine, m, hq, hs, go, ge)
        _counts(info, _expect(m, hq, hs))
        _check(m, res, hq, hs, ("tab", name), go, ge)


def test_refusals_run_over_the_hits_only(engine, golden):
    """A subject of 8192 letters, a query whose profile cannot fit LDS, a query of 8192 letters under a
    small table and a pair past the value bound are in the database: calls that do not name them run,
    calls that do are refused."""
    big = _Multi([_seq(60, 4), _seq(4 * SWEEP + 1, 5), _seq(0, 6)], [_seq(5, 7), _seq(8192, 8), _seq(0, 9)], golden.blosum62)
    m_ok_q, m_ok_s = [0, 0, 2, 1, 2], [0, 2, 1, 2, 2]  # pairs with an empty side are the host's
    st, res, buf, need, info = _raw(engine, big, m_ok_q, m_ok_s, -11, -1, 4096)
    assert st == 0 and info.lane_hits == 1 and info.unsupported == 0 and [r.status for r in res] == [0] * 5
    got = _tuples(res, buf)
    assert got[0] == oo.align(big.queries[0], big.subjects[0], big.subm, -11, -1)
    assert got[1] == (0, 60, 0, 60, 0, "")  # an empty side: score 0, all cells (R, 0)
    assert got[2] == (0, 0, 0, 0, 0, "") and got[4] == (0, 0, 0, 0, 0, "")
    assert got[3] == (0, 4 * SWEEP + 1, 0, 4 * SWEEP + 1, 0, "")
    before = _record(engine)
    for hq, hs in ([0, 0], [0, 1]), ([0, 1], [0, 0]):
        assert _raw(engine, big, hq, hs, -11, -1, 4096)[0] == gsa.NwStat.errorInvalidValue
    rows = _Multi([_seq(8191, 7, 4), _seq(8192, 7, 4), _seq(3, 8, 4)], [_seq(12, 4, 4), _seq(0, 5, 4)], SUB4)
    st, res, buf, need, info = _raw(engine, rows, [0, 2, 1], [0, 0, 1], -4, -4, 1 << 16)
    assert st == 0 and info.lane_hits == 2 and info.unsupported == 0
    got = _tuples(res, buf)
    assert got[0] == oo.align(rows.queries[0], rows.subjects[0], SUB4, -4, -4)
    assert got[1] == oo.align(rows.queries[2], rows.subjects[0], SUB4, -4, -4) and got[2] == (0, 8192, 0, 8192, 0, "")
    assert _raw(engine, rows, [0, 1], [0, 0], -4, -4, 1 << 16)[0] == gsa.NwStat.errorInvalidValue
    s = 65533
    tab = _table(4, s, -s)
    val = _Multi([_seq(4, 1, 4), _seq(3, 5, 4)], [_seq(6, 2, 4), _seq(7, 3, 4)], tab)
    st, res, _, _, info = _raw(engine, val, [0, 1, 1], [0, 0, 1], -1, -1, 4096)   # 4 s + 1 + 10 = 2^18 - 1 at most
    assert st == 0 and info.lane_hits == 3
    for r, (q, x) in zip(res, [(0, 0), (1, 0), (1, 1)]):
        assert (r.score, r.i_end, r.j_end) == oo.score(val.queries[q], val.subjects[x], tab, -1, -1)
    assert _raw(engine, val, [0, 1, 0], [0, 0, 1], -1, -1, 4096)[0] == gsa.NwStat.errorInvalidValue  # 4 s + 1 + 11
    assert _raw(engine, val, [0], [0], -2, -1, 4096)[0] == gsa.NwStat.errorInvalidValue
    assert engine.last_launch() == before


def test_inherited_rejections(engine, golden):
    m = _Multi([_seq(60, 4), _seq(20, 5), _seq(33, 6)], [_seq(int(c), 1300 + c) for c in (5, 80, 41, 17, 66)], golden.blosum62)
    hq, hs = [0, 2, 1], [1, 4, 0]
    before = _record(engine)

    def good():
        res, info = _ov(engine, m, hq, hs, -11, -1)
        _counts(info, _expect(m, hq, hs))
        _check(m, res, hq, hs, "inv", -11, -1)

    def bad(go=-11, ge=-1, q=hq, s=hs, **kw):
        st = _raw(engine, m, q, s, go, ge, kw.pop("cap", 4096), **kw)[0]
        assert st == gsa.NwStat.errorInvalidValue, kw
        assert engine.last_launch() == before

    good()
    for table in ("qoff", "off"):
        src = getattr(m, table)
        equal, dec, neg = src.copy(), src.copy(), src.copy()
        equal[2] = equal[1]
        dec[2] = dec[1] - 1
        neg[0] = -1
        for off in (equal, dec, neg):
            bad(**{table: off})
    bad(nq=0)
    bad(nsubj=0)
    bad(go=-1, ge=-11)
    bad(ge=1, go=-11)
    bad(q=[0, 3, 1])    # a query index outside 0 ... nq - 1
    bad(q=[0, -1, 1])
    bad(s=[1, 5, 0])    # a subject index outside 0 ... nsubj - 1
    bad(s=[1, -1, 0])
    bad(wgs=-1)
    bad(limit=-1)
    bad(nhits=-1)
    bad(cap=-1)
    for name in ("queries", "q_off", "db", "db_off", "hit_query", "hit_subject", "subst", "out", "cigar"):
        bad(null=(name,))
    with pytest.raises(gsa.NwError) as ei:  # hit lists of different lengths never reach the library
        _ov(engine, m, [0, 1], [0], -11, -1)
    assert ei.value.stat == gsa.NwStat.errorInvalidValue
    for substsz in (0, 33):
        with pytest.raises(gsa.NwError) as ei:
            engine.align_db_overlap_dev(m.q.data_ptr(), m.qoff, m.db.data_ptr(), m.off, hq, hs, m.sub.data_ptr(), substsz, -11, -1)
        assert ei.value.stat == gsa.NwStat.errorInvalidValue, substsz
    good()


# -- 7. neighbours ---------------------------------------------------------------------------------

def test_neighbours_keep_their_record_and_their_results(engine, golden):
    """align_db_semi_dev and align_db_multi_dev in both old modes right before and right after, over a
    query of two sweeps: the calls share context buffers.  gsa_last_launch is left alone."""
    queries = [_seq(R, 900 + R) for R in (60, 500, 130)]
    subjects = [_seq(int(c), 950 + i) for i, c in enumerate([80, 200, 33, 150, 7, 260, 90, 121, 64])]
    m = _Multi(queries, subjects, golden.blosum62)
    hq, hs = [1, 0, 1, 2, 1, 0], [5, 1, 0, 3, 8, 5]

    def around():
        out = [engine.align_db_multi_dev(m.q.data_ptr(), m.qoff, m.db.data_ptr(), m.off, hq, hs, m.sub.data_ptr(),
                                         m.substsz, -11, -1, local) for local in (True, False)]
        return out + [engine.align_db_semi_dev(m.q.data_ptr(), m.qoff, m.db.data_ptr(), m.off, hq, hs, m.sub.data_ptr(),
                                               m.substsz, -11, -1)]

    m.single(engine, -11, -1, True)  # a launch record to be left alone
    before = _record(engine)
    first = around()
    res, info = _ov(engine, m, hq, hs, -11, -1)
    assert engine.last_launch() == before
    _counts(info, _expect(m, hq, hs))
    assert info["launches"] == 2, info
    again = around()
    assert all(_same(a, b) for a, b in zip(first, again))
    _check(m, res, hq, hs, "nb", -11, -1)
    res2, _ = _ov(engine, m, hq, hs, -11, -1)
    assert _same(res, res2)


def test_scratch_is_counted_in_mem_stats(golden):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    m = _grid_pool(golden)
    hq, hs = _hit_list(5, 3)
    with gsa.Engine(0) as e:
        e.reset_mem_stats()
        _ov(e, m, hq, hs, -11, -1)
        info = e.last_align_db_overlap_info()
        stats = e.mem_stats()
        assert stats["glmem_peak_allocs"] >= info["code_bytes"] > 0
        # the semi-global call on the same context reuses the slots: nothing new is held
        e.align_db_semi_dev(m.q.data_ptr(), m.qoff, m.db.data_ptr(), m.off, hq, hs, m.sub.data_ptr(), m.substsz, -11, -1)
        assert e.mem_stats()["glmem_peak_allocs"] == stats["glmem_peak_allocs"]


# -- 8. host forms ---------------------------------------------------------------------------------

def test_host_forms(engine, golden):
    """align_db_overlap and search_db_overlap against the oracle, an empty query and an empty subject
    among the pairs; search_db_overlap makes one alignment call."""
    queries = [_seq(R, 1100 + R) for R in (120, 0, 45)]
    subjects = [_seq(int(c), 1200 + i) for i, c in enumerate(np.random.default_rng(8).integers(1, 200, 40))]
    subjects[4] = _seq(0, 1)
    hq, hs = [0, 2, 1, 0, 2, 2, 0], [3, 3, 5, 17, 30, 3, 4]
    sub = golden.blosum62
    for go, ge in [(-11, -1), (-4, -4)]:
        a = engine.align_db_overlap(queries, subjects, hq, hs, sub, go, ge)
        info = engine.last_align_db_overlap_info()
        assert (info["lane_hits"], info["unsupported"], info["lane_queries"]) == (5, 0, 2), info
        assert [_t(r) for r in a] == [oo.align(queries[q], subjects[s], sub, go, ge) for q, s in zip(hq, hs)]
        assert all(r["status"] == 0 for r in a)
        found = engine.search_db_overlap(queries, subjects, sub, go, ge, top=4)
        info = engine.last_align_db_overlap_info()
        assert info["lane_hits"] == 8 and info["chunks"] == 1, info  # one call; the empty query's four hits are the host's
        for q, row in enumerate(found):
            want = [oo.align(queries[q], x, sub, go, ge) for x in subjects]
            order = sorted(range(len(subjects)), key=lambda s: (-want[s][0], s))[:4]
            assert [s for s, _ in row] == order, q
            assert [_t(d) for _, d in row] == [want[s] for s in order], q
    assert engine.align_db_overlap(queries, subjects, [], [], sub, -11, -1) == []
    info = engine.last_align_db_overlap_info()
    assert info["lane_hits"] == 0 and info["chunks"] == 0 and info["launches"] == 0 and info["tasks"] == 0
    assert engine.search_db_overlap(queries, subjects, sub, -11, -1, top=0) == [[], [], []]


# -- 9. after every other family on one context, and on a side stream ------------------------------------

def _both_calls(e, m, hq, hs, stream=None):
    sc = e.score_db_overlap_dev(m.q.data_ptr(), m.qoff, m.db.data_ptr(), m.off, m.sub.data_ptr(), m.substsz, -11, -1,
                                top=3, stream=stream)
    al = e.align_db_overlap_dev(m.q.data_ptr(), m.qoff, m.db.data_ptr(), m.off, hq, hs, m.sub.data_ptr(), m.substsz,
                                -11, -1, stream=stream)
    return sc["scores"].tolist(), sc["hits"].tolist(), [_t(r) for r in al]


def test_after_each_existing_family_and_on_a_side_stream(golden):
    """The score and the align call alone on a fresh engine, then right after every existing entry-point
    family (tests/_families.py) on that one context, then on a non-null stream: the same results every
    time, the oracle's, and gsa_sync reports nothing."""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    from tests._families import FAMILIES, SMALL
    queries = [_seq(R, 900 + R) for R in (60, 500, 130)]
    subjects = [_seq(int(c), 950 + i) for i, c in enumerate([80, 200, 33, 150, 7, 260, 90, 121, 64])]
    hq, hs = [1, 0, 1, 2, 1, 0], [5, 1, 0, 3, 8, 5]
    with gsa.Engine(0) as e:
        m = _Multi(queries, subjects, golden.blosum62)
        first = _both_calls(e, m, hq, hs)
        e.sync()
        assert first[2] == [oo.align(queries[q], subjects[s], golden.blosum62, -11, -1) for q, s in zip(hq, hs)]
        assert first[0] == [[oo.score(Y, X, golden.blosum62, -11, -1)[0] for X in subjects] for Y in queries]
        for f in FAMILIES:
            print("overlap after", f.name)
            f.run(e, SMALL)
            assert _both_calls(e, m, hq, hs) == first, f.name
            e.sync()
        side = torch.cuda.Stream()
        torch.cuda.synchronize()
        assert _both_calls(e, m, hq, hs, stream=side.cuda_stream) == first
        e.sync(side.cuda_stream)
        assert _both_calls(e, m, hq, hs) == first
        e.sync()
