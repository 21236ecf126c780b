"""The alignments of many queries' hits in one call (gsa_align_db_multi_dev; nw_lanes_trace_multi.hip,
DESIGN.md 2.2g): every result exactly what tests/_align_oracle.py gives on all six fields (score, start
cell, end cell, CIGAR), and exactly what align_db_dev gives for that hit's query alone.  Every case
asserts, from gsa_align_db_multi_info, how many hits were traced and in how many chunks, launches, tasks
and units, so that no case passes through another route.  A task is 4 hits of one query, a unit
align_db_multi_unit() tasks, a sweep 384 query rows.  No tolerances anywhere."""
import ctypes

import numpy as np
import pytest

import gpuseqalign_amd as gsa
from tests import _align_oracle as ao
from tests.test_gpu_align_db import AFFINE4, FIELDS, PLANTS, _gap_run, _plant
from tests.test_gpu_score import MODES
from tests.test_gpu_score_db_multi import _Multi, _mixed_subjects, _seq

pytestmark = pytest.mark.gpu

K = 24
SWEEP = 16 * K
TASK = 4
_REF = {}


def _t(r):
    return tuple(r[f] for f in FIELDS)


def _ref(key, m, q, s, go, ge, local):
    """The oracle's alignment of (query q, subject s) of pool `key`, computed once per mode."""
    k = (key, q, s, go, ge, local)
    if k not in _REF:
        _REF[k] = ao.align(m.queries[q], m.subjects[s], m.subm, go, ge, local)
    return _REF[k]


def _multi(engine, m, hq, hs, go, ge, local, **kw):
    res = engine.align_db_multi_dev(m.q.data_ptr(), m.qoff, m.db.data_ptr(), m.off, hq, hs, m.sub.data_ptr(), m.substsz,
                                    go, ge, local, **kw)
    return res, engine.last_align_db_multi_info()


def _loop(engine, m, hq, hs, go, ge, local, limit=0):
    """align_db_dev per query on that query's hits, put back in the order of the hit list."""
    out = [None] * len(hq)
    for q in sorted(set(hq)):
        at = [h for h in range(len(hq)) if hq[h] == q]
        res = engine.align_db_dev(m.q.data_ptr() + 4 * int(m.qoff[q]), len(m.queries[q]), m.db.data_ptr(), m.off,
                                  [hs[h] for h in at], m.sub.data_ptr(), m.substsz, go, ge, local, scratch_limit=limit)
        for h, r in zip(at, res):
            out[h] = r
    return out


def _same(a, b):
    strip = lambda rows: [{k: v for k, v in r.items() if k != "kernel_ms"} for r in rows]
    return strip(a) == strip(b)


def _expect(m, hq, hs):
    """The info's counts for a call whose pairs with letters on both sides are all traced in one chunk."""
    per = {}
    for q, s in zip(hq, hs):
        if len(m.queries[q]) > 1 and len(m.subjects[s]) > 1:
            per[q] = per.get(q, 0) + 1
    unit = gsa.align_db_multi_unit()
    tasks = {q: -(-n // TASK) for q, n in per.items()}
    return {"lane_hits": sum(per.values()), "unsupported": 0, "chunks": 1 if per else 0,
            "launches": len({-(-(len(m.queries[q]) - 1) // SWEEP) for q in per}), "lane_queries": len(per),
            "tasks": sum(tasks.values()), "units": sum(-(-t // unit) for t in tasks.values())}


def _counts(info, want):
    assert {k: info[k] for k in want} == want, info


def _check(m, res, hq, hs, key, go, ge, local):
    assert len(res) == len(hq)
    for q, s, r in zip(hq, hs, res):
        want = _ref(key, m, q, s, go, ge, local)
        assert r["status"] == 0, (key, q, s, r)
        assert _t(r) == want, (key, q, s, len(m.queries[q]) - 1, len(m.subjects[s]) - 1, _t(r), want)


# -- 1. task and unit edges ------------------------------------------------------------------------

_GRID = {}
EMPTY = 35  # _mixed_subjects(70, .): the subject with no letters


def _grid_pool(golden):
    if not _GRID:
        rng = np.random.default_rng(5)
        queries = [_seq(int(c), 4000 + i) for i, c in enumerate(rng.integers(1, 121, 33))]
        _GRID["m"] = _Multi(queries, _mixed_subjects(70, 7), golden.blosum62)
        lens = [len(x) - 1 for x in _GRID["m"].subjects]
        assert lens[0] == 300 and lens[1] == 1 and lens[EMPTY] == 0
    return _GRID["m"]


def _hit_list(nq, shift):
    """Hits per query 0, 1, 3, 4, 5, 4 unit - 1, 4 unit, 4 unit + 1 in turn, the list interleaved by
    query.  Where a query has three hits or more they begin with the 300-letter subject, the 1-letter
    subject and the 1-letter subject again (a repeated pair; subjects 0 and 1 are hit by many queries);
    the fourth is the subject with no letters."""
    unit = TASK * gsa.align_db_multi_unit()
    sizes = [0, 1, 3, 4, 5, unit - 1, unit, unit + 1]
    rng = np.random.default_rng(100 * nq + shift)
    rows = []
    for q in range(nq):
        row = [int(s) for s in rng.integers(2, 70, sizes[(q + shift) % len(sizes)])]
        row[:3] = [0, 1, 1][:len(row)] if len(row) >= 3 else row[:3]
        if len(row) >= 4:
            row[3] = EMPTY
        rows.append(row)
    hq, hs = [], []
    for k in range(max(len(r) for r in rows)):
        for q, row in enumerate(rows):
            if k < len(row):
                hq.append(q)
                hs.append(row[k])
    return hq, hs


@pytest.mark.parametrize("nq", [1, 2, 5, 33])
@pytest.mark.parametrize("go,ge,local", MODES)
def test_task_and_unit_edges(engine, golden, go, ge, local, nq):
    m = _grid_pool(golden)
    for shift in (range(8) if nq <= 2 else (0, 3)):
        hq, hs = _hit_list(nq, shift)
        if nq > 2 and shift == 0:
            # query 8 has no hits, between queries 7 and 9 that have some
            assert 0 not in hq and (nq < 33 or (8 not in hq and 7 in hq and 9 in hq))
        res, info = _multi(engine, m, hq, hs, go, ge, local)
        _counts(info, _expect(m, hq, hs))
        _check(m, res, hq, hs, "grid", go, ge, local)
        assert _same(res, _loop(engine, m, hq, hs, go, ge, local)), (nq, shift)


# -- 2. profile swaps in one workgroup -------------------------------------------------------------

_SWAP = {}


def _swap_pool(golden):
    """Letter 0 -- the header element of the next query in the buffer, what a read past a query's end
    finds -- scores +15 against every subject letter, and no sequence holds it.  A 383-letter query,
    then 5-letter ones, two of them identical."""
    if not _SWAP:
        n = int(round(np.sqrt(golden.blosum62.size)))
        sub = np.array(golden.blosum62, dtype=np.int32).reshape(n, n).copy()
        sub[0, :] = 15

        def letters(c, seed):
            x = _seq(c, seed, 19)
            x[1:] += 1  # letters 1..19
            return x

        queries = [letters(5, 2), letters(SWEEP - 1, 1), letters(5, 3), letters(5, 3)]
        _SWAP["m"] = _Multi(queries, [letters(c, 10 + c) for c in (300, 30, 7, 120, 5, 64)], sub)
    return _SWAP["m"]


@pytest.mark.parametrize("go,ge,local", MODES)
def test_profile_swaps_in_one_workgroup(engine, golden, go, ge, local):
    m = _swap_pool(golden)
    hq = [q for s in range(6) for q in range(4)]
    hs = [s for s in range(6) for q in range(4)]
    r1, i1 = _multi(engine, m, hq, hs, go, ge, local, max_workgroups=1)
    _counts(i1, _expect(m, hq, hs))
    assert i1["workgroups"] == 1 and i1["launches"] == 1 and i1["lane_queries"] == 4, i1
    assert i1["profile_builds"] == i1["lane_queries"], i1
    _check(m, r1, hq, hs, "swap", go, ge, local)
    for h in range(len(hq)):
        if hq[h] == 2:
            assert _t(r1[h]) == _t(r1[h + 1])  # the identical queries
    assert _same(r1, _loop(engine, m, hq, hs, go, ge, local))
    for wg in (2, 0):
        r, info = _multi(engine, m, hq, hs, go, ge, local, max_workgroups=wg)
        _counts(info, _expect(m, hq, hs))
        assert info["profile_builds"] >= info["launches"] and (not wg or info["workgroups"] <= wg), info
        assert _same(r, r1), wg


# -- 3. row, lane and sweep edges in one call --------------------------------------------------------

_ROWS = {}


@pytest.mark.parametrize("go,ge,local", MODES)
def test_row_lane_and_sweep_edges_in_one_call(engine, golden, go, ge, local):
    """The last query row on the first and last register row of a lane, on either side of the hand-off
    between two lanes and of the boundary between two sweeps, one, two and three sweeps: one call."""
    if not _ROWS:
        lens = [1, K - 1, K, K + 1, SWEEP - 1, SWEEP, SWEEP + 1, 2 * SWEEP + 1]
        subjects = [_seq(int(c), 7000 + i) for i, c in enumerate(np.random.default_rng(12).integers(1, 121, 12))]
        _ROWS["m"] = _Multi([_seq(R, 500 + R) for R in lens], subjects, golden.blosum62)
    m = _ROWS["m"]
    rng = np.random.default_rng(3)
    hq = [q for k in range(5) for q in range(8)]
    hs = [int(s) for s in rng.integers(0, 12, 40)]
    res, info = _multi(engine, m, hq, hs, go, ge, local)
    _counts(info, _expect(m, hq, hs))
    assert info["launches"] == 3 and info["lane_hits"] == 40, info
    _check(m, res, hq, hs, "rows", go, ge, local)
    assert _same(res, _loop(engine, m, hq, hs, go, ge, local))


@pytest.mark.parametrize("inserted", [False, True], ids=["removed", "inserted"])
@pytest.mark.parametrize("go,ge,local", AFFINE4)
def test_gaps_across_hand_offs_behind_another_query(engine, golden, go, ge, local, inserted):
    """Gaps of 1 and 30 rows across the DPP hand-off (rows 24 / 25) and across the boundary array
    between two sweeps (rows 384 / 385), planted in queries that are not the first their workgroup
    runs: with one workgroup per launch a longer query of the same sweep class goes first."""
    key = ("plant", inserted)
    if key not in _ROWS:
        queries, subjects, pairs = [_seq(450, 91), _seq(120, 92)], _mixed_subjects(4, 9)[:2], []
        for R, a, b, edge, seed in PLANTS:
            q, x = _plant(R, a, b, seed, inserted)
            queries.append(q)
            subjects.append(x)
            pairs.append((len(queries) - 1, len(subjects) - 1, a, b, edge))
        _ROWS[key] = (_Multi(queries, subjects, golden.blosum62), pairs)
    m, pairs = _ROWS[key]
    for q, s, a, b, edge in pairs:
        want = _ref(key, m, q, s, go, ge, local)
        count, row, col = _gap_run(want[5], want[1], want[2], "D" if inserted else "I")
        assert count == b - a + 1, "the oracle's alignment does not hold the planted block: %s" % want[5]
        if edge is not None:
            first = col if inserted else row
            assert first <= edge < first + count - 1, (first, count, edge)
    hq = [0, 1, 0, 1] + [q for q, _, _, _, _ in pairs] + [q for q, _, _, _, _ in pairs]
    hs = [0, 0, 1, 1] + [s for _, s, _, _, _ in pairs] + [0 for _ in pairs]
    res, info = _multi(engine, m, hq, hs, go, ge, local, max_workgroups=1)
    _counts(info, _expect(m, hq, hs))
    assert info["launches"] == 2 and info["workgroups"] == 1 and info["profile_builds"] == 5, info
    # longest first: the 450-letter query before the 420-letter one, the 120-letter one before the two of 100
    assert len(m.queries[0]) > len(m.queries[4]) > SWEEP and len(m.queries[1]) > len(m.queries[2]) == len(m.queries[3])
    _check(m, res, hq, hs, key, go, ge, local)
    assert _same(res, _loop(engine, m, hq, hs, go, ge, local))


# -- 4. chunks -------------------------------------------------------------------------------------

def _code_bytes(R, C):
    return -(-R // SWEEP) * SWEEP * (C + 1) // 2


def test_chunking(engine, golden):
    """A limit that forces at least three chunks gives the default run's results; a limit below the
    largest hit's own need leaves that hit alone with status 1, its score and end cell intact."""
    m = _grid_pool(golden)
    hq, hs = _hit_list(5, 3)
    first = hs.index(0)  # the 300-letter subject once only: codes depend on C alone within a sweep class
    hs = [2 if s == 0 and h != first else s for h, s in enumerate(hs)]
    go, ge, local = -11, -1, True
    need = [_code_bytes(len(m.queries[q]) - 1, len(m.subjects[s]) - 1) if len(m.subjects[s]) > 1 else 0 for q, s in zip(hq, hs)]
    total, largest = sum(need), max(need)
    limit = total // 3
    assert limit >= largest and 2 * limit < total
    base, ib = _multi(engine, m, hq, hs, go, ge, local)
    _counts(ib, _expect(m, hq, hs))
    assert ib["code_bytes"] == total
    res, info = _multi(engine, m, hq, hs, go, ge, local, scratch_limit=limit)
    assert info["chunks"] >= 3 and 0 < info["code_bytes"] <= limit, (info, limit)
    assert info["lane_hits"] == ib["lane_hits"] and info["unsupported"] == 0 and info["tasks"] >= ib["tasks"], info
    assert info["launches"] == info["chunks"], info  # one sweep class
    assert _same(res, base)
    _check(m, res, hq, hs, "grid", go, ge, local)
    assert _same(res, _loop(engine, m, hq, hs, go, ge, local, limit=limit))

    small = largest - 1
    out = [h for h in range(len(hq)) if need[h] > small]
    assert len(out) == 1, "more than one hit of the largest size"
    res, info = _multi(engine, m, hq, hs, go, ge, local, scratch_limit=small)
    assert info["unsupported"] == 1 and info["lane_hits"] == ib["lane_hits"] - 1 and info["code_bytes"] <= small, info
    for h, r in enumerate(res):
        want = _ref("grid", m, hq[h], hs[h], go, ge, local)
        if h == out[0]:
            assert r["status"] == 1 and r["cigar"] == ""
            assert (r["score"], r["i_end"], r["j_end"]) == (want[0], want[3], want[4])
        else:
            assert r["status"] == 0 and _t(r) == want, (h, r)
    assert _same(res, _loop(engine, m, hq, hs, go, ge, local, limit=small))


# -- 5. routing per pair ---------------------------------------------------------------------------

def _scores(engine, m, go, ge, local):
    return m.single(engine, go, ge, local)


@pytest.mark.parametrize("go,ge,local", [(-11, -1, True), (-11, -11, False)])
def test_query_whose_profile_does_not_fit_lds(engine, golden, go, ge, local):
    """1600 letters are five sweeps: 25 letters x 1924 rows x 4 bytes do not fit 160 KiB of LDS.  Its hits
    are status 1, the other queries' hits in the same call are traced."""
    if "lds" not in _ROWS:
        subjects = [_seq(int(c), 7100 + i) for i, c in enumerate([80, 33, 150, 7, 90, 121])]
        _ROWS["lds"] = _Multi([_seq(100, 61), _seq(1600, 62), _seq(40, 63)], subjects, golden.blosum62)
    m = _ROWS["lds"]
    assert m.substsz * (5 * SWEEP + 4) * 4 > 160 * 1024
    hq = [q for s in range(6) for q in range(3)]
    hs = [s for s in range(6) for q in range(3)]
    want = _scores(engine, m, go, ge, local)
    before = engine.last_launch()
    res, info = _multi(engine, m, hq, hs, go, ge, local)
    assert engine.last_launch() == before  # the status 1 hits' score launches included
    assert (info["lane_hits"], info["unsupported"], info["lane_queries"], info["chunks"], info["launches"]) == (12, 6, 2, 1, 1), info
    for q, s, r in zip(hq, hs, res):
        assert (r["score"], r["i_end"], r["j_end"]) == tuple(want[q, s]), (q, s)
        if q == 1:
            assert r["status"] == 1 and r["cigar"] == ""
        else:
            assert r["status"] == 0 and _t(r) == _ref("lds", m, q, s, go, ge, local)
    assert _same(res, _loop(engine, m, hq, hs, go, ge, local))


def test_local_pair_past_the_key_bound(engine, golden):
    """30000 x min(100, C) does not fit a row's best key (2^18); 30000 x 5 does: the route is per pair."""
    sub = np.full((20, 20), -30000, np.int32)
    np.fill_diagonal(sub, 30000)
    subjects = [_seq(int(c), 2200 + i) for i, c in enumerate([90, 150, 120, 101, 97, 133, 6])]
    m = _Multi([_seq(5, 13), _seq(100, 14), _seq(8, 15)], subjects, sub)
    hq = [q for s in range(7) for q in range(3)]
    hs = [s for s in range(7) for q in range(3)]
    res, info = _multi(engine, m, hq, hs, -11, -1, True)
    # query 1 against the six long subjects: past the bound; against the 6-letter subject: 30000 x 6 fits
    assert (info["lane_hits"], info["unsupported"], info["lane_queries"]) == (15, 6, 3), info
    want = _scores(engine, m, -11, -1, True)
    for q, s, r in zip(hq, hs, res):
        assert (r["score"], r["i_end"], r["j_end"]) == tuple(want[q, s]), (q, s)
        assert r["status"] == (1 if q == 1 and s < 6 else 0), (q, s, r)
        if r["status"] == 0:
            assert _t(r) == _ref("big", m, q, s, -11, -1, True)
    assert _same(res, _loop(engine, m, hq, hs, -11, -1, True))
    res, info = _multi(engine, m, hq, hs, -11, -1, False)  # global: no key
    _counts(info, _expect(m, hq, hs))
    _check(m, res, hq, hs, "big", -11, -1, False)


# -- 6. buffer and tables --------------------------------------------------------------------------

def _raw(engine, m, hq, hs, go, ge, local, cap, limit=0, wgs=0, nhits=None, nq=None, nsubj=None, null=(), qoff=None, off=None):
    """gsa_align_db_multi_dev through the raw ABI: (status, results, buffer, cigar_need, info)."""
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
    st = gsa.lib().gsa_align_db_multi_dev(
        engine._h, arg("queries", m.q.data_ptr()), arg("q_off", qo.ctypes.data_as(i64p)), len(qo) - 1 if nq is None else nq,
        arg("db", m.db.data_ptr()), arg("db_off", of.ctypes.data_as(i64p)), len(of) - 1 if nsubj is None else nsubj,
        arg("hit_query", q.ctypes.data_as(i32p)), arg("hit_subject", s.ctypes.data_as(i32p)), n, arg("subst", m.sub.data_ptr()),
        m.substsz, go, ge, int(local), wgs, limit, arg("out", res), arg("cigar", buf), cap, ctypes.byref(need),
        ctypes.byref(info), ctypes.byref(ms), None)
    return st, res, buf, need.value, info


def test_cigar_buffer(engine, golden):
    """cigar_cap too small for the last two hits: those have status 2, the earlier ones are intact, and
    *cigar_need is the total of the full run."""
    m = _grid_pool(golden)
    hq, hs = [0, 3, 1, 3, 2, 0], [0, 5, 1, 7, 9, 12]
    go, ge, local = -11, -1, False
    st, full, buf, need, _ = _raw(engine, m, hq, hs, go, ge, local, 1 << 16)
    assert st == 0 and 0 < need <= 1 << 16
    strings = [buf.raw[r.cigar_off:r.cigar_off + r.cigar_len].decode() for r in full]
    for q, s, r, c in zip(hq, hs, full, strings):
        want = _ref("grid", m, q, s, go, ge, local)
        assert r.status == 0 and c == want[5] and buf.raw[r.cigar_off + r.cigar_len] == 0
    assert need == sum(len(c) + 1 for c in strings)
    assert [r.cigar_off for r in full] == list(np.cumsum([0] + [len(c) + 1 for c in strings[:-1]]))  # hit order
    cap = int(full[-2].cigar_off) + 1  # the fifth string needs more than its terminator
    assert len(strings[-2]) > 0 and len(strings[-1]) > 0
    st, res, buf2, need2, info = _raw(engine, m, hq, hs, go, ge, local, cap)
    assert st == 0 and need2 == need and info.lane_hits == len(hq) and info.chunks == 1
    assert [r.status for r in res] == [0, 0, 0, 0, 2, 2]
    for r, f, c in zip(res[:4], full[:4], strings[:4]):
        assert (r.cigar_off, r.cigar_len) == (f.cigar_off, f.cigar_len)
        assert buf2.raw[r.cigar_off:r.cigar_off + r.cigar_len + 1] == c.encode() + b"\0"
    for r, f in zip(res, full):
        assert (r.score, r.i_start, r.j_start, r.i_end, r.j_end) == (f.score, f.i_start, f.j_start, f.i_end, f.j_end)


def test_tables(engine, golden):
    """An asymmetric table (row = query letter), one with values outside int8, a 4-letter alphabet."""
    rng = np.random.default_rng(11)
    asym = rng.integers(-6, 12, size=(20, 20)).astype(np.int32)
    assert not np.array_equal(asym, asym.T)
    wide = np.full((20, 20), -200, np.int32)
    np.fill_diagonal(wide, 300)
    dna = np.full((4, 4), -3, np.int32)
    np.fill_diagonal(dna, 2)
    hq = [q for s in range(5) for q in range(3)]
    hs = [int(s) for s in np.random.default_rng(4).integers(0, 10, 15)]
    for name, sub, alphabet, (go, ge, local) in [("asym", asym, 20, (-11, -1, True)), ("wide", wide, 20, (-5, -2, False)),
                                                  ("dna", dna, 4, (-5, -2, True)), ("dna", dna, 4, (-4, -4, False))]:
        if name not in _ROWS:
            subjects = [_seq(int(c), 2100 + i, alphabet) for i, c in enumerate(np.random.default_rng(21).integers(1, 151, 10))]
            _ROWS[name] = _Multi([_seq(90, 13, alphabet), _seq(17, 14, alphabet), _seq(130, 15, alphabet)], subjects, sub)
        m = _ROWS[name]
        assert m.substsz == len(sub)
        res, info = _multi(engine, m, hq, hs, go, ge, local)
        _counts(info, _expect(m, hq, hs))
        _check(m, res, hq, hs, ("tab", name), go, ge, local)
        assert _same(res, _loop(engine, m, hq, hs, go, ge, local))


# -- 7. neighbours ---------------------------------------------------------------------------------

def test_neighbours_keep_their_record_and_their_results(engine, golden):
    """score_db_multi_dev, align_db_dev and score_db_dev right before and right after, over a query of
    two sweeps: they share context buffers with the multi call.  gsa_last_launch is left alone."""
    queries = [_seq(R, 900 + R) for R in (60, 500, 130)]
    subjects = [_seq(int(c), 950 + i) for i, c in enumerate([80, 200, 33, 150, 7, 260, 90, 121, 64])]
    m = _Multi(queries, subjects, golden.blosum62)
    go, ge, local = -11, -1, True
    hq, hs = [1, 0, 1, 2, 1, 0], [5, 1, 0, 3, 8, 5]

    def around():
        ranked, _ = m.run(engine, go, ge, local, top=3)
        al = _loop(engine, m, [1, 1], [5, 0], go, ge, local)
        return ranked["scores"].copy(), ranked["hits"].copy(), al, m.single(engine, go, ge, local)

    first = around()
    before = engine.last_launch()
    assert before["kind"] == "score_lanes", before
    res, info = _multi(engine, m, hq, hs, go, ge, local)
    assert engine.last_launch() == before
    _counts(info, _expect(m, hq, hs))
    assert info["launches"] == 2, info
    again = around()
    assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1])
    assert _same(first[2], again[2]) and np.array_equal(first[3], again[3])
    _check(m, res, hq, hs, "nb", go, ge, local)
    assert _t(first[2][0]) == _ref("nb", m, 1, 5, go, ge, local)
    res2, _ = _multi(engine, m, hq, hs, go, ge, local)
    assert _same(res, res2)


def test_scratch_is_counted_in_mem_stats(golden):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    m = _grid_pool(golden)
    hq, hs = _hit_list(5, 3)
    with gsa.Engine(0) as e:
        e.reset_mem_stats()
        _multi(e, m, hq, hs, -11, -1, True)
        info = e.last_align_db_multi_info()
        assert e.mem_stats()["glmem_peak_allocs"] >= info["code_bytes"] > 0


# -- 8. host forms ---------------------------------------------------------------------------------

def test_host_forms(engine, golden):
    """align_db_multi against the loop of align_db, an empty query and an empty subject among the pairs;
    search_db_multi against the loop of search_db, and that it made one alignment call, not three."""
    queries = [_seq(R, 1100 + R) for R in (120, 0, 45)]
    subjects = [_seq(int(c), 1200 + i) for i, c in enumerate(np.random.default_rng(8).integers(1, 200, 40))]
    subjects[4] = _seq(0, 1)
    hq, hs = [0, 2, 1, 0, 2, 2, 0], [3, 3, 5, 17, 30, 3, 4]
    strip = lambda rows: [{k: v for k, v in d.items() if k != "kernel_ms"} for d in rows]
    for go, ge, local in [(-11, -1, True), (-11, -11, False)]:
        a = engine.align_db_multi(queries, subjects, hq, hs, golden.blosum62, go, ge, local)
        info = engine.last_align_db_multi_info()
        assert (info["lane_hits"], info["unsupported"], info["lane_queries"]) == (5, 0, 2), info
        loop = [engine.align_db(queries[q], subjects, [s], golden.blosum62, go, ge, local)[0] for q, s in zip(hq, hs)]
        assert strip(a) == strip(loop) and all(r["status"] == 0 for r in a)
        # three queries and 39 subjects, all with letters: every one of the 12 hits takes a kernel
        three, full = [queries[0], _seq(7, 1107), queries[2]], [x for x in subjects if len(x) > 1]
        multi = engine.search_db_multi(three, full, golden.blosum62, go, ge, local, top=4)
        info = engine.last_align_db_multi_info()
        assert info["lane_hits"] + info["unsupported"] == 12 and info["chunks"] == 1, info  # one call, not three
        want = [engine.search_db(q, full, golden.blosum62, go, ge, local, top=4) for q in three]
        assert [[(s, strip([d])[0]) for s, d in row] for row in multi] == [[(s, strip([d])[0]) for s, d in row] for row in want]
        assert [len(row) for row in multi] == [4, 4, 4]
    assert engine.align_db_multi(queries, subjects, [], [], golden.blosum62, -11, -1, False) == []
    info = engine.last_align_db_multi_info()
    assert info["lane_hits"] == 0 and info["chunks"] == 0 and info["launches"] == 0 and info["tasks"] == 0


# -- 9. invalid input ------------------------------------------------------------------------------

def test_invalid_input(engine, golden):
    m = _Multi([_seq(60, 4), _seq(20, 5), _seq(33, 6)], [_seq(int(c), 1300 + c) for c in (5, 80, 41, 17, 66)], golden.blosum62)
    hq, hs = [0, 2, 1], [1, 4, 0]
    m.single(engine, -11, -1, False)  # a launch record to be left alone
    before = engine.last_launch()

    def good():
        res, info = _multi(engine, m, hq, hs, -11, -1, False)
        _counts(info, _expect(m, hq, hs))
        _check(m, res, hq, hs, "inv", -11, -1, False)

    def bad(go=-11, ge=-1, q=hq, s=hs, **kw):
        st = _raw(engine, m, q, s, go, ge, False, kw.pop("cap", 4096), **kw)[0]
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
        _multi(engine, m, [0, 1], [0], -11, -1, False)
    assert ei.value.stat == gsa.NwStat.errorInvalidValue
    for substsz in (0, 33):
        with pytest.raises(gsa.NwError) as ei:
            engine.align_db_multi_dev(m.q.data_ptr(), m.qoff, m.db.data_ptr(), m.off, hq, hs, m.sub.data_ptr(), substsz, -11, -1)
        assert ei.value.stat == gsa.NwStat.errorInvalidValue, substsz
    # score_ranges' rule: the longest query against the longest subject, whether or not that pair is a hit
    wide = np.full((20, 20), -(1 << 20), np.int32)
    big = _Multi([_seq(60, 4), _seq(3000, 5)], [_seq(5, 7), _seq(3000, 8)], wide)
    st = _raw(engine, big, [0], [0], -11, -1, False, 4096)[0]
    assert st == gsa.NwStat.errorInvalidValue
    good()
