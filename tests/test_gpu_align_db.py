"""Alignments of database hits (gsa_align_db_dev: the lane kernel's fill with 4-bit move codes and the
walk over them, nw_lanes_trace.hip) against tests/_align_oracle.py, per hit and exactly: score, start
cell, end cell and CIGAR.  Every case asserts status 0 and, from gsa_align_db_info, how many hits were
traced on the device and in how many chunks, so that no case passes through another route.  A lane
holds K = 24 query rows, a hit sits on 16 lanes, one sweep covers 384 rows, a wave task is 4 hits."""
import ctypes

import numpy as np
import pytest

import gpuseqalign_amd as gsa
from tests import _align_oracle as ao
from tests.test_gpu_score import MODES
from tests.test_gpu_score_db import _Db, _many, _mixed_subjects, _seq

pytestmark = pytest.mark.gpu

K = 24            # query rows per lane
SWEEP = 16 * K    # query rows per sweep
TASK = 4          # hits per wave task
AFFINE4 = [(-11, -1, False), (-5, -2, False), (-11, -1, True), (-5, -2, True)]
FIELDS = ("score", "i_start", "j_start", "i_end", "j_end", "cigar")
_REF = {}


def _ref(key, Y, X, sub, go, ge, local):
    """The oracle's alignment, computed once per (pair, table, mode) and shared by the cases."""
    k = (key, go, ge, local)
    if k not in _REF:
        _REF[k] = ao.align(Y, X, sub, go, ge, local)
    return _REF[k]


def _t(r):
    return tuple(r[f] for f in FIELDS)


def _code_bytes(R, C):
    """Move codes of one hit: 4 bits per cell of sweeps x 384 rows x (C + 1) columns."""
    return -(-R // SWEEP) * SWEEP * (C + 1) // 2


def _align(engine, d, hits, go, ge, local, limit=0):
    return engine.align_db_dev(d.q.data_ptr(), d.q.numel(), d.db.data_ptr(), d.off, hits, d.sub.data_ptr(), d.substsz,
                               go, ge, local, scratch_limit=limit)


def _traced(engine, d, hits, chunks=None):
    """gsa_align_db_info of the last call: every hit with letters traced on the device, in one chunk
    (or `chunks`), four hits to a task."""
    n = sum(len(d.subjects[s]) > 1 for s in hits)
    info = engine.last_align_db_info()
    assert info["lane_hits"] == n and info["unsupported"] == 0, info
    if chunks is None:
        assert info["chunks"] == (1 if n else 0) and info["tasks"] == -(-n // TASK), info
    else:
        assert info["chunks"] == chunks, info
    return info


def _check(d, res, hits, key, go, ge, local):
    assert len(res) == len(hits)
    for s, r in zip(hits, res):
        want = _ref((key, s), d.query, d.subjects[s], d.subm, go, ge, local)
        assert r["status"] == 0, (key, s, r)
        assert _t(r) == want, (key, s, len(d.query) - 1, len(d.subjects[s]) - 1, _t(r), want)


_WAVE = {}
WAVE_EMPTY = 35  # _mixed_subjects(70, .): the subject with no letters
HIT_LISTS = {"1": [0], "3": [WAVE_EMPTY, 1, 0], "4": [0, 1, 2, 3], "5": [40, 3, 40, 1, 0], "65": list(range(65))}


def _wave_db(golden):
    if "db" not in _WAVE:
        _WAVE["db"] = _Db(_seq(200, 77), _mixed_subjects(70, 70), golden.blosum62)
        lens = [len(x) - 1 for x in _WAVE["db"].subjects]
        assert lens[0] == 300 and lens[1] == 1 and lens[WAVE_EMPTY] == 0
    return _WAVE["db"]


@pytest.mark.parametrize("hits", sorted(HIT_LISTS), ids=lambda k: "hits" + k)
@pytest.mark.parametrize("go,ge,local", MODES)
def test_wave_and_task_edges(engine, golden, go, ge, local, hits):
    """1, 3, 4, 5 and 65 hits (a task is 4); a subject of one letter beside one of 300; a list out of
    order that names a subject twice; lists that name the subject with no letters."""
    d = _wave_db(golden)
    res = _align(engine, d, HIT_LISTS[hits], go, ge, local)
    _traced(engine, d, HIT_LISTS[hits])
    _check(d, res, HIT_LISTS[hits], "wave", go, ge, local)


_ROWS = {}


@pytest.mark.parametrize("go,ge,local", MODES)
def test_row_lane_and_sweep_edges(engine, golden, go, ge, local):
    """The last query row on the first and last register row of a lane, on either side of the hand-off
    between two lanes and of the boundary between two sweeps: the code address changes at each."""
    for R in [1, K - 1, K, K + 1, 2 * K + 1, 300, SWEEP - 1, SWEEP, SWEEP + 1, 2 * SWEEP + 1]:
        if R not in _ROWS:
            _ROWS[R] = _Db(_seq(R, 500 + R), _many(12, R, 1, 120), golden.blosum62)
        d = _ROWS[R]
        hits = list(range(12))
        res = _align(engine, d, hits, go, ge, local)
        _traced(engine, d, hits)
        _check(d, res, hits, ("rows", R), go, ge, local)


def _hdr(a):
    return np.concatenate([[0], a]).astype(np.int32)


# (query letters, first and last row of the block, the boundary it crosses or None, seed)
PLANTS = [(100, 30, 30, None, 11), (100, 20, 49, K, 12), (420, 370, 399, SWEEP, 13)]


def _plant(R, a, b, seed, inserted):
    """The query, and a subject that is the query with rows a..b removed, or with b - a + 1 random
    letters inserted behind row a - 1."""
    q = _seq(R, seed)
    if not inserted:
        return q, _hdr(np.concatenate([q[1:a], q[b + 1:]]))
    block = _seq(b - a + 1, seed + 100)[1:]
    return q, _hdr(np.concatenate([q[1:a], block, q[a:]]))


def _gap_run(cigar, i0, j0, op):
    """(count, first row, first column) of the only run of `op` in a CIGAR; it must be the only gap."""
    i, j, found = i0, j0, []
    for count, o in ao.runs(cigar):
        if o == op:
            found.append((count, i + 1, j + 1))
        else:
            assert o in "=X", "another gap in %s" % cigar
        i += count if o != "D" else 0
        j += count if o != "I" else 0
    assert len(found) == 1, cigar
    return found[0]


@pytest.mark.parametrize("inserted", [False, True], ids=["removed", "inserted"])
@pytest.mark.parametrize("go,ge,local", AFFINE4)
def test_gaps_across_hand_offs(engine, golden, go, ge, local, inserted):
    """A gap of 30 rows across the DPP hand-off between two lanes (rows 24 / 25) and across the
    boundary array between two sweeps (rows 384 / 385): the F-extended bit of the rows on either side;
    the same blocks inserted in the subject run E along the columns."""
    for R, a, b, edge, seed in PLANTS:
        q, x = _plant(R, a, b, seed, inserted)
        d = _Db(q, _many(3, seed, 1, 90) + [x], golden.blosum62)
        key = ("plant", R, a, inserted)
        want = _ref((key, 3), q, x, d.subm, go, ge, local)
        count, row, col = _gap_run(want[5], want[1], want[2], "D" if inserted else "I")
        assert count == b - a + 1, "the oracle's alignment does not hold the planted block: %s" % want[5]
        if edge is not None:
            first = col if inserted else row
            assert first <= edge < first + count - 1, (first, count, edge)  # rows edge and edge + 1 are in it
        hits = [3, 0, 1, 2]
        res = _align(engine, d, hits, go, ge, local)
        _traced(engine, d, hits)
        _check(d, res, hits, key, go, ge, local)


def _source_ties(path, mats, Y, X, sub, go, ge, local):
    """Cells of the oracle's path (state H) where two sources of H hold the same value."""
    H, E, F = mats
    n = 0
    for i, j, state in path:
        if state != "H" or i == 0 or j == 0:
            continue
        h = int(H[i, j])
        srcs = [int(H[i - 1, j - 1]) + int(sub[Y[i], X[j]]) == h, int(F[i, j]) == h, int(E[i, j]) == h]
        n += sum(srcs) + (1 if local and h == 0 else 0) >= 2
    return n


@pytest.mark.parametrize("go,ge,local", [(-11, -11, False), (-11, -1, False), (-11, -11, True), (-11, -1, True)])
def test_ties(engine, golden, go, ge, local):
    """Homopolymers: every placement of the gap scores the same, so the order diagonal, F, E decides
    the path.  Global: the oracle's path must hold a cell where two sources of H tie.  Local with these
    gap costs no such cell can exist on a homopolymer's path (a gap next to a match always loses), the
    tie there is between the maximal cells of the last column, resolved to the first in row-major
    order: the case asserts that tie instead.  An all-mismatch pair in local mode: score 0 at (0, 0)."""
    n = int(round(np.sqrt(golden.blosum62.size)))
    sub = np.array(golden.blosum62, dtype=np.int32).reshape(n, n)
    A = lambda k: _hdr(np.full(k, 3, np.int32))
    for c, (Y, X) in enumerate([(A(5), A(3)), (A(3), A(5)), (A(40), A(30))]):
        d = _Db(Y, _many(2, 60 + c, 1, 50) + [X], golden.blosum62)
        want = ao.align(Y, X, sub, go, ge, local, want_path=True)
        if local:
            H = want[7][0]
            assert (H == H.max()).sum() >= 2, "one maximal cell only"
        else:
            assert _source_ties(want[6], want[7], Y, X, sub, go, ge, local) >= 1, "no tie on the path"
        _REF[((("ties", c), 2), go, ge, local)] = want[:6]
        res = _align(engine, d, [2, 0, 1], go, ge, local)
        _traced(engine, d, [2, 0, 1])
        _check(d, res, [2, 0, 1], ("ties", c), go, ge, local)
    if local:
        flat = np.full((n, n), -4, np.int32)
        np.fill_diagonal(flat, 5)
        d = _Db(_hdr(np.full(40, 3, np.int32)), [_hdr(np.full(50, 7, np.int32))], flat)
        res = _align(engine, d, [0], go, ge, True)
        _traced(engine, d, [0])
        assert _t(res[0]) == (0, 0, 0, 0, 0, "") and res[0]["status"] == 0


def test_chunking(engine, golden):
    """A scratch limit that forces at least three chunks gives the default run's results; a limit below
    the largest hit's own need leaves that hit alone with status 1, its score and end cell intact."""
    d = _wave_db(golden)
    hits = list(range(65))
    go, ge, local = -11, -1, True
    R = len(d.query) - 1
    need = {s: _code_bytes(R, len(d.subjects[s]) - 1) for s in hits if len(d.subjects[s]) > 1}
    total, largest = sum(need.values()), max(need.values())
    limit = total // 3
    assert limit >= largest and 2 * limit < total  # every hit fits a chunk, and two chunks cannot hold all
    base = _align(engine, d, hits, go, ge, local)
    _traced(engine, d, hits)
    res = _align(engine, d, hits, go, ge, local, limit=limit)
    info = _traced(engine, d, hits, chunks=engine.last_align_db_info()["chunks"])
    assert info["chunks"] >= 3 and 0 < info["code_bytes"] <= limit, (info, limit)
    assert [_t(r) for r in res] == [_t(r) for r in base]
    _check(d, res, hits, "wave", go, ge, local)

    small = largest - 1
    out = [s for s in hits if need.get(s, 0) > small]
    assert len(out) == 1, "more than one hit of the largest size"
    res = _align(engine, d, hits, go, ge, local, limit=small)
    info = engine.last_align_db_info()
    assert info["unsupported"] == 1 and info["lane_hits"] == len(need) - 1 and info["code_bytes"] <= small, info
    for s, r in zip(hits, res):
        want = _ref(("wave", s), d.query, d.subjects[s], d.subm, go, ge, local)
        if s == out[0]:
            assert r["status"] == 1 and r["cigar"] == ""
            assert (r["score"], r["i_end"], r["j_end"]) == (want[0], want[3], want[4])
        else:
            assert r["status"] == 0 and _t(r) == want, (s, r)


def _raw(engine, d, hits, go, ge, local, cap, limit=0, nhits=None, null_hits=False, null_out=False):
    """gsa_align_db_dev through the raw ABI: (status, results, buffer, cigar_need, info)."""
    i64p = ctypes.POINTER(ctypes.c_int64)
    off = np.ascontiguousarray(d.off, dtype=np.int64)
    hit = np.ascontiguousarray(hits, dtype=np.int32)
    n = len(hit) if nhits is None else nhits
    res = (gsa.AlignDbResult * max(len(hit), 1))()
    buf = ctypes.create_string_buffer(max(cap, 1))
    need, info, ms = ctypes.c_int64(-1), gsa.AlignDbInfo(), ctypes.c_float(0.0)
    st = gsa.lib().gsa_align_db_dev(
        engine._h, d.q.data_ptr(), d.q.numel(), d.db.data_ptr(), off.ctypes.data_as(i64p), len(off) - 1,
        None if null_hits else hit.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), n, d.sub.data_ptr(), d.substsz, go,
        ge, int(local), limit, None if null_out else res, buf, cap, ctypes.byref(need), ctypes.byref(info),
        ctypes.byref(ms), None)
    return st, res, buf, need.value, info


def test_cigar_buffer(engine, golden):
    """cigar_cap too small for the last two hits: those have status 2, the earlier ones are intact, and
    *cigar_need is the total of the full run."""
    d = _wave_db(golden)
    hits = [0, 5, 1, 7, 9, 12]
    go, ge, local = -11, -1, False
    st, full, buf, need, _ = _raw(engine, d, hits, go, ge, local, 1 << 16)
    assert st == 0 and 0 < need <= 1 << 16
    strings = [buf.raw[r.cigar_off:r.cigar_off + r.cigar_len].decode() for r in full]
    for s, r, c in zip(hits, full, strings):
        want = _ref(("wave", s), d.query, d.subjects[s], d.subm, go, ge, local)
        assert r.status == 0 and c == want[5] and buf.raw[r.cigar_off + r.cigar_len] == 0
    assert need == sum(len(c) + 1 for c in strings)
    cap = int(full[-2].cigar_off) + 1  # the fifth string needs more than its terminator
    assert len(strings[-2]) > 0 and len(strings[-1]) > 0
    st, res, buf2, need2, info = _raw(engine, d, hits, go, ge, local, cap)
    assert st == 0 and need2 == need and info.lane_hits == len(hits) and info.chunks == 1
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
    hits = list(range(10))
    for name, sub, alphabet, (go, ge, local) in [("asym", asym, 20, (-11, -1, True)), ("wide", wide, 20, (-5, -2, False)),
                                                  ("dna", dna, 4, (-5, -2, True)), ("dna", dna, 4, (-4, -4, False))]:
        d = _Db(_seq(90, 13, alphabet), [_seq(int(c), 2100 + i, alphabet) for i, c in
                                         enumerate(np.random.default_rng(21).integers(1, 151, 10))], sub)
        assert d.substsz == len(sub)
        res = _align(engine, d, hits, go, ge, local)
        _traced(engine, d, hits)
        _check(d, res, hits, ("tab", name), go, ge, local)


@pytest.mark.parametrize("go,ge,local", MODES)
def test_consistent_with_the_search(engine, golden, go, ge, local):
    """score, i_end and j_end of every hit are score_db_dev's entry for that subject."""
    d = _wave_db(golden)
    hits = list(range(70))
    scores = d.run(engine, go, ge, local)
    res = _align(engine, d, hits, go, ge, local)
    _traced(engine, d, hits)
    for s, r in zip(hits, res):
        assert r["status"] == 0
        assert (r["score"], r["i_end"], r["j_end"]) == (scores[s]["score"], scores[s]["i_end"], scores[s]["j_end"]), s


@pytest.mark.parametrize("go,ge,local", [(-11, -1, True), (-11, -11, False), (-11, -1, False)])
def test_back_to_back_calls(engine, golden, go, ge, local):
    """Long hits, then short ones, on one context and a query of two sweeps: stale codes, boundary rows
    or task state would show in the second call; a search between two such calls is undisturbed."""
    import oracle
    q = _seq(500, 31)
    long_ = _Db(q, _many(8, 7, 600, 900), golden.blosum62)
    short = _Db(q, _many(20, 8, 1, 60), golden.blosum62)
    r1 = _align(engine, long_, list(range(8)), go, ge, local)
    _traced(engine, long_, list(range(8)))
    r2 = _align(engine, short, list(range(20)), go, ge, local)
    _traced(engine, short, list(range(20)))
    scores = short.run(engine, go, ge, local)
    r3 = _align(engine, short, list(range(19, -1, -1)), go, ge, local)
    _traced(engine, short, list(range(20)))
    _check(long_, r1, list(range(8)), "b2b-long", go, ge, local)
    _check(short, r2, list(range(20)), "b2b-short", go, ge, local)
    _check(short, r3, list(range(19, -1, -1)), "b2b-short", go, ge, local)
    for s, r in enumerate(scores):
        assert (r["score"], r["i_end"], r["j_end"]) == tuple(oracle.score_ag(q, short.subjects[s], short.subm, go, ge, local))


def test_host_forms(engine, golden):
    d = _wave_db(golden)
    for go, ge, local in [(-11, -1, True), (-11, -11, False)]:
        hits = [4, 0, WAVE_EMPTY, 9]
        a = engine.align_db(d.query, d.subjects, hits, golden.blosum62, go, ge, local)
        _traced(engine, d, hits)
        b = _align(engine, d, hits, go, ge, local)
        assert [_t(r) for r in a] == [_t(r) for r in b] and all(r["status"] == 0 for r in a)
        _check(d, a, hits, "wave", go, ge, local)
        found = engine.search_db(d.query, d.subjects, golden.blosum62, go, ge, local, top=5)
        _traced(engine, d, [s for s, _ in found])
        ref = {s: _ref(("wave", s), d.query, d.subjects[s], d.subm, go, ge, local) for s in range(70)}
        best = sorted(range(70), key=lambda s: (-ref[s][0], s))[:5]
        assert [s for s, _ in found] == best
        for s, r in found:
            assert r["status"] == 0 and _t(r) == ref[s]
    assert _align(engine, d, [], -11, -1, False) == []
    info = engine.last_align_db_info()
    assert info["lane_hits"] == 0 and info["chunks"] == 0 and info["tasks"] == 0


def test_last_launch_record_is_left_alone(engine, golden):
    d = _wave_db(golden)
    d.run(engine, -11, -1, True)
    before = engine.last_launch()
    _align(engine, d, [0, 1, 2], -11, -11, False)
    assert engine.last_launch() == before


def test_outside_the_trace_kernels_limits(engine, golden):
    """A local score bound of 2^18 or more (30000 x 100) does not fit a row's best key: status 1, score
    and end cell from the score path, the launch record still the caller's.  Global has no key and the
    values stay inside the fill's range: traced."""
    sub = np.full((20, 20), -30000, np.int32)
    np.fill_diagonal(sub, 30000)
    d = _Db(_seq(100, 13), _many(6, 22, 90, 150), sub)
    hits = list(range(6))
    _wave_db(golden).run(engine, -11, -1, True)
    before = engine.last_launch()
    res = _align(engine, d, hits, -11, -1, True)
    info = engine.last_align_db_info()
    assert (info["lane_hits"], info["unsupported"], info["chunks"], info["tasks"]) == (0, 6, 0, 0), info
    assert engine.last_launch() == before
    for s, r in zip(hits, res):
        want = _ref(("big", s), d.query, d.subjects[s], d.subm, -11, -1, True)
        assert r["status"] == 1 and r["cigar"] == ""
        assert (r["score"], r["i_end"], r["j_end"]) == (want[0], want[3], want[4])
    res = _align(engine, d, hits, -11, -1, False)
    _traced(engine, d, hits)
    _check(d, res, hits, "big", -11, -1, False)


def test_scratch_is_counted_in_mem_stats(engine, golden):
    d = _wave_db(golden)
    _align(engine, d, list(range(65)), -11, -1, True)
    info = engine.last_align_db_info()
    assert engine.mem_stats()["glmem_peak_allocs"] >= info["code_bytes"] > 0


def test_invalid_input(engine, golden):
    d = _Db(_seq(60, 4), _many(9, 6, 1, 80), golden.blosum62)
    hits = [0, 3, 8]

    def good():
        res = _align(engine, d, hits, -11, -1, False)
        _traced(engine, d, hits)
        _check(d, res, hits, "inv", -11, -1, False)

    def bad(call):
        with pytest.raises(gsa.NwError) as ei:
            call()
        assert ei.value.stat == gsa.NwStat.errorInvalidValue
        good()

    def raw(**kw):
        args = dict(hits=hits, go=-11, ge=-1, local=False, cap=4096)
        args.update(kw)
        engine._check(_raw(engine, d, **args)[0], "gsa_align_db_dev")

    class Off:
        """d with other offsets."""
        def __init__(self, off):
            self.q, self.db, self.sub, self.substsz, self.off = d.q, d.db, d.sub, d.substsz, off

    equal, dec = d.off.copy(), d.off.copy()
    equal[4] = equal[3]
    dec[4] = dec[3] - 1
    good()
    bad(lambda: _align(engine, Off(equal), hits, -11, -1, False))       # what gsa_score_db_dev rejects
    bad(lambda: _align(engine, Off(dec), hits, -11, -1, False))
    bad(lambda: _align(engine, Off(d.off[:1]), [], -11, -1, False))     # nsubj = 0
    bad(lambda: _align(engine, d, hits, -1, -11, False))                # go > ge
    bad(lambda: _align(engine, d, hits, -11, 1, False))                 # ge > 0
    bad(lambda: _align(engine, d, [0, 9], -11, -1, False))              # a hit outside 0 ... nsubj - 1
    bad(lambda: _align(engine, d, [-1], -11, -1, False))
    bad(lambda: _align(engine, d, hits, -11, -1, False, limit=-1))      # negative scratch_limit
    bad(lambda: raw(null_hits=True))                                    # null hits with nhits > 0
    bad(lambda: raw(nhits=-1))
    bad(lambda: raw(cap=-1))
    bad(lambda: raw(null_out=True))
