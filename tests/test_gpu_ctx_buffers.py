"""The context's grow-only buffers (csrc/gsa_ctx.h: Buf, reserve, StageRing) under growth: every entry
point family on a fresh engine at a small shape, one several times larger and the small one again;
the pinned staging rings wrapped with copies still in flight; glmem_peak_allocs over that growth; and
contexts created and destroyed in a row.  Every output exactly against the oracles the other GPU
tests use (oracle.fill_full, oracle.sparse_headers, oracle.trace_sparse, oracle.score_ag,
tests/_align_oracle.py).  A fresh gsa.Engine(0) per test, not the session's, so that growth happens."""
import numpy as np
import pytest

import gpuseqalign_amd as gsa
import oracle
from gpuseqalign_amd import formats as F
from tests import _align_oracle as ao
from tests._data import random_pair

pytestmark = pytest.mark.gpu

SMALL, LARGE = "small", "large"
GROWTH = (SMALL, LARGE, SMALL)
PAIR = {SMALL: (300, 250), LARGE: (3000, 2500)}
TRIPLE = {SMALL: [(300, 250), (250, 300), (120, 280)], LARGE: [(3000, 2500), (2500, 3000), (1200, 2800)]}
G = -11
_REF = {}


def _once(key, fn):
    """A reference computed once and shared by the tests."""
    if key not in _REF:
        _REF[key] = fn()
    return _REF[key]


@pytest.fixture
def fresh():
    """make(): a new engine, closed after the test."""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    made = []

    def make():
        made.append(gsa.Engine(0))
        return made[-1]

    yield make
    for e in made:
        e.close()


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to("cuda:0")


def _empty(n):
    import torch
    return torch.full((int(n),), -7, dtype=torch.int32, device="cuda:0")


def _pair(R, C):
    return random_pair(R, C, 11 * R + C)


def _headers(R, C, tBx):
    Y, X = _pair(R, C)
    return _once(("hdr", R, C, tBx), lambda: oracle.sparse_headers(Y, X, _SUB[0], G, gsa.sparse_tile_by(), tBx))


def _matrix(R, C):
    Y, X = _pair(R, C)
    return _once(("full", R, C), lambda: oracle.fill_full(Y, X, _SUB[0], G)[0])


_SUB = []  # the table (golden.blosum62), set by the `sub` fixture


@pytest.fixture
def sub(golden):
    if not _SUB:
        _SUB.append(golden.blosum62)
    return golden.blosum62


def _substsz(sub):
    return int(round(np.sqrt(np.asarray(sub).size)))


# -- one call of each family at one size, checked -----------------------------------------------

def _sparse_launch(e, sub, R, C, tBx, stream=None):
    """fill_sparse_dev enqueued; (check, tensors kept alive)."""
    Y, X = _pair(R, C)
    geom = gsa.sparse_geometry(len(Y), len(X), tBx)
    y, x, s = _dev(Y), _dev(X), _dev(sub)
    hr, hc = _empty(geom.hrowElems), _empty(geom.hcolElems)
    e.fill_sparse_dev(y.data_ptr(), len(Y), x.data_ptr(), len(X), s.data_ptr(), _substsz(sub), G, tBx, hr.data_ptr(),
                      hc.data_ptr(), stream)
    return (y, x, s, hr, hc), geom


def run_fill_sparse(e, sub, size):
    R, C = PAIR[size]
    (_, _, _, hr, hc), _ = _sparse_launch(e, sub, R, C, 64)
    e.sync()
    assert e.last_launch()["kind"] == "sparse_krow"
    want = _headers(R, C, 64)
    assert np.array_equal(hr.cpu().numpy(), want[0]) and np.array_equal(hc.cpu().numpy(), want[1]), (size, R, C)


def run_fill_full(e, sub, size):
    """A single pair: the fused two-pass fill."""
    R, C = PAIR[size]
    Y, X = _pair(R, C)
    y, x, s = _dev(Y), _dev(X), _dev(sub)
    out = _empty(len(Y) * len(X))
    e.fill_full_dev(y.data_ptr(), len(Y), x.data_ptr(), len(X), s.data_ptr(), _substsz(sub), G, out.data_ptr())
    e.sync()
    assert e.last_launch()["kind"] == "full_fused"
    assert np.array_equal(out.cpu().numpy().reshape(len(Y), len(X)), _matrix(R, C)), (size, R, C)


def _full_batch_launch(e, sub, shapes, stream=None):
    pairs = [_pair(R, C) for R, C in shapes]
    s = _dev(sub)
    ins = [(_dev(Y), _dev(X)) for Y, X in pairs]
    outs = [_empty(len(Y) * len(X)) for Y, X in pairs]
    e.fill_batch_dev([(y.data_ptr(), y.numel(), x.data_ptr(), x.numel(), o.data_ptr()) for (y, x), o in zip(ins, outs)],
                     s.data_ptr(), _substsz(sub), G, mode="full", stream=stream)
    return (s, ins), outs


def _full_batch_check(shapes, outs, what):
    for (R, C), o in zip(shapes, outs):
        assert np.array_equal(o.cpu().numpy().reshape(R + 1, C + 1), _matrix(R, C)), (what, R, C)


def run_fill_full_batch(e, sub, size):
    """Three pairs: the two-pass fill in two launches, its expansion scratch and staging."""
    keep, outs = _full_batch_launch(e, sub, TRIPLE[size])
    e.sync()
    assert e.last_launch()["kind"] == "full_two_launch"
    _full_batch_check(TRIPLE[size], outs, size)


def _run_score(e, sub, size, knob, kind, both_ends=0):
    R, C = PAIR[size]
    Y, X = _pair(R, C)
    y, x, s = _dev(Y), _dev(X), _dev(sub)
    if knob:
        e.set_knob(*knob)
    for go, ge, local in [(-11, -1, False), (-11, -11, True)]:
        r = e.score_dev(y.data_ptr(), len(Y), x.data_ptr(), len(X), s.data_ptr(), _substsz(sub), go, ge, local)
        ll = e.last_launch()
        assert ll["kind"] == kind, ll
        if not local:  # (a local pair may come back from both ends to one direction)
            assert ll["both_ends"] == both_ends, ll
        want = _once(("score", R, C, go, ge, local), lambda: oracle.score_ag(Y, X, sub, go, ge, local))
        assert (r["score"], r["i_end"], r["j_end"]) == want, (size, go, ge, local)


def run_score(e, sub, size):
    _run_score(e, sub, size, None, "score_krow")


def run_score_both_ends(e, sub, size):
    """GSA_SCORE_BIDI=2: from both ends at any size (the tap rows and reversed sequences' buffer)."""
    _run_score(e, sub, size, ("GSA_SCORE_BIDI", "2"), "score_krow", both_ends=1)


def run_score_scan(e, sub, size):
    """GSA_SCORE_SCAN=1: the row scan and its boundary rows."""
    _run_score(e, sub, size, ("GSA_SCORE_SCAN", "1"), "score_scan")


def run_score_batch(e, sub, size):
    shapes = TRIPLE[size]
    pairs = [_pair(R, C) for R, C in shapes]
    s = _dev(sub)
    ins = [(_dev(Y), _dev(X)) for Y, X in pairs]
    ptrs = [(y.data_ptr(), y.numel(), x.data_ptr(), x.numel()) for y, x in ins]
    for go, ge, local in [(-11, -1, False), (-11, -11, True)]:
        res = e.score_batch_dev(ptrs, s.data_ptr(), _substsz(sub), go, ge, local)
        assert e.last_launch()["kind"] == "score_krow" and e.last_launch()["npairs"] == 3
        for (R, C), (Y, X), r in zip(shapes, pairs, res):
            want = _once(("score", R, C, go, ge, local), lambda: oracle.score_ag(Y, X, sub, go, ge, local))
            assert (r["score"], r["i_end"], r["j_end"]) == want, (size, R, C, go, ge, local)


def _sweep_rows(e, sub):
    """Query rows one sweep of the database lane kernel covers (score_db_impl: passes = ceil(R /
    kDbLanesPassRows), 16 lanes of gsa_last_launch's k rows each); a longer query needs the
    boundary-row buffer."""
    if "sweep" not in _REF:
        q, x, s = _dev(F.synthetic_seq(5, 1)), _dev(F.synthetic_seq(7, 2)), _dev(sub)
        e.score_db_dev(q.data_ptr(), q.numel(), x.data_ptr(), [0, x.numel()], s.data_ptr(), _substsz(sub), -11, -1, False)
        ll = e.last_launch()
        assert ll["kind"] == "score_lanes", ll
        _REF["sweep"] = 16 * ll["k"]
    return _REF["sweep"]


def run_db(e, sub, size):
    """score_db_dev and align_db_dev: the small query fits one sweep (no boundary rows), the large one
    takes three."""
    sweep = _sweep_rows(e, sub)
    R = {SMALL: sweep - 84, LARGE: 2 * sweep + 5}[size]
    n, lo, hi = {SMALL: (9, 1, 80), LARGE: (150, 200, 700)}[size]
    rng = np.random.default_rng(R)
    query = F.synthetic_seq(R, 900 + R)
    subjects = [F.synthetic_seq(int(c), 1000 * R + i) for i, c in enumerate(rng.integers(lo, hi + 1, n))]
    q, db, s = _dev(query), _dev(np.concatenate(subjects)), _dev(sub)
    off = np.concatenate([[0], np.cumsum([len(x) for x in subjects])]).astype(np.int64)
    hits = list(range(0, n, max(1, n // 6)))
    for go, ge, local in [(-11, -1, False), (-11, -11, True)]:
        res = e.score_db_dev(q.data_ptr(), q.numel(), db.data_ptr(), off, s.data_ptr(), _substsz(sub), go, ge, local)
        ll = e.last_launch()
        assert ll["kind"] == "score_lanes" and ll["npairs"] == n, ll
        for k, (X, r) in enumerate(zip(subjects, res)):
            want = _once(("db", R, k, go, ge, local), lambda: oracle.score_ag(query, X, sub, go, ge, local))
            assert (r["score"], r["i_end"], r["j_end"]) == want, (size, k, go, ge, local)
        al = e.align_db_dev(q.data_ptr(), q.numel(), db.data_ptr(), off, hits, s.data_ptr(), _substsz(sub), go, ge, local)
        info = e.last_align_db_info()
        assert info["lane_hits"] == len(hits) and info["unsupported"] == 0 and info["chunks"] == 1, info
        for h, r in zip(hits, al):
            want = _once(("adb", R, h, go, ge, local), lambda: ao.align(query, subjects[h], sub, go, ge, local))
            assert r["status"] == 0
            assert tuple(r[f] for f in ("score", "i_start", "j_start", "i_end", "j_end", "cigar")) == want, (size, h)


TRACE_BX = 1024  # a tile too wide for its move codes to sit in LDS (dirs_lds false): they stay in global memory


def run_trace_sparse(e, sub, size):
    R, C = PAIR[size]
    Y, X = _pair(R, C)
    (y, x, s, hr, hc), geom = _sparse_launch(e, sub, R, C, TRACE_BX)
    e.sync()
    got = e.trace_sparse_dev(y.data_ptr(), len(Y), x.data_ptr(), len(X), s.data_ptr(), _substsz(sub), G, geom,
                             hr.data_ptr(), hc.data_ptr())
    ll = e.last_launch()
    assert ll["kind"] == "trace_sparse", ll
    h = _headers(R, C, TRACE_BX)
    want = _once(("trace", R, C), lambda: oracle.trace_sparse(h[0], h[1], h[2], h[3], gsa.sparse_tile_by(), TRACE_BX,
                                                              Y, X, sub, G))
    assert got == want, (size, R, C)


def _run_align_sparse(e, sub, size, overlap):
    R, C = PAIR[size]
    Y, X = _pair(R, C)
    r = e.align_sparse(Y, X, sub, G, tileBx=64, overlap=overlap)
    want = _headers(R, C, 64)
    assert np.array_equal(r.hrow, want[0]) and np.array_equal(r.hcol, want[1]) and r.align_cost == want[4], (size, R, C)


def run_align_sparse(e, sub, size):
    _run_align_sparse(e, sub, size, False)


def run_align_sparse_pt(e, sub, size):
    _run_align_sparse(e, sub, size, True)


FAMILIES = [run_fill_sparse, run_fill_full, run_fill_full_batch, run_score, run_score_both_ends, run_score_scan,
            run_score_batch, run_db, run_trace_sparse, run_align_sparse, run_align_sparse_pt]


@pytest.mark.parametrize("family", FAMILIES, ids=lambda f: f.__name__[4:])
def test_grow_shrink_regrow(fresh, sub, family):
    """Small, then several times larger (every buffer of the family regrows), then small again (in the
    larger buffers): all three results exact."""
    e = fresh()
    for size in GROWTH:
        family(e, sub, size)


def test_trace_tile_keeps_codes_in_global_memory():
    """TRACE_BX is past the width at which gsa_trace_sparse_dev keeps a tile's move codes in LDS
    (trace_lds_bytes(tBy, tBx, ., true) <= 160 KiB: 4 (32 x 32 + 6 (tBy + 1) + tBx + 17) bytes and a
    code word per 16 rows of every column, in blocks of 64 columns)."""
    tBy = gsa.sparse_tile_by()
    words = -(-tBy // 16) * -(-TRACE_BX // 64) * 64
    assert 4 * (32 * 32 + 6 * (tBy + 1) + TRACE_BX + 17) + 4 * words > 160 * 1024


# -- the staging rings ---------------------------------------------------------------------------

RING = 7  # batches in flight: more than the ring's four slots + 2


def _ring_shapes(k):
    """Batch k (1 ... RING): k small pairs, so every batch's descriptors are larger than the last."""
    return [(150 + 10 * p + k, 130 + 7 * k + p) for p in range(k)]


def test_staging_ring_wraps_sparse(fresh, sub):
    """Seven sparse batches of 1 ... 7 pairs on one stream with no sync in between: each pinned slot is
    reused (and regrown) while earlier copies may still be in flight."""
    e = fresh()
    s = _dev(sub)
    jobs = []
    for k in range(1, RING + 1):
        shapes = _ring_shapes(k)
        pairs = [_pair(R, C) for R, C in shapes]
        ins = [(_dev(Y), _dev(X)) for Y, X in pairs]
        geoms = [gsa.sparse_geometry(R + 1, C + 1, 64) for R, C in shapes]
        outs = [(_empty(g.hrowElems), _empty(g.hcolElems)) for g in geoms]
        jobs.append((shapes, ins, outs))
    for shapes, ins, outs in jobs:
        e.fill_batch_dev([(y.data_ptr(), y.numel(), x.data_ptr(), x.numel(), (hr.data_ptr(), hc.data_ptr()))
                          for (y, x), (hr, hc) in zip(ins, outs)], s.data_ptr(), _substsz(sub), G, mode="sparse", tileBx=64)
    e.sync()
    for shapes, ins, outs in jobs:
        for (R, C), (hr, hc) in zip(shapes, outs):
            want = _headers(R, C, 64)
            assert np.array_equal(hr.cpu().numpy(), want[0]) and np.array_equal(hc.cpu().numpy(), want[1]), (len(shapes), R, C)


def test_staging_ring_wraps_full(fresh, sub):
    """The same with seven full batches: the descriptor ring and the expansion's ring."""
    e = fresh()
    jobs = [(_ring_shapes(k),) + _full_batch_launch(e, sub, _ring_shapes(k)) for k in range(1, RING + 1)]
    e.sync()
    for shapes, keep, outs in jobs:
        _full_batch_check(shapes, outs, len(shapes))


# -- accounting ----------------------------------------------------------------------------------

@pytest.mark.parametrize("family", [run_fill_sparse, run_fill_full, run_fill_full_batch, run_score_batch],
                         ids=lambda f: f.__name__[4:])
def test_peak_allocs_follow_the_capacity_held(fresh, sub, family):
    """glmem_peak_allocs is the device capacity held at a launch: a repeated call allocates nothing, a
    larger one raises it, and buffers never shrink."""
    e = fresh()
    peak = lambda: e.mem_stats()["glmem_peak_allocs"]
    e.reset_mem_stats()
    family(e, sub, SMALL)
    p1 = peak()
    assert p1 > 0
    family(e, sub, SMALL)
    assert peak() == p1
    family(e, sub, LARGE)
    p2 = peak()
    assert p2 > p1
    e.reset_mem_stats()
    assert peak() == 0
    family(e, sub, SMALL)
    assert peak() >= p2


# -- lifecycle -----------------------------------------------------------------------------------

def test_create_use_destroy_in_a_row(fresh, sub):
    """Three contexts in a row, each running one call of every family before it is destroyed; a fourth
    still fills correctly."""
    for _ in range(3):
        e = gsa.Engine(0)
        try:
            for family in FAMILIES:
                family(e, sub, SMALL)
                e.set_knob("GSA_SCORE_BIDI", None)
                e.set_knob("GSA_SCORE_SCAN", None)
        finally:
            e.close()
    e = fresh()
    run_fill_sparse(e, sub, SMALL)
    run_fill_full(e, sub, SMALL)
