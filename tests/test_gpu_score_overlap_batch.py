"""Overlap (dovetail) scores of a batch of long pairs in one launch (gsa_score_overlap_batch_dev: the
batched overlap instances of the K-rows score kernel, every pair's row R and column C in its own part of
one row and one column buffer, and one workgroup per pair that takes the first maximum over both,
nw_kscore_overlap_batch.hip) against tests/_overlap_oracle.py, exactly, against
gsa_score_overlap_dev on each pair alone, and with the list reversed.  The lists are
tests/_overlap_batch.py's: the row and column edges, the same pair twice, two pairs on one seqX buffer,
empty sides, a score of 0, both containments and the corner; column buffers side by side; ties."""
import ctypes

import numpy as np
import pytest

import gpuseqalign_amd as gsa
from tests import _overlap_batch as ob
from tests import _overlap_oracle as oo
from tests._overlap_pair import GAPS, hdr

pytestmark = pytest.mark.gpu


def _check_scores(engine, b, go, ge, single=True, align=oo.align):
    n = len(b)
    sc = b.score(engine, go, ge)
    for k in range(n):
        w = b.want(k, go, ge, align)[0]
        assert sc[k] == (w[0], w[3], w[4]), (b.items[k][0], go, ge, sc[k], w[:5])
        if single:
            assert b.pair(k).score(engine, go, ge) == sc[k], b.items[k][0]
    assert b.score(engine, go, ge, list(range(n))[::-1]) == sc[::-1]
    return sc


def _edges(engine, golden, go, ge, k):
    b = ob.edge_list(256 * (k or 4), golden.blosum62)
    sc = _check_scores(engine, b, go, ge)
    by = {key: sc[i] for i, (key, _) in enumerate(b.items)}
    assert by["R0"] == (0, 0, 0) and by["C0"] == (0, 40, 0) and by["zero"] == (0, 40, 0)
    if (go, ge) in ob.STRICT:
        assert by["corner"][1:] == (200, 290)
        yinx = b.pair(b.index("yinx"))  # the contained sequence ends on its own last letter
        assert by["yinx"][1] == yinx.R and by["xiny"][2] == yinx.R


@pytest.mark.parametrize("k", [None, 2])
@pytest.mark.parametrize("go,ge", GAPS)
def test_edges_in_one_batch(engine, golden, knobs, go, ge, k):
    if k:
        knobs("GSA_SCORE_K", k)
    _edges(engine, golden, go, ge, k)


def test_edges_on_the_int16_profile(engine, golden, knobs):
    knobs("GSA_KROW_Q8", 0)
    _edges(engine, golden, -4, -4, None)


@pytest.mark.parametrize("k", [None, 2])
@pytest.mark.parametrize("go,ge", GAPS)
def test_column_buffers_do_not_bleed(engine, knobs, go, ge, k):
    """R = 1 pairs, whose one ticket stores TR rows of column C, around pairs whose only maximum lies on
    column C at rows 1 ... 4 and at row R; a maximum in the last wave of a first ticket next to pairs of
    TR n + 1 rows.  Both list orders (_check_scores)."""
    if k:
        knobs("GSA_SCORE_K", k)
    tr = 256 * (k or 4)
    b = ob.bleed_list(tr)
    sc = _check_scores(engine, b, go, ge)
    if (go, ge) in ob.STRICT:
        for e in (1, 2, 3, 4):
            assert sc[b.index(("colC", e))] == (5 * e, e, 300)
        assert sc[b.index("corner")] == (1000, 200, 290)
        assert sc[b.index(("lastwave", tr - 3))] == (5 * (tr - 3), tr - 3, tr + 60)


@pytest.mark.parametrize("go,ge", GAPS)
def test_ties(engine, go, ge):
    """Two equal maxima on row R (the smaller column wins), on column C (the smaller row wins) and on
    both (row R wins), each between neighbours with larger scores."""
    b = ob.tie_list()
    sc = _check_scores(engine, b, go, ge)
    if (go, ge) in ob.STRICT:
        H = oo.matrices(b.pair(1).Y, b.pair(1).X, ob.ID20, go, ge)[0]
        assert H[40, 58] == H[40, 63] == 200 == H[40].max() >= H[:, -1].max()
        assert sc[1] == (200, 40, 58) and sc[3] == (40, 12, 8) and sc[5] == (200, 80, 40)
        assert min(sc[0][0], sc[2][0], sc[4][0], sc[6][0]) > 200


def test_one_pair_and_kernel_time(engine, golden):
    """A list of one pair (the one-pair layout and grid), and the time of the launch in every dict."""
    b = ob.Batch("one", golden.blosum62)
    b.add("p", *ob.related(2100, 2600, 6))
    for go, ge in ((-11, -1), (-4, -4)):
        _check_scores(engine, b, go, ge)
    r = engine.score_overlap_batch_dev(b.ptrs(), *b.table(), -11, -1)
    assert r[0]["kernel_ms"] > 0


@pytest.mark.parametrize("go,ge", [(-11, -1), (-4, -4)])
def test_mid_size(engine, golden, go, ge):
    """8 related pairs of 3000 x 3000: several tickets per pair in flight."""
    if "mid" not in ob._LISTS:
        b = ob.Batch("mid", golden.blosum62)
        for n in range(8):
            b.add(n, *ob.related(3000, 3000, 500 + n))
        ob._LISTS["mid"] = b
    _check_scores(engine, ob._LISTS["mid"], go, ge, single=False)


def test_value_bound_2_pow_26_is_scored(engine):
    """B on either side of 2^26 in one list: the score call takes both (int64 reference)."""
    go, ge = -11, -1
    sub = np.where(np.eye(20, dtype=bool), 32755, -4).astype(np.int64)
    b = ob.Batch("b26", sub)
    for R in (2048, 2049):
        b.add(R, *ob.dovetail(R, 2100, 1500, 61))
        assert (oo.exact_for(R, 2100, sub, go, ge) < (1 << 26)) == (R == 2048)
    _check_scores(engine, b, go, ge, align=oo.align64)


def _refused(call):
    with pytest.raises(gsa.NwError) as ei:
        call()
    assert ei.value.stat == gsa.NwStat.errorInvalidValue


def _low_table(shift, n=20, seed=3):
    """A table whose values s all have s + shift in (-32768, 32767], the matches at the upper edge: with
    gap costs of `shift` in all, only such a table passes the int16 test."""
    rng = np.random.default_rng(seed)
    v = rng.integers(-32000, 20000, (n, n))
    v[np.diag_indices(n)] = 32767
    return (v - shift).astype(np.int64)


def test_value_bound_2_pow_29_refuses_the_call(engine):
    """B + |gapo| on either side of 2^29, with gape = 0 and gapo = -(2^20 + 32767) as
    tests/test_gpu_score_overlap_pair.py builds it: the pair below the bound is scored among others (int64
    reference); the pair on it, among good ones, refuses the whole call and leaves out untouched."""
    go, ge = -((1 << 20) + 32767), 0
    sub = _low_table(-go - ge)
    smax = int(np.abs(sub).max())
    n_ok = ((1 << 29) - 1 - 2 * (-go)) // smax
    ok, bad = ob.Batch("b29ok", sub), ob.Batch("b29", sub)
    for b in (ok, bad):
        b.add("s", ob.seq(60, 3), ob.seq(80, 4))
    for n, b in ((n_ok, ok), (n_ok + 1, bad)):
        p = b.add(n, ob.seq(n, 5), ob.seq(n + 30, 6))
        B = oo.exact_for(p.R, p.C, sub, go, ge)
        assert (B - go < (1 << 29)) == (b is ok) and oo.span(p.R, p.C, sub, go, ge) < (1 << 28)
        b.add("t", ob.seq(70, 7), ob.seq(50, 8))
    _check_scores(engine, ok, go, ge, align=oo.align64)
    arr = (gsa.PairDev * 3)()
    for k, (yp, ar, xp, ac) in enumerate(bad.ptrs()):
        arr[k].seqY, arr[k].adjrows, arr[k].seqX, arr[k].adjcols = yp, ar, xp, ac
    res = (gsa.ScoreResult * 3)()
    for r in res:
        r.score, r.i_end, r.j_end = -77, -78, -79
    st = gsa.lib().gsa_score_overlap_batch_dev(engine._h, 3, arr, *bad.table(), go, ge, res, None, None)
    assert st == gsa.NwStat.errorInvalidValue
    assert [(r.score, r.i_end, r.j_end) for r in res] == [(-77, -78, -79)] * 3


def test_int16_table_edges(engine, golden):
    """s - gapo - gape at -32767 and 32767 is scored, at -32768 and 32768 the call is refused."""
    go, ge = -11, -1
    Y, X = ob.related(120, 260, 43)
    Y2, X2 = ob.related(300, 90, 44)
    base = np.asarray(golden.blosum62).reshape(25, 25).astype(np.int64)
    for v, ok in ((-32767, True), (-32768, False), (32767, True), (32768, False)):
        sub = base.copy()
        a, c = (int(Y[5]), int(X[70])) if v < 0 else (int(Y[9]), int(Y[9]))
        sub[a, c] = v + go + ge
        b = ob.Batch(("i16", v), sub)
        b.add(0, Y, X)
        b.add(1, Y2, X2)
        if ok:
            _check_scores(engine, b, go, ge, align=oo.align64)
        else:
            _refused(lambda: b.score(engine, go, ge))


@pytest.fixture(scope="module")
def few(engine, golden):
    b = ob.Batch("few", golden.blosum62)
    b.add(0, *ob.related(700, 1650, 91))
    b.add(1, *ob.related(1100, 200, 93))
    b.add(2, ob.seq(30, 3), hdr([]))
    b.add(3, *ob.related(90, 1500, 95))
    return b


def _raw(engine, b, go=-11, ge=-1, npairs=None, null_out=False, null_pairs=False, null_subst=False, patch=None, substsz=None):
    ptrs = b.ptrs()
    n = len(ptrs) if npairs is None else npairs
    arr = (gsa.PairDev * len(ptrs))()
    for k, (yp, ar, xp, ac) in enumerate(ptrs):
        arr[k].seqY, arr[k].adjrows, arr[k].seqX, arr[k].adjcols = yp, ar, xp, ac
    if patch:
        patch(arr)
    res = (gsa.ScoreResult * len(ptrs))()
    sub, ssz = b.table()
    return gsa.lib().gsa_score_overlap_batch_dev(engine._h, n, None if null_pairs else arr, None if null_subst else sub,
                                                 ssz if substsz is None else substsz, go, ge, None if null_out else res,
                                                 None, None)


def test_invalid_input(engine, few):
    def bad(**kw):
        assert _raw(engine, few, **kw) == gsa.NwStat.errorInvalidValue, kw
        assert _raw(engine, few) == 0

    def set_field(k, name, value):
        return lambda arr: setattr(arr[k], name, value)

    bad(go=-1, ge=-11)             # go > ge
    bad(ge=1)                      # ge > 0
    bad(go=-2000010, ge=-2000000)  # outside the value range
    bad(npairs=0)
    bad(npairs=-1)
    bad(null_pairs=True)
    bad(null_subst=True)
    bad(null_out=True)
    bad(substsz=33)
    bad(patch=set_field(1, "adjrows", 0))
    bad(patch=set_field(2, "adjcols", 0))
    bad(patch=set_field(1, "seqY", None))
    bad(patch=set_field(3, "seqX", None))


@pytest.mark.parametrize("go,ge", [(-11, -1), (-4, -4)])
def test_other_calls_before_and_after(engine, few, go, ge):
    """score_overlap_dev, score_semi_batch_dev and score_batch_dev give the same before and after, and
    gsa_last_launch's record stays."""
    def others():
        one = few.pair(0).score(engine, go, ge)
        sg = engine.score_semi_batch_dev(few.ptrs(), *few.table(), go, ge)
        sc = engine.score_batch_dev(few.ptrs(), *few.table(), go, ge, False)
        return one, [(r["score"], r["i_end"], r["j_end"]) for r in sg], [(r["score"], r["i_end"], r["j_end"]) for r in sc]

    before = others()
    record = engine.last_launch()
    sc = _check_scores(engine, few, go, ge)
    assert engine.last_launch() == record
    assert others() == before and sc[0] == before[0]


def test_row_and_column_buffers_are_counted_in_mem_stats(engine, golden):
    e = gsa.Engine(0)
    try:
        b = ob.Batch("mem", golden.blosum62)
        b.add(0, *ob.related(150000, 600, 93))
        b.add(1, *ob.related(100000, 500, 94))
        e.reset_mem_stats()
        base = e.mem_stats()["glmem_peak_allocs"]
        sc = b.score(e, -11, -1)
        # both columns (every ticket whole), both rows, and the checkpoint rows of both pairs' tickets
        tickets = [-(-150000 // 1024), -(-100000 // 1024)]
        cols = 4 * sum(1 + 1024 * t for t in tickets)
        gran = 16 * (tickets[0] * ((600 + 16) & ~15) + tickets[1] * ((500 + 16) & ~15))
        assert e.mem_stats()["glmem_peak_allocs"] - base >= cols + 4 * (1100 + 2 * 208) + gran
        assert sc == [b.pair(k).score(e, -11, -1) for k in range(2)]
    finally:
        e.close()


def test_host_form_with_empty_sides(engine, golden, few):
    pairs = [(p.Y, p.X) for _, p in few.items] + [(hdr([]), few.pair(0).X), (hdr([]), hdr([]))]
    for go, ge in ((-11, -1), (-5, -2)):
        r = engine.score_overlap_batch(pairs, golden.blosum62, go, ge)
        got = [(x["score"], x["i_end"], x["j_end"]) for x in r]
        want = [few.want(k, go, ge)[0] for k in range(4)]
        assert got == [(w[0], w[3], w[4]) for w in want] + [(0, 0, 0), (0, 0, 0)]
        assert got[2] == (0, 30, 0)
    r = engine.score_overlap_batch(pairs[:2], golden.blosum62, -4)
    assert [x["score"] for x in r] == [few.want(k, -4, -4)[0][0] for k in range(2)]
