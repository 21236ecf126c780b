"""Semi-global scores of a batch of long pairs in one launch (gsa_score_semi_batch_dev: the batched
semi-global instances of the K-rows score kernel, every pair's row R in its own part of one row buffer,
and one workgroup per pair that takes the row's first maximum, nw_kscore_semi_batch.hip)
against tests/_semi_oracle.py, exactly, and against gsa_score_semi_dev on each pair alone.  The edges
list is tests/_semi_batch.py's: rows on every register row of a lane and on either side of a strip wave,
a ticket and its checkpoint row, columns on either side of a block, the wave, the hand-off ring and the
profile ring, the same pair twice, two queries on one subject buffer, empty sides, an end on column 0 and
on column C, a negative score."""
import ctypes

import numpy as np
import pytest

import gpuseqalign_amd as gsa
from gpuseqalign_amd import formats as F
from tests import _semi_batch as sb
from tests import _semi_pair as sp
from tests._semi_pair import GAPS, hdr

pytestmark = pytest.mark.gpu


def _check_scores(engine, b, go, ge, single=True, align=sb.so.align):
    n = len(b)
    sc = b.score(engine, go, ge)
    for k in range(n):
        w = b.want(k, go, ge, align)[0]
        assert sc[k] == (w[0], w[3], w[4]), (b.items[k][0], go, ge, sc[k], w)
        if single:
            assert b.pair(k).score(engine, go, ge) == sc[k], b.items[k][0]
    assert b.score(engine, go, ge, list(range(n))[::-1]) == sc[::-1]
    return sc


@pytest.mark.parametrize("k", [None, 2])
@pytest.mark.parametrize("go,ge", GAPS)
def test_edges_in_one_batch(engine, golden, knobs, go, ge, k):
    if k:
        knobs("GSA_SCORE_K", k)
    b = sb.edge_list(256 * (k or 4), golden.blosum62)
    sc = _check_scores(engine, b, go, ge)
    by = {key: sc[i] for i, (key, _) in enumerate(b.items)}
    assert by["R0"] == (0, 0, 0) and by["C0"] == (go + 39 * ge, 40, 0)
    assert by["allI"] == (go + 39 * ge, 40, 0)
    if go < 0:
        assert by["neg"][0] < 0 < by["neg"][2] and by["endC"][2] == 700


def test_one_pair_and_kernel_time(engine, golden):
    """A list of one pair (the one-pair layout), and the time of the launch in every dict."""
    b = sb.Batch("one", golden.blosum62)
    b.add("p", *sb.related(2100, 2600, 5))
    for go, ge in ((-11, -1), (-4, -4)):
        _check_scores(engine, b, go, ge)
    r = engine.score_semi_batch_dev(b.ptrs(), *b.table(), -11, -1)
    assert r[0]["kernel_ms"] > 0


def test_value_bound_2_pow_26_is_scored(engine):
    """B on either side of 2^26 in one list: the score call takes both (int64 reference)."""
    go, ge = -11, -1
    sub = np.where(np.eye(20, dtype=bool), 32755, -4).astype(np.int64)
    x = sb.seq(2100, 61)
    b = sb.Batch("b26", sub)
    for R in (2048, 2049):
        q = F.mutate_seq(hdr(x[11:11 + R + 40]), 62)[1:R + 1]
        b.add(R, hdr(q), x)
        assert (sp.exact_for(R, 2100, sub, go, ge) < (1 << 26)) == (R == 2048)
    _check_scores(engine, b, go, ge, align=sp.align64)


def test_int16_table_edges(engine, golden):
    """s - gapo - gape at -32767 and 32767 is scored, at -32768 and 32768 the call is refused."""
    go, ge = -11, -1
    Y, X = sb.related(120, 260, 43)
    Y2, X2 = sb.related(300, 90, 44)
    base = np.asarray(golden.blosum62).reshape(25, 25).astype(np.int64)
    for v, ok in ((-32767, True), (-32768, False), (32767, True), (32768, False)):
        sub = base.copy()
        a, c = (int(Y[5]), int(X[70])) if v < 0 else (int(Y[9]), int(Y[9]))
        sub[a, c] = v + go + ge
        b = sb.Batch(("i16", v), sub)
        b.add(0, Y, X)
        b.add(1, Y2, X2)
        if ok:
            _check_scores(engine, b, go, ge, align=sp.align64)
        else:
            with pytest.raises(gsa.NwError) as ei:
                b.score(engine, go, ge)
            assert ei.value.stat == gsa.NwStat.errorInvalidValue


def test_refused_call_leaves_out_untouched(engine, golden):
    """Three pairs, the middle one with an empty side.  With a table the call refuses (s - gapo - gape at
    -32768, as in test_int16_table_edges) every word of out stays as it was, the host-answered pair's
    too; with a good table the three are scored as the reference says, the empty side on the host."""
    go, ge = -11, -1
    Y, X = sb.related(120, 260, 43)
    base = np.asarray(golden.blosum62).reshape(25, 25).astype(np.int64)
    bad_sub = base.copy()
    bad_sub[int(Y[5]), int(X[70])] = -32768 + go + ge
    good, bad = sb.Batch("keep", base), sb.Batch("refuse", bad_sub)
    for b in (good, bad):
        b.add("s", sb.seq(60, 3), sb.seq(80, 4))
        b.add("e", hdr([]), sb.seq(80, 5))
        b.add("t", sb.seq(70, 7), sb.seq(50, 8))
    arr = (gsa.PairDev * 3)()
    for k, (yp, ar, xp, ac) in enumerate(bad.ptrs()):
        arr[k].seqY, arr[k].adjrows, arr[k].seqX, arr[k].adjcols = yp, ar, xp, ac
    assert (arr[1].adjrows, arr[1].adjcols) == (1, 81)
    res = (gsa.ScoreResult * 3)()
    for r in res:
        r.score, r.i_end, r.j_end = -77, -78, -79
    st = gsa.lib().gsa_score_semi_batch_dev(engine._h, 3, arr, *bad.table(), go, ge, res, None, None)
    assert st == gsa.NwStat.errorInvalidValue
    assert [(r.score, r.i_end, r.j_end) for r in res] == [(-77, -78, -79)] * 3
    sc = _check_scores(engine, good, go, ge, align=sp.align64)
    assert sc[1] == (0, 0, 0)  # R = 0; R > 0 with C = 0 is test_edges_in_one_batch's "C0": gapo + (R - 1) gape at (R, 0)


@pytest.fixture(scope="module")
def few(engine, golden):
    b = sb.Batch("few", golden.blosum62)
    b.add(0, *sb.related(700, 1650, 91))
    b.add(1, *sb.related(1100, 200, 93))
    b.add(2, sb.seq(30, 3), hdr([]))
    b.add(3, *sb.related(90, 1500, 95))
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
    ms = ctypes.c_float(0)
    sub, ssz = b.table()
    return gsa.lib().gsa_score_semi_batch_dev(engine._h, n, None if null_pairs else arr, None if null_subst else sub,
                                              ssz if substsz is None else substsz, go, ge, None if null_out else res,
                                              ctypes.byref(ms), None)


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
    """score_semi_dev and score_batch_dev give the same before and after, gsa_last_launch's record stays."""
    def others():
        one = few.pair(0).score(engine, go, ge)
        sc = engine.score_batch_dev(few.ptrs(), *few.table(), go, ge, False)
        return one, [(r["score"], r["i_end"], r["j_end"]) for r in sc]

    before = others()
    record = engine.last_launch()
    sc = _check_scores(engine, few, go, ge)
    assert engine.last_launch() == record
    assert others() == before and sc[0] == before[0]


def test_row_buffer_is_counted_in_mem_stats(engine, golden):
    e = gsa.Engine(0)
    try:
        b = sb.Batch("mem", golden.blosum62)
        b.add(0, *sb.related(600, 150000, 93))
        b.add(1, *sb.related(500, 100000, 94))
        e.reset_mem_stats()
        base = e.mem_stats()["glmem_peak_allocs"]
        sc = b.score(e, -11, -1)
        # both rows, and both pairs' checkpoint rows (one ticket each, two arrays of 8-byte words)
        assert e.mem_stats()["glmem_peak_allocs"] - base >= 4 * 250000 + 16 * 250000
        assert sc == [b.pair(k).score(e, -11, -1) for k in range(2)]
    finally:
        e.close()


def test_host_form_with_empty_sides(engine, golden, few):
    pairs = [(p.Y, p.X) for _, p in few.items] + [(hdr([]), few.pair(0).X), (hdr([]), hdr([]))]
    for go, ge in ((-11, -1), (-5, -2)):
        r = engine.score_semi_batch(pairs, golden.blosum62, go, ge)
        got = [(x["score"], x["i_end"], x["j_end"]) for x in r]
        want = [few.want(k, go, ge)[0] for k in range(4)]
        assert got == [(w[0], w[3], w[4]) for w in want] + [(0, 0, 0), (0, 0, 0)]
        assert got[2] == (go + 29 * ge, 30, 0)
    r = engine.score_semi_batch(pairs[:2], golden.blosum62, -4)
    assert [x["score"] for x in r] == [few.want(k, -4, -4)[0][0] for k in range(2)]
