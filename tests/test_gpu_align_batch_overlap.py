"""The overlap (dovetail) alignments of a batch of long pairs in one call (gsa_align_batch_overlap_dev:
the batched overlap score launch, then rounds of one fill launch over the strips of many pairs and one
walk launch with a wave per pair, nw_pair_overlap_trace_batch.hip) against
tests/_overlap_oracle.py, exactly: score, start cell, end cell and CIGAR, status 0; against
gsa_align_pair_overlap_dev on each pair alone; and with the list reversed.  Every case also asserts what
gsa_align_batch_overlap_info says -- pairs traced and answered on the host, strips, checkpoint bytes,
rounds, strips filled and peak code bytes -- restated along the oracle's paths (tests/_overlap_batch.py),
so that no case passes by another route.  A strip is TR rows: 1024 in both gap models, 512 with
GSA_SCORE_K=2; a lane holds TR / 64."""
import ctypes

import numpy as np
import pytest

import gpuseqalign_amd as gsa
from tests import _overlap_batch as ob
from tests import _overlap_oracle as oo
from tests._overlap_batch import check_batch
from tests._overlap_pair import GAPS, hdr, t6

pytestmark = pytest.mark.gpu


# -- 1. the edges in one batch --------------------------------------------------------------------------


def _edges(engine, golden, knobs, go, ge, k, mwg):
    if k:
        knobs("GSA_SCORE_K", k)
    tr = 256 * (k or 4)
    b = ob.edge_list(tr, golden.blosum62)
    res, info, _ = check_batch(engine, b, go, ge, tr, mwg)
    by = {key: res[i] for i, (key, _) in enumerate(b.items)}
    assert t6(by["R0"]) == (0, 0, 0, 0, 0, "") and t6(by["C0"]) == (0, 40, 0, 40, 0, "")
    assert t6(by["zero"]) == (0, 40, 0, 40, 0, "")
    assert info["rounds"] == 1 and info["host_pairs"] >= 3


@pytest.mark.parametrize("k", [None, 2])
@pytest.mark.parametrize("go,ge", GAPS)
def test_edges_in_one_batch(engine, golden, knobs, go, ge, k):
    _edges(engine, golden, knobs, go, ge, k, 0)


@pytest.mark.parametrize("k", [None, 2])
@pytest.mark.parametrize("mwg", [1, 2])
@pytest.mark.parametrize("go,ge", [(-11, -1), (-4, -4)])
def test_edges_under_a_capped_grid(engine, golden, knobs, go, ge, mwg, k):
    _edges(engine, golden, knobs, go, ge, k, mwg)


def test_edges_on_the_int16_profile(engine, golden, knobs):
    knobs("GSA_KROW_Q8", 0)
    _edges(engine, golden, knobs, -4, -4, None, 0)


# -- 2. column buffers, ties ----------------------------------------------------------------------------


@pytest.mark.parametrize("k", [None, 2])
@pytest.mark.parametrize("go,ge", GAPS)
def test_column_buffers_do_not_bleed(engine, knobs, go, ge, k):
    """tests/_overlap_batch.py's bleed_list in both orders: R = 1 pairs around pairs whose only maximum
    lies on column C at rows 1 ... 4 and at row R, and a maximum in the last wave of a first ticket next to
    pairs of TR n + 1 rows."""
    if k:
        knobs("GSA_SCORE_K", k)
    tr = 256 * (k or 4)
    b = ob.bleed_list(tr)
    res, info, _ = check_batch(engine, b, go, ge, tr)
    if (go, ge) in ob.STRICT:
        for e in (1, 2, 3, 4):
            assert t6(res[b.index(("colC", e))]) == (5 * e, 0, 300 - e, e, 300, "%d=" % e)
        e = tr - 3
        assert t6(res[b.index(("lastwave", e))]) == (5 * e, 0, 63, e, tr + 60, "%d=" % e)


@pytest.mark.parametrize("go,ge", GAPS)
def test_ties(engine, go, ge):
    b = ob.tie_list()
    res, _, _ = check_batch(engine, b, go, ge, 1024)
    if (go, ge) in ob.STRICT:
        assert t6(res[1])[3:5] == (40, 58) and t6(res[3]) == (40, 4, 0, 12, 8, "8=")
        assert t6(res[5]) == (200, 40, 0, 80, 40, "40=")


# -- 3. planted dovetails -------------------------------------------------------------------------------

_PL = {}


def _dovetails(tr):
    """Pair 0: the end row on column C above row R, in the first of three tickets.  Pair 1: the start on
    column 0 on row 2 TR + 5 of 3 TR + 100, two strips below strip 0.  Pair 2: a plain dovetail."""
    if tr not in _PL:
        b = ob.Batch("dove%d" % tr, ob.ID20)
        b.add("endc", *ob.end_on_column_c(2 * tr + 50, tr + 20, tr - 40))
        b.add("start0", *ob.start_on_column_0(3 * tr + 100, 2 * tr + 5, 40))
        b.add("plain", *ob.start_on_column_0(500, 120))
        _PL[tr] = b
    return _PL[tr]


@pytest.mark.parametrize("k", [None, 2])
@pytest.mark.parametrize("go,ge", GAPS)
def test_planted_dovetails(engine, knobs, go, ge, k):
    """An end cell on column C in the first of three tickets: strips < ceil(R / TR), the strips below are
    never planned.  A start on column 0 two strips below strip 0 with a limit of one strip per pair per
    round: strips_filled < strips."""
    if k:
        knobs("GSA_SCORE_K", k)
    tr = 256 * (k or 4)
    b = _dovetails(tr)
    res, info, items = check_batch(engine, b, go, ge, tr)
    if (go, ge) in ob.STRICT:
        e = tr - 40
        assert t6(res[0]) == (5 * e, 0, 60, e, tr + 20, "%d=" % e)
        assert t6(res[1])[1:5] == (2 * tr + 5, 0, 3 * tr + 100, tr + 95)
        assert info["strips"] == 1 + 4 + 1 < sum(-(-b.pair(n).R // tr) for n in range(3))
    # one strip per pair per round: the widest strip's bytes
    strip = max(it[1] for it in items) * tr // 2
    one, info1, _ = check_batch(engine, b, go, ge, tr, limit=strip, single=False)
    assert [t6(r) for r in one] == [t6(r) for r in res]
    if (go, ge) in ob.STRICT:
        assert info1["strips_filled"] < info1["strips"], info1
        assert info1["strips_filled"] == 1 + 2 + 1 and info1["rounds"] >= 2


# -- 4. rounds ------------------------------------------------------------------------------------------

_RND = {}


def _rounds_batch(golden, tr):
    """Six pairs of 2 TR + 1 ... 3 TR rows: Y holds a mutated copy of X (400 ... 700 letters) between
    random flanks, so the path runs through X whole and ends on column C."""
    if tr not in _RND:
        from gpuseqalign_amd import formats as F
        b = ob.Batch("rounds%d" % tr, golden.blosum62)
        rows = [2 * tr + 1, 2 * tr + 300, 3 * tr - 1, 3 * tr, 2 * tr + 77, 2 * tr + 511]
        cols = [700, 400, 555, 640, 480, 613]
        for n, (R, C) in enumerate(zip(rows, cols)):
            x = ob.seq(C, 300 + n)
            core = F.mutate_seq(x, 310 + n)[1:]
            tail = 5 + 3 * n
            q = np.concatenate([ob.seq(R, 320 + n)[1:R - len(core) - tail + 1], core, ob.seq(tail, 330 + n)[1:]])[-R:]
            b.add(n, hdr(q), x)
        _RND[tr] = b
    return _RND[tr]


@pytest.mark.parametrize("k", [None, 2])
@pytest.mark.parametrize("go,ge", [(-11, -1), (-4, -4), (-5, -2)])
def test_rounds(engine, golden, knobs, go, ge, k):
    """A limit worth about three of the widest strips: at least three rounds, and rounds, strips_filled
    and code_bytes as the plan restated along the oracle's paths gives them (check_batch).  A limit one
    byte below the widest pair's single strip: that pair has status 1 with its score and end cell, every
    other pair its full answer; one byte more and it has status 0."""
    if k:
        knobs("GSA_SCORE_K", k)
    tr = 256 * (k or 4)
    b = _rounds_batch(golden, tr)
    full, info0, items = check_batch(engine, b, go, ge, tr, single=False)
    assert info0["rounds"] == 1 and len(items) == 6
    widths = [it[1] for it in items]
    strip = max(widths) * tr // 2
    res, info, _ = check_batch(engine, b, go, ge, tr, limit=3 * strip, single=False)
    assert info["rounds"] >= 3 and info["code_bytes"] <= 3 * strip, info
    assert [t6(r) for r in res] == [t6(r) for r in full]
    res, info, _ = check_batch(engine, b, go, ge, tr, mwg=2, limit=strip, single=False, reverse=False)
    assert info["rounds"] >= 3 and [t6(r) for r in res] == [t6(r) for r in full]
    # one byte less: the widest pair (a single one, by the widths above) is left out
    wide = widths.index(max(widths))
    assert widths.count(max(widths)) == 1
    res, info = b.align(engine, go, ge, 0, strip - 1)
    for n, r in enumerate(res):
        if n == wide:
            assert r["status"] == 1 and r["cigar"] == "" and (r["i_start"], r["j_start"]) == (0, 0)
            assert (r["score"], r["i_end"], r["j_end"]) == (full[n]["score"], full[n]["i_end"], full[n]["j_end"])
        else:
            assert r["status"] == 0 and t6(r) == t6(full[n])
    assert info["batch_pairs"] == 5 and info["code_bytes"] <= strip - 1


# -- 5. mid-size ----------------------------------------------------------------------------------------


@pytest.mark.parametrize("go,ge", [(-11, -1), (-4, -4)])
def test_mid_size(engine, golden, go, ge):
    """8 related pairs of 3000 x 3000: several workgroups and tickets per pair in flight."""
    if "mid" not in ob._LISTS:
        b = ob.Batch("mid", golden.blosum62)
        for n in range(8):
            b.add(n, *ob.related(3000, 3000, 500 + n))
        ob._LISTS["mid"] = b
    res, info, _ = check_batch(engine, ob._LISTS["mid"], go, ge, 1024, single=False, reverse=False)
    assert info["batch_pairs"] == 8 and info["rounds"] == 1


# -- 6. value ranges ------------------------------------------------------------------------------------


def _refused(call):
    with pytest.raises(gsa.NwError) as ei:
        call()
    assert ei.value.stat == gsa.NwStat.errorInvalidValue


def test_value_bound_2_pow_26(engine):
    """The fill keeps 4 x value + source: B < 2^26 per pair.  A list with one pair below the bound is
    aligned (int64 reference); with one pair a row beyond it the alignment call is refused whole."""
    go, ge = -11, -1
    sub = np.where(np.eye(20, dtype=bool), 32755, -4).astype(np.int64)
    ok, both = ob.Batch("b26ok", sub), ob.Batch("b26", sub)
    for R in (2048, 2049):
        Y, X = ob.dovetail(R, 2100, 1500, 61)
        B = oo.exact_for(R, 2100, sub, go, ge)
        assert (B < (1 << 26)) == (R == 2048) and abs(B - (1 << 26)) < 40000
        both.add(R, Y, X)
        if R == 2048:
            ok.add(R, Y, X)
            ok.add("small", *ob.related(100, 300, 63))
    check_batch(engine, ok, go, ge, 1024, align=oo.align64)
    _refused(lambda: both.align(engine, go, ge))


def test_int16_table_edges(engine, golden):
    """s - gapo - gape at -32767 and 32767 is aligned, at -32768 and 32768 refused."""
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
            check_batch(engine, b, go, ge, 1024, align=oo.align64)
        else:
            _refused(lambda: b.align(engine, go, ge))


# -- 7. around the call ---------------------------------------------------------------------------------


@pytest.fixture(scope="module")
def few(engine, golden):
    b = ob.Batch("few", golden.blosum62)
    b.add(0, *ob.related(700, 1650, 91))
    b.add(1, *ob.related(1100, 200, 93))
    b.add(2, ob.seq(30, 3), hdr([]))
    b.add(3, *ob.related(90, 1500, 95))
    return b


def _raw(engine, b, go=-11, ge=-1, mwg=0, limit=0, cap=1 << 16, npairs=None, null_out=False, null_cigar=False,
         null_pairs=False, null_subst=False, null_info=False, patch=None, fill=None):
    ptrs = b.ptrs()
    n = len(ptrs) if npairs is None else npairs
    arr = (gsa.PairDev * len(ptrs))()
    for k, (yp, ar, xp, ac) in enumerate(ptrs):
        arr[k].seqY, arr[k].adjrows, arr[k].seqX, arr[k].adjcols = yp, ar, xp, ac
    if patch:
        patch(arr)
    res, info = (gsa.AlignDbResult * len(ptrs))(), gsa.AlignBatchOverlapInfo()
    if fill is not None:
        for r in res:
            r.score = fill
    need, ms = ctypes.c_int64(-1), ctypes.c_float(0)
    buf = ctypes.create_string_buffer(max(cap, 1))
    sub, ssz = b.table()
    st = gsa.lib().gsa_align_batch_overlap_dev(engine._h, n, None if null_pairs else arr, None if null_subst else sub, ssz,
                                               go, ge, mwg, limit, None if null_out else res, None if null_cigar else buf,
                                               cap, ctypes.byref(need), None if null_info else ctypes.byref(info),
                                               None if null_info else ctypes.byref(ms), None)
    return st, res, need.value, buf


def test_short_cigar_buffer(engine, few):
    cigs = [few.want(k, -11, -1)[0][5] for k in range(4)]
    total = sum(len(c) + 1 for c in cigs)
    offs = np.cumsum([0] + [len(c) + 1 for c in cigs])
    for null_info in (False, True):  # (null info and kernel_ms)
        st, res, need, buf = _raw(engine, few, cap=total, null_info=null_info)
        assert st == 0 and need == total
        for k, c in enumerate(cigs):
            assert (res[k].status, res[k].cigar_off, res[k].cigar_len) == (0, offs[k], len(c))
            assert buf.raw[offs[k]:offs[k] + len(c) + 1] == c.encode() + b"\0"
    # room for the first string and all of the second but its NUL: the later ones do not fit either,
    # except the empty one of pair 2, whose NUL still has no room
    cap = int(offs[1]) + len(cigs[1])
    st, res, need, buf = _raw(engine, few, cap=cap)
    assert st == 0 and need == total
    assert [res[k].status for k in range(4)] == [0, 2, 2, 2]
    assert (res[0].cigar_off, res[0].cigar_len) == (0, len(cigs[0]))
    for k in range(4):
        want = few.want(k, -11, -1)[0]
        assert (res[k].score, res[k].i_start, res[k].j_start, res[k].i_end, res[k].j_end) == want[:5]
    st, res, need, _ = _raw(engine, few, cap=0, null_cigar=True)
    assert st == 0 and need == total and [res[k].status for k in range(4)] == [2, 2, 2, 2]


def test_invalid_input(engine, few):
    def good():
        st, res, _, _ = _raw(engine, few)
        assert st == 0 and [res[k].status for k in range(4)] == [0, 0, 0, 0]

    def bad(**kw):
        st, res, _, _ = _raw(engine, few, fill=-77, **kw)
        assert st == gsa.NwStat.errorInvalidValue, kw
        assert [r.score for r in res] == [-77] * 4  # nothing changed in out
        good()

    def set_field(k, name, value):
        return lambda arr: setattr(arr[k], name, value)

    good()
    bad(go=-1, ge=-11)                         # go > ge
    bad(ge=1)                                  # ge > 0
    bad(go=-2000010, ge=-2000000)              # outside the value range
    bad(npairs=0)
    bad(npairs=-1)
    bad(null_pairs=True)
    bad(null_subst=True)
    bad(patch=set_field(1, "adjrows", 0))
    bad(patch=set_field(2, "adjcols", 0))
    bad(patch=set_field(1, "seqY", None))
    bad(patch=set_field(3, "seqX", None))
    bad(limit=-1)
    bad(cap=-1)
    bad(mwg=-1)
    bad(null_cigar=True, cap=16)
    assert _raw(engine, few, null_out=True)[0] == gsa.NwStat.errorInvalidValue
    st = gsa.lib().gsa_align_batch_overlap_dev(engine._h, 1, (gsa.PairDev * 1)(), few.table()[0], 33, -11, -1, 0, 0,
                                               (gsa.AlignDbResult * 1)(), None, 0, None, None, None, None)
    assert st == gsa.NwStat.errorInvalidValue


@pytest.mark.parametrize("go,ge", [(-11, -1), (-4, -4)])
def test_other_calls_before_and_after(engine, few, go, ge):
    """score_overlap_dev, align_pair_overlap_dev, score_semi_batch_dev, align_batch_semi_dev and
    align_batch_dev give the same before and after the new calls, and gsa_last_launch's record is left as
    it was."""
    def others():
        p = few.pair(1)
        one = engine.align_pair_overlap_dev(*p.args(), go, ge)
        sg = engine.score_semi_batch_dev(few.ptrs(), *few.table(), go, ge)
        ag = engine.align_batch_semi_dev(few.ptrs(), *few.table(), go, ge)
        al = engine.align_batch_dev(few.ptrs(), *few.table(), go, ge, False)
        return (p.score(engine, go, ge), t6(one), [(r["score"], r["i_end"], r["j_end"]) for r in sg],
                [(r["status"], t6(r)) for r in ag], [(r["status"], t6(r)) for r in al])

    before = others()
    record = engine.last_launch()
    res, _, _ = check_batch(engine, few, go, ge, 1024)
    assert engine.last_launch() == record
    assert others() == before
    assert t6(res[1]) == before[1]


def test_scratch_is_counted_in_mem_stats(engine, golden):
    e = gsa.Engine(0)
    try:
        b = ob.Batch("mem", golden.blosum62)
        b.add(0, *ob.dovetail(60000, 900, 600, 93))
        b.add(1, *ob.dovetail(40000, 700, 500, 94))
        e.reset_mem_stats()
        base = e.mem_stats()["glmem_peak_allocs"]
        sc = b.score(e, -11, -1)
        after = e.mem_stats()["glmem_peak_allocs"]
        tickets = [-(-60000 // 1024), -(-40000 // 1024)]
        cols = 4 * sum(1 + 1024 * t for t in tickets)
        gran = 16 * (tickets[0] * ((900 + 16) & ~15) + tickets[1] * ((700 + 16) & ~15))
        assert after - base >= cols + 4 * (1600 + 2 * 208) + gran  # column and row buffers, checkpoint rows
        res, info = b.align(e, -11, -1)
        assert [(r["score"], r["i_end"], r["j_end"]) for r in res] == sc and info["code_bytes"] > 0
        assert info["gran_bytes"] == gran
        assert e.mem_stats()["glmem_peak_allocs"] >= after + info["code_bytes"]
    finally:
        e.close()


def test_host_form_with_empty_sides(engine, golden, few):
    pairs = [(p.Y, p.X) for _, p in few.items] + [(hdr([]), few.pair(0).X), (hdr([]), hdr([]))]
    for go, ge in ((-11, -1), (-5, -2)):
        res = engine.align_batch_overlap(pairs, golden.blosum62, go, ge)
        assert [r["status"] for r in res] == [0] * 6
        assert [t6(r) for r in res[:4]] == [few.want(k, go, ge)[0] for k in range(4)]
        assert t6(res[2]) == (0, 30, 0, 30, 0, "")
        assert [t6(r) for r in res[4:]] == [(0, 0, 0, 0, 0, "")] * 2
        info = engine.last_align_batch_overlap_info()
        assert info["batch_pairs"] == 3 and info["host_pairs"] == 3
    res = engine.align_batch_overlap(pairs[:2], golden.blosum62, -4)
    assert [t6(r) for r in res] == [few.want(k, -4, -4)[0] for k in range(2)]
    res = engine.align_batch_overlap(pairs[4:], golden.blosum62, -11, -1)  # nothing for the device
    assert [t6(r) for r in res] == [(0, 0, 0, 0, 0, "")] * 2
    assert engine.last_align_batch_overlap_info()["strip_rows"] == 0
