"""The semi-global alignments of a batch of long pairs in one call (gsa_align_batch_semi_dev: the batched
semi-global score launch, then rounds of one fill launch over the strips of many pairs, each over its
pair's column window, and one walk launch with a wave per pair, nw_pair_semi_trace_batch.hip; DESIGN.md
2.2l) against tests/_semi_oracle.py, exactly: score, start cell, end cell and CIGAR, status 0; against
gsa_align_pair_semi_dev on each pair alone; and with the list reversed.  Every case also asserts what
gsa_align_batch_semi_info says -- pairs traced and answered on the host, strips, window columns,
checkpoint bytes, rounds, strips filled and peak code bytes -- restated along the oracle's paths
(tests/_semi_batch.py), so that no case passes by another route.  A strip is TR rows: 1024 in both gap
models, 512 with GSA_SCORE_K=2; a lane holds TR / 64."""
import ctypes

import numpy as np
import pytest

import gpuseqalign_amd as gsa
from gpuseqalign_amd import formats as F
from tests import _semi_batch as sb
from tests import _semi_pair as sp
from tests._semi_batch import check_batch
from tests._semi_pair import GAPS, hdr, t6

pytestmark = pytest.mark.gpu


# -- 1. the edges in one batch --------------------------------------------------------------------------


def _edges(engine, golden, knobs, go, ge, k, mwg):
    if k:
        knobs("GSA_SCORE_K", k)
    tr = 256 * (k or 4)
    b = sb.edge_list(tr, golden.blosum62)
    res, info, _ = check_batch(engine, b, go, ge, tr, mwg)
    by = {key: res[i] for i, (key, _) in enumerate(b.items)}
    assert t6(by["R0"]) == (0, 0, 0, 0, 0, "") and t6(by["C0"]) == (go + 39 * ge, 0, 0, 40, 0, "40I")
    assert t6(by["allI"]) == (go + 39 * ge, 0, 0, 40, 0, "40I")
    if go < 0:
        assert by["neg"]["score"] < 0 < by["neg"]["j_end"] and by["endC"]["j_end"] == 700
    assert info["rounds"] == 1 and info["strips_filled"] == info["strips"]


@pytest.mark.parametrize("k", [None, 2])
@pytest.mark.parametrize("go,ge", GAPS)
def test_edges_in_one_batch(engine, golden, knobs, go, ge, k):
    _edges(engine, golden, knobs, go, ge, k, 0)


@pytest.mark.parametrize("k", [None, 2])
@pytest.mark.parametrize("mwg", [1, 2])
@pytest.mark.parametrize("go,ge", [(-11, -1), (-4, -4)])
def test_edges_under_a_capped_grid(engine, golden, knobs, go, ge, mwg, k):
    _edges(engine, golden, knobs, go, ge, k, mwg)


# -- 2. windows -----------------------------------------------------------------------------------------

_WIN = {}


def _window_batch(golden):
    if "b" not in _WIN:
        C = 6000
        b = sb.Batch("win", golden.blosum62)
        x = sb.seq(C, 77)
        for at in (0, 1, 700, C - 300):
            if at == C - 300:  # the query ends with the subject's last letters
                q = F.mutate_seq(hdr(x[C - 329:C - 2]), 78 + at)[1:]
                q = np.concatenate([q, x[C - 2:C + 1]])[-300:]
            else:
                q = F.mutate_seq(hdr(x[1 + at:1 + at + 330]), 78 + at)[1:301]
            assert len(q) == 300
            b.add(("at", at), hdr(q), x)
        b.add("unrelated", sb.seq(200, 21), sb.seq(1500, 22))
        b.add("two", sb.seq(2, 23), sb.seq(2, 24))
        _WIN["b"] = b
    return _WIN["b"]


@pytest.mark.parametrize("go,ge", GAPS)
def test_windows(engine, golden, go, ge):
    """A 300-letter query planted, mutated, at four offsets of 6000-letter subjects, an unrelated pair
    and a 2-letter pair: jW = 0 and jW > 0 in one round; window_cols is the header's formula summed
    (check_batch asserts it) and the codes are the windows'."""
    b = _window_batch(golden)
    res, info, items = check_batch(engine, b, go, ge, 1024)
    assert info["rounds"] == 1 and info["code_bytes"] == info["window_cols"] * 512
    jw = [it[2] for it in items]
    if ge < 0:
        assert min(jw) == 0 < max(jw), jw
        assert info["window_cols"] < sum(it[1] for it in items)
    else:
        assert max(jw) == 0


# -- 3. rounds ------------------------------------------------------------------------------------------

_RND = {}


def _rounds_batch(golden, tr):
    """Six pairs of 2 TR + 1 ... 3 TR rows against subjects of 400 ... 700 letters: the query holds a
    mutated copy of the subject between random flanks."""
    if tr not in _RND:
        b = sb.Batch("rounds%d" % tr, golden.blosum62)
        rows = [2 * tr + 1, 2 * tr + 300, 3 * tr - 1, 3 * tr, 2 * tr + 77, 2 * tr + 511]
        cols = [700, 400, 555, 640, 480, 613]
        for n, (R, C) in enumerate(zip(rows, cols)):
            x = sb.seq(C, 300 + n)
            core = F.mutate_seq(x, 310 + n)[1:]
            head = (R - len(core)) // 2
            q = np.concatenate([sb.seq(head, 320 + n)[1:], core, sb.seq(R, 330 + n)[1:]])[:R]
            b.add(n, hdr(q), x)
        _RND[tr] = b
    return _RND[tr]


@pytest.mark.parametrize("k", [None, 2])
@pytest.mark.parametrize("go,ge", [(-11, -1), (-4, -4), (-5, -2)])
def test_rounds(engine, golden, knobs, go, ge, k):
    """A limit worth about three of the widest strips: at least three rounds, and rounds, strips_filled
    and code_bytes as the plan restated along the oracle's paths gives them (check_batch).  A limit one
    byte below the widest pair's single strip: that pair has status 1 with its score and end cell, every
    other pair its full answer."""
    if k:
        knobs("GSA_SCORE_K", k)
    tr = 256 * (k or 4)
    b = _rounds_batch(golden, tr)
    full, info0, items = check_batch(engine, b, go, ge, tr, single=False)
    assert info0["rounds"] == 1
    widths = [it[1] - it[2] for it in items]
    assert len(items) == 6
    strip = max(widths) * tr // 2
    res, info, _ = check_batch(engine, b, go, ge, tr, limit=3 * strip, single=False)
    assert info["rounds"] >= 3 and info["code_bytes"] <= 3 * strip, info
    assert [t6(r) for r in res] == [t6(r) for r in full]
    res, info, _ = check_batch(engine, b, go, ge, tr, mwg=2, limit=strip, single=False, reverse=False)
    assert info["rounds"] >= 6 and [t6(r) for r in res] == [t6(r) for r in full]
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


# -- 4. many workgroups ---------------------------------------------------------------------------------

_MANY = {}


@pytest.mark.parametrize("go,ge", [(-11, -1), (-4, -4)])
def test_many_workgroups(engine, golden, go, ge):
    """8 related pairs of about 3000 letters in 12 000-letter windows: several workgroups and tickets per
    pair in flight."""
    if "b" not in _MANY:
        b = sb.Batch("many", golden.blosum62)
        for n in range(8):
            b.add(n, *sb.related(2900 + 37 * n, 12000 + 16 * n - 5, 500 + 3 * n))
        _MANY["b"] = b
    res, info, _ = check_batch(engine, _MANY["b"], go, ge, 1024, single=False, reverse=False)
    strips = sum(-(-(2900 + 37 * n) // 1024) for n in range(8))  # three or four tickets per pair
    assert info["batch_pairs"] == 8 and info["strips"] == strips >= 24 and info["rounds"] == 1


# -- 5. value ranges ------------------------------------------------------------------------------------


def _refused(call):
    with pytest.raises(gsa.NwError) as ei:
        call()
    assert ei.value.stat == gsa.NwStat.errorInvalidValue


def test_value_bound_2_pow_26(engine):
    """The fill keeps 4 x value + source: B < 2^26 per pair.  A list with one pair on the bound is
    aligned; with one pair a row beyond it the alignment call is refused whole, and the score call
    still answers both (tests/test_gpu_score_semi_batch.py checks its values)."""
    go, ge = -11, -1
    sub = np.where(np.eye(20, dtype=bool), 32755, -4).astype(np.int64)
    x = sb.seq(2100, 61)
    ok, both = sb.Batch("b26ok", sub), sb.Batch("b26", sub)
    for R in (2048, 2049):
        q = F.mutate_seq(hdr(x[11:11 + R + 40]), 62)[1:R + 1]
        B = sp.exact_for(R, 2100, sub, go, ge)
        assert (B < (1 << 26)) == (R == 2048) and abs(B - (1 << 26)) < 40000
        both.add(R, hdr(q), x)
        if R == 2048:
            ok.add(R, hdr(q), x)
            ok.add("small", *sb.related(100, 300, 63))
    check_batch(engine, ok, go, ge, 1024, align=sp.align64)
    _refused(lambda: both.align(engine, go, ge))
    sc = both.score(engine, go, ge)
    assert sc == [(w[0], w[3], w[4]) for w in (both.want(k, go, ge, sp.align64)[0] for k in range(2))]


def test_int16_table_edges(engine, golden):
    """s - gapo - gape at -32767 and 32767 is aligned, at -32768 and 32768 refused."""
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
            check_batch(engine, b, go, ge, 1024, align=sp.align64)
        else:
            _refused(lambda: b.align(engine, go, ge))


# -- 6. around the call ---------------------------------------------------------------------------------


@pytest.fixture(scope="module")
def few(engine, golden):
    b = sb.Batch("few", golden.blosum62)
    b.add(0, *sb.related(700, 1650, 91))
    b.add(1, *sb.related(1100, 200, 93))
    b.add(2, sb.seq(30, 3), hdr([]))
    b.add(3, *sb.related(90, 1500, 95))
    return b


def _raw(engine, b, go=-11, ge=-1, mwg=0, limit=0, cap=1 << 16, npairs=None, null_out=False, null_cigar=False,
         null_pairs=False, null_subst=False, patch=None):
    ptrs = b.ptrs()
    n = len(ptrs) if npairs is None else npairs
    arr = (gsa.PairDev * len(ptrs))()
    for k, (yp, ar, xp, ac) in enumerate(ptrs):
        arr[k].seqY, arr[k].adjrows, arr[k].seqX, arr[k].adjcols = yp, ar, xp, ac
    if patch:
        patch(arr)
    res, info = (gsa.AlignDbResult * len(ptrs))(), gsa.AlignBatchSemiInfo()
    need, ms = ctypes.c_int64(-1), ctypes.c_float(0)
    buf = ctypes.create_string_buffer(max(cap, 1))
    sub, ssz = b.table()
    st = gsa.lib().gsa_align_batch_semi_dev(engine._h, n, None if null_pairs else arr, None if null_subst else sub, ssz,
                                            go, ge, mwg, limit, None if null_out else res, None if null_cigar else buf,
                                            cap, ctypes.byref(need), ctypes.byref(info), ctypes.byref(ms), None)
    return st, res, need.value, buf


def test_short_cigar_buffer(engine, few):
    cigs = [few.want(k, -11, -1)[0][5] for k in range(4)]
    total = sum(len(c) + 1 for c in cigs)
    offs = np.cumsum([0] + [len(c) + 1 for c in cigs])
    st, res, need, buf = _raw(engine, few, cap=total)
    assert st == 0 and need == total
    for k, c in enumerate(cigs):
        assert (res[k].status, res[k].cigar_off, res[k].cigar_len) == (0, offs[k], len(c))
        assert buf.raw[offs[k]:offs[k] + len(c) + 1] == c.encode() + b"\0"
    # room for the first two strings and all of the third but its NUL: the fourth does not fit either
    cap = int(offs[2]) + len(cigs[2])
    st, res, need, buf = _raw(engine, few, cap=cap)
    assert st == 0 and need == total
    assert [res[k].status for k in range(4)] == [0, 0, 2, 2]
    for k in (0, 1):
        assert (res[k].cigar_off, res[k].cigar_len) == (offs[k], len(cigs[k]))
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
        st = _raw(engine, few, **kw)[0]
        assert st == gsa.NwStat.errorInvalidValue, kw
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
    bad(null_out=True)
    bad(null_cigar=True, cap=16)
    st = gsa.lib().gsa_align_batch_semi_dev(engine._h, 1, (gsa.PairDev * 1)(), few.table()[0], 33, -11, -1, 0, 0,
                                            (gsa.AlignDbResult * 1)(), None, 0, None, None, None, None)
    assert st == gsa.NwStat.errorInvalidValue


@pytest.mark.parametrize("go,ge", [(-11, -1), (-4, -4)])
def test_other_calls_before_and_after(engine, few, go, ge):
    """score_semi_dev, align_pair_semi_dev, score_batch_dev and align_batch_dev give the same before and
    after the new calls, and gsa_last_launch's record is left as it was."""
    def others():
        p = few.pair(1)
        one = engine.align_pair_semi_dev(*p.args(), go, ge)
        sc = engine.score_batch_dev(few.ptrs(), *few.table(), go, ge, False)
        al = engine.align_batch_dev(few.ptrs(), *few.table(), go, ge, False)
        return (p.score(engine, go, ge), t6(one), [(r["score"], r["i_end"], r["j_end"]) for r in sc],
                [(r["status"], t6(r)) for r in al])

    before = others()
    record = engine.last_launch()
    res, _, _ = check_batch(engine, few, go, ge, 1024)
    assert engine.last_launch() == record
    assert others() == before
    assert t6(res[1]) == before[1]


def test_scratch_is_counted_in_mem_stats(engine, golden):
    e = gsa.Engine(0)
    try:
        b = sb.Batch("mem", golden.blosum62)
        b.add(0, *sb.related(600, 150000, 93))
        b.add(1, *sb.related(500, 100000, 94))
        e.reset_mem_stats()
        base = e.mem_stats()["glmem_peak_allocs"]
        sc = b.score(e, -11, -1)
        rows = e.mem_stats()["glmem_peak_allocs"]
        assert rows - base >= 4 * 250000 + 16 * 250000  # the row buffer and the checkpoint rows
        res, info = b.align(e, -11, -1)
        assert [(r["score"], r["i_end"], r["j_end"]) for r in res] == sc and info["code_bytes"] > 0
        # one ticket each: 16 bytes per subject column, the row's length rounded up to 16 words
        assert info["gran_bytes"] == 16 * (((150000 + 16) & ~15) + ((100000 + 16) & ~15))
        assert e.mem_stats()["glmem_peak_allocs"] >= rows + info["code_bytes"]
    finally:
        e.close()


def test_host_form_with_empty_sides(engine, golden, few):
    pairs = [(p.Y, p.X) for _, p in few.items] + [(hdr([]), few.pair(0).X), (hdr([]), hdr([]))]
    for go, ge in ((-11, -1), (-5, -2)):
        res = engine.align_batch_semi(pairs, golden.blosum62, go, ge)
        assert [r["status"] for r in res] == [0] * 6
        assert [t6(r) for r in res[:4]] == [few.want(k, go, ge)[0] for k in range(4)]
        assert t6(res[2]) == (go + 29 * ge, 0, 0, 30, 0, "30I")
        assert [t6(r) for r in res[4:]] == [(0, 0, 0, 0, 0, "")] * 2
        info = engine.last_align_batch_semi_info()
        assert info["batch_pairs"] == 3 and info["host_pairs"] == 3
    res = engine.align_batch_semi(pairs[:2], golden.blosum62, -4)
    assert [t6(r) for r in res] == [few.want(k, -4, -4)[0] for k in range(2)]
    res = engine.align_batch_semi(pairs[4:], golden.blosum62, -11, -1)  # nothing for the device
    assert [t6(r) for r in res] == [(0, 0, 0, 0, 0, "")] * 2
    assert engine.last_align_batch_semi_info()["strip_rows"] == 0
