"""The semi-global alignment of one long pair (gsa_align_pair_semi_dev: the K-rows score kernel's
semi-global instance in one direction, then the strip fill with 4-bit move codes over a column window
seeded from its checkpoint rows, and the walk that stops in row 0, nw_pair_semi_trace.hip; DESIGN.md
2.2k) against tests/_semi_oracle.py, exactly: score, start cell, end cell and CIGAR.  Every case also
asserts the score call's result, the status and, from gsa_align_pair_semi_info, the strip height, the
strips, the strips filled, the chunks, the code bytes and the window, all computed here along the
oracle's path (tests/_semi_pair.py), so that no case passes by another route.  A strip is TR rows:
1024 for linear gaps, 512 for affine ones (GSA_SCORE_K = 2 / 4: 512 / 1024); a lane holds TR / 64."""
import ctypes

import numpy as np
import pytest

import gpuseqalign_amd as gsa
from gpuseqalign_amd import formats as F
from tests import _semi_oracle as so
from tests import _semi_pair as sp
from tests._semi_pair import GAPS, Pair, check, hdr, strip_rows, t6, want

pytestmark = pytest.mark.gpu


def _seq(n, seed, alphabet=20):
    return F.synthetic_seq(n, seed, alphabet)


def _related(R, C, seed):
    """A query of R letters, a mutated stretch of the subject (C letters) from its middle, cut or
    padded with random letters."""
    x = _seq(C, seed)
    at = max(0, (C - R) // 2)
    mut = F.mutate_seq(hdr(x[1 + at:1 + at + R]), seed + 1)[1:]
    mut = np.concatenate([mut, _seq(R, seed + 2)[1:]])[:R]
    return hdr(mut), x


# -- 1. row and column edges --------------------------------------------------------------------------

_EDGE = {}
RC = [1, 65, 300]
CE = [1, 15, 16, 17, 63, 64, 65, 300, 511, 512, 513, 1023, 1024, 1025, 2100]


def edge_shapes(tr):
    """Every row edge against C in {1, 65, 300}, every column edge against R in {9, TR + 1}: row R on
    every register row of a lane, on either side of a strip of the score kernel (64 K rows), of a
    ticket and its checkpoint row; columns on either side of a block, the wave, the hand-off ring
    (512) and the profile ring (1024)."""
    k = tr // 256
    rows = [1, 2, 3, 4, 5, 7, 8, 9, 64 * k - 1, 64 * k, 64 * k + 1, tr - 1, tr, tr + 1, 2 * tr, 2 * tr + 1, 3 * tr + 1]
    shapes = [(R, C) for R in rows for C in RC] + [(R, C) for C in CE for R in (9, tr + 1)]
    return sorted(set(shapes))


def edge_pair(kind, R, C, sub):
    k = (kind, R, C)
    if k not in _EDGE:
        Y, X = (_seq(R, 7 * R + C), _seq(C, 7 * R + C + 1)) if kind == "random" else _related(R, C, 3 * R + C)
        _EDGE[k] = Pair(Y, X, sub)
    return _EDGE[k]


@pytest.mark.parametrize("kind", ["random", "related"])
@pytest.mark.parametrize("go,ge", GAPS)
def test_row_and_column_edges(engine, golden, go, ge, kind):
    for R, C in edge_shapes(strip_rows(go, ge)):
        check(engine, edge_pair(kind, R, C, golden.blosum62), ("edge", kind, R, C), go, ge)


@pytest.mark.parametrize("k", [2, 4])
@pytest.mark.parametrize("go,ge", [(-11, -1), (-4, -4)])
def test_row_and_column_edges_forced_k(engine, golden, knobs, go, ge, k):
    """Each gap family on the other geometry too."""
    knobs("GSA_SCORE_K", k)
    for R, C in edge_shapes(256 * k):
        check(engine, edge_pair("related", R, C, golden.blosum62), ("edge", "related", R, C), go, ge, k=k)


# -- 2. end column and ties ---------------------------------------------------------------------------

_END = {}


@pytest.mark.parametrize("go,ge", GAPS)
def test_query_planted_twice_the_smaller_end_wins(engine, golden, go, ge):
    """A periodic query of 8 units of 5 letters in a subject that holds 9 units: two end columns 5
    apart attain the score.  The two ends lie in one 16-column block, in two blocks, and on either
    side of column 512."""
    unit = np.array([3, 7, 11, 2, 16])
    for a in (0, 18, 467):
        if a not in _END:
            junk = (_seq(a + 60, 5 + a)[1:] % 3) + 17  # letters the unit does not use
            X = hdr(np.concatenate([junk[:a], np.tile(unit, 9), junk[a:]]))
            _END[a] = Pair(hdr(np.tile(unit, 8)), X, golden.blosum62)
        p = _END[a]
        H = so.matrices(p.Y, p.X, p.subm, go, ge)[0]
        ends = np.nonzero(H[p.R] == H[p.R].max())[0]
        assert len(ends) >= 2 and ends[0] == a + 40 and a + 45 in ends, ends
        if a == 0:
            assert ends[0] // 16 == (a + 45) // 16
        if a == 467:
            assert ends[0] < 512 <= a + 45
        r, _ = check(engine, p, ("twice", a), go, ge)
        assert r["j_end"] == a + 40


@pytest.mark.parametrize("go,ge", GAPS)
def test_all_negative_table_ends_on_column_0(engine, go, ge):
    """R > C, unrelated, every table value below every gap cost: the all-insert alignment on column 0 is
    the best."""
    if "neg" not in _END:
        _END["neg"] = Pair(_seq(700, 3, 4), _seq(90, 4, 4), np.full((4, 4), -20))
    r, info = check(engine, _END["neg"], "neg", go, ge)
    assert (r["j_end"], r["j_start"], r["cigar"]) == (0, 0, "700I") and info["chunks"] == 0
    assert r["score"] == go + 699 * ge


@pytest.mark.parametrize("go,ge", GAPS)
def test_negative_score_and_leading_inserts(engine, golden, go, ge):
    if "low" not in _END:
        sub = np.where(np.eye(20, dtype=bool), 1, -5)
        _END["low"] = Pair(_seq(50, 11), _seq(60, 12), sub)
        x = _seq(400, 13, 19)
        # ten letters the subject does not hold, then the subject's head: the path reaches column 0 first
        _END["lead"] = Pair(hdr(np.concatenate([np.full(10, 19), x[1:201]])), x, golden.blosum62)
    r, _ = check(engine, _END["low"], "low", go, ge)
    if go < 0:
        assert r["score"] < 0
    r, _ = check(engine, _END["lead"], "lead", go, ge)
    if ge < 0:
        assert r["cigar"].startswith("10I") and r["j_start"] == 0


# -- 3. planted gaps ------------------------------------------------------------------------------------

_PLANT = {}


def _plant(R, a, n, seed, inserted):
    """A query of R letters and a subject that holds it between two flanks of 150 letters: with the
    query's rows a ... a + n - 1 removed (a vertical gap there), or with n letters inserted behind row
    a - 1 (a horizontal gap on row a - 1).  The gap's letters are a letter the rest does not use."""
    y = _seq(R, seed, 19)
    if not inserted:
        y = y.copy()
        y[a:a + n] = 19
        core = np.concatenate([y[1:a], y[a + n:]])
    else:
        core = np.concatenate([y[1:a], np.full(n, 19), y[a:]])
    return y, hdr(np.concatenate([_seq(150, seed + 1, 19)[1:], core, _seq(150, seed + 2, 19)[1:]]))


@pytest.mark.parametrize("inserted", [False, True], ids=["removed", "inserted"])
@pytest.mark.parametrize("go,ge", GAPS)
def test_planted_gaps(engine, golden, go, ge, inserted):
    """A 1-letter and a 30-letter gap across a hand-off between two lanes of the fill (a lane holds 8
    rows at TR = 512, 16 at 1024: the hand-off 40 lanes down, deep enough for the gap to pay) and
    across the checkpoint row TR / TR + 1.  A vertical gap takes the rows on both sides of the
    boundary, a horizontal one lies between its two rows."""
    tr = strip_rows(go, ge)
    kr = tr // 64
    R = tr + 300
    for b in (40 * kr, tr):
        for n in (1, 30):
            a = b + 1 if inserted else b + 1 - (n + 1) // 2  # rows a ... a + n - 1 lie across the boundary b / b + 1
            k = (tr, b, n, inserted)
            if k not in _PLANT:
                _PLANT[k] = Pair(*_plant(R, a, n, 31 * b + n, inserted), golden.blosum62)
            p = _PLANT[k]
            w, _ = want(("plant",) + k, p, go, ge)
            if (go, ge) in ((-11, -1), (-4, -4), (-5, -2)) and not (go == ge and n == 30):
                # the oracle places the one gap where it was planted (30 letters at -4 each may split)
                op = "D" if inserted else "I"
                runs = [(int(c), o) for c, o in _runs(w[5]) if o in "ID"]
                assert runs == [(n, op)], (w[5], n, op)
                assert a <= b + 1 <= a + n
            check(engine, p, ("plant",) + k, go, ge)


def _runs(cigar):
    num, out = "", []
    for ch in cigar:
        if ch.isdigit():
            num += ch
        else:
            out.append((num, ch))
            num = ""
    return out


# -- 4. the column window -----------------------------------------------------------------------------

_WIN = {}


@pytest.mark.parametrize("go,ge", GAPS)
def test_window_of_a_planted_query(engine, golden, go, ge):
    """A 300-letter query planted, mutated, at the offsets 0, 1, 700 and C - 300 of a 6000-letter
    subject: j_window is the header's formula and code_bytes the windowed size (check() asserts both);
    with a gap extension cost the window cuts the codes of the far offset."""
    C = 6000
    for at in (0, 1, 700, C - 300):
        if at not in _WIN:
            x = _seq(C, 77)
            if at == C - 300:  # the query ends with the subject's last letters
                q = F.mutate_seq(hdr(x[C - 329:C - 2]), 78 + at)[1:]
                q = np.concatenate([q, x[C - 2:C + 1]])[-300:]
            else:
                q = F.mutate_seq(hdr(x[1 + at:1 + at + 330]), 78 + at)[1:301]
            assert len(q) == 300
            _WIN[at] = Pair(hdr(q), x, golden.blosum62)
        p = _WIN[at]
        r, info = check(engine, p, ("win", at), go, ge)
        tr = strip_rows(go, ge)
        assert info["code_bytes"] == (r["j_end"] - info["j_window"]) * tr // 2
        if at == C - 300 and go < 0:
            assert r["j_end"] == C
        if ge < 0 and at == C - 300:
            # j_start > 0 with no 'D' in front; the window cuts the codes (with blosum62 a match scores
            # about half of pmax, so dmax is a few thousand and only the far offset has jW > 0)
            assert r["j_start"] > info["j_window"] > 0 and _runs(r["cigar"])[0][1] != "D", (r, info)
            assert info["code_bytes"] < r["j_end"] * tr // 2
        if ge == 0:
            assert info["j_window"] == 0


@pytest.mark.parametrize("go,ge", GAPS)
def test_window_unrelated_and_low_complexity(engine, golden, go, ge):
    """An unrelated pair: the score is low, dmax large and the window opens to column 0.  A
    low-complexity pair (2 letters, R = 600, C = 3000), where ties abound."""
    if "unrel" not in _WIN:
        _WIN["unrel"] = Pair(_seq(200, 21), _seq(1500, 22), golden.blosum62)
        _WIN["lowc"] = Pair(_seq(600, 23, 2), _seq(3000, 24, 2), np.array([[2, -3], [-3, 2]]))
    _, info = check(engine, _WIN["unrel"], "unrel", go, ge)
    if ge > -4:  # (at -4 a letter dmax is about 500 and a window remains; check() asserts its formula)
        assert info["j_window"] == 0
    check(engine, _WIN["lowc"], "lowc", go, ge)


# -- 5. chunks ----------------------------------------------------------------------------------------

_CH = {}


@pytest.mark.parametrize("go,ge", GAPS)
def test_chunks(engine, golden, go, ge):
    """R = 3 TR + 1: a limit of exactly one strip's windowed codes gives a chunk per strip (at least
    three) and the default run's result; a byte less is errorInvalidValue."""
    tr = strip_rows(go, ge)
    if tr not in _CH:
        _CH[tr] = Pair(*_related(3 * tr + 1, 3 * tr + 700, 17), golden.blosum62)
    p = _CH[tr]
    one, info1 = check(engine, p, ("chunks", tr), go, ge)
    strip = (one["j_end"] - info1["j_window"]) * tr // 2
    r, info = check(engine, p, ("chunks", tr), go, ge, limit=strip)
    assert t6(r) == t6(one) and info["chunks"] >= 3 and info["strips_filled"] == 4, info
    assert info["code_bytes"] == strip
    r, info = check(engine, p, ("chunks", tr), go, ge, limit=2 * strip + 1)
    assert t6(r) == t6(one) and info["chunks"] >= 2 and info["code_bytes"] <= 2 * strip + 1, info
    with pytest.raises(gsa.NwError) as ei:
        p.align(engine, go, ge, strip - 1)
    assert ei.value.stat == gsa.NwStat.errorInvalidValue
    check(engine, p, ("chunks", tr), go, ge)


# -- 6. tables ----------------------------------------------------------------------------------------


@pytest.mark.parametrize("go,ge", GAPS)
def test_tables(engine, golden, go, ge):
    Y, X = _related(700, 1300, 41)
    rng = np.random.default_rng(5)
    asym = rng.integers(-6, 9, (20, 20))
    assert (asym != asym.T).any()
    check(engine, Pair(Y, X, asym), "asym", go, ge)  # row = the query's letter
    # outside int8 after the shift: at 4 rows per lane the int16 instance runs behind the declining int8 one
    wide = np.asarray(golden.blosum62).reshape(25, 25).copy()
    wide[np.diag_indices_from(wide)] = 300
    check(engine, Pair(Y, X, wide), "wide", go, ge)
    four = np.where(np.eye(4, dtype=bool), 5, -4)
    check(engine, Pair(hdr(Y[1:] % 4), hdr(X[1:] % 4), four), "four", go, ge)


# -- 7. value ranges ----------------------------------------------------------------------------------


def _refused(call):
    with pytest.raises(gsa.NwError) as ei:
        call()
    assert ei.value.stat == gsa.NwStat.errorInvalidValue


def test_alignment_value_bound_2_pow_26(engine):
    """The fill keeps 4 x value + source: B < 2^26.  The largest table value that passes the int16
    test is 32767 + gapo + gape, so the smallest shape on the bound has 2048 query letters; one row
    more is refused by the alignment call, and the score call still answers."""
    go, ge = -11, -1
    sub = np.where(np.eye(20, dtype=bool), 32755, -4).astype(np.int64)
    C = 2100
    x = _seq(C, 61)
    for R, ok in ((2048, True), (2049, False)):
        q = F.mutate_seq(hdr(x[11:11 + R + 40]), 62)[1:R + 1]
        assert len(q) == R
        p = Pair(hdr(q), x, sub)
        B = sp.exact_for(R, C, sub, go, ge)
        assert (B < (1 << 26)) == ok and abs(B - (1 << 26)) < 40000
        if ok:
            check(engine, p, ("b26", R), go, ge, align=sp.align64)
        else:
            _refused(lambda: p.align(engine, go, ge))
            w = sp.align64(p.Y, p.X, sub, go, ge)
            assert p.score(engine, go, ge) == (w[0], w[3], w[4])


def test_alignment_at_the_int16_table_edges(engine, golden):
    """s - gapo - gape at -32767 and 32767 is aligned, at -32768 and 32768 refused."""
    go, ge = -11, -1
    Y, X = _related(120, 260, 43)
    base = np.asarray(golden.blosum62).reshape(25, 25).astype(np.int64)
    for v, ok in ((-32767, True), (-32768, False), (32767, True), (32768, False)):
        sub = base.copy()
        a, b = (int(Y[5]), int(X[70])) if v < 0 else (int(Y[9]), int(Y[9]))
        sub[a, b] = v + go + ge
        p = Pair(Y, X, sub)
        if ok:
            check(engine, p, ("i16", v), go, ge, align=sp.align64)
        else:
            _refused(lambda: p.align(engine, go, ge))
            _refused(lambda: p.score(engine, go, ge))


# -- 8. around the call -------------------------------------------------------------------------------


def _raw(engine, p, go=-11, ge=-1, limit=0, cap=4096, null_out=False, null_cigar=False, null_y=False):
    res, info = gsa.AlignDbResult(), gsa.AlignPairSemiInfo()
    need, ms = ctypes.c_int64(-1), ctypes.c_float(0)
    buf = ctypes.create_string_buffer(max(cap, 1))
    st = gsa.lib().gsa_align_pair_semi_dev(engine._h, None if null_y else p.y.data_ptr(), p.y.numel(), p.x.data_ptr(),
                                           p.x.numel(), p.sub.data_ptr(), p.substsz, go, ge, limit,
                                           None if null_out else ctypes.byref(res), None if null_cigar else buf, cap,
                                           ctypes.byref(need), ctypes.byref(info), ctypes.byref(ms), None)
    return st, res, need.value, buf


@pytest.fixture(scope="module")
def small(engine, golden):
    return Pair(*_related(600, 1500, 91), golden.blosum62)


def test_short_cigar_buffer(engine, small):
    w, _ = want("small", small, -11, -1)
    n = len(w[5])
    st, res, need, _ = _raw(engine, small, cap=n)
    assert st == 0 and res.status == 2 and need == n + 1
    assert (res.score, res.i_start, res.j_start, res.i_end, res.j_end) == w[:5]
    st, res, need, buf = _raw(engine, small, cap=need)
    assert st == 0 and res.status == 0 and need == n + 1 and res.cigar_off == 0 and res.cigar_len == n
    assert buf.raw[:n + 1] == w[5].encode() + b"\0"
    st, res, need, _ = _raw(engine, small, cap=0, null_cigar=True)
    assert st == 0 and res.status == 2 and need == n + 1


@pytest.mark.parametrize("go,ge", [(-11, -1), (-4, -4)])
def test_neighbours_keep_their_results(engine, small, go, ge):
    """score_dev and align_pair_dev in a global and a local mode right before and after the semi
    calls; gsa_last_launch's record is left as it was."""
    p = small

    def others():
        out = []
        for local in (False, True):
            s = engine.score_dev(*p.args(), go, ge, local)
            a = engine.align_pair_dev(*p.args(), go, ge, local)
            out.append(((s["score"], s["i_end"], s["j_end"]), t6(a), a["status"]))
        return out

    before = others()
    record = engine.last_launch()
    check(engine, p, "small", go, ge)
    assert engine.last_launch() == record
    assert others() == before
    check(engine, p, "small", go, ge)


def test_scratch_is_counted_in_mem_stats(engine, golden):
    e = gsa.Engine(0)
    try:
        p = Pair(*_related(600, 200000, 93), golden.blosum62)
        e.reset_mem_stats()
        base = e.mem_stats()["glmem_peak_allocs"]
        s = e.score_semi_dev(*p.args(), -11, -1)
        row = e.mem_stats()["glmem_peak_allocs"]
        assert row - base >= 4 * (p.C + 1)  # the row buffer (and the hand-off rows)
        r = e.align_pair_semi_dev(*p.args(), -11, -1)
        info = e.last_align_pair_semi_info()
        assert (r["score"], r["j_end"]) == (s["score"], s["j_end"])
        assert e.mem_stats()["glmem_peak_allocs"] >= row + info["code_bytes"] > row
    finally:
        e.close()


def test_host_form_and_empty_sides(engine, golden, small):
    for go, ge in [(-11, -1), (-5, -2)]:
        r = engine.align_pair_semi(small.Y, small.X, golden.blosum62, go, ge)
        assert r["status"] == 0 and t6(r) == want("small", small, go, ge)[0]
    r = engine.align_pair_semi(small.Y, small.X, golden.blosum62, -4)
    assert t6(r) == want("small", small, -4, -4)[0]
    r = engine.align_pair_semi(small.Y, small.X[:1], golden.blosum62, -11, -1)  # an empty subject
    assert r["status"] == 0 and t6(r) == (-11 - 599, 0, 0, 600, 0, "600I")
    for X in (small.X, small.X[:1]):  # an empty query
        r = engine.align_pair_semi(small.Y[:1], X, golden.blosum62, -11, -1)
        assert r["status"] == 0 and t6(r) == (0, 0, 0, 0, 0, "")


def test_invalid_input(engine, small):
    p = small
    _refused(lambda: p.align(engine, -1, -11))             # go > ge
    _refused(lambda: p.align(engine, -11, 1))              # ge > 0
    _refused(lambda: p.align(engine, -2000010, -2000000))  # outside the value range
    _refused(lambda: p.align(engine, -11, -1, limit=-1))   # negative scratch_limit
    for kw in (dict(cap=-1), dict(null_out=True), dict(null_cigar=True, cap=16), dict(null_y=True)):
        _refused(lambda: engine._check(_raw(engine, p, **kw)[0], "gsa_align_pair_semi_dev"))
    _refused(lambda: engine.align_pair_semi_dev(p.y.data_ptr(), 0, p.x.data_ptr(), p.x.numel(), p.sub.data_ptr(),
                                                p.substsz, -11, -1))
    _refused(lambda: engine.align_pair_semi_dev(p.y.data_ptr(), p.y.numel(), p.x.data_ptr(), p.x.numel(),
                                                p.sub.data_ptr(), 33, -11, -1))
    check(engine, p, "small", -11, -1)


def test_agreement_with_the_database_search(engine, golden):
    """On shapes both take (C <= 2000, B < 2^18) score_db_semi and align_db_semi return the same score,
    cells and CIGAR."""
    for n, (R, C) in enumerate([(1, 1), (9, 300), (64, 65), (129, 2000), (300, 300), (513, 700), (700, 90), (1025, 1500)]):
        Y, X = _related(R, C, 200 + n)
        for go, ge in ((-11, -1), (-4, -4)):
            assert sp.value_bound(R, C, golden.blosum62, go, ge) < (1 << 18)
            r = engine.align_pair_semi(Y, X, golden.blosum62, go, ge)
            db = engine.align_db_semi([Y], [X], [0], [0], golden.blosum62, go, ge)[0]
            assert t6(r) == t6(db), (R, C, go, ge, r, db)
            hit = engine.score_db_semi([Y], [X], golden.blosum62, go, ge)
            assert int(np.asarray(hit["scores"]).ravel()[0]) == r["score"]
