"""The overlap (dovetail) alignment of one long pair (gsa_align_pair_overlap_dev: the K-rows score
kernel's overlap instances in one direction, then the strip fill with 4-bit move codes under a free row
0 and a free column 0 seeded from its checkpoint rows, and the walk that stops on either border,
nw_pair_overlap_trace.hip) against tests/_overlap_oracle.py, exactly: score, start cell,
end cell and CIGAR.  Every case also asserts the score call's result, the status and, from
gsa_align_pair_overlap_info, the strip height, the strips, the strips filled, the chunks and the code
bytes, all computed here along the oracle's path (tests/_overlap_pair.py), so that no case passes by
another route.  A strip is TR rows: 1024 for linear gaps, 512 for affine ones (GSA_SCORE_K = 2 / 4:
512 / 1024); a lane of the score kernel holds K = TR / 256 rows, a wave 64 K."""
import ctypes

import numpy as np
import pytest

import gpuseqalign_amd as gsa
from gpuseqalign_amd import formats as F
from tests import _overlap_oracle as oo
from tests._overlap_pair import GAPS, Pair, check, hdr, strip_rows, t6, want

pytestmark = pytest.mark.gpu

# 5 a match, -4 a mismatch: with parts over disjoint alphabets nothing but the planted part scores
ID20 = np.where(np.eye(20, dtype=bool), 5, -4)
STRICT = [(-11, -1), (-4, -4), (-5, -2)]  # the gap models under which a planted layout is the only optimum


def _seq(n, seed, alphabet=20):
    return F.synthetic_seq(n, seed, alphabet)


def _part(n, seed, lo, hi):
    """n letters of lo ... hi - 1, no header."""
    return _seq(n, seed, hi - lo)[1:] + lo


def dovetail(R, C, ov, seed):
    """Y's last ov letters, mutated, are X's first letters: the path starts on column 0 and ends on row R."""
    core = _seq(ov, seed)
    mut = F.mutate_seq(core, seed + 1)[1:]
    y = np.concatenate([_seq(max(R - ov, 0), seed + 2)[1:], core[1:]])[-R:]
    x = np.concatenate([mut, _seq(C, seed + 3)[1:]])[:C]
    return hdr(y), hdr(x)


def mirror(R, C, ov, seed):
    """X's last letters are Y's first ov letters, mutated: the path starts on row 0 and ends on column C."""
    x, y = dovetail(C, R, ov, seed)
    return y, x


def related(R, C, seed):
    kind = seed % 3
    if kind == 0:
        return dovetail(R, C, max(1, 2 * min(R, C) // 3), seed)
    if kind == 1:
        return mirror(R, C, max(1, 2 * min(R, C) // 3), seed)
    # the shorter one, mutated, inside the longer one
    if R <= C:
        x = _seq(C, seed)
        at = (C - R) // 2
        y = np.concatenate([F.mutate_seq(hdr(x[1 + at:1 + at + R]), seed + 1)[1:], _seq(R, seed + 2)[1:]])[:R]
        return hdr(y), x
    x, y = related(C, R, seed)
    return y, x


# -- 1. row and column edges --------------------------------------------------------------------------

_EDGE = {}
RC = [1, 65, 300]
# the column-0 blocks (0 .. 3) and the column-C blocks (C >> 4 .. (C + 63) >> 4) coincide or just separate;
# then either side of the hand-off ring (512) and of the profile ring (1024)
CE = [1, 2, 15, 16, 17, 47, 63, 64, 65, 79, 80, 300, 511, 512, 513, 1023, 1024, 1025, 2100]


def edge_shapes(tr):
    """Every row edge against C in {1, 65, 300}, every column edge against R in {9, TR + 1}: row R on
    every register row of a lane, on either side of a wave's strip (64 K rows), of a ticket and of two."""
    k = tr // 256
    rows = [1, 2, 3, 4, 5, 7, 8, 9, 64 * k - 1, 64 * k, 64 * k + 1, tr - 1, tr, tr + 1, 2 * tr, 2 * tr + 1, 3 * tr + 1]
    shapes = [(R, C) for R in rows for C in RC] + [(R, C) for C in CE for R in (9, tr + 1)]
    return sorted(set(shapes))


def edge_pair(kind, R, C, sub):
    k = (kind, R, C)
    if k not in _EDGE:
        Y, X = (_seq(R, 7 * R + C), _seq(C, 7 * R + C + 1)) if kind == "random" else related(R, C, 3 * R + C)
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


def test_int16_profile_alone(engine, golden, knobs):
    """One family under GSA_KROW_Q8 = 0: the int16 instances at 4 rows per lane."""
    knobs("GSA_KROW_Q8", 0)
    for R, C in edge_shapes(1024):
        check(engine, edge_pair("related", R, C, golden.blosum62), ("edge", "related", R, C), -4, -4)


# -- 2. planted dovetails -----------------------------------------------------------------------------

_PLANT = {}


def end_on_column_c(tr, e):
    """Y = core + junk, X = junk + core: the core's e letters end on (e, C), in the first of three tickets
    (in the second for e = TR + 1); C = 300, or e + 60 for a longer core."""
    R, C = 2 * tr + 50, max(300, e + 60)
    core = _part(e, 11 + e, 0, 12)
    return hdr(np.concatenate([core, _part(R - e, 12 + e, 16, 20)])), hdr(np.concatenate([_part(C - e, 13 + e, 12, 16), core]))


def start_on_column_0(tr, s):
    """Y = junk + core, X = core + junk: the path starts on (s, 0) and ends on row R = 2 TR + 50."""
    R = 2 * tr + 50
    core = _part(R - s, 21 + s, 0, 12)
    return hdr(np.concatenate([_part(s, 22 + s, 16, 20), core])), hdr(np.concatenate([core, _part(30, 23 + s, 12, 16)]))


def lane_rows(tr):
    """Rows on every register row of lane 0 and of lane 63 of the first wave, on either side of that
    wave's strip and of the first ticket."""
    k = tr // 256
    return sorted(set(list(range(1, k + 1)) + list(range(63 * k + 1, 64 * k + 2)) + [tr - 1, tr, tr + 1]))


@pytest.mark.parametrize("go,ge", GAPS)
def test_end_row_on_column_c(engine, go, ge):
    tr = strip_rows(go, ge)
    for e in lane_rows(tr):
        if ("endc", tr, e) not in _PLANT:
            _PLANT[("endc", tr, e)] = Pair(*end_on_column_c(tr, e), ID20)
        p = _PLANT[("endc", tr, e)]
        r, info = check(engine, p, ("endc", tr, e), go, ge)
        if (go, ge) in STRICT:
            assert t6(r) == (5 * e, 0, p.C - e, e, p.C, "%d=" % e), r
            assert info["strips"] == -(-e // tr) == info["strips_filled"]  # the strips below the end cell are left alone


@pytest.mark.parametrize("go,ge", GAPS)
def test_start_row_on_column_0(engine, go, ge):
    tr = strip_rows(go, ge)
    for s in lane_rows(tr):
        if ("start0", tr, s) not in _PLANT:
            _PLANT[("start0", tr, s)] = Pair(*start_on_column_0(tr, s), ID20)
        p = _PLANT[("start0", tr, s)]
        r, _ = check(engine, p, ("start0", tr, s), go, ge)
        if (go, ge) in STRICT:
            assert t6(r) == (5 * (p.R - s), s, 0, p.R, p.R - s, "%d=" % (p.R - s)), r


@pytest.mark.parametrize("go,ge", GAPS)
def test_corner_and_containments(engine, golden, go, ge):
    """The end at the corner (R, C) with a start on row 0 and with a start on column 0; Y within X and X
    within Y, mutated, under blosum62."""
    if "corner0" not in _PLANT:
        core = _part(200, 31, 0, 12)
        _PLANT["corner0"] = Pair(hdr(core), hdr(np.concatenate([_part(90, 32, 12, 16), core])), ID20)
        _PLANT["corner1"] = Pair(hdr(np.concatenate([_part(90, 33, 16, 20), core])), hdr(core), ID20)
        x = _seq(1400, 34)
        y = F.mutate_seq(hdr(x[301:901]), 35)
        _PLANT["yinx"] = Pair(y, x, golden.blosum62)
        _PLANT["xiny"] = Pair(x, y, golden.blosum62)
    r, _ = check(engine, _PLANT["corner0"], "corner0", go, ge)
    if (go, ge) in STRICT:
        assert t6(r) == (1000, 0, 90, 200, 290, "200=")
    r, _ = check(engine, _PLANT["corner1"], "corner1", go, ge)
    if (go, ge) in STRICT:
        assert t6(r) == (1000, 90, 0, 290, 200, "200=")
    r, _ = check(engine, _PLANT["yinx"], "yinx", go, ge)
    if (go, ge) in STRICT:
        assert (r["i_start"], r["i_end"]) == (0, _PLANT["yinx"].R) and 0 < r["j_start"] < r["j_end"] < 1400
    r, _ = check(engine, _PLANT["xiny"], "xiny", go, ge)
    if (go, ge) in STRICT:
        assert (r["j_start"], r["j_end"]) == (0, _PLANT["xiny"].C) and 0 < r["i_start"] < r["i_end"] < 1400


# -- 3. ties ------------------------------------------------------------------------------------------

_TIE = {}
UNIT = np.array([3, 7, 11, 2, 16])


@pytest.mark.parametrize("go,ge", GAPS)
def test_two_maxima_on_row_r_the_smaller_column_wins(engine, golden, go, ge):
    """8 units of 5 letters down the rows, 9 units in X: two end columns 5 apart attain the score, in
    one 16-column block, in two blocks, and on either side of column 512."""
    for a in (0, 18, 467):
        if ("row", a) not in _TIE:
            junk = (_seq(a + 60, 5 + a)[1:] % 3) + 17  # letters the unit does not use
            X = hdr(np.concatenate([junk[:a], np.tile(UNIT, 9), junk[a:]]))
            _TIE[("row", a)] = Pair(hdr(np.tile(UNIT, 8)), X, golden.blosum62)
        p = _TIE[("row", a)]
        H = oo.matrices(p.Y, p.X, p.subm, go, ge)[0]
        ends = np.nonzero(H[p.R] == H[p.R].max())[0]
        assert len(ends) >= 2 and ends[0] == a + 40 and a + 45 in ends and H[p.R].max() >= H[:, p.C].max(), ends
        r, _ = check(engine, p, ("tie-row", a), go, ge)
        assert (r["i_end"], r["j_end"]) == (p.R, a + 40)


@pytest.mark.parametrize("k", [2, 4])
@pytest.mark.parametrize("go,ge", [(-11, -1), (-4, -4), (-5, -2)])
def test_two_maxima_on_column_c_the_smaller_row_wins(engine, knobs, go, ge, k):
    """X is 8 times one letter and Y holds 9 of them behind `a` other letters: the rows a + 8 and a + 9 of
    column C both score 8 matches.  The two rows lie in one lane of the score kernel, in two lanes, in
    two waves' strips and in two tickets."""
    knobs("GSA_SCORE_K", k)
    tr = 256 * k
    for name, a in (("lane", 1), ("lanes", 4), ("waves", 64 * k - 8), ("tickets", tr - 8)):
        r0, r1 = a + 8, a + 9
        same_lane = (r0 - 1) // k == (r1 - 1) // k
        assert same_lane == (name == "lane")
        if name == "waves":
            assert (r0 - 1) // (64 * k) + 1 == (r1 - 1) // (64 * k)
        if name == "tickets":
            assert (r0 - 1) // tr + 1 == (r1 - 1) // tr
        if ("col", a) not in _TIE:
            Y = hdr(np.concatenate([_part(a, 41 + a, 12, 16), np.full(9, 5), _part(40, 42 + a, 16, 20)]))
            _TIE[("col", a)] = Pair(Y, hdr(np.full(8, 5)), ID20)
        p = _TIE[("col", a)]
        H = oo.matrices(p.Y, p.X, p.subm, go, ge)[0]
        assert H[r0, p.C] == H[r1, p.C] == 40 == H[:, p.C].max() > H[p.R].max()
        r, _ = check(engine, p, ("tie-col", a), go, ge, k=k)
        assert t6(r) == (40, a, 0, r0, 8, "8=")


@pytest.mark.parametrize("go,ge", GAPS)
def test_equal_maxima_on_row_r_and_on_column_c_row_r_wins(engine, go, ge):
    """Y = A + B, X = B + A with |A| = |B| = 40 and a constant match score: (R, 40) and (40, C) tie."""
    if "ab" not in _TIE:
        A, B = _part(40, 51, 0, 10), _part(40, 52, 10, 20)
        _TIE["ab"] = Pair(hdr(np.concatenate([A, B])), hdr(np.concatenate([B, A])), ID20)
    p = _TIE["ab"]
    if (go, ge) in STRICT:
        H = oo.matrices(p.Y, p.X, p.subm, go, ge)[0]
        assert H[80, 40] == H[40, 80] == 200 == H.max()
    r, _ = check(engine, p, "ab", go, ge)
    if (go, ge) in STRICT:
        assert t6(r) == (200, 40, 0, 80, 40, "40=")


@pytest.mark.parametrize("go,ge", GAPS)
def test_score_0_on_an_unrelated_pair(engine, go, ge):
    """Nothing in common: 0 at (R, 0), an empty CIGAR and no fill."""
    if "zero" not in _TIE:
        _TIE["zero"] = Pair(hdr(_part(700, 61, 0, 10)), hdr(_part(90, 62, 10, 20)), np.where(np.eye(20, dtype=bool), 5, -20))
    r, info = check(engine, _TIE["zero"], "zero", go, ge)
    if go < 0:
        assert t6(r) == (0, 700, 0, 700, 0, "") and info["chunks"] == 0 and info["strips_filled"] == 0


# -- 4. planted gaps ------------------------------------------------------------------------------------

_GAP = {}


def _plant(R, a, n, seed, inserted):
    """Y of R letters and an X that holds it between two flanks of 150 letters: with Y's rows a ... a + n
    - 1 removed (a vertical gap there), or with n letters inserted behind row a - 1 (a horizontal gap on
    row a - 1).  The gap's letters are a letter the rest does not use."""
    y = _seq(R, seed, 19)
    if not inserted:
        y = y.copy()
        y[a:a + n] = 19
        core = np.concatenate([y[1:a], y[a + n:]])
    else:
        core = np.concatenate([y[1:a], np.full(n, 19), y[a:]])
    return y, hdr(np.concatenate([_seq(150, seed + 1, 19)[1:], core, _seq(150, seed + 2, 19)[1:]]))


def _runs(cigar):
    num, out = "", []
    for ch in cigar:
        if ch.isdigit():
            num += ch
        else:
            out.append((num, ch))
            num = ""
    return out


@pytest.mark.parametrize("inserted", [False, True], ids=["removed", "inserted"])
@pytest.mark.parametrize("go,ge", GAPS)
def test_planted_gaps(engine, golden, go, ge, inserted):
    """A 1-letter and a 30-letter gap across a hand-off between two lanes of the fill (a lane holds 8
    rows at TR = 512, 16 at 1024: the hand-off 40 lanes down) and across the checkpoint row TR / TR + 1."""
    tr = strip_rows(go, ge)
    kr = tr // 64
    R = tr + 300
    for b in (40 * kr, tr):
        for n in (1, 30):
            a = b + 1 if inserted else b + 1 - (n + 1) // 2  # rows a ... a + n - 1 lie across the boundary b / b + 1
            k = (tr, b, n, inserted)
            if k not in _GAP:
                _GAP[k] = Pair(*_plant(R, a, n, 31 * b + n, inserted), golden.blosum62)
            p = _GAP[k]
            w, _ = want(("plant",) + k, p, go, ge)
            if (go, ge) in STRICT and not (go == ge and n == 30):
                op = "D" if inserted else "I"
                runs = [(int(c), o) for c, o in _runs(w[5]) if o in "ID"]
                assert runs == [(n, op)], (w[5], n, op)
            check(engine, p, ("plant",) + k, go, ge)


# -- 5. strips left alone, chunks ---------------------------------------------------------------------

_CH = {}


@pytest.mark.parametrize("go,ge", GAPS)
def test_strips_above_the_start_are_not_filled(engine, go, ge):
    """The path reaches column 0 on row 2 TR + 5, two strips below strip 0, of R = 3 TR + 100 rows: with
    a chunk per strip the two strips that hold it are filled and the two above are left alone; with the
    default limit all four fit one chunk and are filled in one launch."""
    tr = strip_rows(go, ge)
    if ("top", tr) not in _CH:
        s, R = 2 * tr + 5, 3 * tr + 100
        core = _part(R - s, 71, 0, 12)
        _CH[("top", tr)] = Pair(hdr(np.concatenate([_part(s, 72, 16, 20), core])),
                                hdr(np.concatenate([core, _part(40, 73, 12, 16)])), ID20)
    p = _CH[("top", tr)]
    one, info = check(engine, p, ("top", tr), go, ge)
    if (go, ge) in STRICT:
        assert (one["i_start"], one["j_start"]) == (2 * tr + 5, 0) and (info["strips"], info["strips_filled"]) == (4, 4)
    strip = one["j_end"] * tr // 2
    r, info = check(engine, p, ("top", tr), go, ge, limit=strip)
    assert t6(r) == t6(one)
    if (go, ge) in STRICT:
        assert (info["strips"], info["strips_filled"], info["chunks"]) == (4, 2, 2), info


@pytest.mark.parametrize("go,ge", GAPS)
def test_chunks(engine, golden, go, ge):
    """R = 3 TR + 1, Y within X: a limit of exactly one strip's codes gives a chunk per strip (at least
    three) and the default run's result; a byte less is errorInvalidValue."""
    tr = strip_rows(go, ge)
    if tr not in _CH:
        x = _seq(3 * tr + 700, 17)
        _CH[tr] = Pair(F.mutate_seq(hdr(x[301:301 + 3 * tr + 60]), 18)[:3 * tr + 2], x, golden.blosum62)
    p = _CH[tr]
    assert p.R == 3 * tr + 1
    one, info1 = check(engine, p, ("chunks", tr), go, ge)
    strip = one["j_end"] * tr // 2
    r, info = check(engine, p, ("chunks", tr), go, ge, limit=strip)
    assert t6(r) == t6(one) and info["chunks"] >= 3 and info["code_bytes"] == strip, info
    r, info = check(engine, p, ("chunks", tr), go, ge, limit=2 * strip + 1)
    assert t6(r) == t6(one) and info["chunks"] >= 2 and info["code_bytes"] <= 2 * strip + 1, info
    with pytest.raises(gsa.NwError) as ei:
        p.align(engine, go, ge, strip - 1)
    assert ei.value.stat == gsa.NwStat.errorInvalidValue
    check(engine, p, ("chunks", tr), go, ge)


# -- 6. tables ----------------------------------------------------------------------------------------


@pytest.mark.parametrize("go,ge", GAPS)
def test_tables(engine, golden, go, ge):
    Y, X = dovetail(700, 1300, 450, 41)
    rng = np.random.default_rng(5)
    asym = rng.integers(-6, 9, (20, 20))
    assert (asym != asym.T).any()
    check(engine, Pair(Y, X, asym), "asym", go, ge)  # row = Y's letter
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
    """The fill keeps 4 x value + source: B < 2^26.  The largest table value that passes the int16 test is
    32767 + gapo + gape, so the smallest shape on the bound has 2048 rows; one row more is refused by
    the alignment call, and the score call still answers."""
    go, ge = -11, -1
    sub = np.where(np.eye(20, dtype=bool), 32755, -4).astype(np.int64)
    C = 2100
    x = _seq(C, 61)
    for R, ok in ((2048, True), (2049, False)):
        q = F.mutate_seq(hdr(x[1:R + 41]), 62)[1:R + 1]  # Y's tail on X's head, and more
        assert len(q) == R
        p = Pair(hdr(np.concatenate([_seq(30, 63)[1:], q])[-R:]), x, sub)
        B = oo.exact_for(R, C, sub, go, ge)
        assert (B < (1 << 26)) == ok and abs(B - (1 << 26)) < 40000
        if ok:
            check(engine, p, ("b26", R), go, ge, align=oo.align64)
        else:
            _refused(lambda: p.align(engine, go, ge))
            w = oo.align64(p.Y, p.X, sub, go, ge)
            assert p.score(engine, go, ge) == (w[0], w[3], w[4])


def test_alignment_at_the_int16_table_edges(engine, golden):
    """s - gapo - gape at -32767 and 32767 is aligned, at -32768 and 32768 refused."""
    go, ge = -11, -1
    Y, X = dovetail(120, 260, 90, 43)
    base = np.asarray(golden.blosum62).reshape(25, 25).astype(np.int64)
    for v, ok in ((-32767, True), (-32768, False), (32767, True), (32768, False)):
        sub = base.copy()
        a, b = (int(Y[5]), int(X[70])) if v < 0 else (int(Y[100]), int(Y[100]))
        sub[a, b] = v + go + ge
        p = Pair(Y, X, sub)
        if ok:
            check(engine, p, ("i16", v), go, ge, align=oo.align64)
        else:
            _refused(lambda: p.align(engine, go, ge))
            _refused(lambda: p.score(engine, go, ge))


# -- 8. around the call -------------------------------------------------------------------------------


def _raw(engine, p, go=-11, ge=-1, limit=0, cap=4096, null_out=False, null_cigar=False, null_y=False, null_info=False):
    res, info = gsa.AlignDbResult(), gsa.AlignPairOverlapInfo()
    need, ms = ctypes.c_int64(-1), ctypes.c_float(0)
    buf = ctypes.create_string_buffer(max(cap, 1))
    st = gsa.lib().gsa_align_pair_overlap_dev(engine._h, None if null_y else p.y.data_ptr(), p.y.numel(), p.x.data_ptr(),
                                              p.x.numel(), p.sub.data_ptr(), p.substsz, go, ge, limit,
                                              None if null_out else ctypes.byref(res), None if null_cigar else buf, cap,
                                              ctypes.byref(need), None if null_info else ctypes.byref(info),
                                              None if null_info else ctypes.byref(ms), None)
    return st, res, need.value, buf


@pytest.fixture(scope="module")
def small(engine, golden):
    return Pair(*dovetail(600, 1500, 420, 91), golden.blosum62)


def test_short_cigar_buffer_and_null_info(engine, small):
    w, _ = want("small", small, -11, -1)
    n = len(w[5])
    assert n > 3
    st, res, need, _ = _raw(engine, small, cap=n)
    assert st == 0 and res.status == 2 and need == n + 1
    assert (res.score, res.i_start, res.j_start, res.i_end, res.j_end) == w[:5]
    st, res, need, buf = _raw(engine, small, cap=need)
    assert st == 0 and res.status == 0 and need == n + 1 and res.cigar_off == 0 and res.cigar_len == n
    assert buf.raw[:n + 1] == w[5].encode() + b"\0"
    st, res, need, _ = _raw(engine, small, cap=0, null_cigar=True)
    assert st == 0 and res.status == 2 and need == n + 1
    st, res, need, buf = _raw(engine, small, null_info=True)  # null info and null kernel_ms
    assert st == 0 and res.status == 0 and buf.raw[:n + 1] == w[5].encode() + b"\0"


@pytest.mark.parametrize("go,ge", [(-11, -1), (-4, -4)])
def test_neighbours_keep_their_results(engine, small, go, ge):
    """score_dev and align_pair_dev in a global and a local mode, score_semi_dev and align_pair_semi_dev
    right before and after the overlap calls; gsa_last_launch's record is left as it was."""
    p = small

    def others():
        out = []
        for local in (False, True):
            s = engine.score_dev(*p.args(), go, ge, local)
            a = engine.align_pair_dev(*p.args(), go, ge, local)
            out.append(((s["score"], s["i_end"], s["j_end"]), t6(a), a["status"]))
        s = engine.score_semi_dev(*p.args(), go, ge)
        a = engine.align_pair_semi_dev(*p.args(), go, ge)
        out.append(((s["score"], s["i_end"], s["j_end"]), t6(a), a["status"], engine.last_align_pair_semi_info()["chunks"]))
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
        p = Pair(*mirror(150000, 600, 400, 93), golden.blosum62)
        e.reset_mem_stats()
        base = e.mem_stats()["glmem_peak_allocs"]
        s = e.score_overlap_dev(*p.args(), -11, -1)
        col = e.mem_stats()["glmem_peak_allocs"]
        assert col - base >= 4 * (p.R + 1)  # the column buffer (and the row buffer and the hand-off rows)
        r = e.align_pair_overlap_dev(*p.args(), -11, -1)
        info = e.last_align_pair_overlap_info()
        assert (r["score"], r["i_end"], r["j_end"]) == (s["score"], s["i_end"], s["j_end"])
        assert info["chunks"] >= 1 and e.mem_stats()["glmem_peak_allocs"] >= col + info["code_bytes"] > col
    finally:
        e.close()


def test_host_form_and_empty_sides(engine, golden, small):
    for go, ge in [(-11, -1), (-5, -2)]:
        r = engine.align_pair_overlap(small.Y, small.X, golden.blosum62, go, ge)
        assert r["status"] == 0 and t6(r) == want("small", small, go, ge)[0]
    r = engine.align_pair_overlap(small.Y, small.X, golden.blosum62, -4)
    assert t6(r) == want("small", small, -4, -4)[0]
    r = engine.align_pair_overlap(small.Y, small.X[:1], golden.blosum62, -11, -1)  # C = 0
    assert r["status"] == 0 and t6(r) == (0, 600, 0, 600, 0, "") == oo.align(small.Y, small.X[:1], golden.blosum62, -11, -1)
    for X in (small.X, small.X[:1]):  # R = 0
        r = engine.align_pair_overlap(small.Y[:1], X, golden.blosum62, -11, -1)
        assert r["status"] == 0 and t6(r) == (0, 0, 0, 0, 0, "") == oo.align(small.Y[:1], X, golden.blosum62, -11, -1)
    assert engine.last_align_pair_overlap_info()["chunks"] == 0


def test_invalid_input(engine, small):
    p = small
    _refused(lambda: p.align(engine, -1, -11))             # go > ge
    _refused(lambda: p.align(engine, -11, 1))              # ge > 0
    _refused(lambda: p.align(engine, -2000010, -2000000))  # outside the value range
    _refused(lambda: p.align(engine, -11, -1, limit=-1))   # negative scratch_limit
    for kw in (dict(cap=-1), dict(null_out=True), dict(null_cigar=True, cap=16), dict(null_y=True)):
        _refused(lambda: engine._check(_raw(engine, p, **kw)[0], "gsa_align_pair_overlap_dev"))
    _refused(lambda: engine.align_pair_overlap_dev(p.y.data_ptr(), 0, p.x.data_ptr(), p.x.numel(), p.sub.data_ptr(),
                                                   p.substsz, -11, -1))
    _refused(lambda: engine.align_pair_overlap_dev(p.y.data_ptr(), p.y.numel(), p.x.data_ptr(), p.x.numel(),
                                                   p.sub.data_ptr(), 33, -11, -1))
    check(engine, p, "small", -11, -1)


def test_agreement_with_the_semi_global_call_on_containments(engine, golden):
    """Y planted whole inside X, between flanks the table scores against: on 8 shapes the overlap result
    is align_pair_semi's field for field."""
    for n, (R, C) in enumerate([(1, 40), (9, 300), (64, 165), (129, 2000), (300, 700), (513, 900), (700, 1990), (1025, 1500)]):
        at = (C - R) // 2
        core = _part(R, 200 + n, 0, 12)
        Y = hdr(core)
        X = hdr(np.concatenate([_part(at, 300 + n, 12, 16), core, _part(C - R - at, 400 + n, 16, 20)]))
        for go, ge in ((-11, -1), (-4, -4)):
            r = engine.align_pair_overlap(Y, X, ID20, go, ge)
            s = engine.align_pair_semi(Y, X, ID20, go, ge)
            assert t6(r) == t6(s) == (5 * R, 0, at, R, at + R, "%d=" % R), (R, C, go, ge, r, s)


def test_swapping_the_sequences_and_transposing_the_table(engine, golden):
    rng = np.random.default_rng(7)
    asym = rng.integers(-6, 9, (20, 20))
    for n, (R, C) in enumerate([(9, 300), (300, 513), (700, 90), (1025, 1500)]):
        Y, X = related(R, C, 500 + n)
        for go, ge in ((-11, -1), (-4, -4)):
            a = engine.score_overlap(Y, X, asym, go, ge)
            b = engine.score_overlap(X, Y, asym.T.copy(), go, ge)
            assert a["score"] == b["score"] == oo.score(Y, X, asym, go, ge)[0]
