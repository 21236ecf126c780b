"""The overlap (dovetail) score of one long pair (gsa_score_overlap_dev: the K-rows score kernel's
overlap instances -- a free row 0 and a free column 0, row R captured over every column and column C
over every row, and the small kernel that takes the first maximum over both) against
tests/_overlap_oracle.py: score and end cell.  The inputs at the value-range guards go against the
oracle's int64 fill.  tests/test_gpu_align_pair_overlap.py checks the score call again in every one of
its cases."""
import numpy as np
import pytest

import gpuseqalign_amd as gsa
from tests import _overlap_oracle as oo
from tests import _overlap_pair as op
from tests._overlap_pair import GAPS, Pair, hdr, want
from tests.test_gpu_align_pair_overlap import ID20, _part, _seq, dovetail, edge_pair, edge_shapes, mirror, related

pytestmark = pytest.mark.gpu


def _score(engine, p, key, go, ge, align=oo.align):
    w, _ = want(key, p, go, ge, align)
    got = p.score(engine, go, ge)
    assert got == (w[0], w[3], w[4]), (key, go, ge, p.R, p.C, got, w[:5])
    return got


@pytest.mark.parametrize("k", [None, 2, 4])
@pytest.mark.parametrize("go,ge", GAPS)
def test_row_and_column_edges(engine, golden, knobs, go, ge, k):
    """The alignment tests' edge shapes on unrelated pairs, every gap model on both geometries."""
    knobs("GSA_SCORE_K", k)
    for R, C in edge_shapes(op.strip_rows(go, ge, k)):
        _score(engine, edge_pair("random", R, C, golden.blosum62), ("edge", "random", R, C), go, ge)


@pytest.mark.parametrize("q8", [0, 2])
@pytest.mark.parametrize("go,ge", [(-11, -1), (-4, -4)])
def test_profile_knob_is_honoured(engine, golden, knobs, go, ge, q8):
    """GSA_KROW_Q8 = 0 / 2: the int16 profile alone, the int8 one at 2 rows per lane too."""
    knobs("GSA_KROW_Q8", q8)
    for R, C in [(9, 300), (513, 47), (513, 1025), (1025, 2100)]:
        _score(engine, edge_pair("related", R, C, golden.blosum62), ("edge", "related", R, C), go, ge)


def test_one_row_or_one_column(engine, golden):
    """R = 1 or C = 1: the analytic candidates H(R, 0) = H(0, C) = 0 compete with a single cell."""
    for n in (1, 2, 9, 513):
        for a, b in ((5, 5), (5, 0)):
            for p, key in ((Pair(hdr(np.full(n, a)), hdr([b]), golden.blosum62), ("c1", n, a, b)),
                           (Pair(hdr([b]), hdr(np.full(n, a)), golden.blosum62), ("r1", n, a, b))):
                for go, ge in GAPS:
                    _score(engine, p, key, go, ge)


@pytest.mark.parametrize("k", [2, 4])
def test_end_row_on_column_c_in_every_ticket_of_three(engine, knobs, k):
    """Column C is captured in every strip of every ticket: the end row in the first, second and third
    ticket, in each of a ticket's four waves."""
    knobs("GSA_SCORE_K", k)
    tr = 256 * k
    R, C = 3 * tr - 20, 60
    for e in [tk * tr + w * 64 * k + 37 for tk in range(3) for w in range(4) if 60 <= tk * tr + w * 64 * k + 37 < R]:
        X = hdr(_part(C, 80 + e, 0, 12))  # X whole on Y's rows e - 59 ... e
        Y = hdr(np.concatenate([_part(e - 60, 81 + e, 16, 20), X[1:], _part(R - e, 82 + e, 16, 20)]))
        for go, ge in ((-11, -1), (-4, -4)):
            assert _score(engine, Pair(Y, X, ID20), ("ticket", k, e), go, ge) == (300, e, C)


# -- value ranges ---------------------------------------------------------------------------------------


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


def test_global_value_bound_2_pow_29(engine):
    """B + |gapo| < 2^29 with gape = 0 and gapo = -(2^20 + 32767): the table lies 2^20 below the int16
    window and B grows by about 2^20 a row, so the bound falls between two square shapes of about 500
    letters.  The span is |gapo| + smax, far below 2^28."""
    go, ge = -((1 << 20) + 32767), 0
    sub = _low_table(-go - ge)
    smax = int(np.abs(sub).max())
    n_ok = ((1 << 29) - 1 - 2 * (-go)) // smax
    assert 400 < n_ok < 520
    for n, ok in ((n_ok, True), (n_ok + 1, False)):
        p = Pair(_seq(n, 5), _seq(n + 30, 6), sub)
        B = oo.exact_for(p.R, p.C, sub, go, ge)
        assert (B - go < (1 << 29)) == ok and oo.span(p.R, p.C, sub, go, ge) < (1 << 28)
        if ok:
            _score(engine, p, ("b29", n), go, ge, align=oo.align64)
        else:
            _refused(lambda: p.score(engine, go, ge))


def test_span_2_pow_28(engine):
    """span = (R + C) |gape| + (gape - gapo) + smax < 2^28 with linear gaps of -2^20: a column more adds
    2^20, so the bound falls between two X of about 250 letters against a 3-letter Y, while B + |gapo|
    stays below 2^29."""
    go = ge = -(1 << 20)
    sub = _low_table(-go - ge)
    R = 3
    smax = int(np.abs(sub).max())
    c_ok = ((1 << 28) - 1 - smax) // (-ge) - R
    assert 200 < c_ok < 260
    for C, ok in ((c_ok, True), (c_ok + 1, False)):
        p = Pair(_seq(R, 7), _seq(C, 8), sub)
        B = oo.exact_for(R, C, sub, go, ge)
        assert (oo.span(R, C, sub, go, ge) < (1 << 28)) == ok and B - go < (1 << 29)
        if ok:
            _score(engine, p, ("span", C), go, ge, align=oo.align64)
        else:
            _refused(lambda: p.score(engine, go, ge))


def test_int16_table_edges(engine, golden):
    """s - gapo - gape at -32767 and 32767 is scored, at -32768 and 32768 refused."""
    Y, X = dovetail(120, 260, 90, 43)
    base = np.asarray(golden.blosum62).reshape(25, 25).astype(np.int64)
    for go, ge in ((-11, -1), (-4, -4)):
        for v, ok in ((-32767, True), (-32768, False), (32767, True), (32768, False)):
            sub = base.copy()
            a, b = (int(Y[5]), int(X[70])) if v < 0 else (int(Y[100]), int(Y[100]))
            sub[a, b] = v + go + ge
            p = Pair(Y, X, sub)
            if ok:
                _score(engine, p, ("i16", v), go, ge, align=oo.align64)
            else:
                _refused(lambda: p.score(engine, go, ge))


# -- around the call --------------------------------------------------------------------------------


@pytest.mark.parametrize("go,ge", [(-11, -1), (-4, -4)])
def test_neighbours_keep_their_results(engine, golden, go, ge):
    p = Pair(*dovetail(600, 1500, 420, 91), golden.blosum62)

    def others():
        out = [tuple(engine.score_dev(*p.args(), go, ge, local)[k] for k in ("score", "i_end", "j_end"))
               for local in (False, True)]
        return out + [tuple(engine.score_semi_dev(*p.args(), go, ge)[k] for k in ("score", "i_end", "j_end"))]

    before = others()
    record = engine.last_launch()
    _score(engine, p, "small", go, ge)
    assert engine.last_launch() == record
    assert others() == before
    _score(engine, p, "small", go, ge)


def test_column_buffer_is_counted_in_mem_stats(engine, golden):
    e = gsa.Engine(0)
    try:
        p = Pair(_seq(300000, 1), _seq(40, 2), golden.blosum62)
        e.reset_mem_stats()
        base = e.mem_stats()["glmem_peak_allocs"]
        e.score_semi_dev(*p.args(), -4, -4)
        semi = e.mem_stats()["glmem_peak_allocs"] - base
        e.score_overlap_dev(*p.args(), -4, -4)
        both = e.mem_stats()["glmem_peak_allocs"] - base
        assert both - semi >= 4 * (p.R + 1), (semi, both)  # one word per row, next to what the semi-global call holds
    finally:
        e.close()


def test_host_form_and_empty_sides(engine, golden):
    Y, X = dovetail(300, 900, 200, 95)
    for go, ge in GAPS:
        r = engine.score_overlap(Y, X, golden.blosum62, go, ge)
        assert (r["score"], r["i_end"], r["j_end"]) == oo.score(Y, X, golden.blosum62, go, ge)
    r = engine.score_overlap(Y, X, golden.blosum62, -4)
    assert (r["score"], r["i_end"], r["j_end"]) == oo.score(Y, X, golden.blosum62, -4, -4)
    r = engine.score_overlap(Y, X[:1], golden.blosum62, -11, -1)  # C = 0
    assert (r["score"], r["i_end"], r["j_end"]) == (0, 300, 0) == oo.score(Y, X[:1], golden.blosum62, -11, -1)
    for x in (X, X[:1]):  # R = 0
        r = engine.score_overlap(Y[:1], x, golden.blosum62, -11, -1)
        assert (r["score"], r["i_end"], r["j_end"]) == (0, 0, 0) == oo.score(Y[:1], x, golden.blosum62, -11, -1)


def test_invalid_input(engine, golden):
    p = Pair(*dovetail(100, 200, 60, 97), golden.blosum62)
    _refused(lambda: p.score(engine, -1, -11))  # go > ge
    _refused(lambda: p.score(engine, -11, 1))   # ge > 0
    _refused(lambda: engine.score_overlap_dev(p.y.data_ptr(), 0, p.x.data_ptr(), p.x.numel(), p.sub.data_ptr(), p.substsz, -11, -1))
    _refused(lambda: engine.score_overlap_dev(p.y.data_ptr(), p.y.numel(), p.x.data_ptr(), p.x.numel(), p.sub.data_ptr(), 33, -11, -1))
    _refused(lambda: engine.score_overlap_dev(0, p.y.numel(), p.x.data_ptr(), p.x.numel(), p.sub.data_ptr(), p.substsz, -11, -1))
    _score(engine, p, "inv", -11, -1)


def test_a_long_pair(engine, golden):
    """A side far past the lane kernels' 8191 letters: a 300-letter read hanging over the head of a
    40 000-letter sequence, and 40 000 rows whose head X's tail lies on."""
    for name, (Y, X) in (("dove", dovetail(300, 40000, 200, 99)), ("mirror", mirror(40000, 300, 200, 101))):
        p = Pair(Y, X, golden.blosum62)
        for go, ge in ((-11, -1), (-4, -4)):
            assert p.score(engine, go, ge) == oo.score(Y, X, golden.blosum62, go, ge), name
