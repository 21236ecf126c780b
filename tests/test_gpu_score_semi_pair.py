"""The semi-global score of one long pair (gsa_score_semi_dev: the K-rows score kernel's semi-global
instances, a free row 0 over a global column 0, row R captured over every column and its first maximum
taken by a small kernel) against tests/_semi_oracle.py: score and end cell (R, the
smallest column that attains the score).  The inputs at the value-range guards go against the int64
reference of tests/_semi_pair.py.  tests/test_gpu_align_pair_semi.py checks the score call again in
every one of its cases."""
import numpy as np
import pytest

import gpuseqalign_amd as gsa
from gpuseqalign_amd import formats as F
from tests import _semi_oracle as so
from tests import _semi_pair as sp
from tests._semi_pair import GAPS, Pair, hdr, want
from tests.test_gpu_align_pair_semi import _related, _seq, edge_pair, edge_shapes

pytestmark = pytest.mark.gpu


def _score(engine, p, key, go, ge, align=so.align):
    w, _ = want(key, p, go, ge, align)
    got = p.score(engine, go, ge)
    assert got == (w[0], w[3], w[4]), (key, go, ge, p.R, p.C, got, w)
    return got


@pytest.mark.parametrize("k", [None, 2, 4])
@pytest.mark.parametrize("go,ge", GAPS)
def test_row_and_column_edges(engine, golden, knobs, go, ge, k):
    """The alignment tests' edge shapes on unrelated pairs, every gap model on both geometries."""
    knobs("GSA_SCORE_K", k)
    for R, C in edge_shapes(sp.strip_rows(go, ge, k)):
        _score(engine, edge_pair("random", R, C, golden.blosum62), ("edge", "random", R, C), go, ge)


@pytest.mark.parametrize("q8", [0, 2])
@pytest.mark.parametrize("go,ge", [(-11, -1), (-4, -4)])
def test_profile_knob_is_honoured(engine, golden, knobs, go, ge, q8):
    """GSA_KROW_Q8 = 0 / 2: the int16 profile alone, the int8 one at 2 rows per lane too."""
    knobs("GSA_KROW_Q8", q8)
    for R, C in [(9, 300), (513, 1025), (1025, 2100)]:
        _score(engine, edge_pair("related", R, C, golden.blosum62), ("edge", "related", R, C), go, ge)


def test_c_equals_one_column_0_is_global(engine, golden):
    """C = 1: H(R, 0) = gapo + (R - 1) gape comes out of the free row by itself and competes with H(R, 1)."""
    for R in (1, 2, 9, 513):
        for x in (0, 5):
            p = Pair(hdr(np.full(R, 5)), hdr([x]), golden.blosum62)
            for go, ge in GAPS:
                H = so.matrices(p.Y, p.X, p.subm, go, ge)[0]
                assert H[R, 0] == go + (R - 1) * ge
                _score(engine, p, ("c1", R, x), go, ge)


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
        B = sp.exact_for(p.R, p.C, sub, go, ge)
        assert (B - go < (1 << 29)) == ok and sp.span(p.R, p.C, sub, go, ge) < (1 << 28)
        if ok:
            _score(engine, p, ("b29", n), go, ge, align=sp.align64)
        else:
            _refused(lambda: p.score(engine, go, ge))


def test_span_2_pow_28(engine):
    """span = (R + C) |gape| + (gape - gapo) + smax < 2^28 with linear gaps of -2^20: a column more adds
    2^20, so the bound falls between two subjects of about 250 letters under a 3-letter query, while
    B + |gapo| stays below 2^29."""
    go = ge = -(1 << 20)
    sub = _low_table(-go - ge)
    R = 3
    smax = int(np.abs(sub).max())
    c_ok = ((1 << 28) - 1 - smax) // (-ge) - R
    assert 200 < c_ok < 260
    for C, ok in ((c_ok, True), (c_ok + 1, False)):
        p = Pair(_seq(R, 7), _seq(C, 8), sub)
        B = sp.exact_for(R, C, sub, go, ge)
        assert (sp.span(R, C, sub, go, ge) < (1 << 28)) == ok and B - go < (1 << 29)
        if ok:
            _score(engine, p, ("span", C), go, ge, align=sp.align64)
        else:
            _refused(lambda: p.score(engine, go, ge))


def test_int16_table_edges(engine, golden):
    """s - gapo - gape at -32767 and 32767 is scored, at -32768 and 32768 refused."""
    Y, X = _related(120, 260, 43)
    base = np.asarray(golden.blosum62).reshape(25, 25).astype(np.int64)
    for go, ge in ((-11, -1), (-4, -4)):
        for v, ok in ((-32767, True), (-32768, False), (32767, True), (32768, False)):
            sub = base.copy()
            a, b = (int(Y[5]), int(X[70])) if v < 0 else (int(Y[9]), int(Y[9]))
            sub[a, b] = v + go + ge
            p = Pair(Y, X, sub)
            if ok:
                _score(engine, p, ("i16", v), go, ge, align=sp.align64)
            else:
                _refused(lambda: p.score(engine, go, ge))


# -- around the call --------------------------------------------------------------------------------


@pytest.mark.parametrize("go,ge", [(-11, -1), (-4, -4)])
def test_neighbours_keep_their_results(engine, golden, go, ge):
    p = Pair(*_related(600, 1500, 91), golden.blosum62)

    def others():
        return [tuple(engine.score_dev(*p.args(), go, ge, local)[k] for k in ("score", "i_end", "j_end"))
                for local in (False, True)]

    before = others()
    record = engine.last_launch()
    _score(engine, p, "small", go, ge)
    assert engine.last_launch() == record
    assert others() == before
    _score(engine, p, "small", go, ge)


def test_host_form_and_empty_sides(engine, golden):
    Y, X = _related(300, 900, 95)
    for go, ge in GAPS:
        r = engine.score_semi(Y, X, golden.blosum62, go, ge)
        assert (r["score"], r["i_end"], r["j_end"]) == so.score(Y, X, golden.blosum62, go, ge)
    r = engine.score_semi(Y, X, golden.blosum62, -4)
    assert (r["score"], r["i_end"], r["j_end"]) == so.score(Y, X, golden.blosum62, -4, -4)
    r = engine.score_semi(Y, X[:1], golden.blosum62, -11, -1)  # an empty subject
    assert (r["score"], r["i_end"], r["j_end"]) == (-11 - 299, 300, 0)
    for x in (X, X[:1]):  # an empty query
        r = engine.score_semi(Y[:1], x, golden.blosum62, -11, -1)
        assert (r["score"], r["i_end"], r["j_end"]) == (0, 0, 0)


def test_invalid_input(engine, golden):
    p = Pair(*_related(100, 200, 97), golden.blosum62)
    _refused(lambda: p.score(engine, -1, -11))  # go > ge
    _refused(lambda: p.score(engine, -11, 1))   # ge > 0
    _refused(lambda: engine.score_semi_dev(p.y.data_ptr(), 0, p.x.data_ptr(), p.x.numel(), p.sub.data_ptr(), p.substsz, -11, -1))
    _refused(lambda: engine.score_semi_dev(p.y.data_ptr(), p.y.numel(), p.x.data_ptr(), p.x.numel(), p.sub.data_ptr(), 33, -11, -1))
    _refused(lambda: engine.score_semi_dev(0, p.y.numel(), p.x.data_ptr(), p.x.numel(), p.sub.data_ptr(), p.substsz, -11, -1))
    _score(engine, p, "inv", -11, -1)


def test_a_long_subject(engine, golden):
    """A subject far past the lane kernels' 8191 letters: a 300-letter query in 40000."""
    Y, X = _related(300, 40000, 99)
    p = Pair(Y, X, golden.blosum62)
    for go, ge in ((-11, -1), (-4, -4)):
        assert p.score(engine, go, ge) == so.score(Y, X, golden.blosum62, go, ge)
