"""gsa_align_pair_band_ext_dev (and, in every case, gsa_score_band_ext_dev) on the GPU against the
extension oracle (tests/_band_ext_oracle.py): tests/_band_ext_cases.py's `check` asserts the score call, all
six fields, the CIGAR, the status, every info field and the CIGAR's replay.  Shapes: the tiny ones with every
valid band; the rows at the lane's and the strip's edges; a planted unique maximum on either side of every
boundary of the argmax scheme (lane, strip, a wave's second strip); ties across the same boundaries and
within a row; band widths and positions at the edges of a super-step; the end cell on the band's edges and
in the corner; score 0; trimming; the buffers, the limits and the refusals; the calls' neighbours."""
import ctypes

import numpy as np
import pytest

import gpuseqalign_amd as gsa
from tests import _band_ext_oracle as eo
from tests import _band_oracle as bo
from tests._band_ext_cases import (FIELDS, GAP_IDS, GAPS, UNIT, blosum_like, check, geometry, plan_of, planted,
                                   planted_want, random_seq, related, table, tied)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def geo(engine):
    """(TR, KR, lag, NWV), read from a first call's info."""
    y = random_seq(np.random.default_rng(0), 4, 5)
    engine.align_pair_band_ext(y, y, table(), -2, -1, band=1)
    return geometry(engine.last_align_pair_band_ext_info())


@pytest.mark.parametrize("go,ge", GAPS, ids=GAP_IDS)
def test_tiny_shapes_every_valid_band(engine, go, ge):
    rng = np.random.default_rng(31)
    sub = table(2, 2, -1)
    for R in (1, 2, 3):
        for C in (1, 2, 3):
            y, x = random_seq(rng, 2, R), random_seq(rng, 2, C)
            for lo in range(-R, 1):
                for hi in range(0, C + 1):
                    check(engine, y, x, sub, go, ge, lo, hi)
            check(engine, y, x, sub, go, ge, -R - 2, C + 3)  # clamped from far outside


@pytest.mark.parametrize("go,ge", GAPS, ids=GAP_IDS)
def test_row_geometry(engine, geo, go, ge):
    TR, KR, _, _ = geo
    rng = np.random.default_rng(32)
    sub = blosum_like(rng)
    for k, R in enumerate((KR, KR + 1, TR - 1, TR, TR + 1, 2 * TR + 1)):
        y = random_seq(rng, 20, R)
        C = R + (-3, 0, 5)[k % 3]
        x = related(rng, y, 20, C) if k % 2 else random_seq(rng, 20, C)
        check(engine, y, x, sub, go, ge, -4, 6)


@pytest.mark.parametrize("go,ge", GAPS, ids=GAP_IDS)
def test_planted_maximum_at_every_boundary(engine, geo, go, ge):
    """p at a lane's last row and the next lane's first, a strip's last row and the next strip's first; the
    expected result needs no oracle."""
    TR, KR, _, _ = geo
    rng = np.random.default_rng(33)
    R, C = 2 * TR + 9, 2 * TR + 30
    for p in (1, KR, KR + 1, 5 * KR, 5 * KR + 1, TR, TR + 1, TR + KR, TR + KR + 1, 2 * TR, 2 * TR + 1, R):
        y, x = planted(rng, p, R, C)
        check(engine, y, x, UNIT, go, ge, -7, 12, want=planted_want(p))


@pytest.mark.parametrize("go,ge", GAPS, ids=GAP_IDS)
def test_planted_maximum_in_a_waves_second_strip(engine, geo, go, ge):
    """More strips than waves: the end cell in a strip of index >= NWV (its wave's second) and, within the
    same pair, in the first strip, which the same wave ran before."""
    TR, KR, lag, nwv = geo
    rng = np.random.default_rng(34)
    R = (nwv + 2) * TR + 5
    for p in (nwv * TR + 3, (nwv + 1) * TR, (nwv + 1) * TR + 1, R, 7):
        y, x = planted(rng, p, R, R + 40)
        a, info = check(engine, y, x, UNIT, go, ge, -100, 100, want=planted_want(p))
        assert info["strips"] == nwv + 3 > info["waves"] == nwv


@pytest.mark.parametrize("go,ge", GAPS, ids=GAP_IDS)
def test_ties_across_lanes_strips_and_waves(engine, geo, go, ge):
    """The same maximum at (p, p) and at (p + 2, p + 2), with p + 2 across a lane's, a strip's (and so a
    wave's) boundary and, for the wave's second strip, across NWV strips: the first in row-major order wins."""
    TR, KR, _, nwv = geo
    rng = np.random.default_rng(35)
    R = TR + 40
    for p in (KR - 1, KR, TR - 1, TR, 3 * KR + 2):
        y, x = tied(rng, p, R, R + 10)
        want = eo.align(y, x, UNIT, go, ge, -5, 8, want_cells=True)
        cells = want[6]
        assert len(cells) >= 2 and (want[3], want[4]) == cells[0] == min(cells)
        if go < 0:
            assert cells[0] == (p, p) and (p + 2, p + 2) in cells
        check(engine, y, x, UNIT, go, ge, -5, 8, want=want[:6])


@pytest.mark.parametrize("go,ge", GAPS, ids=GAP_IDS)
def test_ties_within_a_row(engine, go, ge):
    """Two maximal cells in one row, at two columns: small pairs searched with the oracle until the first two
    maximal cells share their row (a table whose matches can pay for a gap makes them frequent: the search
    ends within 500 pairs for every gap model)."""
    rng = np.random.default_rng(36)
    found = 0
    for _ in range(2000):
        sub = blosum_like(rng, 3)
        R, C = int(rng.integers(2, 10)), int(rng.integers(3, 12))
        y, x = random_seq(rng, 3, R), random_seq(rng, 3, C)
        want = eo.align(y, x, sub, go, ge, -3, 6, want_cells=True)
        cells = want[6]
        if want[0] > 0 and len(cells) >= 2 and cells[0][0] == cells[1][0]:
            check(engine, y, x, sub, go, ge, -3, 6, want=want[:6])
            found += 1
            if found == 4:
                break
    assert found == 4


@pytest.mark.parametrize("go,ge", GAPS, ids=GAP_IDS)
def test_band_widths(engine, geo, go, ge):
    """W = 1 is the pure diagonal: the longest best prefix of it.  The others sit around a super-step's 64
    columns."""
    TR = geo[0]
    rng = np.random.default_rng(37)
    sub = table()
    R = max(TR + 150, 700)  # more rows than half the widest band: nothing is clamped
    y = random_seq(rng, 4, R)
    for W in (1, 2, 63, 64, 65, 129, 1025):
        for x in (related(rng, y, 4, R), random_seq(rng, 4, R)):
            lo = -(W // 2)
            a, info = check(engine, y, x, sub, go, ge, lo, lo + W - 1)
            assert info["band_hi"] - info["band_lo"] + 1 == W
            if W == 1:
                assert a["cigar"].count("I") == a["cigar"].count("D") == 0 and a["i_end"] == a["j_end"]
                run = np.concatenate([[0], np.cumsum(sub[y[1:], x[1:]])])
                assert a["score"] == run.max() and a["i_end"] == int(np.argmax(run))


@pytest.mark.parametrize("go,ge", GAPS, ids=GAP_IDS)
def test_band_position_at_the_edges_of_64_columns(engine, geo, go, ge):
    TR = geo[0]
    rng = np.random.default_rng(38)
    sub = blosum_like(rng)
    R = TR + 70
    y = random_seq(rng, 20, R)
    x = related(rng, y, 20, R + 20, 0.2)
    for lo in (-2, -1, 0, -66, -65, -64):
        for hi in (62, 63, 64):
            check(engine, y, x, sub, go, ge, lo, hi)


@pytest.mark.parametrize("go,ge", GAPS, ids=GAP_IDS)
def test_end_cell_on_the_band_edges(engine, geo, go, ge):
    """A subject with g letters more (fewer) in front of a long common run: the best cell lies on diagonal
    g (-g), which is band_hi (band_lo)."""
    TR = geo[0]
    rng = np.random.default_rng(39)
    sub = table(4, 5, -4)
    g = 3
    core = rng.integers(0, 4, size=TR + 60)
    head = rng.integers(0, 4, size=20)
    extra = rng.integers(0, 4, size=g)
    a_ = np.concatenate([[0], head, core]).astype(np.int32)
    b_ = np.concatenate([[0], head, extra, core]).astype(np.int32)
    for y, x, lo, hi, d in ((a_, b_, -2, g, g), (b_, a_, -g, 2, -g)):
        a, info = check(engine, y, x, sub, go, ge, lo, hi)
        if go < 0:
            assert a["j_end"] - a["i_end"] == d and a["score"] > 5 * TR
        # one diagonal short, the band misses the run: the oracle's lower score
        b, _ = check(engine, y, x, sub, go, ge, lo + (d < 0), hi - (d > 0))
        assert b["score"] <= a["score"]


@pytest.mark.parametrize("go,ge", GAPS, ids=GAP_IDS)
def test_the_end_in_the_corner_equals_the_global_banded_call(engine, geo, go, ge):
    TR = geo[0]
    rng = np.random.default_rng(40)
    sub = table(4, 5, -4)
    R = TR + 33
    y = random_seq(rng, 4, R)
    x = related(rng, y, 4, R, 0.03)
    x[-3:] = y[-3:]
    x[1:3] = y[1:3]
    a, info = check(engine, y, x, sub, go, ge, -6, 9)
    assert (a["i_end"], a["j_end"]) == (R, R)
    g = engine.align_pair_band(y, x, sub, go, ge, band_lo=-6, band_hi=9)
    assert g["status"] == 0 and {k: a[k] for k in FIELDS} == {k: g[k] for k in FIELDS}


@pytest.mark.parametrize("go,ge", GAPS, ids=GAP_IDS)
def test_score_zero(engine, geo, go, ge):
    TR = geo[0]
    rng = np.random.default_rng(41)
    sub = -1 - np.abs(blosum_like(rng))  # all negative
    for R, C in ((5, 7), (TR + 3, TR + 9)):
        y, x = random_seq(rng, 20, R), random_seq(rng, 20, C)
        a, info = check(engine, y, x, sub, go, ge, -4, 5, want=(0, 0, 0, 0, 0, ""))
        # pmax = 0: a path that leaves the band scores at most go + band_hi ge, which only 0 0 does not put below 0
        assert info["proved_optimal"] == (1 if go < 0 else 0)
    # a positive table and unrelated first letters: still 0 under a pure diagonal
    y, x = np.array([0, 1, 1, 1], np.int32), np.array([0, 2, 2, 2], np.int32)
    check(engine, y, x, table(), go, ge, 0, 0, want=(0, 0, 0, 0, 0, ""))


@pytest.mark.parametrize("go,ge", GAPS, ids=GAP_IDS)
def test_trimming(engine, geo, go, ge):
    TR, KR, lag, nwv = geo
    rng = np.random.default_rng(42)
    sub = blosum_like(rng)
    # rows beyond C - lo hold no cell: one strip of 120 rows out of 3 TR
    y = random_seq(rng, 20, 3 * TR)
    x = related(rng, y, 20, 100)
    a, info = check(engine, y, x, sub, go, ge, -20, 7)
    assert (info["rows_used"], info["cols_used"], info["strips"]) == (120, 100, 1)
    for k in ("strips", "supersteps", "code_bytes"):
        assert info[k] == plan_of(TR, lag, nwv, 120, 100, -20, 7)[k]
    # columns beyond R + hi likewise
    y = random_seq(rng, 20, 90)
    x = related(rng, y, 20, 20 * TR)
    a, info = check(engine, y, x, sub, go, ge, -5, 30)
    assert (info["rows_used"], info["cols_used"], info["strips"]) == (90, 120, 1)
    for k in ("strips", "supersteps", "code_bytes"):
        assert info[k] == plan_of(TR, lag, nwv, 90, 120, -5, 30)[k]
    # the prefixes give the same six fields
    b = engine.align_pair_band_ext(y, x[:121], sub, go, ge, band_lo=-5, band_hi=30)
    assert {k: a[k] for k in FIELDS} == {k: b[k] for k in FIELDS}
    # a band that holds 0 but not C - R: taken here, refused by the global call
    assert not bo.valid(90, 20 * TR, -5, 30)
    with pytest.raises(gsa.NwError) as err:
        engine.align_pair_band(y, x, sub, go, ge, band_lo=-5, band_hi=30)
    assert err.value.stat == gsa.NwStat.errorInvalidValue


def test_scratch_limit_exact_and_one_byte_short(engine):
    rng = np.random.default_rng(43)
    sub = table()
    y = random_seq(rng, 4, 700)
    x = related(rng, y, 4, 690)
    x[400:] = random_seq(rng, 4, 690)[400:]  # related for the first 400 letters
    want = eo.align(y, x, sub, -5, -2, -30, 25)
    assert 0 < want[3] < 690
    a, info = check(engine, y, x, sub, -5, -2, -30, 25, want=want)
    need = info["code_bytes"]
    a = engine.align_pair_band_ext(y, x, sub, -5, -2, band_lo=-30, band_hi=25, scratch_limit=need)
    assert a["status"] == 0 and tuple(a[k] for k in FIELDS) == want
    b = engine.align_pair_band_ext(y, x, sub, -5, -2, band_lo=-30, band_hi=25, scratch_limit=need - 1)
    info = engine.last_align_pair_band_ext_info()
    assert (b["status"], b["score"], b["i_start"], b["j_start"], b["i_end"], b["j_end"], b["cigar"]) == \
        (1, want[0], 0, 0, want[3], want[4], "")
    assert info["code_bytes"] == need and info["walk_ms"] == 0 and info["score_ms"] > 0
    assert info["proved_optimal"] == eo.certificate(700, 690, -30, 25, sub, -5, -2, want[0])


def _raw(engine, y, x, sub, go, ge, lo, hi, cap, scratch_limit=0, null_out=False, null_cigar=False):
    import torch
    dev = torch.device("cuda", engine.device)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)
    dS, dY, dX = up(np.asarray(sub).ravel()), up(y), up(x)
    torch.cuda.synchronize(dev)
    res, info = gsa.AlignDbResult(), gsa.AlignPairBandExtInfo()
    need, ms = ctypes.c_int64(-1), ctypes.c_float(-1.0)
    buf = ctypes.create_string_buffer(max(cap, 1))
    st = gsa.lib().gsa_align_pair_band_ext_dev(engine._h, dY.data_ptr(), dY.numel(), dX.data_ptr(), dX.numel(),
                                               dS.data_ptr(), len(sub), go, ge, lo, hi, scratch_limit,
                                               None if null_out else ctypes.byref(res), None if null_cigar else buf, cap,
                                               ctypes.byref(need), ctypes.byref(info), ctypes.byref(ms), None)
    return st, res, buf, need.value, info


def test_cigar_buffer_and_refusals_through_the_raw_abi(engine):
    rng = np.random.default_rng(44)
    sub = table()
    y = random_seq(rng, 4, 90)
    x = related(rng, y, 4, 95, 0.2)
    want = eo.align(y, x, sub, -4, -4, -6, 9)
    n = len(want[5])
    assert n > 0
    st, res, buf, need, _ = _raw(engine, y, x, sub, -4, -4, -6, 9, n + 1)
    assert (st, res.status, need, res.cigar_off, res.cigar_len) == (0, 0, n + 1, 0, n) and buf.value.decode() == want[5]
    st, res, buf, need, info = _raw(engine, y, x, sub, -4, -4, -6, 9, n)
    assert (st, res.status, need, res.cigar_len) == (0, 2, n + 1, 0)
    assert (res.score, res.i_start, res.j_start, res.i_end, res.j_end) == want[:5] and info.code_bytes > 0
    st, res, _, need, _ = _raw(engine, y, x, sub, -4, -4, -6, 9, 0, null_cigar=True)
    assert (st, res.status, need) == (0, 2, n + 1)
    inv = gsa.NwStat.errorInvalidValue
    assert _raw(engine, y, x, sub, -4, -4, -6, 9, 8, null_cigar=True)[0] == inv
    assert _raw(engine, y, x, sub, -4, -4, -6, 9, -1)[0] == inv                       # a negative cap
    assert _raw(engine, y, x, sub, -4, -4, -6, 9, 400, scratch_limit=-1)[0] == inv
    assert _raw(engine, y, x, sub, -4, -4, -6, 9, 400, null_out=True)[0] == inv
    assert _raw(engine, y, x, sub, -4, -1, -6, 9, 400)[0] == 0
    assert _raw(engine, y, x, sub, -1, -4, -6, 9, 400)[0] == inv                      # gapo > gape
    assert _raw(engine, y, x, sub, -4, 1, -6, 9, 400)[0] == inv                       # gape > 0
    assert _raw(engine, y, x, sub, -4, -4, 1, 9, 400)[0] == inv                       # lo > 0
    assert _raw(engine, y, x, sub, -4, -4, -6, -1, 400)[0] == inv                     # hi < 0
    assert _raw(engine, y, x, sub, -4, -4, 0, -1, 400)[0] == inv                      # lo > hi around 0
    assert _raw(engine, y, x, sub, -4, -4, 3, 2, 400)[0] == inv                       # lo > hi


def test_invalid_bands_the_width_limit_and_empty_sides(engine):
    rng = np.random.default_rng(45)
    sub = table()
    y, x = random_seq(rng, 4, 40), random_seq(rng, 4, 47)
    for lo, hi in ((1, 7), (1, 0), (5, 9), (-3, -1), (3, 2)):
        for call in (engine.score_band_ext, engine.align_pair_band_ext):
            with pytest.raises(gsa.NwError) as err:
                call(y, x, sub, -3, -1, band_lo=lo, band_hi=hi)
            assert err.value.stat == gsa.NwStat.errorInvalidValue
    for call in (engine.score_band_ext, engine.align_pair_band_ext):
        with pytest.raises(gsa.NwError):
            call(y, x, sub, -3, -1, band=-1)
    # a width over the limit after clamping is refused; at the limit it runs
    limit = gsa.band_max_width()
    L = limit + 10
    yl = random_seq(rng, 4, L)
    xl = related(rng, yl, 4, L, 0.3)
    for call in (engine.score_band_ext, engine.align_pair_band_ext):
        with pytest.raises(gsa.NwError) as err:
            call(yl, xl, sub, -3, -1, band_lo=-(limit // 2), band_hi=limit - limit // 2)
        assert err.value.stat == gsa.NwStat.errorInvalidValue
    s = engine.score_band_ext(yl, xl, sub, -3, -1, band_lo=-(limit // 2), band_hi=limit - limit // 2 - 1)
    assert s["score"] > 0
    # an empty side is answered on the host: score 0 at (0, 0), whatever the gap model
    e = np.array([0], np.int32)
    for go, ge in GAPS:
        for yy, xx in ((y, e), (e, x), (e, e)):
            a = engine.align_pair_band_ext(yy, xx, sub, go, ge, band_lo=-5, band_hi=50)
            assert tuple(a[k] for k in FIELDS) == (0, 0, 0, 0, 0, "") and a["status"] == 0 and a["kernel_ms"] == 0
            info = engine.last_align_pair_band_ext_info()
            R, C = len(yy) - 1, len(xx) - 1
            assert (info["band_lo"], info["band_hi"]) == eo.clamp(R, C, -5, 50)
            assert (info["rows_used"], info["cols_used"]) == eo.trim(R, C, -5, 50)
            assert (info["strips"], info["code_bytes"], info["proved_optimal"]) == (0, 0, 1)
            assert engine.score_band_ext(yy, xx, sub, go, ge, band_lo=-5, band_hi=50) == \
                dict(score=0, i_end=0, j_end=0, kernel_ms=0.0)
    for call in (engine.score_band_ext, engine.align_pair_band_ext):
        with pytest.raises(gsa.NwError):
            call(y, e, sub, -3, -1, band_lo=1, band_hi=2)


def test_neighbours_launch_record_and_a_stream(engine):
    import torch
    rng = np.random.default_rng(46)
    sub = blosum_like(rng)
    y = random_seq(rng, 20, 1500)
    x = related(rng, y, 20, 1450, 0.15)
    x[900:] = random_seq(rng, 20, 1450)[900:]
    dev = torch.device("cuda", engine.device)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)
    dS, dY, dX = up(sub.ravel()), up(y), up(x)
    torch.cuda.synchronize(dev)
    args = (dY.data_ptr(), dY.numel(), dX.data_ptr(), dX.numel(), dS.data_ptr(), 20, -11, -1)

    def others():
        s = engine.score_dev(*args)
        a = engine.align_pair_dev(*args)
        b = engine.align_pair_band_dev(*args, -80, 30)
        for d in (s, a, b):
            d.pop("kernel_ms")
        return s, a, b

    before = others()
    launch = engine.last_launch()
    want = eo.align(y, x, sub, -11, -1, -80, 30)
    assert 0 < want[3] < 1500
    st = torch.cuda.Stream(device=dev)
    for stream in (None, st.cuda_stream):
        a = engine.align_pair_band_ext_dev(*args, -80, 30, 0, stream)
        assert a["status"] == 0 and tuple(a[k] for k in FIELDS) == want
        s = engine.score_band_ext_dev(*args, -80, 30, stream)
        assert (s["score"], s["i_end"], s["j_end"]) == (want[0], want[3], want[4])
    assert engine.last_launch() == launch  # the calls report through their own info struct
    assert others() == before
