"""gsa_align_pair_band_dev (and, in every case, gsa_score_band_dev) on the GPU against the banded oracle
(tests/_band_oracle.py): tests/_band_cases.py's `check` asserts the score call, all six fields, the CIGAR,
the status, every info field and the CIGAR's replay.  Shapes: the tiny ones with every valid band; the
rows at the lane's and the strip's edges; more strips than waves; band widths and positions at the
edges of a super-step; pairs whose end cell lies on the band's edge; clamping; a planted gap run that the
band holds or misses by one diagonal; the buffers, the limits and the refusals; the calls' neighbours."""
import ctypes

import numpy as np
import pytest

import gpuseqalign_amd as gsa
from tests import _align_oracle as ao
from tests import _band_oracle as bo
from tests._band_cases import FIELDS, GAP_IDS, GAPS, blosum_like, check, geometry, random_seq, related, table

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def geo(engine):
    """(TR, KR, lag, NWV), read from a first call's info."""
    y = random_seq(np.random.default_rng(0), 4, 5)
    engine.align_pair_band(y, y, table(), -2, -1, band=1)
    return geometry(engine.last_align_pair_band_info())


@pytest.mark.parametrize("go,ge", GAPS, ids=GAP_IDS)
def test_tiny_shapes_every_valid_band(engine, go, ge):
    rng = np.random.default_rng(11)
    sub = table(2, 2, -1)
    for R in (1, 2, 3):
        for C in (1, 2, 3):
            y, x = random_seq(rng, 2, R), random_seq(rng, 2, C)
            for lo in range(-R, min(0, C - R) + 1):
                for hi in range(max(0, C - R), C + 1):
                    check(engine, y, x, sub, go, ge, lo, hi)
            check(engine, y, x, sub, go, ge, -R - 2, C + 3)  # clamped to the whole matrix


@pytest.mark.parametrize("go,ge", GAPS, ids=GAP_IDS)
def test_row_geometry(engine, geo, go, ge):
    TR, KR, _, _ = geo
    rng = np.random.default_rng(12)
    sub = blosum_like(rng)
    for k, R in enumerate((KR, KR + 1, TR - 1, TR, TR + 1, 2 * TR + 1)):
        y = random_seq(rng, 20, R)
        C = R + (-3, 0, 5)[k % 3]
        x = related(rng, y, 20, C) if k % 2 else random_seq(rng, 20, C)
        check(engine, y, x, sub, go, ge, min(0, C - R) - 4, max(0, C - R) + 6)


@pytest.mark.parametrize("go,ge", GAPS, ids=GAP_IDS)
def test_band_widths(engine, geo, go, ge):
    """W = 1 is the pure diagonal of a square pair; the others sit around a super-step's 64 columns."""
    TR = geo[0]
    rng = np.random.default_rng(13)
    sub = table()
    R = max(TR + 150, 700)  # more rows than half the widest band: nothing is clamped
    y = random_seq(rng, 4, R)
    for W in (1, 2, 63, 64, 65, 129, 1025):
        for x in (related(rng, y, 4, R), random_seq(rng, 4, R)):
            lo = -(W // 2)
            a, info = check(engine, y, x, sub, go, ge, lo, lo + W - 1)
            assert info["band_hi"] - info["band_lo"] + 1 == W
            if W == 1:
                assert a["cigar"].count("I") == a["cigar"].count("D") == 0


@pytest.mark.parametrize("go,ge", GAPS, ids=GAP_IDS)
def test_band_position_at_the_edges_of_64_columns(engine, geo, go, ge):
    """o(s) = s TR + 1 + lo and o(s) + Wc = (s + 1) TR + hi + 1 on either side of a multiple of 64."""
    TR = geo[0]
    rng = np.random.default_rng(14)
    sub = blosum_like(rng)
    R = TR + 70
    y = random_seq(rng, 20, R)
    x = related(rng, y, 20, R + 20, 0.2)
    for lo in (-2, -1, 0, -66, -65, -64):
        for hi in (62, 63, 64):
            assert (1 + lo) % 64 in (63, 0, 1) and (hi + 1) % 64 in (63, 0, 1)
            check(engine, y, x, sub, go, ge, lo, hi)


@pytest.mark.parametrize("go,ge", GAPS, ids=GAP_IDS)
def test_end_cell_on_the_band_edge(engine, go, ge):
    rng = np.random.default_rng(15)
    sub = table()
    R = 640
    y = random_seq(rng, 4, R)
    for delta in (-300, -70, -1, 1, 70, 300):
        x = related(rng, y, 4, R + delta)
        lo, hi = min(0, delta), max(0, delta)
        check(engine, y, x, sub, go, ge, lo, hi)            # the minimal band: (R, C) and (0, 0) on its edges
        check(engine, y, x, sub, go, ge, lo - 9, hi + 17)   # and a wider one


@pytest.mark.parametrize("go,ge", GAPS, ids=GAP_IDS)
def test_clamping_and_the_full_band(engine, geo, go, ge):
    TR = geo[0]
    rng = np.random.default_rng(16)
    sub = blosum_like(rng)
    y = random_seq(rng, 20, 300)
    x = related(rng, y, 20, 310)
    a, info = check(engine, y, x, sub, go, ge, -1000, 2000)
    assert (info["band_lo"], info["band_hi"]) == (-300, 310)
    a2, info2 = check(engine, y, x, sub, go, ge, -300, 310)
    assert {k: a2[k] for k in FIELDS} == {k: a[k] for k in FIELDS} and info2["code_bytes"] == info["code_bytes"]
    # the full band of a pair of about TR + 1: Engine.align_pair's global result, field for field
    y = random_seq(rng, 20, TR + 1)
    x = related(rng, y, 20, TR + 3)
    a, info = check(engine, y, x, sub, go, ge, -(TR + 1), TR + 3)
    full = engine.align_pair(y, x, sub, go, ge)
    assert full["status"] == 0 and {k: a[k] for k in FIELDS} == {k: full[k] for k in FIELDS}
    assert info["proved_optimal"] == 1


def _planted(rng, R, p1, p2, g, first):
    """y and x equal but for g letters only y has from row p1 + 1 and g letters only x has behind row p2
    (first = "I"), or the other way round ("D"): the alignment leaves diagonal 0 for -g (g) between."""
    core = rng.integers(0, 4, size=R)
    extra = rng.integers(0, 4, size=g)
    a = np.concatenate([core[:p1], extra, core[p1:p2], core[p2:]])
    b = np.concatenate([core[:p1], core[p1:p2], rng.integers(0, 4, size=g), core[p2:]])
    y, x = (a, b) if first == "I" else (b, a)
    return np.concatenate([[0], y]).astype(np.int32), np.concatenate([[0], x]).astype(np.int32)


@pytest.mark.parametrize("go,ge", GAPS, ids=GAP_IDS)
def test_the_band_decides(engine, geo, go, ge):
    TR, KR, _, _ = geo
    rng = np.random.default_rng(17)
    sub = table(4, 5, -4)
    g = 20
    # the run of g gap letters crosses a lane hand-off (rows KR, 2 KR) or the strip boundary (row TR)
    for p1 in (KR - 3, TR - 10):
        for first in ("I", "D"):
            y, x = _planted(rng, TR + 200, p1, p1 + 150, g, first)
            R, C = len(y) - 1, len(x) - 1
            assert R == C
            full = ao.align(y, x, sub, go, ge, False)
            lo, hi = (-g, 3) if first == "I" else (-3, g)
            a, info = check(engine, y, x, sub, go, ge, lo, hi)
            assert tuple(a[k] for k in FIELDS) == full
            # one diagonal short: a lower score, the banded oracle's, and no certificate
            lo, hi = (-g + 1, 3) if first == "I" else (-3, g - 1)
            b, info = check(engine, y, x, sub, go, ge, lo, hi)
            assert b["score"] < full[0] and info["proved_optimal"] == 0


@pytest.mark.parametrize("go,ge", GAPS, ids=GAP_IDS)
def test_more_strips_than_waves(engine, geo, go, ge):
    """The wave-reuse case: strips > NWV + 1, a narrow band, so that waves take a second strip.  The
    full-matrix oracle would be too large, so the pair is made to satisfy the certificate and the result
    must be Engine.align_pair's."""
    TR, KR, lag, nwv = geo
    rng = np.random.default_rng(18)
    sub = table(4, 1, -1)
    R = (nwv + 2) * TR + 5
    y = random_seq(rng, 4, R)
    x = related(rng, y, 4, R, 0.005)
    # by construction: the pure diagonal alone beats every path that leaves the band
    diagonal = int(sub[y[1:], x[1:]].sum())
    assert bo.certificate(R, R, -100, 100, sub, go, ge, diagonal) == 1
    a = engine.align_pair_band(y, x, sub, go, ge, band=100)
    info = engine.last_align_pair_band_info()
    assert info["strips"] == nwv + 3 > info["waves"] + 1 == nwv + 1
    assert info["supersteps"] == (nwv + 2) * lag + -(-(201 + TR - 1 + 63) // 64)
    assert info["code_bytes"] == (nwv + 3) * (201 + TR - 1) * TR // 2
    assert a["score"] >= diagonal
    assert info["proved_optimal"] == 1 == bo.certificate(R, R, -100, 100, sub, go, ge, a["score"])
    full = engine.align_pair(y, x, sub, go, ge)
    assert full["status"] == 0 and a["status"] == 0 and {k: a[k] for k in FIELDS} == {k: full[k] for k in FIELDS}
    assert ao.rescore(a["cigar"], y, x, 0, 0, sub, go, ge) == (a["score"], R, R)
    assert engine.score_band(y, x, sub, go, ge, band=100)["score"] == a["score"]


def test_scratch_limit_exact_and_one_byte_short(engine):
    rng = np.random.default_rng(19)
    sub = table()
    y = random_seq(rng, 4, 700)
    x = related(rng, y, 4, 690)
    want = bo.align(y, x, sub, -5, -2, -30, 25)
    a, info = check(engine, y, x, sub, -5, -2, -30, 25, want=want)
    need = info["code_bytes"]
    a = engine.align_pair_band(y, x, sub, -5, -2, band_lo=-30, band_hi=25, scratch_limit=need)
    assert a["status"] == 0 and tuple(a[k] for k in FIELDS) == want
    b = engine.align_pair_band(y, x, sub, -5, -2, band_lo=-30, band_hi=25, scratch_limit=need - 1)
    info = engine.last_align_pair_band_info()
    assert (b["status"], b["score"], b["i_end"], b["j_end"], b["cigar"]) == (1, want[0], 700, 690, "")
    assert info["code_bytes"] == need and info["walk_ms"] == 0 and info["score_ms"] > 0
    assert info["proved_optimal"] == bo.certificate(700, 690, -30, 25, sub, -5, -2, want[0])


def _raw(engine, y, x, sub, go, ge, lo, hi, cap, scratch_limit=0, null_out=False, null_cigar=False):
    import torch
    dev = torch.device("cuda", engine.device)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)
    dS, dY, dX = up(np.asarray(sub).ravel()), up(y), up(x)
    torch.cuda.synchronize(dev)
    res, info = gsa.AlignDbResult(), gsa.AlignPairBandInfo()
    need, ms = ctypes.c_int64(-1), ctypes.c_float(-1.0)
    buf = ctypes.create_string_buffer(max(cap, 1))
    st = gsa.lib().gsa_align_pair_band_dev(engine._h, dY.data_ptr(), dY.numel(), dX.data_ptr(), dX.numel(), dS.data_ptr(),
                                           len(sub), go, ge, lo, hi, scratch_limit,
                                           None if null_out else ctypes.byref(res), None if null_cigar else buf, cap,
                                           ctypes.byref(need), ctypes.byref(info), ctypes.byref(ms), None)
    return st, res, buf, need.value, info


def test_cigar_buffer_through_the_raw_abi(engine):
    rng = np.random.default_rng(20)
    sub = table()
    y = random_seq(rng, 4, 90)
    x = related(rng, y, 4, 95, 0.2)
    want = bo.align(y, x, sub, -4, -4, -6, 9)
    n = len(want[5])
    st, res, buf, need, _ = _raw(engine, y, x, sub, -4, -4, -6, 9, n + 1)
    assert (st, res.status, need, res.cigar_off, res.cigar_len) == (0, 0, n + 1, 0, n) and buf.value.decode() == want[5]
    st, res, buf, need, info = _raw(engine, y, x, sub, -4, -4, -6, 9, n)
    assert (st, res.status, need, res.cigar_len) == (0, 2, n + 1, 0)
    assert (res.score, res.i_start, res.j_start, res.i_end, res.j_end) == want[:5] and info.code_bytes > 0
    st, res, _, need, _ = _raw(engine, y, x, sub, -4, -4, -6, 9, 0, null_cigar=True)
    assert (st, res.status, need) == (0, 2, n + 1)
    inv = gsa.NwStat.errorInvalidValue
    assert _raw(engine, y, x, sub, -4, -4, -6, 9, 8, null_cigar=True)[0] == inv
    assert _raw(engine, y, x, sub, -4, -4, -6, 9, -1)[0] == inv
    assert _raw(engine, y, x, sub, -4, -4, -6, 9, 400, scratch_limit=-1)[0] == inv
    assert _raw(engine, y, x, sub, -4, -4, -6, 9, 400, null_out=True)[0] == inv
    assert _raw(engine, y, x, sub, -4, -1, -6, 9, 400)[0] == 0 and _raw(engine, y, x, sub, -1, -4, -6, 9, 400)[0] == inv
    assert _raw(engine, y, x, sub, -4, 1, -6, 9, 400)[0] == inv


def test_invalid_bands_and_empty_sides(engine):
    rng = np.random.default_rng(21)
    sub = table()
    y, x = random_seq(rng, 4, 40), random_seq(rng, 4, 47)
    for lo, hi in ((0, 6), (1, 7), (1, 0), (5, 9), (-3, -1), (8, 20), (3, 2)):
        assert not bo.valid(40, 47, lo, hi)
        for call in (engine.score_band, engine.align_pair_band):
            with pytest.raises(gsa.NwError) as err:
                call(y, x, sub, -3, -1, band_lo=lo, band_hi=hi)
            assert err.value.stat == gsa.NwStat.errorInvalidValue
    for call in (engine.score_band, engine.align_pair_band):
        with pytest.raises(gsa.NwError):
            call(x, y, sub, -3, -1, band_lo=-6, band_hi=0)  # R = 47, C = 40 needs diagonal -7
        with pytest.raises(gsa.NwError):
            call(y, x, sub, -3, -1, band=-1)
    check(engine, y, x, sub, -3, -1, 0, 7)
    # an empty side is answered on the host, under the same validity rule
    e = np.array([0], np.int32)
    for go, ge in GAPS:
        a = engine.align_pair_band(y, e, sub, go, ge, band_lo=-40, band_hi=0)
        assert tuple(a[k] for k in FIELDS) == (go + 39 * ge, 0, 0, 40, 0, "40I") and a["status"] == 0
        info = engine.last_align_pair_band_info()
        assert (info["band_lo"], info["band_hi"], info["strips"], info["code_bytes"], info["proved_optimal"]) == (-40, 0, 0, 0, 1)
        a = engine.align_pair_band(e, x, sub, go, ge, band_lo=-5, band_hi=50)
        assert tuple(a[k] for k in FIELDS) == (go + 46 * ge, 0, 0, 0, 47, "47D")
        info = engine.last_align_pair_band_info()
        assert (info["band_lo"], info["band_hi"]) == (0, 47)
        assert engine.score_band(e, x, sub, go, ge, band=0) == dict(score=go + 46 * ge, i_end=0, j_end=47, kernel_ms=0.0)
        a = engine.align_pair_band(e, e, sub, go, ge, band=0)
        assert tuple(a[k] for k in FIELDS) == (0, 0, 0, 0, 0, "")
    for call in (engine.score_band, engine.align_pair_band):
        with pytest.raises(gsa.NwError):
            call(y, e, sub, -3, -1, band_lo=-39, band_hi=0)
        # the one gap run of an empty side is held to the value range: 41 x 2^28 is refused, 41 x 2^22 taken
        with pytest.raises(gsa.NwError) as err:
            call(y, e, sub, -(1 << 28), -(1 << 28), band_lo=-40, band_hi=0)
        assert err.value.stat == gsa.NwStat.errorInvalidValue
        assert call(y, e, sub, -(1 << 22), -(1 << 22), band_lo=-40, band_hi=0)["score"] == -40 * (1 << 22)
        with pytest.raises(gsa.NwError):
            call(e, x, sub, -3, -1, band_lo=0, band_hi=46)


def test_neighbours_launch_record_and_a_stream(engine):
    import torch
    rng = np.random.default_rng(22)
    sub = blosum_like(rng)
    y = random_seq(rng, 20, 1500)
    x = related(rng, y, 20, 1450, 0.15)
    dev = torch.device("cuda", engine.device)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)
    dS, dY, dX = up(sub.ravel()), up(y), up(x)
    torch.cuda.synchronize(dev)
    args = (dY.data_ptr(), dY.numel(), dX.data_ptr(), dX.numel(), dS.data_ptr(), 20, -11, -1)

    def others():
        s = engine.score_dev(*args)
        a = engine.align_pair_dev(*args)
        m = engine.align_pair_semi_dev(*args)
        for d in (s, a, m):
            d.pop("kernel_ms")
        return s, a, m

    before = others()
    launch = engine.last_launch()
    want = bo.align(y, x, sub, -11, -1, -80, 30)
    st = torch.cuda.Stream(device=dev)
    for stream in (None, st.cuda_stream):
        a = engine.align_pair_band_dev(*args, -80, 30, 0, stream)
        assert a["status"] == 0 and tuple(a[k] for k in FIELDS) == want
        assert engine.score_band_dev(*args, -80, 30, stream)["score"] == want[0]
    assert engine.last_launch() == launch  # the calls report through their own info struct
    assert others() == before


def test_mem_stats_count_the_codes(engine):
    """On fresh contexts, so that no earlier call's larger buffers stand in for the band's: the alignment
    call's peak holds the move codes, the score call's does not.  (The session engine is asked for only so that
    the test is skipped where the others are.)"""
    rng = np.random.default_rng(23)
    sub = table()
    y = random_seq(rng, 4, 1500)
    x = related(rng, y, 4, 1490)
    with gsa.Engine(0) as e:
        assert e.align_pair_band(y, x, sub, -5, -2, band=200)["status"] == 0
        code_bytes = e.last_align_pair_band_info()["code_bytes"]
        stats = e.mem_stats()
        assert code_bytes > 400000 and stats["glmem_peak_allocs"] >= code_bytes + 1500 + 1490
        # the fill's LDS (the table and the hand-off rings) and registers, no scratch
        assert stats["shmem_peak_allocs"] >= 4096 and stats["regmem_peak_allocs"] > 0 and stats["locmem_peak_allocs"] == 0
    with gsa.Engine(0) as e:
        e.score_band(y, x, sub, -5, -2, band=200)
        stats = e.mem_stats()
        assert 0 < stats["glmem_peak_allocs"] < code_bytes and stats["shmem_peak_allocs"] >= 4096
