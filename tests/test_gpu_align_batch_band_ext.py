"""gsa_align_batch_band_ext_dev (and, in every case, gsa_score_band_ext_batch_dev) on the GPU.  The yardstick
for every pair is the single-pair call on the same engine -- gsa_align_pair_band_ext_dev /
gsa_score_band_ext_dev, themselves pinned to tests/_band_ext_oracle.py by
tests/test_gpu_align_pair_band_ext.py -- field for field plus the per-pair info
(tests/_band_ext_cases.py); pairs small enough are also checked against the oracle directly, and every CIGAR
is replayed.  Cases: a mixed batch (one strip, several strips, trimmed, score 0, empty sides, two entries
naming the same buffers) in every order, on 4, 8 and 16 waves and on capped grids; one workgroup that runs a
high-scoring pair and then a pair of score 0; a wave's second strip on 4 waves; rounds under small scratch
limits and a pair whose codes exceed the limit; the CIGAR buffer through the raw ABI; the refusals; the
calls' neighbours and a stream."""
import numpy as np
import pytest

import gpuseqalign_amd as gsa
from tests import _band_batch_cases as bc
from tests import _band_ext_cases as ec
from tests._band_ext_cases import FIELDS, GAP_IDS, GAPS, UNIT, blosum_like, geometry, planted, random_seq, related, table, tied

pytestmark = pytest.mark.gpu
INV = gsa.NwStat.errorInvalidValue


@pytest.fixture(scope="module")
def geo(engine):
    """(TR, KR, lag, NWV), read from a first call's info."""
    y = random_seq(np.random.default_rng(0), 4, 5)
    engine.align_pair_band_ext(y, y, table(), -2, -1, band=1)
    return geometry(engine.last_align_pair_band_ext_info())


def _mixed(geo):
    TR, KR, _, _ = geo
    rng = np.random.default_rng(81)
    pairs, bands = [], []

    def add(y, x, lo, hi):
        pairs.append((y, x))
        bands.append((lo, hi))

    def ends(R, C, lo, hi, frac, rate=0.1):
        """Related for the first frac of the subject, unrelated behind."""
        y = random_seq(rng, 4, R)
        x = related(rng, y, 4, C, rate)
        cut = int(frac * C)
        x[1 + cut:] = random_seq(rng, 4, C)[1 + cut:]
        add(y, x, lo, hi)

    ends(1, 2, 0, 1, 1.0)
    ends(2, 1, -1, 0, 1.0)
    ends(3, 3, 0, 0, 1.0)                        # W = 1
    ends(KR, KR + 1, -2, 3, 1.0)
    ends(KR + 1, KR + 71, 0, 70, 0.5)
    ends(TR - 1, TR - 71, -75, 6, 0.7)           # one strip
    ends(TR, TR + 300, -3, 300, 0.3)
    ends(2 * TR + 1, 2 * TR - 20, -31, 12, 0.9)  # three strips
    y = random_seq(rng, 4, 700)
    x = related(rng, y, 4, 700)
    x[500:] = random_seq(rng, 4, 700)[500:]
    add(y, x, -31, 31)                           # W = 63
    add(y, x, -32, 31)                           # the same buffers with another band: W = 64
    ends(700, 690, -64, 64, 0.6)                 # W = 129
    ends(700, 700, -512, 512, 0.8)               # W = 1025
    ends(3 * TR, 100, -20, 7, 1.0)               # trimmed to 120 rows: one strip
    ends(90, 9 * TR, -5, 30, 1.0)                # trimmed to 120 columns
    ends(300, 310, -1000, 2000, 0.5)             # clamped to the whole matrix
    e = np.array([0], np.int32)
    add(y, e, -700, 0)                           # an empty side
    add(e, e, 0, 0)
    add(e, x, -3, 3)
    add(y, x, -31, 31)                           # the entry of W = 63 once more
    add(*planted(rng, 0, TR + 9, TR + 5), -9, 9)  # score 0 on two strips
    add(*planted(rng, TR + 1, 2 * TR, 2 * TR), -6, 6)
    add(*tied(rng, TR - 1, TR + 30, TR + 30), -5, 8)  # a tie across the strip boundary
    add(random_seq(rng, 4, 400), random_seq(rng, 4, 380), -40, 30)  # unrelated
    ends(2, 2, 0, 1, 1.0)
    return pairs, bands


@pytest.mark.parametrize("go,ge", GAPS, ids=GAP_IDS)
def test_mixed_batch_in_every_order_on_every_waves_count_and_grid(engine, geo, go, ge):
    pairs, bands = _mixed(geo)
    sub = UNIT
    n = len(pairs)
    assert n == 24
    dev = ec.DevBatch(engine, pairs, sub)
    first, info = dev.align(go, ge, bands)
    sfirst = dev.score(go, ge, bands)
    ec.against_single(first, info["pairs"], sfirst, ec.singles(engine, pairs, bands, sub, go, ge), pairs, sub, go, ge)
    ec.against_oracle(first, info["pairs"], pairs, bands, sub, go, ge)
    assert (info["batch_pairs"], info["host_pairs"], info["nocode_pairs"], info["rounds"]) == (n - 3, 3, 0, 1)
    assert info["strip_rows"] == geo[0] and info["waves"] == 4  # every band here is at most 1218 wide
    assert info["code_bytes"] == sum(q["code_bytes"] for q in info["pairs"])
    assert info["rows_used"] == sum(q["rows_used"] for q in info["pairs"] if q["round"] >= 0)
    assert info["cols_used"] == sum(q["cols_used"] for q in info["pairs"] if q["round"] >= 0)
    assert info["fill_ms"] > 0 and info["walk_ms"] > 0 and info["nocode_ms"] == 0
    assert first[19] == dict(zip(FIELDS, (0, 0, 0, 0, 0, "")), status=0)
    orders = [list(range(n)), list(range(n))[::-1], [int(p) for p in np.random.default_rng(82).permutation(n)]]
    for order in orders:
        for waves in (0, 4, 8, 16):
            for wgs in (0, 1, 3):
                got, inf = dev.align(go, ge, bands, order, waves=waves, max_workgroups=wgs)
                assert got == first, (order, waves, wgs)
                assert inf["pairs"] == info["pairs"]
                assert inf["waves"] == (waves or 4)
                assert dev.score(go, ge, bands, order, waves=waves, max_workgroups=wgs) == sfirst, (order, waves, wgs)


@pytest.mark.parametrize("waves", (0, 4, 8, 16))
def test_one_workgroup_runs_a_high_score_and_then_a_score_of_zero(engine, geo, waves):
    """max_workgroups = 1: the pairs run one after the other, longest first.  The short pair behind the long
    high-scoring one must still return 0 at (0, 0): the best value is set anew per pair."""
    TR, KR, lag, nwv = geo
    rng = np.random.default_rng(83)
    R = 5 * TR + 7  # on 4 waves the first wave takes a second strip
    big = planted(rng, R - 2, R, R + 30)
    zero = (np.array([0, 2, 2, 2, 2], np.int32), np.array([0, 3, 3, 3, 3, 3], np.int32))
    mid = planted(rng, KR + 1, TR + 3, TR + 3)
    pairs, bands = [zero, big, zero, mid], [(-4, 5), (-20, 20), (0, 0), (-8, 8)]
    dev = ec.DevBatch(engine, pairs, UNIT)
    z = dict(zip(FIELDS, (0, 0, 0, 0, 0, "")), status=0)
    want = [z, dict(zip(FIELDS, ec.planted_want(R - 2)), status=0), z, dict(zip(FIELDS, ec.planted_want(KR + 1)), status=0)]
    for wgs in (1, 0, 3):
        for go, ge in ((-3, -1), (0, 0)):
            got, info = dev.align(go, ge, bands, waves=waves, max_workgroups=wgs)
            assert got == want, (waves, wgs, go, ge)
            assert info["pairs"][1]["strips"] == 6 and info["waves"] == (waves or 4)
            assert [(q["score"], q["i_end"], q["j_end"]) for q in dev.score(go, ge, bands, waves=waves, max_workgroups=wgs)] == \
                [(q["score"], q["i_end"], q["j_end"]) for q in want]


@pytest.mark.parametrize("go,ge", [(-11, -1), (-4, -4)], ids=["-11_-1", "-4_-4"])
def test_rounds_under_small_scratch_limits(engine, geo, go, ge):
    TR = geo[0]
    rng = np.random.default_rng(84)
    sub = blosum_like(rng)
    pairs, bands = [], []
    for R, C, lo, hi in ((900, 880, -40, 40), (300, 310, -10, 20), (520, 500, -64, 64), (TR, TR, -3, 3), (2 * TR + 5, 90, -30, 8),
                         (700, 720, -100, 100)):
        y = random_seq(rng, 20, R)
        x = related(rng, y, 20, C, 0.15)
        x[1 + (2 * C) // 3:] = random_seq(rng, 20, C)[1 + (2 * C) // 3:]
        pairs.append((y, x))
        bands.append((lo, hi))
    dev = ec.DevBatch(engine, pairs, sub)
    whole, info = dev.align(go, ge, bands)
    sc = dev.score(go, ge, bands)
    ec.against_single(whole, info["pairs"], sc, ec.singles(engine, pairs, bands, sub, go, ge), pairs, sub, go, ge)
    cb = [q["code_bytes"] for q in info["pairs"]]
    assert info["rounds"] == 1 and info["code_bytes"] == sum(cb)
    # the largest pair's bytes: every pair fits alone, several rounds
    limit = max(cb)
    rounds, round_of, peak = bc.plan_rounds(cb, limit)
    assert len(rounds) >= 2
    got, inf = dev.align(go, ge, bands, scratch_limit=limit)
    assert got == whole and inf["rounds"] == len(rounds) and inf["code_bytes"] == peak
    assert [q["round"] for q in inf["pairs"]] == round_of
    for waves in (4, 16):
        assert dev.align(go, ge, bands, scratch_limit=limit, waves=waves, max_workgroups=1)[0] == whole
    # one byte short of the largest: that pair runs without codes (status 1), the others are unaffected
    big = cb.index(limit)
    got, inf = dev.align(go, ge, bands, scratch_limit=limit - 1)
    rounds, round_of, peak = bc.plan_rounds(cb, limit - 1)
    assert inf["nocode_pairs"] == 1 and inf["nocode_ms"] > 0 and [q["round"] for q in inf["pairs"]] == round_of
    assert round_of[big] == -2 and inf["rounds"] == len(rounds) >= 2
    for p in range(len(pairs)):
        if p == big:
            assert got[p] == dict(whole[p], status=1, cigar="")
        else:
            assert got[p] == whole[p]
    ec.against_single(got, inf["pairs"], sc, ec.singles(engine, pairs, bands, sub, go, ge, scratch_limit=limit - 1),
                      pairs, sub, go, ge)


def test_cigar_buffer_through_the_raw_abi(engine):
    rng = np.random.default_rng(85)
    sub = table()
    pairs, bands = [], []
    for R, C in ((90, 95), (40, 30), (5, 5)):
        y = random_seq(rng, 4, R)
        pairs.append((y, related(rng, y, 4, C, 0.2)))
        bands.append((-6, 9))
    e = np.array([0], np.int32)
    pairs.append((e, pairs[0][1]))
    bands.append((0, 4))
    dev = ec.DevBatch(engine, pairs, sub)
    want, _ = dev.align(-4, -4, bands)
    lens = [len(w["cigar"]) for w in want]
    assert lens[3] == 0 and min(lens[:3]) > 0
    total = sum(l + 1 for l in lens)
    st, res, buf, need, pinfo, info = dev.raw_align(-4, -4, bands, total)
    assert (st, need) == (0, total) and [r.status for r in res] == [0, 0, 0, 0]
    at = 0
    for p, w in enumerate(want):
        assert (res[p].cigar_off, res[p].cigar_len) == (at, lens[p])
        assert buf.raw[at:at + lens[p] + 1] == w["cigar"].encode() + b"\0"
        assert (res[p].score, res[p].i_start, res[p].j_start, res[p].i_end, res[p].j_end) == tuple(w[k] for k in FIELDS[:5])
        at += lens[p] + 1
    # one byte short: the last string that needs the byte does not fit; offsets do not depend on the cap
    st, res, buf, need, _, _ = dev.raw_align(-4, -4, bands, total - 1)
    assert (st, need) == (0, total) and [r.status for r in res] == [0, 0, 0, 2]
    st, res, _, need, _, _ = dev.raw_align(-4, -4, bands, 0, null_cigar=True)
    assert (st, need) == (0, total) and [r.status for r in res] == [2, 2, 2, 2]
    assert [(r.score, r.i_end, r.j_end) for r in res] == [(w["score"], w["i_end"], w["j_end"]) for w in want]


def test_refusals_leave_out_untouched(engine):
    rng = np.random.default_rng(86)
    sub = table()
    y = random_seq(rng, 4, 400)
    pairs = [(y, related(rng, y, 4, 410)), (random_seq(rng, 4, 9), random_seq(rng, 4, 4))]
    bands = [(-10, 20), (-5, 0)]
    dev = ec.DevBatch(engine, pairs, sub)
    fill = 777

    def untouched(res):
        return all((q.score, q.status, q.i_end, q.cigar_off) == (fill,) * 4 for q in res)

    for kw in (dict(waves=3), dict(waves=32), dict(max_workgroups=-1), dict(npairs=-1), dict(go=-1, ge=-4), dict(go=-4, ge=1),
               dict(scratch_limit=-1), dict(cap=-1), dict(cap=8, null_cigar=True)):
        go, ge, cap = kw.pop("go", -3), kw.pop("ge", -1), kw.pop("cap", 4000)
        st, res, _, _, _, _ = dev.raw_align(go, ge, bands, cap, fill=fill, **kw)
        assert st == INV and untouched(res), kw
    assert dev.raw_align(-3, -1, bands, 4000, null_out=True)[0] == INV
    for bad in ((1, 20), (-10, -1), (5, 3)):
        st, res, _, _, _, _ = dev.raw_align(-3, -1, [bands[0], bad], 4000, fill=fill)  # one invalid pair refuses the call
        assert st == INV and untouched(res), bad
    st, res, _, need, _, info = dev.raw_align(-3, -1, bands, 4000, fill=fill)
    assert st == 0 and not untouched(res) and info.batch_pairs == 2
    st, res, _, need, _, info = dev.raw_align(-3, -1, bands, 4000, npairs=0, fill=fill)
    assert (st, need, info.batch_pairs, info.rounds) == (0, 0, 0, 0) and untouched(res)


def test_neighbours_launch_record_and_a_stream(engine):
    import torch
    rng = np.random.default_rng(87)
    sub = blosum_like(rng)
    pairs, bands = [], []
    for R, C in ((1500, 1450), (300, 320)):
        y = random_seq(rng, 20, R)
        x = related(rng, y, 20, C, 0.15)
        x[C // 2:] = random_seq(rng, 20, C)[C // 2:]
        pairs.append((y, x))
        bands.append((-30, 40))
    dev = ec.DevBatch(engine, pairs, sub)
    args = dev.ptrs[0] + (dev.dS.data_ptr(), 20, -11, -1)

    def others():
        s = engine.score_dev(*args)
        a = engine.align_pair_dev(*args)
        b = engine.align_batch_band_dev(dev.ptrs, dev.dS.data_ptr(), 20, -11, -1, bands=[(-80, 30), (-10, 30)])
        s.pop("kernel_ms")
        a.pop("kernel_ms")
        return s, a, bc.strip_ms(b)

    before = others()
    launch = engine.last_launch()
    want, info = dev.align(-11, -1, bands)
    ec.against_oracle(want, info["pairs"], pairs, bands, sub, -11, -1, max_cells=3000000)
    st = torch.cuda.Stream(device=torch.device("cuda", engine.device))
    assert dev.align(-11, -1, bands, stream=st.cuda_stream)[0] == want
    assert engine.last_launch() == launch
    assert others() == before
