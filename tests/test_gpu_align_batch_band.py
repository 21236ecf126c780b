"""gsa_align_batch_band_dev (and, in every case, gsa_score_band_batch_dev) on the GPU.  The yardstick for every
pair is the single-pair call on the same engine -- gsa_align_pair_band_dev / gsa_score_band_dev, themselves
pinned to tests/_band_oracle.py by tests/test_gpu_align_pair_band.py -- field for field plus the per-pair
info (tests/_band_batch_cases.py); pairs small enough are also checked against the oracle directly, and every
CIGAR is replayed.  Cases: a mixed batch in every order, on 4, 8 and 16 waves and on capped grids; waves
that take a second strip on fewer than 16 waves, at the width limits; one workgroup that runs pair after
pair; the rounds at three scratch limits against the plan; the CIGAR buffer through the raw ABI; the
refusals; the calls' neighbours, a stream and the memory statistics; and 64 near-identical pairs against
Engine.align_batch."""
import numpy as np
import pytest

import gpuseqalign_amd as gsa
from tests import _band_batch_cases as bc
from tests import _band_oracle as bo
from tests._band_cases import FIELDS, GAP_IDS, GAPS, blosum_like, geometry, random_seq, related, table

pytestmark = pytest.mark.gpu
INV = gsa.NwStat.errorInvalidValue


@pytest.fixture(scope="module")
def geo(engine):
    """(TR, KR, lag, NWV), read from a first call's info."""
    y = random_seq(np.random.default_rng(0), 4, 5)
    engine.align_pair_band(y, y, table(), -2, -1, band=1)
    return geometry(engine.last_align_pair_band_info())


def _mixed(geo):
    """About 24 pairs: the rows at the lane's and the strip's edges, end cells on the band's edge or inside
    it, widths around a super-step's 64 columns, a clamped and a full band, one pair twice, one pair with two
    bands, empty sides."""
    TR, KR, _, _ = geo
    rng = np.random.default_rng(31)
    pairs, bands = [], []

    def add(y, x, lo, hi):
        pairs.append((y, x))
        bands.append((lo, hi))

    def rel(R, C, lo, hi, rate=0.1):
        y = random_seq(rng, 4, R)
        add(y, related(rng, y, 4, C, rate), lo, hi)

    rel(1, 2, 0, 1)                             # delta +1, minimal
    rel(2, 1, -1, 0)                            # delta -1, minimal
    rel(3, 3, 0, 0)                             # W = 1
    rel(KR, KR + 1, -2, 3)
    rel(KR + 1, KR + 71, 0, 70)                 # delta +70, minimal
    rel(TR - 1, TR - 71, -75, 6)                # delta -70, wider
    rel(TR, TR + 300, 0, 300)                   # delta +300, minimal
    rel(TR + 1, TR + 1, -1, 0)                  # W = 2
    rel(2 * TR + 1, 2 * TR - 299, -310, 12)     # delta -300, wider
    y = random_seq(rng, 4, 700)
    x = related(rng, y, 4, 700)
    add(y, x, -31, 31)                          # W = 63
    add(y, x, -32, 31)                          # the same buffers with another band: W = 64
    rel(700, 701, -32, 32, 0.2)                 # W = 65
    rel(700, 690, -64, 64)                      # W = 129
    rel(700, 700, -512, 512)                    # W = 1025
    rel(300, 310, -1000, 2000)                  # clamped to the whole matrix
    rel(TR + 1, TR + 3, -(TR + 1), TR + 3)      # the full band
    e = np.array([0], np.int32)
    add(y, e, -700, 0)                          # an empty side
    add(e, e, 0, 0)
    rel(1, 301, 0, 300)
    add(y, x, -31, 31)                          # the entry of W = 63 once more
    rel(2 * TR + 1, 2 * TR + 2, 0, 1)
    rel(3, 2, -3, 2)
    add(random_seq(rng, 4, 400), random_seq(rng, 4, 380), -40, 30)  # unrelated
    rel(2, 2, 0, 1)
    return pairs, bands


@pytest.mark.parametrize("go,ge", GAPS, ids=GAP_IDS)
def test_mixed_batch_in_every_order_on_every_waves_count_and_grid(engine, geo, go, ge):
    pairs, bands = _mixed(geo)
    sub = table()
    n = len(pairs)
    assert n == 24
    dev = bc.DevBatch(engine, pairs, sub)
    first, info = dev.align(go, ge, bands)
    sfirst = dev.score(go, ge, bands)
    bc.against_single(first, info["pairs"], sfirst, bc.singles(engine, pairs, bands, sub, go, ge), pairs, sub, go, ge)
    bc.against_oracle(first, info["pairs"], pairs, bands, sub, go, ge)
    assert (info["batch_pairs"], info["host_pairs"], info["nocode_pairs"], info["rounds"]) == (n - 2, 2, 0, 1)
    assert info["strip_rows"] == geo[0] and info["waves"] == 4  # every band here is at most 1218 wide
    assert info["code_bytes"] == sum(q["code_bytes"] for q in info["pairs"])
    assert info["fill_ms"] > 0 and info["walk_ms"] > 0 and info["nocode_ms"] == 0
    orders = [list(range(n)), list(range(n))[::-1], [int(p) for p in np.random.default_rng(32).permutation(n)]]
    for order in orders:
        for waves in (0, 4, 8, 16):
            for wgs in (0, 1, 2):
                got, inf = dev.align(go, ge, bands, order, waves=waves, max_workgroups=wgs)
                assert got == first, (order, waves, wgs)
                assert [{k: v for k, v in q.items()} for q in inf["pairs"]] == info["pairs"]
                assert inf["waves"] == (waves or 4)
                assert dev.score(go, ge, bands, order, waves=waves, max_workgroups=wgs) == sfirst, (order, waves, wgs)


@pytest.mark.parametrize("go,ge", [(-11, -1), (-4, -4)], ids=["-11_-1", "-4_-4"])
def test_waves_take_a_second_strip_at_the_width_limits(engine, geo, go, ge):
    """9 strips on 4 waves at W = 1218 (nq = 4 lag) and 1217, 17 strips on 8 waves at 2754 and 2753, 19
    strips on 16 waves at the width limit."""
    TR, KR, lag, nwv = geo
    assert (TR, lag, nwv) == (256, 6, 16)
    rng = np.random.default_rng(33)
    sub = table(4, 2, -3)
    cases = [(8 * TR + 5, 1218, 4), (8 * TR + 5, 1217, 4), (16 * TR + 5, 2754, 8), (16 * TR + 5, 2753, 8),
             (18 * TR + 5, gsa.band_max_width(), 16)]
    pairs, bands = [], []
    for R, W, _ in cases:
        y = random_seq(rng, 4, R)
        pairs.append((y, related(rng, y, 4, R + 3, 0.05)))
        bands.append((-(W // 2), -(W // 2) + W - 1))
    want = bc.singles(engine, pairs, bands, sub, go, ge)
    for p, (R, W, waves) in enumerate(cases):
        dev = bc.DevBatch(engine, [pairs[p]], sub)
        got, info = dev.align(go, ge, [bands[p]])
        q = info["pairs"][0]
        assert q["band_hi"] - q["band_lo"] + 1 == W and q["strips"] == -(-R // TR) > waves and info["waves"] == waves
        assert bc.nq_of(W) == waves * lag or bc.nq_of(W + 1) == waves * lag
        s = dev.score(go, ge, [bands[p]])
        bc.against_single(got, info["pairs"], s, [want[p]], [pairs[p]], sub, go, ge)
        for forced in (w for w in bc.WAVES if w > waves):
            assert dev.align(go, ge, [bands[p]], waves=forced)[0] == got and dev.score(go, ge, [bands[p]], waves=forced) == s
        for forced in (w for w in bc.WAVES if w < waves):
            with pytest.raises(gsa.NwError) as err:
                dev.align(go, ge, [bands[p]], waves=forced)
            assert err.value.stat == INV
    # all five in one launch: its waves are the widest pair's, the answers the same
    dev = bc.DevBatch(engine, pairs, sub)
    got, info = dev.align(go, ge, bands)
    assert info["waves"] == 16
    bc.against_single(got, info["pairs"], dev.score(go, ge, bands), want, pairs, sub, go, ge)


def test_forced_waves_too_few_for_one_pair(engine, geo):
    TR = geo[0]
    rng = np.random.default_rng(34)
    sub = table()
    y5, y4 = random_seq(rng, 4, 4 * TR + 1), random_seq(rng, 4, 4 * TR)
    small = random_seq(rng, 4, 50)
    band = (-609, 609)  # W = 1219
    many = [(small, small), (y5, related(rng, y5, 4, 4 * TR + 1))]  # 5 strips
    few = [(small, small), (y4, related(rng, y4, 4, 4 * TR))]       # 4 strips
    dm, df = bc.DevBatch(engine, many, sub), bc.DevBatch(engine, few, sub)
    bands = [(-50, 50), band]
    for call in (dm.align, dm.score):
        with pytest.raises(gsa.NwError) as err:
            call(-5, -2, bands, waves=4)
        assert err.value.stat == INV
    got, info = dm.align(-5, -2, bands)
    assert info["waves"] == 8 and info["pairs"][1]["strips"] == 5
    got, info = df.align(-5, -2, bands, waves=4)
    assert info["waves"] == 4 and info["pairs"][1]["strips"] == 4
    bc.against_single(got, info["pairs"], df.score(-5, -2, bands, waves=4), bc.singles(engine, few, bands, sub, -5, -2), few,
                      sub, -5, -2)
    for waves in (1, 2, 3, 5, 32, -4):
        for call in (df.align, df.score):
            with pytest.raises(gsa.NwError) as err:
                call(-5, -2, bands, waves=waves)
            assert err.value.stat == INV


@pytest.mark.parametrize("go,ge", [(-11, -1), (-4, -4)], ids=["-11_-1", "-4_-4"])
def test_one_workgroup_runs_pair_after_pair(engine, geo, go, ge):
    """max_workgroups = 1: big, tiny, big, empty, big.  The workgroup takes them by T descending: 6 strips,
    5 strips, then 2 strips -- fewer than the 4 waves, straight after one with more -- then one row."""
    TR = geo[0]
    rng = np.random.default_rng(35)
    sub = blosum_like(rng)
    e = np.array([0], np.int32)

    def rel(R, C):
        y = random_seq(rng, 20, R)
        return y, related(rng, y, 20, C, 0.15)

    pairs = [rel(5 * TR + 120, 5 * TR + 100), rel(1, 3), rel(4 * TR + 76, 4 * TR + 90), (e, random_seq(rng, 20, 9)),
             rel(TR + 44, TR + 60)]
    bands = [(-120, 80), (0, 2), (-50, 78), (0, 9), (-200, 216)]
    dev = bc.DevBatch(engine, pairs, sub)
    want = bc.singles(engine, pairs, bands, sub, go, ge)
    free, info0 = dev.align(go, ge, bands)
    for waves in (4, 8, 16):
        got, info = dev.align(go, ge, bands, waves=waves, max_workgroups=1)
        assert [q["strips"] for q in info["pairs"]] == [6, 1, 5, 0, 2] and info["waves"] == waves
        T = [q["supersteps"] for q in info["pairs"]]
        assert T[0] > T[2] > T[4] > T[1] > T[3] == 0
        s = dev.score(go, ge, bands, waves=waves, max_workgroups=1)
        bc.against_single(got, info["pairs"], s, want, pairs, sub, go, ge)
        assert got == free and info["pairs"] == info0["pairs"]
    bc.against_oracle(free, info0["pairs"], pairs, bands, sub, go, ge, max_cells=3000000)


def test_rounds_at_three_scratch_limits(engine, geo):
    TR = geo[0]
    rng = np.random.default_rng(36)
    sub = table()
    e = np.array([0], np.int32)
    shapes = [(300, 20), (900, 64), (520, 10), (1300, 30), (260, 100), (800, 5), (40, 3)]
    pairs, bands = [], []
    for R, k in shapes:
        y = random_seq(rng, 4, R)
        pairs.append((y, related(rng, y, 4, R - 7)))
        bands.append((-7 - k, k))
    pairs.insert(3, (e, pairs[0][1]))
    bands.insert(3, (0, len(pairs[0][1]) - 1))
    dev = bc.DevBatch(engine, pairs, sub)
    go, ge = -5, -2
    base, info = dev.align(go, ge, bands)
    cb = [q["code_bytes"] if q["strips"] else -1 for q in info["pairs"]]
    big = max(cb)
    assert cb.count(big) == 1 and cb[3] == -1 and info["rounds"] == 1 and info["code_bytes"] == sum(b for b in cb if b > 0)
    for limit in (big, big - 1, sum(b for b in cb if b > 0)):
        rounds, round_of, peak = bc.plan_rounds(cb, limit)
        got, inf = dev.align(go, ge, bands, scratch_limit=limit)
        assert inf["rounds"] == len(rounds) and inf["code_bytes"] == peak <= limit
        assert [q["round"] for q in inf["pairs"]] == [-1 if r == -3 else r for r in round_of]
        assert inf["nocode_pairs"] == round_of.count(-2) and inf["batch_pairs"] == sum(len(r) for r in rounds)
        assert (inf["nocode_ms"] > 0) == (round_of.count(-2) > 0)
        # the single call under the same limit: status 1 for the one pair over it, the rest unchanged
        want = bc.singles(engine, pairs, bands, sub, go, ge, scratch_limit=limit)
        bc.against_single(got, inf["pairs"], dev.score(go, ge, bands), want, pairs, sub, go, ge)
        for p in range(len(pairs)):
            if round_of[p] == -2:
                assert (got[p]["status"], got[p]["cigar"], got[p]["i_start"], got[p]["j_start"]) == (1, "", 0, 0)
                assert (got[p]["score"], got[p]["i_end"], got[p]["j_end"]) == tuple(base[p][k] for k in ("score", "i_end", "j_end"))
            else:
                assert got[p] == base[p]
    assert len(bc.plan_rounds(cb, big)[0]) > 2 and bc.plan_rounds(cb, big - 1)[1].count(-2) == 1
    assert len(bc.plan_rounds(cb, sum(b for b in cb if b > 0))[0]) == 1


def test_cigar_buffer_through_the_raw_abi(engine):
    rng = np.random.default_rng(37)
    sub = table()
    e = np.array([0], np.int32)
    pairs, bands = [], []
    for R, C in ((90, 95), (30, 30), (0, 4), (300, 280), (61, 64)):
        y = random_seq(rng, 4, R) if R else e
        pairs.append((y, related(rng, y, 4, C, 0.2) if R else random_seq(rng, 4, C)))
        bands.append((min(0, C - R) - 6, max(0, C - R) + 9))
    dev = bc.DevBatch(engine, pairs, sub)
    want, _ = dev.align(-4, -4, bands)
    lens = [len(w["cigar"]) for w in want]
    total = sum(lens) + len(lens)
    offs = [sum(lens[:p]) + p for p in range(len(lens))]

    def fields(r):
        return (r.score, r.i_start, r.j_start, r.i_end, r.j_end)

    st, res, buf, need, pinfo, info = dev.raw_align(-4, -4, bands, total)
    assert (st, need) == (0, total)
    for p, w in enumerate(want):
        assert (res[p].status, res[p].cigar_off, res[p].cigar_len) == (0, offs[p], lens[p])
        assert buf.raw[offs[p]:offs[p] + lens[p] + 1] == w["cigar"].encode() + b"\0"
        assert fields(res[p]) == tuple(w[k] for k in FIELDS[:5])
    st, res, buf, need, _, _ = dev.raw_align(-4, -4, bands, total - 1)
    assert (st, need) == (0, total)
    for p, w in enumerate(want):
        last = p == len(want) - 1
        assert res[p].status == (2 if last else 0) and fields(res[p]) == tuple(w[k] for k in FIELDS[:5])
        if not last:
            assert (res[p].cigar_off, res[p].cigar_len) == (offs[p], lens[p])
            assert buf.raw[offs[p]:offs[p] + lens[p] + 1] == w["cigar"].encode() + b"\0"
    st, res, _, need, _, _ = dev.raw_align(-4, -4, bands, 0, null_cigar=True)
    assert (st, need) == (0, total) and [r.status for r in res] == [2] * len(want)
    assert [fields(r) for r in res] == [tuple(w[k] for k in FIELDS[:5]) for w in want]
    assert dev.raw_align(-4, -4, bands, 8, null_cigar=True)[0] == INV
    assert dev.raw_align(-4, -4, bands, -1)[0] == INV
    assert dev.raw_align(-4, -4, bands, total, scratch_limit=-1)[0] == INV
    assert dev.raw_align(-4, -4, bands, total, max_workgroups=-1)[0] == INV
    assert dev.raw_align(-4, -4, bands, total, null_out=True)[0] == INV
    assert dev.raw_align(-4, -4, bands, total, npairs=-1)[0] == INV
    assert dev.raw_align(-1, -4, bands, total)[0] == INV and dev.raw_align(-4, 1, bands, total)[0] == INV


def test_one_bad_pair_refuses_the_batch_and_leaves_out_untouched(engine):
    rng = np.random.default_rng(38)
    sub = table()
    y, x = random_seq(rng, 4, 40), random_seq(rng, 4, 47)
    yl = random_seq(rng, 4, 3000)
    xl = related(rng, yl, 4, 3000)
    limit = gsa.band_max_width()
    good = [(y, x), (x, y), (yl, xl)]
    gbands = [(0, 7), (-7, 0), (-20, 20)]
    fill = 12345

    def refused(pairs, bands, go=-3, ge=-1):
        dev = bc.DevBatch(engine, pairs, sub)
        st, res, _, _, _, _ = dev.raw_align(go, ge, bands, 100000, fill=fill)
        assert st == INV and all((r.score, r.status, r.i_end, r.cigar_off) == (fill,) * 4 for r in res)
        st, res, _ = dev.raw_score(go, ge, bands, fill=fill)
        assert st == INV and all((r.score, r.i_end, r.j_end) == (fill,) * 3 for r in res)

    # the good ones alone are taken
    dev = bc.DevBatch(engine, good, sub)
    got, info = dev.align(-3, -1, gbands)
    bc.against_single(got, info["pairs"], dev.score(-3, -1, gbands), bc.singles(engine, good, gbands, sub, -3, -1), good, sub,
                      -3, -1)
    for where in (0, 1, 3):
        for bad, band in (((y, x), (0, 6)), ((y, x), (1, 7)), ((x, y), (-6, 0)), ((y, x), (3, 2)),   # invalid bands
                          ((yl, xl), (-(limit // 2), limit - limit // 2)),                          # W = limit + 1
                          ((np.array([0], np.int32), x), (0, 46))):                                  # empty side, invalid
            pairs, bands = list(good), list(gbands)
            pairs.insert(where, bad)
            bands.insert(where, band)
            refused(pairs, bands)
    # the widest band is taken
    wide = (-(limit // 2), limit - 1 - limit // 2)
    d1 = bc.DevBatch(engine, [(yl, xl)], sub)
    got, info = d1.align(-3, -1, [wide])
    assert info["pairs"][0]["band_hi"] - info["pairs"][0]["band_lo"] + 1 == limit and info["waves"] == 16
    bc.against_single(got, info["pairs"], d1.score(-3, -1, [wide]), bc.singles(engine, [(yl, xl)], [wide], sub, -3, -1),
                      [(yl, xl)], sub, -3, -1)
    # the value range: B + |go| reaches 2^29 for the long pair alone.  smax 3, R = C = 3000:
    # B = 9000 + g + 6000 g with go = ge = -g; B + g = 9000 + 6002 g
    g = -(-((1 << 29) - 9000) // 6002)
    assert 9000 + 6002 * g >= 1 << 29 > 9000 + 6002 * (g - 1)
    refused(good, gbands, -g, -g)
    dev = bc.DevBatch(engine, good, sub)
    got, info = dev.align(-(g - 1), -(g - 1), gbands)
    bc.against_single(got, info["pairs"], dev.score(-(g - 1), -(g - 1), gbands),
                      bc.singles(engine, good, gbands, sub, -(g - 1), -(g - 1)), good, sub, -(g - 1), -(g - 1))
    assert [r["status"] for r in got] == [0, 0, 1]  # B of the long pair is past 2^26: score and end cell only


def test_value_bound_of_the_coded_fill_and_an_empty_batch(engine):
    """B = smax min(R, C) + |go| + (R + C) |ge| at 2^26 - 1 and at 2^26: the second is status 1, for that
    pair alone."""
    rng = np.random.default_rng(39)
    sub = table()  # smax 3
    y = random_seq(rng, 4, 100)
    pairs = [(random_seq(rng, 4, 50), random_seq(rng, 4, 50)), (y, related(rng, y, 4, 100)),
             (random_seq(rng, 4, 30), random_seq(rng, 4, 33))]
    bands = [(-5, 5), (-9, 9), (-2, 6)]
    dev = bc.DevBatch(engine, pairs, sub)
    for B, status in (((1 << 26) - 1, 0), (1 << 26, 1)):
        go = -(B - 300)
        got, info = dev.align(go, 0, bands)
        assert [r["status"] for r in got] == [0, status, 0]
        assert [q["round"] for q in info["pairs"]] == [0, -2 if status else 0, 0]
        assert (info["nocode_pairs"], info["batch_pairs"]) == (status, 3 - status)
        bc.against_single(got, info["pairs"], dev.score(go, 0, bands), bc.singles(engine, pairs, bands, sub, go, 0), pairs,
                          sub, go, 0)
    # npairs = 0: nothing launched
    assert engine.align_batch_band([], sub, -3, -1, bands=[]) == [] == engine.score_band_batch([], sub, -3, -1, band=3)
    info = engine.last_align_batch_band_info()
    assert info["pairs"] == [] and (info["batch_pairs"], info["rounds"], info["waves"], info["strip_rows"]) == (0, 0, 0, 0)
    st, _, _, need, _, _ = dev.raw_align(-3, -1, bands, 0, null_cigar=True, npairs=0)
    assert (st, need) == (0, 0) and dev.raw_score(-3, -1, bands, npairs=0)[0] == 0
    # the host forms: band=k is Engine._band_of per pair
    a = engine.align_batch_band(pairs, sub, -3, -1, band=4)
    b = engine.align_batch_band(pairs, sub, -3, -1, bands=[gsa.Engine._band_of(len(p[0]) - 1, len(p[1]) - 1, None, None, 4)
                                                            for p in pairs])
    assert bc.strip_ms(a) == bc.strip_ms(b) and all(r["kernel_ms"] > 0 for r in a)
    for p, (yy, xx) in enumerate(pairs):
        one = engine.align_pair_band(yy, xx, sub, -3, -1, band=4)
        assert {k: a[p][k] for k in FIELDS} == {k: one[k] for k in FIELDS}
    s = engine.score_band_batch(pairs, sub, -3, -1, band=4)
    assert [r["score"] for r in s] == [r["score"] for r in a] and all(r["kernel_ms"] > 0 for r in s)


def test_neighbours_launch_record_and_a_stream(engine):
    import torch
    rng = np.random.default_rng(40)
    sub = blosum_like(rng)
    pairs, bands = [], []
    for R, C in ((1500, 1450), (700, 720), (1100, 1100)):
        y = random_seq(rng, 20, R)
        pairs.append((y, related(rng, y, 20, C, 0.15)))
        bands.append((min(0, C - R) - 30, max(0, C - R) + 30))
    dev = bc.DevBatch(engine, pairs, sub)
    args = dev.ptrs[0] + (dev.dS.data_ptr(), 20, -11, -1)

    def others():
        s = engine.score_dev(*args)
        a = engine.align_pair_band_dev(*args, -80, 30)
        b = engine.align_batch_dev(dev.ptrs, dev.dS.data_ptr(), 20, -11, -1)
        s.pop("kernel_ms")
        a.pop("kernel_ms")
        return s, a, bc.strip_ms(b)

    before = others()
    launch = engine.last_launch()
    want = bc.singles(engine, pairs, bands, sub, -11, -1)
    st = torch.cuda.Stream(device=torch.device("cuda", engine.device))
    for stream in (None, st.cuda_stream):
        got, info = dev.align(-11, -1, bands, stream=stream)
        bc.against_single(got, info["pairs"], dev.score(-11, -1, bands, stream=stream), want, pairs, sub, -11, -1)
    assert engine.last_launch() == launch  # the calls report through their own info struct
    assert others() == before


def test_mem_stats_count_a_rounds_codes(engine):
    """On fresh contexts, so that no earlier call's larger buffers stand in for the batch's.  (The session
    engine is asked for only so that the test is skipped where the others are.)"""
    rng = np.random.default_rng(41)
    sub = table()
    pairs = []
    for R in (1500, 1200, 900):
        y = random_seq(rng, 4, R)
        pairs.append((y, related(rng, y, 4, R - 10)))
    with gsa.Engine(0) as e:
        assert [r["status"] for r in e.align_batch_band(pairs, sub, -5, -2, band=200)] == [0, 0, 0]
        info = e.last_align_batch_band_info()
        stats = e.mem_stats()
        assert info["rounds"] == 1 and info["code_bytes"] == sum(q["code_bytes"] for q in info["pairs"]) > 1000000
        assert stats["glmem_peak_allocs"] >= info["code_bytes"] + sum(len(y) + len(x) - 2 for y, x in pairs)
        # the fill's LDS (the table and the hand-off rings) and registers, no scratch
        assert stats["shmem_peak_allocs"] >= 4096 and stats["regmem_peak_allocs"] > 0 and stats["locmem_peak_allocs"] == 0
        code_bytes = info["code_bytes"]
    with gsa.Engine(0) as e:
        e.score_band_batch(pairs, sub, -5, -2, band=200)
        stats = e.mem_stats()
        assert 0 < stats["glmem_peak_allocs"] < code_bytes and stats["shmem_peak_allocs"] >= 4096


@pytest.mark.parametrize("go,ge", [(-11, -1), (-4, -4)], ids=["-11_-1", "-4_-4"])
def test_64_near_identical_pairs_against_the_unbanded_batch(engine, go, ge):
    """Every pair satisfies the certificate by construction (the pure diagonal, or the one planted gap's
    path, alone beats every path that leaves the band), so the result is Engine.align_batch's."""
    rng = np.random.default_rng(42)
    sub = table(4, 2, -3)
    base = random_seq(rng, 4, 3000)
    pairs = []
    for p in range(64):
        R = int(rng.integers(2000, 3000))
        y = base[:R + 1].copy()
        body = y[1:].copy()
        m = rng.random(R) < 0.004
        body[m] = rng.integers(0, 4, size=int(m.sum()))
        if p % 3 == 0:  # and one deletion of a few letters
            at, g = int(rng.integers(100, R - 100)), int(rng.integers(1, 6))
            body = np.concatenate([body[:at], body[at + g:]])
        pairs.append((y, np.concatenate([[0], body]).astype(np.int32)))
    got = engine.align_batch_band(pairs, sub, go, ge, band=64)
    info = engine.last_align_batch_band_info()
    assert [q["proved_optimal"] for q in info["pairs"]] == [1] * 64
    assert info["batch_pairs"] == 64 and info["rounds"] == 1 and info["waves"] == 4
    full = engine.align_batch(pairs, sub, go, ge)
    for p in range(64):
        assert got[p]["status"] == 0 == full[p]["status"]
        assert {k: got[p][k] for k in FIELDS} == {k: full[p][k] for k in FIELDS}, p
    s = engine.score_band_batch(pairs, sub, go, ge, band=64)
    assert [r["score"] for r in s] == [r["score"] for r in got]
