"""gsa_score_band_batch_dev on the GPU.  The yardstick for every pair is gsa_score_band_dev on the same engine
(pinned to tests/_band_oracle.py by tests/test_gpu_score_band.py); pairs small enough are also checked
against the oracle directly.  The alignment call's tests (tests/test_gpu_align_batch_band.py) run this call
next to theirs in every case; here are the cases of its own: tiny shapes with every valid band in one
batch, the result struct and the launch's time, pairs whose values only the fill without codes takes, the
refusals through the raw ABI, a stream and the call's neighbours."""
import numpy as np
import pytest

import gpuseqalign_amd as gsa
from tests import _band_batch_cases as bc
from tests import _band_oracle as bo
from tests._band_cases import GAP_IDS, GAPS, blosum_like, random_seq, related, table

pytestmark = pytest.mark.gpu
INV = gsa.NwStat.errorInvalidValue


@pytest.mark.parametrize("go,ge", GAPS, ids=GAP_IDS)
def test_tiny_shapes_every_valid_band_in_one_batch(engine, go, ge):
    rng = np.random.default_rng(51)
    sub = table(2, 2, -1)
    seqs = {L: random_seq(rng, 2, L) for L in (1, 2, 3)}
    pairs, bands = [], []
    for R in (1, 2, 3):
        for C in (1, 2, 3):
            y, x = seqs[R], random_seq(rng, 2, C)
            for lo in range(-R, min(0, C - R) + 1):
                for hi in range(max(0, C - R), C + 1):
                    pairs.append((y, x))  # the same buffers under every band
                    bands.append((lo, hi))
            pairs.append((y, x))
            bands.append((-R - 2, C + 3))  # clamped to the whole matrix
    dev = bc.DevBatch(engine, pairs, sub)
    got = dev.score(go, ge, bands)
    assert len(got) == len(pairs) > 60
    for p, ((y, x), (lo, hi)) in enumerate(zip(pairs, bands)):
        want = bo.align(y, x, sub, go, ge, lo, hi)
        assert got[p] == dict(score=want[0], i_end=len(y) - 1, j_end=len(x) - 1), (p, lo, hi)
    for waves in (4, 8, 16):
        for wgs in (1, 3):
            assert dev.score(go, ge, bands, waves=waves, max_workgroups=wgs) == got


@pytest.mark.parametrize("go,ge", GAPS, ids=GAP_IDS)
def test_batch_against_the_single_call(engine, go, ge):
    rng = np.random.default_rng(52)
    sub = blosum_like(rng)
    e = np.array([0], np.int32)
    pairs, bands = [], []
    for R, C, k in ((700, 690, 20), (1, 1, 0), (257, 300, 3), (1030, 1024, 600), (5, 260, 0), (64, 64, 64)):
        y = random_seq(rng, 20, R)
        pairs.append((y, related(rng, y, 20, C, 0.2)))
        bands.append((min(0, C - R) - k, max(0, C - R) + k))
    pairs += [(e, pairs[0][1]), (pairs[0][0], e)]
    bands += [(0, 690), (-700, 0)]
    r = engine.score_band_batch(pairs, sub, go, ge, bands=bands)
    assert len({q["kernel_ms"] for q in r}) == 1 and r[0]["kernel_ms"] > 0  # the launch's time, in every dict
    for p, ((y, x), (lo, hi)) in enumerate(zip(pairs, bands)):
        one = engine.score_band(y, x, sub, go, ge, band_lo=lo, band_hi=hi)
        assert (r[p]["score"], r[p]["i_end"], r[p]["j_end"]) == (one["score"], one["i_end"], one["j_end"]), p
        if len(y) > 1 and len(x) > 1:
            assert r[p]["score"] == bo.align(y, x, sub, go, ge, lo, hi)[0], p
    # calc_kernel_ms is 0 in every result; the launch's time comes back on its own
    dev = bc.DevBatch(engine, pairs, sub)
    st, res, ms = dev.raw_score(go, ge, bands)
    assert st == 0 and ms > 0 and all(q.calc_kernel_ms == 0 for q in res)
    assert [q.score for q in res] == [q["score"] for q in r]
    # every pair answered on the host: nothing is launched
    host = bc.DevBatch(engine, pairs[-2:], sub)
    st, res, ms = host.raw_score(go, ge, bands[-2:])
    assert st == 0 and ms == 0 and [q.score for q in res] == [go + 689 * ge, go + 699 * ge]


def test_values_past_the_coded_fill_and_the_refusals(engine):
    rng = np.random.default_rng(53)
    sub = table()
    y = random_seq(rng, 4, 400)
    yl = random_seq(rng, 4, 3000)
    pairs = [(y, related(rng, y, 4, 410)), (yl, related(rng, yl, 4, 3000)), (random_seq(rng, 4, 9), random_seq(rng, 4, 4))]
    bands = [(-10, 20), (-30, 30), (-5, 0)]
    dev = bc.DevBatch(engine, pairs, sub)
    # B of the long pair past 2^26 (the alignment call's status 1): the score call takes it, up to B + |go| < 2^29
    g = -(-((1 << 29) - 9000) // 6002)
    got = dev.score(-(g - 1), -(g - 1), bands)
    for p, ((yy, xx), (lo, hi)) in enumerate(zip(pairs, bands)):
        assert got[p]["score"] == engine.score_band(yy, xx, sub, -(g - 1), -(g - 1), band_lo=lo, band_hi=hi)["score"]
    assert got[0]["score"] == bo.align(pairs[0][0], pairs[0][1], sub, -(g - 1), -(g - 1), -10, 20)[0]
    fill = 777
    for kw in (dict(go=-g, ge=-g), dict(waves=3), dict(waves=32), dict(max_workgroups=-1), dict(npairs=-1),
               dict(go=-1, ge=-4), dict(go=-4, ge=1)):
        go, ge = kw.pop("go", -3), kw.pop("ge", -1)
        st, res, _ = dev.raw_score(go, ge, bands, fill=fill, **kw)
        assert st == INV and all((q.score, q.i_end, q.j_end) == (fill,) * 3 for q in res), kw
    for bad in ((1, 20), (-10, 9), (5, 3)):
        st, res, _ = dev.raw_score(-3, -1, [bad] + bands[1:], fill=fill)
        assert st == INV and all((q.score, q.i_end, q.j_end) == (fill,) * 3 for q in res), bad
    with pytest.raises(gsa.NwError) as err:
        engine.score_band_batch_dev(dev.ptrs, dev.dS.data_ptr(), 4, -3, -1, bands=bands, waves=5)
    assert err.value.stat == INV
    assert dev.raw_score(-3, -1, bands)[0] == 0


def test_neighbours_and_a_stream(engine):
    import torch
    rng = np.random.default_rng(54)
    sub = blosum_like(rng)
    pairs, bands = [], []
    for R, C in ((1500, 1450), (300, 320)):
        y = random_seq(rng, 20, R)
        pairs.append((y, related(rng, y, 20, C, 0.15)))
        bands.append((min(0, C - R) - 30, max(0, C - R) + 30))
    dev = bc.DevBatch(engine, pairs, sub)
    args = dev.ptrs[0] + (dev.dS.data_ptr(), 20, -11, -1)

    def others():
        s = engine.score_dev(*args)
        b = engine.score_band_dev(*args, -80, 30)
        s.pop("kernel_ms")
        b.pop("kernel_ms")
        return s, b

    before = others()
    launch = engine.last_launch()
    want = [engine.score_band(y, x, sub, -11, -1, band_lo=lo, band_hi=hi)["score"] for (y, x), (lo, hi) in zip(pairs, bands)]
    st = torch.cuda.Stream(device=torch.device("cuda", engine.device))
    for stream in (None, st.cuda_stream):
        assert [q["score"] for q in dev.score(-11, -1, bands, stream=stream)] == want
    assert engine.last_launch() == launch
    assert others() == before
