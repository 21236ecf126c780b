"""gsa_score_band_ext_batch_dev on the GPU.  The yardstick for every pair is gsa_score_band_ext_dev on the
same engine (pinned to tests/_band_ext_oracle.py by tests/test_gpu_score_band_ext.py and
tests/test_gpu_align_pair_band_ext.py); pairs small enough are also checked against the oracle directly.
The alignment call's tests (tests/test_gpu_align_batch_band_ext.py) run this call next to theirs in every
case; here are the cases of its own: tiny shapes with every valid band in one batch under every waves count
and grid cap, the result struct and the launch's time, a best value that must not survive into the next pair
of a workgroup, the refusals through the raw ABI, a stream and the call's neighbours."""
import numpy as np
import pytest

import gpuseqalign_amd as gsa
from tests import _band_ext_cases as ec
from tests import _band_ext_oracle as eo
from tests._band_ext_cases import GAP_IDS, GAPS, UNIT, blosum_like, planted, random_seq, related, table

pytestmark = pytest.mark.gpu
INV = gsa.NwStat.errorInvalidValue


@pytest.mark.parametrize("go,ge", GAPS, ids=GAP_IDS)
def test_tiny_shapes_every_valid_band_in_one_batch(engine, go, ge):
    rng = np.random.default_rng(71)
    sub = table(2, 2, -1)
    seqs = {L: random_seq(rng, 2, L) for L in (1, 2, 3)}
    pairs, bands = [], []
    for R in (1, 2, 3):
        for C in (1, 2, 3):
            y, x = seqs[R], random_seq(rng, 2, C)
            for lo in range(-R, 1):
                for hi in range(0, C + 1):
                    pairs.append((y, x))  # the same buffers under every band
                    bands.append((lo, hi))
            pairs.append((y, x))
            bands.append((-R - 2, C + 3))  # clamped from far outside
    dev = ec.DevBatch(engine, pairs, sub)
    got = dev.score(go, ge, bands)
    assert len(got) == len(pairs) > 80
    for p, ((y, x), (lo, hi)) in enumerate(zip(pairs, bands)):
        want = eo.score(y, x, sub, go, ge, lo, hi)
        assert got[p] == dict(score=want[0], i_end=want[1], j_end=want[2]), (p, lo, hi)
    for waves in (4, 8, 16):
        for wgs in (1, 3):
            assert dev.score(go, ge, bands, waves=waves, max_workgroups=wgs) == got


@pytest.mark.parametrize("go,ge", GAPS, ids=GAP_IDS)
def test_batch_against_the_single_call(engine, go, ge):
    rng = np.random.default_rng(72)
    sub = blosum_like(rng)
    e = np.array([0], np.int32)
    pairs, bands = [], []
    for R, C, lo, hi in ((700, 690, -20, 20), (1, 1, 0, 0), (257, 300, -3, 46), (1030, 1024, -600, 600), (5, 260, 0, 9),
                         (64, 64, -64, 64), (800, 100, -20, 5)):
        y = random_seq(rng, 20, R)
        x = related(rng, y, 20, C, 0.2)
        cut = int(rng.integers(C // 3, C + 1))
        x[1 + cut:] = random_seq(rng, 20, C)[1 + cut:]
        pairs.append((y, x))
        bands.append((lo, hi))
    pairs += [(e, pairs[0][1]), (pairs[0][0], e)]
    bands += [(0, 690), (-700, 0)]
    r = engine.score_band_ext_batch(pairs, sub, go, ge, bands=bands)
    assert len({q["kernel_ms"] for q in r}) == 1 and r[0]["kernel_ms"] > 0  # the launch's time, in every dict
    for p, ((y, x), (lo, hi)) in enumerate(zip(pairs, bands)):
        one = engine.score_band_ext(y, x, sub, go, ge, band_lo=lo, band_hi=hi)
        assert (r[p]["score"], r[p]["i_end"], r[p]["j_end"]) == (one["score"], one["i_end"], one["j_end"]), p
        assert (r[p]["score"], r[p]["i_end"], r[p]["j_end"]) == eo.score(y, x, sub, go, ge, lo, hi), p
    # band=w is (-w, w) on every pair
    w = engine.score_band_ext_batch(pairs[:3], sub, go, ge, band=30)
    for p, (y, x) in enumerate(pairs[:3]):
        assert (w[p]["score"], w[p]["i_end"], w[p]["j_end"]) == eo.score(y, x, sub, go, ge, -30, 30), p
    # calc_kernel_ms is 0 in every result; the launch's time comes back on its own
    dev = ec.DevBatch(engine, pairs, sub)
    st, res, ms = dev.raw_score(go, ge, bands)
    assert st == 0 and ms > 0 and all(q.calc_kernel_ms == 0 for q in res)
    assert [q.score for q in res] == [q["score"] for q in r]
    # every pair answered on the host: nothing is launched
    host = ec.DevBatch(engine, pairs[-2:], sub)
    st, res, ms = host.raw_score(go, ge, bands[-2:])
    assert st == 0 and ms == 0 and [(q.score, q.i_end, q.j_end) for q in res[:2]] == [(0, 0, 0), (0, 0, 0)]


@pytest.mark.parametrize("waves", (0, 4, 8, 16))
def test_the_best_value_is_reset_between_the_pairs_of_a_workgroup(engine, waves):
    """One workgroup: a long pair of a high score, then a short pair of score 0, then a middling one."""
    rng = np.random.default_rng(73)
    engine.align_pair_band_ext(random_seq(rng, 4, 5), random_seq(rng, 4, 5), UNIT, -2, -1, band=1)
    TR = engine.last_align_pair_band_ext_info()["strip_rows"]
    big = planted(rng, 3 * TR + 7, 3 * TR + 50, 3 * TR + 60)
    zero = (np.array([0, 2, 2, 2, 2], np.int32), np.array([0, 3, 3, 3, 3, 3], np.int32))
    mid = planted(rng, 9, TR + 3, TR + 3)
    pairs, bands = [big, zero, mid, zero], [(-20, 20), (-4, 5), (-8, 8), (0, 0)]
    dev = ec.DevBatch(engine, pairs, UNIT)
    for wgs in (1, 0, 3):
        got = dev.score(-3, -1, bands, waves=waves, max_workgroups=wgs)
        assert got == [dict(score=3 * TR + 7, i_end=3 * TR + 7, j_end=3 * TR + 7), dict(score=0, i_end=0, j_end=0),
                       dict(score=9, i_end=9, j_end=9), dict(score=0, i_end=0, j_end=0)], (waves, wgs)


def test_refusals_leave_out_untouched(engine):
    rng = np.random.default_rng(74)
    sub = table()
    y = random_seq(rng, 4, 400)
    pairs = [(y, related(rng, y, 4, 410)), (random_seq(rng, 4, 9), random_seq(rng, 4, 4))]
    bands = [(-10, 20), (-5, 0)]
    dev = ec.DevBatch(engine, pairs, sub)
    fill = 777
    for kw in (dict(waves=3), dict(waves=32), dict(max_workgroups=-1), dict(npairs=-1), dict(go=-1, ge=-4), dict(go=-4, ge=1)):
        go, ge = kw.pop("go", -3), kw.pop("ge", -1)
        st, res, _ = dev.raw_score(go, ge, bands, fill=fill, **kw)
        assert st == INV and all((q.score, q.i_end, q.j_end) == (fill,) * 3 for q in res), kw
    for bad in ((1, 20), (-10, -1), (5, 3)):
        st, res, _ = dev.raw_score(-3, -1, [bands[0], bad], fill=fill)  # one invalid pair refuses the whole call
        assert st == INV and all((q.score, q.i_end, q.j_end) == (fill,) * 3 for q in res), bad
    with pytest.raises(gsa.NwError) as err:
        engine.score_band_ext_batch_dev(dev.ptrs, dev.dS.data_ptr(), 4, -3, -1, bands=bands, waves=5)
    assert err.value.stat == INV
    assert dev.raw_score(-3, -1, bands)[0] == 0
    st, res, ms = dev.raw_score(-3, -1, bands, npairs=0, fill=fill)  # nothing to do: success, nothing launched
    assert st == 0 and ms == 0 and res[0].score == fill


def test_neighbours_and_a_stream(engine):
    import torch
    rng = np.random.default_rng(75)
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
        b = engine.score_band_dev(*args, -80, 30)
        s.pop("kernel_ms")
        b.pop("kernel_ms")
        return s, b

    before = others()
    launch = engine.last_launch()
    want = [dict(zip(("score", "i_end", "j_end"), eo.score(y, x, sub, -11, -1, lo, hi))) for (y, x), (lo, hi) in zip(pairs, bands)]
    st = torch.cuda.Stream(device=torch.device("cuda", engine.device))
    for stream in (None, st.cuda_stream):
        assert dev.score(-11, -1, bands, stream=stream) == want
    assert engine.last_launch() == launch
    assert others() == before
