"""gsa_score_band_dev on the GPU: scores against the banded oracle on pairs of several strips, the value
guards at 2^26 (where gsa_align_pair_band_dev falls back to the instance without codes) and at 2^29 against
the int64 reference, the width limit, and long related pairs without a CPU oracle, built so that the
certificate holds and the unbanded calls give the reference."""
import numpy as np
import pytest

import gpuseqalign_amd as gsa
from tests import _align_oracle as ao
from tests import _band_oracle as bo
from tests._band_cases import FIELDS, GAP_IDS, GAPS, blosum_like, check, geometry, random_seq, related, table

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("go,ge", GAPS, ids=GAP_IDS)
def test_scores_over_several_strips(engine, go, ge):
    """Random and related pairs of three to four strips with the end cell off the main diagonal."""
    rng = np.random.default_rng(31)
    sub = blosum_like(rng)
    for R, C, lo, hi in ((1600, 1500, -130, 20), (1100, 1700, -1, 640), (1537, 1537, -64, 63)):
        y = random_seq(rng, 20, R)
        for x in (related(rng, y, 20, C, 0.2), random_seq(rng, 20, C)):
            want = bo.score(y, x, sub, go, ge, lo, hi)
            s = engine.score_band(y, x, sub, go, ge, band_lo=lo, band_hi=hi)
            assert (s["score"], s["i_end"], s["j_end"]) == (want, R, C) and s["kernel_ms"] > 0
            assert want <= engine.score(y, x, sub, go, ge)["score"]
    # band=k: k diagonals beyond the ones (0, 0) and (R, C) need
    assert engine.score_band(y, x, sub, go, ge, band=40)["score"] == bo.score(y, x, sub, go, ge, -40, 40)


def _big_table(smax):
    t = np.full((4, 4), -smax, np.int32)
    np.fill_diagonal(t, smax)
    return t


def test_value_bound_on_either_side_of_2_pow_26(engine):
    """B = smax min(R, C) + |go| + (R + C) |ge| = 2^26 - 1: codes, status 0.  B = 2^26: status 1, the score
    from the instance on plain int32 values, still exact against the int64 reference."""
    rng = np.random.default_rng(32)
    y = random_seq(rng, 4, 64)
    x = related(rng, y, 4, 64, 0.3)
    smax = (1 << 20) - 3
    sub = _big_table(smax)
    for go, status in ((-63, 0), (-64, 1)):
        B = smax * 64 - go + 128
        assert (B < (1 << 26)) == (status == 0) and B in ((1 << 26) - 1, 1 << 26)
        want = bo.align(y, x, sub, go, -1, -5, 7, wide=True)
        assert engine.score_band(y, x, sub, go, -1, band_lo=-5, band_hi=7)["score"] == want[0]
        a = engine.align_pair_band(y, x, sub, go, -1, band_lo=-5, band_hi=7)
        info = engine.last_align_pair_band_info()
        assert a["status"] == status and (a["score"], a["i_end"], a["j_end"]) == (want[0], 64, 64)
        assert info["code_bytes"] == (13 + info["strip_rows"] - 1) * info["strip_rows"] // 2
        assert info["proved_optimal"] == bo.certificate(64, 64, -5, 7, sub, go, -1, want[0])
        if status == 0:
            assert tuple(a[k] for k in FIELDS) == want
            assert ao.rescore(a["cigar"], y, x, 0, 0, sub, go, -1) == (want[0], 64, 64)
        else:
            assert a["cigar"] == "" and info["walk_ms"] == 0


def test_value_bound_on_either_side_of_2_pow_29(engine):
    """B + |go| = 2^29 - 2 is taken (score only: status 1), 2^29 is refused by both calls."""
    rng = np.random.default_rng(33)
    y = random_seq(rng, 4, 64)
    x = related(rng, y, 4, 64, 0.3)
    smax = (1 << 23) - 3
    sub = _big_table(smax)
    go = -31
    assert smax * 64 + 128 - 2 * go == (1 << 29) - 2
    want = bo.score(y, x, sub, go, -1, -9, 4, wide=True)
    assert engine.score_band(y, x, sub, go, -1, band_lo=-9, band_hi=4)["score"] == want
    a = engine.align_pair_band(y, x, sub, go, -1, band_lo=-9, band_hi=4)
    assert (a["status"], a["score"], a["cigar"]) == (1, want, "")
    go = -32
    assert smax * 64 + 128 - 2 * go == 1 << 29
    for call in (engine.score_band, engine.align_pair_band):
        with pytest.raises(gsa.NwError) as err:
            call(y, x, sub, go, -1, band_lo=-9, band_hi=4)
        assert err.value.stat == gsa.NwStat.errorInvalidValue


def test_width_limit(engine):
    """W = gsa_band_max_width() is accepted, one more diagonal is refused."""
    wmax = gsa.band_max_width()
    assert wmax >= 4096
    rng = np.random.default_rng(34)
    sub = table()
    R = wmax // 2
    y = random_seq(rng, 4, R)
    x = related(rng, y, 4, R, 0.2)
    lo, hi = -(R - 1), R  # hi = C: W = 2 R = wmax or wmax - 1
    lo -= wmax - (hi - lo + 1)
    assert hi - lo + 1 == wmax and lo >= -R
    a, info = check(engine, y, x, sub, -5, -2, lo, hi)
    assert info["band_hi"] - info["band_lo"] + 1 == wmax
    x2 = related(rng, y, 4, R + 1, 0.2)
    assert bo.valid(R, R + 1, lo, hi + 1)
    for call in (engine.score_band, engine.align_pair_band):
        with pytest.raises(gsa.NwError) as err:
            call(y, x2, sub, -5, -2, band_lo=lo, band_hi=hi + 1)
        assert err.value.stat == gsa.NwStat.errorInvalidValue
    # wider than the limit before clamping only: taken
    assert engine.score_band(y, x, sub, -5, -2, band_lo=lo, band_hi=hi + 10 ** 6)["score"] == a["score"]


@pytest.mark.parametrize("go,ge", GAPS, ids=GAP_IDS)
def test_widest_band_with_more_strips_than_waves(engine, go, ge):
    """The boundary the width limit exists for: W = gsa_band_max_width(), so a strip's super-steps are as many
    as NWV strips' starts (nq = NWV lag), and more strips than waves, so a wave takes its next strip in the
    super-step after it has ended the last.  Score only, against Engine.score under the certificate."""
    wmax = gsa.band_max_width()
    rng = np.random.default_rng(37)
    sub = table(4, 1, -1)
    y = random_seq(rng, 4, 8)
    engine.align_pair_band(y, y, sub, -2, -1, band=1)
    TR, KR, lag, nwv = geometry(engine.last_align_pair_band_info())
    R = (nwv + 2) * TR + 5
    assert 2 * R + 1 > wmax  # the band is narrower than the matrix
    y = random_seq(rng, 4, R)
    x = related(rng, y, 4, R, 0.005)
    lo, hi = -((wmax - 1) // 2), wmax // 2
    assert hi - lo + 1 == wmax and -(-(wmax + TR - 1 + 63) // 64) == nwv * lag
    diagonal = int(sub[y[1:], x[1:]].sum())
    assert bo.certificate(R, R, lo, hi, sub, go, ge, diagonal) == 1
    s = engine.score_band(y, x, sub, go, ge, band_lo=lo, band_hi=hi)
    assert s["score"] >= diagonal and (s["i_end"], s["j_end"]) == (R, R)
    assert s["score"] == engine.score(y, x, sub, go, ge)["score"]
    a = engine.align_pair_band(y, x, sub, go, ge, band_lo=lo, band_hi=hi)
    info = engine.last_align_pair_band_info()
    assert (a["status"], a["score"]) == (0, s["score"]) and info["proved_optimal"] == 1
    assert info["strips"] == nwv + 3 and info["supersteps"] == (nwv + 2) * lag + nwv * lag
    assert ao.rescore(a["cigar"], y, x, 0, 0, sub, go, ge) == (a["score"], R, R)


def _related_long(rng, L, sub_rate, indels):
    """y of L letters and x: y with substitutions at sub_rate and `indels` short insertions or deletions;
    also the score of that planted alignment under match 1, mismatch -1, gaps -2 / -1."""
    y = rng.integers(0, 4, size=L)
    cuts = np.sort(rng.choice(np.arange(100, L - 100), size=indels, replace=False))
    out, score, prev = [], 0, 0
    for k, c in enumerate(cuts):
        seg = y[prev:c].copy()
        m = rng.random(len(seg)) < sub_rate
        seg[m] = (seg[m] + rng.integers(1, 4, size=int(m.sum()))) % 4
        out.append(seg)
        score += len(seg) - 2 * int(m.sum())
        n = int(rng.integers(1, 9))
        if k % 2:
            out.append(rng.integers(0, 4, size=n))  # letters only x has
            prev = c
        else:
            prev = c + n                             # letters only y has
        score += -2 - (n - 1)
    seg = y[prev:]
    out.append(seg)
    score += len(seg)
    x = np.concatenate(out)
    return (np.concatenate([[0], y]).astype(np.int32), np.concatenate([[0], x]).astype(np.int32), score)


def test_long_pair_20k_equals_the_unbanded_alignment(engine):
    """About 2001 diagonals on a related 20k pair whose planted alignment alone beats every path that
    leaves the band: proved_optimal = 1 by construction, and the result is Engine.align_pair's."""
    rng = np.random.default_rng(35)
    sub = table(4, 1, -1)
    y, x, planted = _related_long(rng, 20000, 0.02, 12)
    R, C = len(y) - 1, len(x) - 1
    lo, hi = min(0, C - R) - 1000, max(0, C - R) + 1000
    assert bo.certificate(R, C, lo, hi, sub, -2, -1, planted) == 1
    a = engine.align_pair_band(y, x, sub, -2, -1, band=1000)
    info = engine.last_align_pair_band_info()
    assert a["status"] == 0 and a["score"] >= planted and info["proved_optimal"] == 1
    assert (info["band_lo"], info["band_hi"]) == (lo, hi)
    full = engine.align_pair(y, x, sub, -2, -1)
    assert full["status"] == 0 and {k: a[k] for k in FIELDS} == {k: full[k] for k in FIELDS}
    assert ao.rescore(a["cigar"], y, x, 0, 0, sub, -2, -1) == (a["score"], R, C)
    assert engine.score_band(y, x, sub, -2, -1, band=1000)["score"] == a["score"]


def test_long_pair_200k_scores_as_the_unbanded_call(engine):
    rng = np.random.default_rng(36)
    sub = table(4, 1, -1)
    y, x, planted = _related_long(rng, 200000, 0.004, 16)
    R, C = len(y) - 1, len(x) - 1
    lo, hi = min(0, C - R) - 1000, max(0, C - R) + 1000
    assert bo.certificate(R, C, lo, hi, sub, -2, -1, planted) == 1
    s = engine.score_band(y, x, sub, -2, -1, band=1000)
    assert s["score"] >= planted and (s["i_end"], s["j_end"]) == (R, C)
    assert s["score"] == engine.score(y, x, sub, -2, -1)["score"]
