"""What tests/test_gpu_score_band.py and tests/test_gpu_align_pair_band.py share: the gap models, the
tables, the pairs, and `check`, which runs both banded calls on a pair and asserts everything they return
against tests/_band_oracle.py and the formulas of gpuseqalign_amd/csrc/nw_band_plan.h as DESIGN.md 2.2p
states them.  The geometry (TR, KR, NWV) is read from the info struct and the width limit, not assumed."""
import numpy as np

import gpuseqalign_amd as gsa
from tests import _align_oracle as ao
from tests import _band_oracle as bo

GAPS = [(-11, -1), (-4, -4), (-5, -2), (0, 0), (-7, 0)]
GAP_IDS = ["%d_%d" % g for g in GAPS]
FIELDS = ("score", "i_start", "j_start", "i_end", "j_end", "cigar")


def table(n=4, match=3, mismatch=-2):
    t = np.full((n, n), mismatch, np.int32)
    np.fill_diagonal(t, match)
    return t


def blosum_like(rng, n=20):
    t = rng.integers(-4, 2, size=(n, n))
    t = np.minimum(t, t.T)
    np.fill_diagonal(t, rng.integers(4, 12, size=n))
    return t.astype(np.int32)


def random_seq(rng, n, L):
    return np.concatenate([[0], rng.integers(0, n, size=L)]).astype(np.int32)


def related(rng, y, n, C, sub_rate=0.1):
    """A subject of C letters related to y: y's letters (cut or continued at random) with substitutions."""
    R = len(y) - 1
    body = y[1:C + 1] if C <= R else np.concatenate([y[1:], rng.integers(0, n, size=C - R)])
    body = body.copy()
    m = rng.random(C) < sub_rate
    body[m] = rng.integers(0, n, size=int(m.sum()))
    return np.concatenate([[0], body]).astype(np.int32)


def geometry(info):
    """(TR, KR, lag, NWV) from the info struct and the width limit: max_width = 64 NWV lag - TR + 1 - 63."""
    TR = info["strip_rows"]
    assert TR % 64 == 0
    KR = TR // 64
    lag = KR + 2
    nwv, rem = divmod(gsa.band_max_width() + TR - 1 + 63, 64 * lag)
    assert rem == 0
    return TR, KR, lag, nwv


def want_info(info, R, C, lo, hi):
    """The info fields the plan's formulas give for a pair with R, C >= 1."""
    TR, KR, lag, nwv = geometry(info)
    clo, chi = bo.clamp(R, C, lo, hi)
    W = chi - clo + 1
    strips = -(-R // TR)
    nq = -(-(W + TR - 1 + 63) // 64)
    return dict(strip_rows=TR, strips=strips, waves=min(nwv, strips), supersteps=(strips - 1) * lag + nq,
                band_lo=clo, band_hi=chi, code_bytes=strips * (W + TR - 1) * TR // 2)


def check(engine, y, x, sub, go, ge, lo, hi, want=None, wide=False):
    """Both calls on one pair: the score call, all six fields, the CIGAR, status and every info field
    against the oracle (or `want`), and the CIGAR replayed on the host.  Returns (result, info)."""
    R, C = len(y) - 1, len(x) - 1
    if want is None:
        want = bo.align(y, x, sub, go, ge, lo, hi, wide=wide)
    s = engine.score_band(y, x, sub, go, ge, band_lo=lo, band_hi=hi)
    assert (s["score"], s["i_end"], s["j_end"]) == (want[0], R, C)
    assert s["kernel_ms"] > 0
    a = engine.align_pair_band(y, x, sub, go, ge, band_lo=lo, band_hi=hi)
    assert a["status"] == 0
    assert tuple(a[k] for k in FIELDS) == tuple(want), (R, C, lo, hi, go, ge)
    assert ao.rescore(a["cigar"], y, x, 0, 0, sub, go, ge) == (a["score"], R, C)
    info = engine.last_align_pair_band_info()
    for k, v in want_info(info, R, C, lo, hi).items():
        assert info[k] == v, (k, info[k], v)
    assert info["proved_optimal"] == bo.certificate(R, C, lo, hi, sub, go, ge, a["score"])
    assert info["score_ms"] > 0 and info["walk_ms"] > 0
    assert abs(a["kernel_ms"] - (info["score_ms"] + info["walk_ms"])) < 1e-3
    return a, info
