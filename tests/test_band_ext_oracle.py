"""tests/_band_ext_oracle.py pinned to facts it does not compute itself, on pairs with
R, C <= 12 and seven gap models:

  * the score is max(0, the best global score of any pair of prefixes), by tests/_band_oracle.score on
    the full band, and the end cell is the first such prefix pair in row-major order;
  * replaying the CIGAR with tests/_align_oracle.rescore gives (score, i_end, j_end);
  * trimming: the result on the prefixes of R' = min(R, C - lo), C' = min(C, R + hi) letters is the
    result on the whole pair, and the band holds (R', C');
  * the certificate: whenever it is 1, the six fields are those of the full band -R ... C; at least a
    third of the proper bands tried are certified, so the property is not vacuous."""
import numpy as np

from tests import _align_oracle as ao
from tests import _band_ext_oracle as eo
from tests import _band_oracle as bo

GAPS7 = [(-11, -1), (-4, -4), (-5, -2), (0, 0), (-7, 0), (-1, -1), (-3, -1)]


def _table(rng, n, kind):
    if kind == 0:
        t = np.full((n, n), -1, np.int32)
        np.fill_diagonal(t, 1)
    elif kind == 1:
        t = np.full((n, n), -2, np.int32)
        np.fill_diagonal(t, 3)
    else:
        t = rng.integers(-4, 3, size=(n, n))
        t = np.minimum(t, t.T)
        np.fill_diagonal(t, rng.integers(1, 6, size=n))
    return t.astype(np.int32)


def _pair(rng, n, R, C):
    y = np.concatenate([[0], rng.integers(0, n, size=R)]).astype(np.int32)
    if rng.random() < 0.6 and R and C:
        # related for a prefix, unrelated behind
        body = np.concatenate([y[1:], rng.integers(0, n, size=C)])[:C].copy()
        cut = int(rng.integers(0, C + 1))
        body[cut:] = rng.integers(0, n, size=C - cut)
        x = np.concatenate([[0], body]).astype(np.int32)
    else:
        x = np.concatenate([[0], rng.integers(0, n, size=C)]).astype(np.int32)
    return y, x


def _cases(seed, count):
    rng = np.random.default_rng(seed)
    for k in range(count):
        n = int(rng.integers(2, 5))
        R, C = int(rng.integers(0, 13)), int(rng.integers(0, 13))
        y, x = _pair(rng, n, R, C)
        sub = _table(rng, n, k % 3)
        go, ge = GAPS7[k % len(GAPS7)]
        yield rng, y, x, sub, go, ge, R, C


def test_score_is_the_best_global_score_of_any_prefix_pair():
    for rng, y, x, sub, go, ge, R, C in _cases(11, 120):
        lo, hi = -R, C
        best, cell = 0, (0, 0)
        for i in range(0, R + 1):
            for j in range(0, C + 1):
                if i == 0 and j == 0:
                    continue
                s = bo.score(y[:i + 1], x[:j + 1], sub, go, ge, -i, j)
                if s > best:
                    best, cell = s, (i, j)
        assert eo.score(y, x, sub, go, ge, lo, hi) == (best,) + cell, (R, C, go, ge)


def test_cigar_replays_to_score_and_end_cell():
    for rng, y, x, sub, go, ge, R, C in _cases(12, 300):
        lo, hi = -int(rng.integers(0, R + 2)), int(rng.integers(0, C + 2))
        s, i0, j0, ie, je, cig = eo.align(y, x, sub, go, ge, lo, hi)
        assert (i0, j0) == (0, 0) and s >= 0 and lo <= je - ie <= hi
        assert ao.rescore(cig, y, x, 0, 0, sub, go, ge) == (s, ie, je), (cig, R, C, lo, hi)
        if s == 0:
            assert (ie, je, cig) == (0, 0, "")


def test_trimming_identity():
    trimmed = 0
    for rng, y, x, sub, go, ge, R, C in _cases(13, 400):
        lo, hi = -int(rng.integers(0, R + 3)), int(rng.integers(0, C + 3))
        Ru, Cu = eo.trim(R, C, lo, hi)
        clo, chi = eo.clamp(R, C, lo, hi)
        assert 0 <= Ru <= R and 0 <= Cu <= C and (Ru == R or Cu == C)
        assert bo.valid(Ru, Cu, clo, chi)  # the global plan takes the trimmed pair
        assert bo.clamp(Ru, Cu, clo, chi) == (clo, chi)
        trimmed += (Ru, Cu) != (R, C)
        assert eo.align(y[:Ru + 1], x[:Cu + 1], sub, go, ge, lo, hi) == eo.align(y, x, sub, go, ge, lo, hi)
    assert trimmed >= 50


def test_certified_results_are_the_unbanded_ones():
    proper = certified = 0
    for rng, y, x, sub, go, ge, R, C in _cases(14, 500):
        if R == 0 or C == 0:
            continue
        full = eo.align(y, x, sub, go, ge, -R, C)
        for lo in range(-R, 1):
            for hi in range(0, C + 1):
                if (lo, hi) == (-R, C) or rng.random() < 0.7:
                    continue
                got = eo.align(y, x, sub, go, ge, lo, hi)
                assert got[0] <= full[0]
                proper += 1
                if eo.certificate(R, C, lo, hi, sub, go, ge, got[0]):
                    certified += 1
                    assert got == full, (R, C, lo, hi, go, ge, got, full)
    assert proper > 3000 and 3 * certified >= proper, (proper, certified)
