"""The banded oracle (tests/_band_oracle.py) against the unbanded one (tests/_align_oracle.py), and the
certificate of include/gsa.h on random small pairs.  CPU only."""
import numpy as np
import pytest

from tests import _align_oracle as ao
from tests import _band_oracle as bo

GAPS = [(-11, -1), (-4, -4), (-5, -2), (0, 0), (-7, 0)]


def _table(rng, n):
    t = rng.integers(-4, 1, size=(n, n))
    t = np.minimum(t, t.T)
    np.fill_diagonal(t, rng.integers(1, 6, size=n))
    return t.astype(np.int32)


def _pair(rng, n, related):
    R = int(rng.integers(1, 40))
    y = rng.integers(0, n, size=R)
    if related:
        x = []
        for v in y:
            u = rng.random()
            if u < 0.08:
                continue
            x.append(int(v) if u > 0.2 else int(rng.integers(0, n)))
            if rng.random() < 0.08:
                x.extend(int(w) for w in rng.integers(0, n, size=int(rng.integers(1, 6))))
        x = np.array(x if x else [0])
    else:
        x = rng.integers(0, n, size=int(rng.integers(1, 40)))
    return np.concatenate([[0], y]).astype(np.int32), np.concatenate([[0], x]).astype(np.int32)


def _cases(count, seed):
    rng = np.random.default_rng(seed)
    for k in range(count):
        n = 2 if k % 2 else 4
        y, x = _pair(rng, n, related=k % 3 != 0)
        yield rng, y, x, _table(rng, n), GAPS[k % len(GAPS)]


def test_full_band_is_the_unbanded_alignment():
    for rng, y, x, sub, (go, ge) in _cases(60, 1):
        R, C = len(y) - 1, len(x) - 1
        want = ao.align(y, x, sub, go, ge, False)
        assert bo.align(y, x, sub, go, ge, -R, C) == want
        assert bo.align(y, x, sub, go, ge, -R - 7, C + 9) == want
        assert bo.align(y, x, sub, go, ge, -R, C, wide=True) == want


def test_banded_score_is_no_larger_and_the_walk_stays_inside():
    for rng, y, x, sub, (go, ge) in _cases(120, 2):
        R, C = len(y) - 1, len(x) - 1
        lo = min(0, C - R) - int(rng.integers(0, 4))
        hi = max(0, C - R) + int(rng.integers(0, 4))
        full = ao.align(y, x, sub, go, ge, False)
        s, i0, j0, i1, j1, cig, path = bo.align(y, x, sub, go, ge, lo, hi, want_path=True)
        assert s <= full[0]
        assert (i0, j0, i1, j1) == (0, 0, R, C)
        assert all(lo <= j - i <= hi for i, j in path)
        assert ao.rescore(cig, y, x, 0, 0, sub, go, ge) == (s, R, C)
        assert bo.score(y, x, sub, go, ge, lo, hi) == s
        assert bo.align(y, x, sub, go, ge, lo, hi, wide=True)[:6] == (s, i0, j0, i1, j1, cig)


def test_certificate_on_random_pairs():
    fired = unfired = lower = other_cigar = 0
    for rng, y, x, sub, (go, ge) in _cases(400, 3):
        R, C = len(y) - 1, len(x) - 1
        k = int(rng.integers(0, 6))
        lo, hi = min(0, C - R) - k, max(0, C - R) + k
        full = ao.align(y, x, sub, go, ge, False)
        got = bo.align(y, x, sub, go, ge, lo, hi)
        if bo.certificate(R, C, lo, hi, sub, go, ge, got[0]):
            fired += 1
            assert got == full, (y, x, sub, go, ge, lo, hi)
        else:
            unfired += 1
            lower += got[0] < full[0]
            other_cigar += got[5] != full[5]
    assert fired >= 50 and unfired >= 50 and lower >= 5 and other_cigar >= 5, (fired, unfired, lower, other_cigar)


def test_validity_and_clamping():
    assert bo.valid(5, 9, 0, 4) and bo.valid(9, 5, -4, 0) and bo.valid(3, 3, 0, 0)
    assert not bo.valid(5, 9, 0, 3) and not bo.valid(5, 9, 1, 4) and not bo.valid(9, 5, -3, 0)
    assert not bo.valid(3, 3, 1, 0)
    assert bo.clamp(5, 9, -100, 100) == (-5, 9) and bo.clamp(5, 9, -2, 6) == (-2, 6)
    # a band that reaches both corners cannot be left: the certificate holds whatever the score
    assert bo.certificate(5, 9, -5, 9, np.array([[1]]), -3, -1, -10 ** 6) == 1
    with pytest.raises(AssertionError):
        bo.align([0, 1, 1], [0, 1], np.array([[1, 0], [0, 1]]), -1, -1, 0, 0)
