"""The alignment oracle (tests/_align_oracle.py) pinned on the CPU: its score and end cell are
oracle.score_ag's, its CIGAR replays to that score and cell, local alignments begin and end on a
diagonal move at a cell with H = 0.  No GPU."""
import numpy as np
import pytest

import oracle
from gpuseqalign_amd import formats as F
from tests import _align_oracle as ao
from tests.test_gpu_score import MODES


def _pairs():
    rng = np.random.default_rng(2025)
    out = []
    for k in range(40):
        R, C = (int(v) for v in rng.integers(1, 121, 2))
        y = F.synthetic_seq(R, 3000 + 2 * k)
        if k % 3 == 0:
            # a related pair: the subject is the query with a block cut out and some letters changed
            x = y[1:].copy()
            cut = int(rng.integers(0, max(1, R // 3)))
            at = int(rng.integers(0, R - cut + 1))
            x = np.concatenate([x[:at], x[at + cut:]])
            flip = rng.random(len(x)) < 0.1
            x[flip] = rng.integers(0, 20, int(flip.sum()))
            x = np.concatenate([[0], x]).astype(np.int32) if len(x) else F.synthetic_seq(1, 9)
        else:
            x = F.synthetic_seq(C, 3001 + 2 * k)
        out.append((y, x))
    return out


@pytest.fixture(scope="module")
def pairs():
    return _pairs()


@pytest.mark.parametrize("go,ge,local", MODES)
def test_oracle_against_score_oracle(golden, pairs, go, ge, local):
    sub = golden.blosum62
    for y, x in pairs:
        score, i0, j0, i1, j1, cigar, path, (H, E, Fm) = ao.align(y, x, sub, go, ge, local, want_path=True)
        assert (score, i1, j1) == tuple(oracle.score_ag(y, x, sub, go, ge, local))
        assert ao.rescore(cigar, y, x, i0, j0, sub, go, ge) == (score, i1, j1)
        if local:
            assert H[i0, j0] == 0
            r = ao.runs(cigar)
            if score > 0:
                assert r[0][1] in "=X" and r[-1][1] in "=X", cigar
            else:
                assert cigar == "" and (i0, j0, i1, j1) == (0, 0, 0, 0)
        else:
            assert (i0, j0) == (0, 0)


def test_oracle_known_answers():
    """Match +5, everything else -4: small cases by hand, the tie rule included."""
    sub = np.full((4, 4), -4, np.int32)
    np.fill_diagonal(sub, 5)
    s = lambda letters: np.array([0] + list(letters), np.int32)
    # diagonal before F before E: A x 3 against A x 2, global, linear -- the gap letter comes first
    assert ao.align(s([1, 1, 1]), s([1, 1]), sub, -2, -2, False) == (8, 0, 0, 3, 2, "1I2=")
    assert ao.align(s([1, 1]), s([1, 1, 1]), sub, -2, -2, False) == (8, 0, 0, 2, 3, "1D2=")
    # a gap of three letters opened once: go + 2 ge
    assert ao.align(s([1, 2, 3, 3, 3, 1, 2]), s([1, 2, 1, 2]), sub, -5, -1, False) == (13, 0, 0, 7, 4, "2=3I2=")
    # local: the flanks are left out
    assert ao.align(s([3, 1, 2, 1, 3]), s([2, 1, 2, 1, 2]), sub, -5, -1, True) == (15, 1, 1, 4, 4, "3=")
    # nothing matches: score 0 at (0, 0), no moves
    assert ao.align(s([1, 1]), s([2, 2, 2]), sub, -5, -1, True) == (0, 0, 0, 0, 0, "")
    # empty subject: the query against a gap
    assert ao.align(s([1, 2, 3]), s([]), sub, -5, -1, False) == (-7, 0, 0, 3, 0, "3I")
