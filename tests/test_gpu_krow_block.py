"""The K-rows strip wave's block (kr_strip in nw_krow.hip: the halo read ahead of the progress check,
the hand-off, the profile reads, the header-column captures) at the smallest shapes where each of
its paths runs: tile headers word for word against the oracle for the sparse fill in every geometry
and both profile widths, and every cell of two full fills, whose pass 1 runs the same strip wave
(the fused kernel's direct and staged instances)."""
import numpy as np
import pytest

import gpuseqalign_amd as gsa
import oracle
from tests._data import random_pair, related_pair

pytestmark = pytest.mark.gpu

# (R, C, tBx, related)
SHAPES_DEFAULT = [
    (257, 15, 256, False),    # two strips (halo and hand-off run), ramp blocks only
    (257, 63, 256, False),
    (257, 200, 64, True),     # captures in both copies of the block body
    (1024, 1000, 256, True),  # four strips, an even number of blocks
    (1024, 1009, 256, False),  # ... an odd one
    (1025, 300, 256, False),  # two tickets: the granule feed and the drain
    (4096, 600, 256, True),   # 16 strips trailing at the minimum lag: spin, then the halo read again
]
SHAPES_GEOMETRY = [(1025, 300, 256, False), (4096, 600, 256, True)]

_ORACLE = {}


def _pair(R, C, related):
    if related:
        Y, X = related_pair(max(R, C), 31)
    else:
        Y, X = random_pair(R, C, 17)
    return Y[:R + 1], X[:C + 1]


def _headers(Y, X, sub, gapo, tBx, key):
    """The oracle's headers, computed once per (shape, gap)."""
    if key not in _ORACLE:
        hr, hc, _, _, cost = oracle.sparse_headers(Y, X, sub, gapo, gsa.sparse_tile_by(), tBx)
        _ORACLE[key] = (hr, hc, cost)
    return _ORACLE[key]


def _check(engine, golden, R, C, tBx, related, gapo, ns, k, q8):
    Y, X = _pair(R, C, related)
    res = engine.align_sparse(Y, X, golden.blosum62, gapo, tileBx=tBx)
    ll = engine.last_launch()
    assert (ll["kind"], ll["ns"], ll["k"], ll["npairs"]) == ("sparse_krow", ns, k, 1), ll
    # the int8 instance runs first and declines a table outside int8 (the int16 one then fills)
    assert ll["q8"] == 1 and ll["q8_declined"] == (0 if q8 else 1), ll
    hr, hc, cost = _headers(Y, X, golden.blosum62, gapo, tBx, (R, C, tBx, related, gapo))
    assert np.array_equal(res.hrow, hr)
    assert np.array_equal(res.hcol, hc)
    assert res.align_cost == cost


@pytest.mark.parametrize("gapo,q8", [(-11, True), (-60, False)])
@pytest.mark.parametrize("R,C,tBx,related", SHAPES_DEFAULT)
def test_krow_block_default_geometry(engine, golden, knobs, R, C, tBx, related, gapo, q8):
    """The default geometry (4 strips, 4 rows per lane), int8 profile and the int16 fallback (gap -60:
    s - 2g leaves int8)."""
    knobs("GSA_SPARSE_KERNEL", None)
    knobs("GSA_KROW_NS", None)
    knobs("GSA_KROW_K", None)
    knobs("GSA_KROW_Q8", None)
    _check(engine, golden, R, C, tBx, related, gapo, 4, 4, q8)


@pytest.mark.parametrize("gapo,q8", [(-11, True), (-60, False)])
@pytest.mark.parametrize("ns,k", [(4, 2), (2, 4), (8, 4)])
@pytest.mark.parametrize("R,C,tBx,related", SHAPES_GEOMETRY)
def test_krow_block_other_geometries(engine, golden, knobs, R, C, tBx, related, ns, k, gapo, q8):
    """The other instantiated geometries at the two-ticket and the minimum-lag shapes."""
    knobs("GSA_SPARSE_KERNEL", "krow")
    knobs("GSA_KROW_NS", str(ns))
    knobs("GSA_KROW_K", str(k))
    knobs("GSA_KROW_Q8", None)
    _check(engine, golden, R, C, tBx, related, gapo, ns, k, q8)


@pytest.mark.parametrize("staged", ["0", "1"])
@pytest.mark.parametrize("R,C", [(700, 900), (2049, 1100)])
def test_krow_block_fused_full_fill(engine, golden, knobs, R, C, staged):
    """The fused single-pair full fill, whose strips store their rows 64m themselves
    (GSA_FUSED_STAGED=0) or stage them in LDS at the next block's start (1): every cell."""
    knobs("GSA_FULL_KERNEL", "twopass")
    knobs("GSA_FULL_FUSED", "1")
    knobs("GSA_FUSED_STAGED", staged)
    Y, X = random_pair(R, C, 13 * R + C)
    r = engine.align_full(Y, X, golden.blosum62, -11)
    ll = engine.last_launch()
    assert ll["kind"] == "full_fused" and ll["staged"] == int(staged), ll
    key = ("full", R, C)
    if key not in _ORACLE:
        _ORACLE[key] = oracle.fill_full(Y, X, golden.blosum62, -11)
    S, cost = _ORACLE[key]
    assert np.array_equal(r.score, S)
    assert r.align_cost == cost
