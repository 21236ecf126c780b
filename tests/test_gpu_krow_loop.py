"""The K-rows strip wave's block loop (kr_strip in nw_krow.hip): the ramp's 4 blocks, then whole pairs
of blocks in a straight-line body with one loop test, then the odd block; "everything published"
behind the last hand-off; the state a persistent workgroup restarts per ticket; the capture's
bookkeeping from boundary to boundary.  Tile headers word for word and the cost against
oracle.sparse_headers, every cell of the full fills against oracle.fill_full.

The loop runs NB = ceil((Cp + 65) / 16) blocks, Cp = tcols * tBx the padded width (tBx >= 64, a
multiple of 16), so NB = tcols * tBx / 16 + 5.  With tBx a multiple of 64 (64, 256: the full fills'
pass 1 too, whose tile width is 256) NB is odd whatever C is -- the blocks behind the ramp are
odd in number and the loop always ends in its odd block; with tBx = 80, NB = 5 tcols + 5 is even for an odd
tcols, and the loop ends on a whole pair.  The fewest blocks the library can ask for are NB = 9 (one tile
column of 64): a strip with ONE block behind the ramp (NB = 5, Cp < 16) does not exist behind the C API, so
the shortest case here is tBx 64, C = 1.

The watchdog path (a wait that fails ends the loop through its bound) is an induced stall and is not run
here; tests/test_gpu_mlsppt.py and tests/test_gpu_fill_value_ranges.py have the launches that fail."""
import numpy as np
import pytest

import gpuseqalign_amd as gsa
import oracle
from tests._data import random_pair, related_pair

pytestmark = pytest.mark.gpu

CS = [1, 16, 17, 48, 250, 256, 257, 1000, 1009]

_ORACLE = {}


def nb_blocks(C, tBx):
    """Blocks of a strip's loop for C columns (adjcols = C + 1) at tile width tBx."""
    tcols = max(1, -(-C // tBx))
    return (tcols * tBx + 65 + 15) // 16


def _pair(R, C, related=False):
    if related:
        Y, X = related_pair(max(R, C), 31)
    else:
        Y, X = random_pair(R, C, 17)
    return Y[:R + 1], X[:C + 1]


def _headers(Y, X, sub, gapo, tBx, key):
    if key not in _ORACLE:
        hr, hc, _, _, cost = oracle.sparse_headers(Y, X, sub, gapo, gsa.sparse_tile_by(), tBx)
        _ORACLE[key] = (hr, hc, cost)
    return _ORACLE[key]


def _full(Y, X, sub, gapo, key):
    if key not in _ORACLE:
        _ORACLE[key] = oracle.fill_full(Y, X, sub, gapo)
    return _ORACLE[key]


def _default_knobs(knobs):
    for name in ("GSA_SPARSE_KERNEL", "GSA_KROW_NS", "GSA_KROW_K", "GSA_KROW_Q8"):
        knobs(name, None)


def _check_sparse(engine, sub, R, C, tBx, gapo, ns, k, related=False, q8=1, declined=0, overlap=False):
    Y, X = _pair(R, C, related)
    res = engine.align_sparse(Y, X, sub, gapo, tileBx=tBx, overlap=overlap)
    ll = engine.last_launch()
    assert (ll["kind"], ll["ns"], ll["k"], ll["npairs"]) == ("sparse_krow", ns, k, 1), ll
    assert (ll["q8"], ll["q8_declined"]) == (q8, declined), ll
    if overlap:
        assert ll["mlsppt"] == 1, ll
    hr, hc, cost = _headers(Y, X, sub, gapo, tBx, (R, C, tBx, related, gapo))
    assert np.array_equal(res.hrow, hr)
    assert np.array_equal(res.hcol, hc)
    assert res.align_cost == cost


def test_block_counts_cover_both_parities():
    """The cases below, from the geometry: tBx 80 gives an even NB at C = 1 .. 48 (10), 1000 and 1009 (70)
    and an odd one at 250 .. 257 (25); tBx 256 and 64 give odd ones only (21, 37, 69; 9 the shortest)."""
    assert [nb_blocks(C, 80) for C in CS] == [10, 10, 10, 10, 25, 25, 25, 70, 70]
    assert [nb_blocks(C, 256) for C in CS] == [21, 21, 21, 21, 21, 21, 37, 69, 69]
    assert nb_blocks(1, 64) == 9 and min(nb_blocks(C, t) for C in CS for t in (64, 80, 256)) == 9
    assert {nb_blocks(C, t) % 2 for C in CS for t in (80, 256)} == {0, 1}


@pytest.mark.parametrize("tBx", [80, 256])
@pytest.mark.parametrize("C", CS)
@pytest.mark.parametrize("R", [257, 1024])
def test_loop_parity_and_odd_block(engine, golden, knobs, R, C, tBx):
    """Two strips (R = 257) and four (1024): every strip but the first waits for "everything published"
    in its last four blocks, whether the loop ends on a pair (tBx 80, C <= 48 or >= 1000) or on the odd
    block."""
    _default_knobs(knobs)
    _check_sparse(engine, golden.blosum62, R, C, tBx, -11, 4, 4)


def test_loop_shortest(engine, golden, knobs):
    """NB = 9: the ramp, two pairs and the odd block."""
    _default_knobs(knobs)
    _check_sparse(engine, golden.blosum62, 257, 1, 64, -11, 4, 4)


@pytest.mark.parametrize("tBx", [80, 256])
@pytest.mark.parametrize("C", [17, 257, 1009])
def test_three_tickets_middle_fed_and_drained(engine, golden, knobs, C, tBx):
    """R = 2049: three tickets; the middle one's first strip is fed through granules and its last one
    drained, both behind strips that published kBig after their loops."""
    _default_knobs(knobs)
    _check_sparse(engine, golden.blosum62, 2049, C, tBx, -11, 4, 4)


@pytest.mark.parametrize("ns", [4, 8])
def test_batch_restarts_state_per_ticket(engine, golden, knobs, ns):
    """One persistent launch over three pairs of different NB parity (tBx 80: 25, 70 and 140 blocks) and
    2, 3 and 1 tile rows: the loop bound, the ring offset, the next boundary and the header-column
    pointer are a ticket's own."""
    import torch
    knobs("GSA_SPARSE_KERNEL", "krow")
    knobs("GSA_KROW_NS", str(ns))
    knobs("GSA_KROW_K", "4")
    knobs("GSA_KROW_Q8", None)
    tBx = 80
    shapes = [(1025, 300), (2500, 1009), (300, 2100)]
    assert [nb_blocks(C, tBx) % 2 for _, C in shapes] == [1, 0, 0]
    dev = torch.device("cuda:0")
    sub = golden.blosum62
    s = torch.from_numpy(sub).to(dev)
    pairs = [_pair(R, C) for R, C in shapes]
    ins = [(torch.from_numpy(Y).to(dev), torch.from_numpy(X).to(dev)) for Y, X in pairs]
    geoms = [gsa.sparse_geometry(len(Y), len(X), tBx) for Y, X in pairs]
    assert [g.tileHdrMatRows for g in geoms] == [2, 3, 1]
    outs = [(torch.full((g.hrowElems,), -7, dtype=torch.int32, device=dev),
             torch.full((g.hcolElems,), -7, dtype=torch.int32, device=dev)) for g in geoms]
    engine.fill_batch_dev([(y.data_ptr(), y.numel(), x.data_ptr(), x.numel(), (hr.data_ptr(), hc.data_ptr()))
                           for (y, x), (hr, hc) in zip(ins, outs)], s.data_ptr(), 25, -11, tileBx=tBx)
    engine.sync()
    ll = engine.last_launch()
    assert (ll["kind"], ll["ns"], ll["k"], ll["npairs"]) == ("sparse_krow", ns, 4, 3), ll
    for (R, C), (Y, X), (hr, hc) in zip(shapes, pairs, outs):
        ohr, ohc, _ = _headers(Y, X, sub, -11, tBx, (R, C, tBx, False, -11))
        assert np.array_equal(hr.cpu().numpy(), ohr), (R, C)
        assert np.array_equal(hc.cpu().numpy(), ohc), (R, C)


# (C, tBx): every block captures and the boundary advances every 4 blocks (64); no boundary (255, 256: one
# tile column), one (257), three (1000)
CAPTURES = [(200, 64), (255, 256), (256, 256), (257, 256), (1000, 256)]


@pytest.mark.parametrize("gapo", [-11, 3])
@pytest.mark.parametrize("C,tBx", CAPTURES)
def test_capture_bookkeeping(engine, golden, knobs, C, tBx, gapo):
    """The header columns of two tickets (R = 1025), with a negative and a positive gap cost (the
    un-shift (row + column) g of a captured value changes sign)."""
    _default_knobs(knobs)
    _check_sparse(engine, golden.blosum62, 1025, C, tBx, gapo, 4, 4)


@pytest.mark.parametrize("ns,k", [(4, 2), (2, 4), (8, 4)])
@pytest.mark.parametrize("R,C,related", [(1025, 300, False), (4096, 600, True)])
def test_other_geometries(engine, golden, knobs, R, C, related, ns, k):
    knobs("GSA_SPARSE_KERNEL", "krow")
    knobs("GSA_KROW_NS", str(ns))
    knobs("GSA_KROW_K", str(k))
    knobs("GSA_KROW_Q8", None)
    _check_sparse(engine, golden.blosum62, R, C, 256, -11, ns, k, related)


@pytest.mark.parametrize("R,C,related", [(1025, 300, False), (4096, 600, True)])
def test_int16_profile(engine, golden, knobs, R, C, related):
    """GSA_KROW_Q8=0: the int16-profile instance alone."""
    _default_knobs(knobs)
    knobs("GSA_KROW_Q8", "0")
    _check_sparse(engine, golden.blosum62, R, C, 256, -11, 4, 4, related, q8=0)


def test_mlsppt(engine, golden, knobs):
    """The instance that publishes its header columns per chunk of tile columns."""
    _default_knobs(knobs)
    _check_sparse(engine, golden.blosum62, 1100, 1029, 256, -11, 4, 4, overlap=True)


@pytest.mark.parametrize("fused,staged", [("0", "0"), ("1", "0"), ("1", "1")])
@pytest.mark.parametrize("R,C", [(700, 900), (2049, 1100)])
def test_full_fills(engine, golden, knobs, R, C, fused, staged):
    """Pass 1 of the full fill is the same strip wave: the XR instance (two launches) and both fused
    instances (the strips store their rows 64m themselves, or stage them in LDS), every cell."""
    knobs("GSA_FULL_KERNEL", "twopass")
    knobs("GSA_FULL_FUSED", fused)
    knobs("GSA_FUSED_STAGED", staged)
    Y, X = random_pair(R, C, 13 * R + C)
    r = engine.align_full(Y, X, golden.blosum62, -11)
    ll = engine.last_launch()
    if fused == "1":
        assert ll["kind"] == "full_fused" and ll["staged"] == int(staged), ll
    else:
        assert ll["kind"] == "full_two_launch", ll
    S, cost = _full(Y, X, golden.blosum62, -11, ("full", R, C))
    assert np.array_equal(r.score, S)
    assert r.align_cost == cost
