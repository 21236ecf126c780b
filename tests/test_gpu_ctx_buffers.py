"""The context's grow-only buffers (csrc/gsa_ctx.h: Buf, reserve, StageRing) under growth: every entry
point family on a fresh engine at a small shape, one several times larger and the small one again;
the pinned staging rings wrapped with copies still in flight; glmem_peak_allocs over that growth; and
contexts created and destroyed in a row.  Every output exactly against the CPU references: the runners
and their references are tests/_families.py's, one per entry-point family.  A fresh gsa.Engine(0) per
test, not the session's, so that growth happens."""
import numpy as np
import pytest

import gpuseqalign_amd as gsa
from tests import _families as fam
from tests._families import BY_NAME, FAMILIES, G, LARGE, SMALL, TRACE_BX, _dev, _empty, _pair

pytestmark = pytest.mark.gpu

GROWTH = (SMALL, LARGE, SMALL)


@pytest.fixture
def fresh():
    """make(): a new engine, closed after the test."""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    made = []

    def make():
        made.append(gsa.Engine(0))
        return made[-1]

    yield make
    for e in made:
        e.close()


@pytest.fixture
def sub():
    return fam.table()


def _substsz(sub):
    return int(round(np.sqrt(np.asarray(sub).size)))


def _headers(R, C, tBx):
    Y, X = _pair(R, C)
    return fam._once(("hdr", R, C, tBx), lambda: fam.headers(Y, X, fam.table(), tBx))


def _matrix(R, C):
    Y, X = _pair(R, C)
    return fam._once(("full", R, C), lambda: fam.matrix(Y, X, fam.table()))


# -- one call of each family at one size, checked: tests/_families.py ---------------------------------

def _full_batch_launch(e, sub, shapes, stream=None):
    pairs = [_pair(R, C) for R, C in shapes]
    s = _dev(sub)
    ins = [(_dev(Y), _dev(X)) for Y, X in pairs]
    outs = [_empty(len(Y) * len(X)) for Y, X in pairs]
    e.fill_batch_dev([(y.data_ptr(), y.numel(), x.data_ptr(), x.numel(), o.data_ptr()) for (y, x), o in zip(ins, outs)],
                     s.data_ptr(), _substsz(sub), G, mode="full", stream=stream)
    return (s, ins), outs


def _full_batch_check(shapes, outs, what):
    for (R, C), o in zip(shapes, outs):
        assert np.array_equal(o.cpu().numpy().reshape(R + 1, C + 1), _matrix(R, C)), (what, R, C)


@pytest.mark.parametrize("family", FAMILIES, ids=lambda f: f.name)
def test_grow_shrink_regrow(fresh, family):
    """Small, then several times larger (every buffer of the family regrows), then small again (in the
    larger buffers): all three results exact."""
    e = fresh()
    for size in GROWTH:
        family.run(e, size)


def test_trace_tile_keeps_codes_in_global_memory():
    """TRACE_BX is past the width at which gsa_trace_sparse_dev keeps a tile's move codes in LDS
    (trace_lds_bytes(tBy, tBx, ., true) <= 160 KiB: 4 (32 x 32 + 6 (tBy + 1) + tBx + 17) bytes and a
    code word per 16 rows of every column, in blocks of 64 columns)."""
    tBy = gsa.sparse_tile_by()
    words = -(-tBy // 16) * -(-TRACE_BX // 64) * 64
    assert 4 * (32 * 32 + 6 * (tBy + 1) + TRACE_BX + 17) + 4 * words > 160 * 1024


# -- the staging rings ---------------------------------------------------------------------------

RING = 7  # batches in flight: more than the ring's four slots + 2


def _ring_shapes(k):
    """Batch k (1 ... RING): k small pairs, so every batch's descriptors are larger than the last."""
    return [(150 + 10 * p + k, 130 + 7 * k + p) for p in range(k)]


def test_staging_ring_wraps_sparse(fresh, sub):
    """Seven sparse batches of 1 ... 7 pairs on one stream with no sync in between: each pinned slot is
    reused (and regrown) while earlier copies may still be in flight."""
    e = fresh()
    s = _dev(sub)
    jobs = []
    for k in range(1, RING + 1):
        shapes = _ring_shapes(k)
        pairs = [_pair(R, C) for R, C in shapes]
        ins = [(_dev(Y), _dev(X)) for Y, X in pairs]
        geoms = [gsa.sparse_geometry(R + 1, C + 1, 64) for R, C in shapes]
        outs = [(_empty(g.hrowElems), _empty(g.hcolElems)) for g in geoms]
        jobs.append((shapes, ins, outs))
    for shapes, ins, outs in jobs:
        e.fill_batch_dev([(y.data_ptr(), y.numel(), x.data_ptr(), x.numel(), (hr.data_ptr(), hc.data_ptr()))
                          for (y, x), (hr, hc) in zip(ins, outs)], s.data_ptr(), _substsz(sub), G, mode="sparse", tileBx=64)
    e.sync()
    for shapes, ins, outs in jobs:
        for (R, C), (hr, hc) in zip(shapes, outs):
            want = _headers(R, C, 64)
            assert np.array_equal(hr.cpu().numpy(), want[0]) and np.array_equal(hc.cpu().numpy(), want[1]), (len(shapes), R, C)


def test_staging_ring_wraps_full(fresh, sub):
    """The same with seven full batches: the descriptor ring and the expansion's ring."""
    e = fresh()
    jobs = [(_ring_shapes(k),) + _full_batch_launch(e, sub, _ring_shapes(k)) for k in range(1, RING + 1)]
    e.sync()
    for shapes, keep, outs in jobs:
        _full_batch_check(shapes, outs, len(shapes))


# -- accounting ----------------------------------------------------------------------------------

@pytest.mark.parametrize("family", [BY_NAME[n] for n in ("fill_sparse", "fill_full", "fill_full_batch", "score_batch")],
                         ids=lambda f: f.name)
def test_peak_allocs_follow_the_capacity_held(fresh, family):
    """glmem_peak_allocs is the device capacity held at a launch: a repeated call allocates nothing, a
    larger one raises it, and buffers never shrink."""
    e = fresh()
    peak = lambda: e.mem_stats()["glmem_peak_allocs"]
    e.reset_mem_stats()
    family.run(e, SMALL)
    p1 = peak()
    assert p1 > 0
    family.run(e, SMALL)
    assert peak() == p1
    family.run(e, LARGE)
    p2 = peak()
    assert p2 > p1
    e.reset_mem_stats()
    assert peak() == 0
    family.run(e, SMALL)
    assert peak() >= p2


# -- lifecycle -----------------------------------------------------------------------------------

def test_create_use_destroy_in_a_row(fresh, sub):
    """Three contexts in a row, each running one call of every family before it is destroyed; a fourth
    still fills correctly."""
    for _ in range(3):
        e = gsa.Engine(0)
        try:
            for family in FAMILIES:
                family.run(e, SMALL)  # (a runner unsets the knob it set)
        finally:
            e.close()
    e = fresh()
    BY_NAME["fill_sparse"].run(e, SMALL)
    BY_NAME["fill_full"].run(e, SMALL)
