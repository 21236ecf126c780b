"""tests/_families.py without a GPU: every family's inputs build at both sizes, the decoy has the same
shapes and another result, every letter is below substsz and every table value inside int8, the small
long pairs really span two strips at both strip heights, every accepted input lies inside the
value-range guards of include/gsa.h (B = smax min(R, C) + |go| + (R + C) |ge|: under 2^18 for the
database lane kernels, under 2^26 for the traced long pairs and the fills), and the dirty predecessors lie
on the side of their guard they are meant to.  This keeps the GPU tests from being vacuous."""
import numpy as np
import pytest

from tests import _families as fam
from tests._families import DIRTY, FAMILIES, LARGE, SIZES, SMALL, SUBSTSZ

NAMES_BEFORE = ["fill_sparse", "fill_full", "fill_full_batch", "score", "score_both_ends", "score_scan", "score_batch", "db",
                "trace_sparse", "align_sparse", "align_sparse_pt"]
ENTRY_POINTS_ADDED = ["score_db_multi", "align_db_multi", "score_db_semi", "align_db_semi", "align_pair", "align_batch",
                      "score_semi", "align_pair_semi", "score_semi_batch", "align_batch_semi", "score_overlap",
                      "align_pair_overlap", "score_overlap_batch", "align_batch_overlap"]
VERIFICATION = ["check_sparse", "check_full", "hash_full", "trace_full"]
SEQUENCES = ("y", "x", "q", "db")  # the device inputs that hold letters (also y0, x0, ...)


def test_every_family_is_listed():
    assert [f.name for f in FAMILIES] == NAMES_BEFORE + ENTRY_POINTS_ADDED + VERIFICATION


def _bound(R, C, smax, go, ge):
    return smax * min(R, C) + (-go) + (R + C) * (-ge)


def _gaps(mode):
    return (fam.G, fam.G) if mode is None else mode[:2]


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("family", FAMILIES, ids=lambda f: f.name)
def test_inputs_and_decoy(family, size):
    modes = family.modes(size)
    true, decoy = family.inputs(size), family.inputs(size, decoy=True)
    assert len(true) == len(decoy) == len(modes) >= 1
    for mode, c, d in zip(modes, true, decoy):
        assert sorted(c["dev"]) == sorted(d["dev"])
        differs = 0
        for k in c["dev"]:
            a, b = np.asarray(c["dev"][k]), np.asarray(d["dev"][k])
            assert a.shape == b.shape and a.dtype == b.dtype == np.int32, (k, a.shape, b.shape)
            differs += not np.array_equal(a, b)
            if k.rstrip("0123456789") in SEQUENCES:
                for v in (a, b):
                    assert v.min() >= 0 and v.max() < 20 <= SUBSTSZ, k
            elif k == "sub":
                for v in (a, b):
                    assert v.size == SUBSTSZ * SUBSTSZ and -128 <= v.min() and v.max() <= 127
        assert differs == len(c["dev"]), "a decoy input equals the true one"
        for t in (c, d):  # the value-range guards
            go, ge = _gaps(mode)
            smax = int(np.abs(t["dev"]["sub"]).max())
            if "subjects" in t:
                R = max(len(q) for q in t["queries"]) - 1
                C = max(len(s) for s in t["subjects"]) - 1
                assert _bound(R, C, smax, go, ge) < 1 << 18, (family.name, size, mode)
                assert C <= 8191
            else:
                for k in t["dev"]:
                    if k.startswith("y"):
                        R, C = len(t["dev"][k]) - 1, len(t["dev"]["x" + k[1:]]) - 1
                        assert _bound(R, C, smax, go, ge) < 1 << 26, (family.name, size, mode)
                        assert all(-32767 <= s - go - ge <= 32767 for s in (int(t["dev"]["sub"].min()), smax))
    want = family.want(size)  # (asserts that the decoy's result differs)
    assert len(want) == len(modes)
    assert family.want(size) is want


def test_database_queries_against_the_sweep():
    """The small query lies under one sweep of 16 lanes x 24 rows, the large one over two; the two queries
    of the multi calls differ."""
    for size, lo, hi in [(SMALL, 1, fam.SWEEP), (LARGE, 2 * fam.SWEEP + 1, 3 * fam.SWEEP)]:
        queries, subjects, hits = fam.db_pool(size)
        assert all(lo <= len(q) - 1 <= hi for q in queries) and not np.array_equal(*queries)
        assert len(subjects) == {SMALL: 9, LARGE: 150}[size] and len(set(hits)) == len(hits) >= 6


LONG_ALIGN = ["align_pair", "align_pair_semi", "align_pair_overlap"]
LONG_ALIGN_BATCH = ["align_batch", "align_batch_semi", "align_batch_overlap"]


@pytest.mark.parametrize("name", LONG_ALIGN + LONG_ALIGN_BATCH)
def test_small_long_pairs_span_two_strips(name):
    """At both strip heights (512 rows under -11 / -1, 1024 under -4 / -4 and in every batch) the reference's
    path crosses a strip boundary at a column inside the matrix: the trace fills two strips and reads the
    checkpoint row between them."""
    family = fam.BY_NAME[name]
    heights = set()
    for mode, c, w in zip(family.modes(SMALL), family.inputs(SMALL), family.want(SMALL)):
        tr = fam.BATCH_STRIP if name in LONG_ALIGN_BATCH else family.tr(mode)
        heights.add(tr)
        for k, al in enumerate([w] if name in LONG_ALIGN else w):
            R = len(c["dev"]["y" if name in LONG_ALIGN else "y%d" % k]) - 1
            assert tr < R <= 2 * tr, (name, mode, R, tr)
            assert fam.crosses(al, tr) == 2, (name, mode, k, al[:5])
    assert heights == ({512, 1024} if name in LONG_ALIGN else {1024})


@pytest.mark.parametrize("name", ["score_semi", "score_overlap", "score_semi_batch", "score_overlap_batch"])
def test_small_long_scores_span_two_strips(name):
    family = fam.BY_NAME[name]
    for mode, c in zip(family.modes(SMALL), family.inputs(SMALL)):
        tr = fam.strip_rows(*mode[:2])
        assert all(len(v) - 1 > tr for k, v in c["dev"].items() if k.startswith("y")), (name, mode)


def test_large_is_three_times_small():
    for family in FAMILIES:
        for cs, cl in zip(family.inputs(SMALL), family.inputs(LARGE)):
            for k in cs["dev"]:
                if k != "sub" and k not in ("hr", "hc", "score"):
                    assert len(cl["dev"][k]) >= 2.5 * len(cs["dev"][k]), (family.name, k)


@pytest.mark.parametrize("dirty", DIRTY, ids=lambda d: d.name)
def test_dirty_predecessors_lie_where_they_should(dirty):
    dirty.inputs()
    dirty.guard()
