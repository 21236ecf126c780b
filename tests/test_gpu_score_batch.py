"""Batched score-only NW / SW (gsa_score_batch_dev: many pairs in one persistent launch of the
K-rows score kernel, per-pair result words, a finalize kernel) against oracle.score_ag per pair.
Every test that expects the batch kernel also asserts gsa_last_launch: kind score_krow and npairs =
the batch size, so a hidden loop over single pairs would not pass.  A ticket is 512 rows at K = 2
rows per lane and 1024 at K = 4."""
import numpy as np
import pytest

import gpuseqalign_amd as gsa
from gpuseqalign_amd import shard
from tests._data import random_pair
from tests.test_gpu_score import MODES

pytestmark = pytest.mark.gpu

_REF = {}


def _ref(key, Y, X, sub, go, ge, local, **kw):
    """oracle.score_ag, computed once per (pair, table, mode) and shared by the parametrised cases."""
    import oracle
    k = (key, go, ge, local)
    if k not in _REF:
        _REF[k] = oracle.score_ag(Y, X, sub, go, ge, local, **kw)
    return _REF[k]


class _Dev:
    """Pairs and table on the device; `same` maps a pair index to the one whose tensors it shares."""

    def __init__(self, pairs, sub, same=None):
        import torch
        dev = torch.device("cuda:0")
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)
        self.sub = up(np.asarray(sub).ravel())
        self.substsz = int(round(np.sqrt(np.asarray(sub).size)))
        self.t = []
        for i, (y, x) in enumerate(pairs):
            self.t.append(self.t[same[i]] if same and i in same else (up(y), up(x)))
        self.ptrs = [(y.data_ptr(), y.numel(), x.data_ptr(), x.numel()) for y, x in self.t]
        torch.cuda.synchronize(dev)

    def run(self, engine, go, ge, local):
        return engine.score_batch_dev(self.ptrs, self.sub.data_ptr(), self.substsz, go, ge, local)


def _t(r):
    return (r["score"], r["i_end"], r["j_end"])


def _ran_batch(engine, n, **more):
    ll = engine.last_launch()
    assert ll["kind"] == "score_krow" and ll["npairs"] == n and ll["both_ends"] == 0, ll
    for k, v in more.items():
        assert ll[k] == v, (k, ll)
    return ll


# one-, two- and three-ticket pairs at either K, the result cell on every row of a lane, pairs of
# different C sharing the key packing; the last pair is pair 6 again, on the same device pointers
_MIXED = [(1, 3000), (63, 65), (64, 1), (65, 64), (511, 257), (512, 900), (513, 3000), (1024, 65), (1025, 257),
          (2049, 900), (2052, 257), (3071, 3000), (3071, 64), (513, 3000)]


def _mixed_pairs():
    return [random_pair(R, C, 23 * R + C) for R, C in _MIXED]


@pytest.fixture(scope="module")
def mixed(engine, golden):
    return _Dev(_mixed_pairs(), golden.blosum62, same={13: 6})


@pytest.mark.parametrize("q8", ["0", "1", "2"])
@pytest.mark.parametrize("k", ["2", "4"])
@pytest.mark.parametrize("go,ge,local", MODES)
def test_mixed_shapes_one_batch(engine, golden, mixed, knobs, go, ge, local, k, q8):
    knobs("GSA_SCORE_K", k)
    knobs("GSA_KROW_Q8", q8)
    res = mixed.run(engine, go, ge, local)
    tr = 256 * int(k)
    _ran_batch(engine, len(_MIXED), k=int(k), pair_major=0, tickets=sum(-(-R // tr) for R, _ in _MIXED))
    for i, ((Y, X), r) in enumerate(zip(_mixed_pairs(), res)):
        assert _t(r) == _ref(("mixed", _MIXED[i]), Y, X, golden.blosum62, go, ge, local), (i, _MIXED[i])
    assert _t(res[13]) == _t(res[6])


@pytest.mark.parametrize("k", ["2", "4"])
@pytest.mark.parametrize("go,ge,local", MODES)
def test_both_schedules(engine, golden, mixed, knobs, go, ge, local, k):
    """Round-robin (default) and pair-major (GSA_BATCH_ORDER=pair): the same results, and the launch
    record names the order it took."""
    knobs("GSA_SCORE_K", k)
    knobs("GSA_BATCH_ORDER", "pair")
    rp = mixed.run(engine, go, ge, local)
    _ran_batch(engine, len(_MIXED), pair_major=1)
    knobs("GSA_BATCH_ORDER", None)
    rr = mixed.run(engine, go, ge, local)
    _ran_batch(engine, len(_MIXED), pair_major=0)
    assert [_t(r) for r in rp] == [_t(r) for r in rr]
    for i, ((Y, X), r) in enumerate(zip(_mixed_pairs(), rp)):
        assert _t(r) == _ref(("mixed", _MIXED[i]), Y, X, golden.blosum62, go, ge, local), (i, _MIXED[i])


@pytest.mark.parametrize("go,ge,local", [(-11, -1, True), (-11, -11, False)])
def test_more_tickets_than_cus(engine, golden, go, ge, local):
    """cu_count + 40 single-ticket pairs, long (200 x 3000) and short (64 x 65) in turn: workgroups
    take a short pair after a long one, whose profile columns and rings must not show through (the
    failure test_profile_widths_and_stale_columns records for single pairs)."""
    shapes = [(200, 3000), (64, 65)]
    two = [random_pair(R, C, 11 * R + C) for R, C in shapes]
    n = engine.cu_count + 40
    d = _Dev([two[i % 2] for i in range(n)], golden.blosum62, same={i: i % 2 for i in range(2, n)})
    res = d.run(engine, go, ge, local)
    _ran_batch(engine, n, tickets=n)
    want = [_ref(("stale", shapes[i]), *two[i], golden.blosum62, go, ge, local) for i in range(2)]
    assert [_t(r) for r in res] == [want[i % 2] for i in range(n)]


@pytest.mark.parametrize("go,ge", [(-11, -11), (-11, -1), (-5, -2)])
def test_local_specifics_per_pair(engine, golden, go, ge):
    """The planted-motif pair of test_local_ties_first_in_row_major (two equal maxima: the first in
    row-major order) and an all-mismatch pair ((0, 0, 0)) among random pairs: each answer belongs
    to its pair.  Match +5, everything else -4."""
    n = int(round(np.sqrt(golden.blosum62.size)))
    sub = np.full((n, n), -4, np.int32)
    np.fill_diagonal(sub[:20, :20], 5)
    gapR = 250
    rng = np.random.default_rng(gapR + 7)
    motif = rng.integers(0, 20, 300).astype(np.int32)
    fl = lambda k: np.full(k, 22, np.int32)
    Yp = np.concatenate([[0], fl(5), motif, fl(gapR + 1), motif, fl(9)]).astype(np.int32)
    Xp = np.concatenate([[0], fl(50), motif, fl(40)]).astype(np.int32)
    Ym = np.concatenate([[0], np.full(700, 3)]).astype(np.int32)
    Xm = np.concatenate([[0], np.full(900, 7)]).astype(np.int32)
    shapes = [(130, 700), (600, 90), (1030, 257)]
    pairs = [random_pair(*shapes[0], 5), (Yp, Xp), random_pair(*shapes[1], 6), (Ym, Xm), random_pair(*shapes[2], 7)]
    res = _Dev(pairs, sub).run(engine, go, ge, True)
    _ran_batch(engine, len(pairs))
    assert _t(res[1]) == (1500, 305, 350)
    assert _t(res[3]) == (0, 0, 0)
    for i, (Y, X) in enumerate(pairs):
        assert _t(res[i]) == _ref(("motif", i), Y, X, sub, go, ge, True), i


@pytest.mark.parametrize("go,ge,local", MODES)
def test_empty_pairs_in_a_batch(engine, golden, go, ge, local):
    shapes = [(0, 0), (300, 200), (0, 9), (7, 0), (65, 600), (0, 0)]
    pairs = [random_pair(R, C, 3 * R + C + 1) for R, C in shapes]
    res = _Dev(pairs, golden.blosum62).run(engine, go, ge, local)
    _ran_batch(engine, len(pairs), tickets=2)
    for i, (Y, X) in enumerate(pairs):
        assert _t(res[i]) == _ref(("empty", shapes[i]), Y, X, golden.blosum62, go, ge, local), shapes[i]
    # only empty pairs: nothing to launch, every pair still answered
    only = [pairs[i] for i in (0, 2, 3)]
    res = _Dev(only, golden.blosum62).run(engine, go, ge, local)
    _ran_batch(engine, 3, tickets=0)
    for (Y, X), r, i in zip(only, res, (0, 2, 3)):
        assert _t(r) == _ref(("empty", shapes[i]), Y, X, golden.blosum62, go, ge, local), shapes[i]


def _small_pairs():
    shapes = [(130, 700), (700, 130), (65, 63), (1030, 257)]
    return shapes, [random_pair(R, C, 7 * R + C) for R, C in shapes]


def test_fallback_local_zero_gaps(engine, golden):
    """go == ge == 0, local: the kernel's condition go < 0 fails for every pair (results only)."""
    shapes, pairs = _small_pairs()
    res = _Dev(pairs, golden.blosum62).run(engine, 0, 0, True)
    for i, (Y, X) in enumerate(pairs):
        assert _t(res[i]) == _ref(("small", shapes[i]), Y, X, golden.blosum62, 0, 0, True), shapes[i]


def test_fallback_large_score_pair(engine, golden):
    """A table whose diagonal is 30000 and one identical 2600 x 2600 pair (score >= 2^26) among short
    pairs: that pair runs alone, the others in the batch (results only)."""
    n = int(round(np.sqrt(golden.blosum62.size)))
    sub = np.full((n, n), -30000, np.int32)
    np.fill_diagonal(sub, 30000)
    Yb, _ = random_pair(2600, 10, 12)
    shapes, pairs = _small_pairs()
    pairs = pairs[:2] + [(Yb, Yb.copy())] + pairs[2:]
    res = _Dev(pairs, sub).run(engine, -11, -1, True)
    assert res[2]["score"] >= 1 << 26
    for i, (Y, X) in enumerate(pairs):
        assert _t(res[i]) == _ref(("big", i), Y, X, sub, -11, -1, True), i


@pytest.mark.parametrize("go,ge,local", [(-11, -1, False), (-11, -11, True)])
def test_fallback_profile_does_not_fit(engine, golden, go, ge, local):
    """substsz = 32: the K-rows score kernel's profile exceeds LDS, every pair runs alone (results only)."""
    rng = np.random.default_rng(3207)
    sub = rng.integers(-6, 12, size=(32, 32)).astype(np.int32)
    shapes = [(1500, 1100), (64, 65), (513, 300)]
    pairs = [random_pair(R, C, R + C, alphabet=32) for R, C in shapes]
    res = _Dev(pairs, sub).run(engine, go, ge, local)
    for i, (Y, X) in enumerate(pairs):
        assert _t(res[i]) == _ref(("a32", shapes[i]), Y, X, sub, go, ge, local), shapes[i]


@pytest.mark.parametrize("go,ge,local", [(-11, -1, False), (-11, -11, True)])
def test_fallback_forced_row_scan(engine, golden, knobs, go, ge, local):
    """GSA_SCORE_SCAN=1: every pair through the row scan (results only; the last launch is its)."""
    knobs("GSA_SCORE_SCAN", "1")
    shapes, pairs = _small_pairs()
    res = _Dev(pairs, golden.blosum62).run(engine, go, ge, local)
    assert engine.last_launch()["kind"] == "score_scan"
    for i, (Y, X) in enumerate(pairs):
        assert _t(res[i]) == _ref(("small", shapes[i]), Y, X, golden.blosum62, go, ge, local), shapes[i]


def test_invalid_input(engine, golden):
    shapes, pairs = _small_pairs()
    d = _Dev(pairs, golden.blosum62)

    def good():
        res = d.run(engine, -11, -1, False)
        _ran_batch(engine, len(pairs))
        for i, (Y, X) in enumerate(pairs):
            assert _t(res[i]) == _ref(("small", shapes[i]), Y, X, golden.blosum62, -11, -1, False), shapes[i]

    for go, ge in [(-1, -11), (-3, 2)]:
        with pytest.raises(gsa.NwError):
            d.run(engine, go, ge, False)
        good()
    with pytest.raises(gsa.NwError):
        engine.score_batch_dev([], d.sub.data_ptr(), d.substsz, -11, -1, False)
    good()


def test_single_pair_calls_unchanged_by_a_batch(engine, golden, mixed, knobs):
    """After a batch, gsa_score of one pair takes its own path: npairs 1, and from both ends when
    forced (the batch mapping did not capture the kernel's both-ends form)."""
    import oracle
    mixed.run(engine, -11, -1, False)
    _ran_batch(engine, len(_MIXED))
    Y, X = random_pair(2052, 257, 99)
    r = engine.score(Y, X, golden.blosum62, -11, -1, False)
    ll = engine.last_launch()
    assert ll["kind"] == "score_krow" and ll["npairs"] == 1 and ll["both_ends"] == 0, ll
    assert _t(r) == oracle.score_ag(Y, X, golden.blosum62, -11, -1, False)
    mixed.run(engine, -11, -1, False)
    knobs("GSA_SCORE_BIDI", "2")
    r = engine.score(Y, X, golden.blosum62, -11, -1, False)
    ll = engine.last_launch()
    assert ll["kind"] == "score_krow" and ll["both_ends"] == 1, ll
    assert _t(r) == oracle.score_ag(Y, X, golden.blosum62, -11, -1, False)


@pytest.mark.parametrize("go,ge,local", [(-11, -11, False), (-11, -11, True)])
def test_config4_sized_batch(engine, golden, go, ge, local):
    """16 pairs of 18-22k (shard.synthetic_batch, the config-4 generator), NW-LG and SW-LG: the batch
    against the oracle's tiled OpenMP restatement and against gsa_score of every pair alone."""
    pairs = shard.synthetic_batch(16, 18000, 22000)
    res = engine.score_batch(pairs, golden.blosum62, go, ge, local)
    _ran_batch(engine, len(pairs))
    for i, (Y, X) in enumerate(pairs):
        ref = _ref(("cfg4", i), Y, X, golden.blosum62, go, ge, local, mt=True, blocksz=256, nthreads=16)
        assert _t(res[i]) == ref, i
        assert _t(engine.score(Y, X, golden.blosum62, go, ge, local)) == ref, i


@pytest.mark.parametrize("ge,local", [(-1, False), (-11, True)])
def test_sharding_adapter(golden, ge, local):
    """shard_align over shard.gpu_batch_score without torch.distributed: scores in pair order."""
    shapes = [(40, 50), (120, 30), (7, 9), (64, 64), (200, 150), (1, 5), (90, 91), (33, 256), (150, 12), (1030, 700),
              (2049, 300), (513, 1500)]
    pairs = [random_pair(R, C, 29 * R + C) for R, C in shapes]
    launch = {}
    rep = shard.shard_align(pairs, golden.blosum62, -11, shard.gpu_batch_score(0, ge, local, launch=launch))
    assert launch["kind"] == "score_krow" and launch["npairs"] == len(pairs), launch
    want = [_ref(("shard", shapes[i]), Y, X, golden.blosum62, -11, ge, local)[0] for i, (Y, X) in enumerate(pairs)]
    assert [r.align_cost for r in rep.results] == want
    assert rep.world == 1 and rep.elapsed_s > 0
