"""The NW-LG fill family at its value-range edges: gsa_fill_sparse_dev, gsa_fill_full_dev, their batch
forms, gsa_align_sparse, gsa_align_sparse_pt, gsa_align_full, and the device check and trace behind
them.  Every expectation is tests/_exact.py's (fill_lg, headers_lg, homopolymer_lg: int64, written from
the recurrence), never the oracle's, whose int32 C shares its width with the kernels.  Every case names
the instance it reached from Engine.last_launch(): kind, ns, k, q8, q8_declined, staged, mlsppt, npairs.

The inputs are built by plain functions at the top, without a GPU: tests/test_exact_fill.py runs the
oracle over the same ones.

The edges, as include/gsa.h states them for the fills, with q = s - 2 g over the whole table:
  K-rows instances (sparse, mlsppt, batches, pass 1 of the two-pass and fused full fills):
      every q in [-128, 127]: the int8 profile; else every q in [-32768, 32767]: the int8 instance
      declines and the int16 one fills; else error bit 2, errorKernelFailure from the sync
  strip kernel (GSA_SPARSE_KERNEL=strip): every q in [-32767, 32767] (-32768 is its column sentinel)
  lane fill (GSA_FULL_KERNEL=lane): unshifted int32, no profile: every table
  shifted accumulator H' = H - (i + j) g of the K-rows and strip kernels: max(q, 0) m < 2^31 with m
      the largest min(i, j) over the cells the output depends on; else error bit 2
  substsz in 1 .. 32, else errorInvalidValue before anything is enqueued."""
import functools

import numpy as np
import pytest

import gpuseqalign_amd as gsa
from gpuseqalign_amd import formats as F
from tests import _exact

pytestmark = pytest.mark.gpu

TBY = 1024  # gsa_sparse_tile_by(); the GPU tests compare
# two tickets of the largest geometry (64 x 4 x 8 = 2048 rows) with a partial last one and columns that
# are no multiple of 16; fewer rows than a strip; five tile rows with one wide tile column and a narrow one
SHAPES = [(63, 2000, 64), (2049, 3001, 112), (4100, 1030, 512)]
FOLLOW_SHAPE = (300, 400, 64)  # the ordinary fill behind a declined or refused one
BATCH_LENS = [(300, 2600), (2600, 300), (1024, 1025), (1500, 700), (2049, 640), (64, 2048), (777, 1999),
              (2300, 2300), (1, 900), (513, 1300), (1900, 333), (1025, 1024)]
BATCH_TBX = 128


# -- tables ----------------------------------------------------------------------------------------

def table(n, seed=2031):
    """n letters, values in -4 .. 11, not symmetric (n >= 2): row = seqY letter, column = seqX letter."""
    if n == 1:
        return np.array([[7]], np.int32)
    t = np.random.default_rng(seed + n).integers(-4, 12, (n, n)).astype(np.int32)
    t[0, n - 1], t[n - 1, 0] = 11, -4
    assert t.min() == -4 and t.max() == 11 and not np.array_equal(t, t.T)
    return t


MAX_PAIR, MIN_PAIR = (3, 7), (5, 11)  # (seqY letter, seqX letter) of a planted extreme entry
RUN = 48


def edge_table(kind, edge, g):
    """table(20) with one entry moved so that max(s - 2 g) (kind "max") or min(s - 2 g) ("min") over the
    table is exactly `edge`; the transposed entry keeps its ordinary value."""
    t = table(20)
    a, b = MAX_PAIR if kind == "max" else MIN_PAIR
    t[a, b] = edge + 2 * g
    q = t.astype(np.int64) - 2 * g
    assert (q.max() if kind == "max" else q.min()) == edge and (q == edge).sum() == 1, (kind, edge, g)
    assert -4 <= t[b, a] <= 11
    return t


def q_range(sub, g):
    q = np.asarray(sub, np.int64) - 2 * int(g)
    return int(q.min()), int(q.max())


# -- pairs -----------------------------------------------------------------------------------------

def random_pair(R, C, alphabet, seed):
    return F.synthetic_seq(R, seed, alphabet), F.synthetic_seq(C, seed + 1, alphabet)


def related_pair(R, C, alphabet, seed):
    """seqX random, seqY a mutated copy of it (15 % substitutions, 2 % indels), cut or extended to R."""
    base = F.synthetic_seq(max(R, C) + R // 16 + 64, seed, alphabet)
    Y = F.mutate_seq(base, seed + 1, alphabet=alphabet)
    assert len(Y) >= R + 1
    return np.ascontiguousarray(Y[:R + 1]), np.ascontiguousarray(base[:C + 1])


def plant_run(Y, X, a, b):
    """A run of RUN letters a in seqY opposite a run of letters b in seqX, on the diagonal (shorter where
    the shorter sequence has fewer than 2 RUN letters)."""
    n = min(len(Y), len(X)) - 1
    run, p = min(RUN, n // 2), max(1, n // 4)
    Y[p:p + run], X[p:p + run] = a, b
    return Y, X


class Case:
    """One input of the family: a table, a gap cost, a shape and how its pairs are made."""

    def __init__(self, name, sub, g, shape, related, plant=None):
        self.name, self.sub, self.g, self.shape, self.related, self.plant = name, sub, int(g), shape, related, plant
        self.substsz = sub.shape[0]
        self.qmin, self.qmax = q_range(sub, g)

    def __repr__(self):
        return self.name

    def make(self, R, C, seed):
        Y, X = (related_pair if self.related else random_pair)(R, C, self.substsz, seed)
        if self.plant:
            Y, X = plant_run(Y, X, *self.plant)
        return Y, X

    def pair(self):
        R, C, _ = self.shape
        return self.make(R, C, 31 * R + C)

    def batch(self):
        return [self.make(R, C, 7000 + 13 * k) for k, (R, C) in enumerate(BATCH_LENS)]

    @property
    def int8(self):
        return -128 <= self.qmin and self.qmax <= 127

    @property
    def int16(self):
        return -32768 <= self.qmin and self.qmax <= 32767


def table_cases():
    """Asymmetric 20-letter tables on every shape, a random and a related pair each, g = -11; the other
    gap signs; 1, 2, 4 and 32 letters, and 26 and 27, the last table the fused fill's staging fits
    beside and the first it does not."""
    out = []
    for i, shape in enumerate(SHAPES):
        for related in (False, True):
            out.append(Case("t20-%dx%d-%s" % (shape[0], shape[1], "rel" if related else "rnd"), table(20), -11, shape,
                            related))
    out.append(Case("t20-g0", table(20), 0, SHAPES[1], True))
    out.append(Case("t20-g+5", table(20), 5, SHAPES[2], False))
    for k, n in enumerate((1, 2, 4, 32, 26, 27)):
        out.append(Case("t%d" % n, table(n), -11, SHAPES[(k + 1) % 3], n >= 26))
    return out


# (kind, edge, the negative gap cost used beside g = 0)
EDGES = [("max", 127, -40), ("max", 128, -40), ("max", 32767, -8000), ("max", 32768, -8000),
         ("min", -128, -11), ("min", -129, -11), ("min", -32767, -11), ("min", -32768, -11), ("min", -32769, -11)]


def edge_cases():
    """Every profile edge from both sides, with g = 0 (q = s) and with a negative g.  The maximum sits
    on the optimal path: a run of its letter pair on the diagonal of a related pair (its neighbours there
    are ordinary letters, negative q among them at g = 0).  The minimum's letter pair (5, 11) meets in
    about one cell of 400 of a random pair, everywhere off the path, between positive q."""
    out = []
    for i, (kind, edge, gneg) in enumerate(EDGES):
        for g in (0, gneg):
            out.append(Case("%s%d-g%d" % (kind, edge, g), edge_table(kind, edge, g), g, SHAPES[(i + 1 + (g != 0)) % 3],
                            kind == "max", MAX_PAIR if kind == "max" else None))
    return out


def plain_case():
    """An ordinary fill: table(20), g = -11, inside int8."""
    return Case("plain", table(20), -11, FOLLOW_SHAPE, False)


CHECK_CASES = ("t20-2049x3001-rel", "t32", "max32767-g-8000")  # the check and trace run on these
BATCH_CASES = ("t20-2049x3001-rel", "t32", "max127-g-40", "max128-g0", "max32767-g-8000", "max32768-g0",
               "min-128-g0", "min-129-g-11", "min-32768-g0", "min-32769-g-11")

# the accumulator: runs of letter 0, s(0, 0) = 16767, g = -8000, q = 32767
ACC_V, ACC_G, ACC_TBX = 16767, -8000, 256
ACC_INSIDE, ACC_PAST, ACC_RECT = 65537, 65539, (65539, 70000)


def acc_table():
    return np.array([[ACC_V]], np.int32)


def all_cases():
    return table_cases() + edge_cases()


def case_named(name):
    return next(c for c in all_cases() + [plain_case()] if c.name == name)


def answered_inputs():
    """(case, Y, X, tBx) of every input the tests below expect an answer for from some instance (the lane
    fill answers past int16 too), the two 65k pairs excepted; tests/test_exact_fill.py runs the oracle
    over them."""
    plain = plain_case()
    yield (plain,) + plain.pair() + (FOLLOW_SHAPE[2],)
    for c in all_cases():
        yield (c,) + c.pair() + (c.shape[2],)
    for name in BATCH_CASES:
        c = case_named(name)
        for Y, X in c.batch():
            yield c, Y, X, BATCH_TBX


# -- references, computed once per input --------------------------------------------------------------

class Ref:
    """fill_lg of the padded pair: the headers, the unpadded matrix, the cost."""

    def __init__(self, Y, X, sub, g, tBx):
        Yp, Xp, trows, tcols = _exact.pad_to_tiles(Y, X, TBY, tBx)
        H = _exact.fill_lg(Yp, Xp, sub, g)
        assert np.abs(H).max() < 2 ** 31  # out of scope: inputs whose int32 H overflows
        self.hrow, self.hcol = (a.astype(np.int32) for a in _exact.headers_of(H, trows, tcols, TBY, tBx))
        self.full = np.ascontiguousarray(H[:len(Y), :len(X)].astype(np.int32))
        self.cost = int(H[len(Y) - 1, len(X) - 1])


@functools.lru_cache(maxsize=4)
def ref_single(name):
    c = case_named(name)
    return Ref(*c.pair(), c.sub, c.g, c.shape[2])


@functools.lru_cache(maxsize=2)
def ref_batch(name):
    c = case_named(name)
    return [Ref(Y, X, c.sub, c.g, BATCH_TBX) for Y, X in c.batch()]


# -- instances ---------------------------------------------------------------------------------------

class Inst:
    """One kernel instance of the family: how to select it, and what its launch record says."""

    def __init__(self, name, family, knobs, kind, ns=None, k=None, staged=0, mlsppt=0, full=False):
        self.name, self.family, self.knobs, self.kind = name, family, knobs, kind
        self.ns, self.k, self.staged, self.mlsppt, self.full = ns, k, staged, mlsppt, full

    def __repr__(self):
        return self.name

    def select(self, knobs):
        for name in ("GSA_SPARSE_KERNEL", "GSA_KROW_NS", "GSA_KROW_K", "GSA_KROW_Q8", "GSA_FULL_KERNEL", "GSA_FULL_FUSED",
                     "GSA_FUSED_STAGED"):
            knobs(name, self.knobs.get(name))

    def staged_for(self, substsz):
        """The fused fill's staging takes 32 KiB of LDS beside pass 1's profile (4.4 KiB a letter in
        int16): it fits up to 26 letters of 160 KiB, and the strips of a larger table store directly."""
        return 1 if self.staged and substsz <= 26 else 0

    def q8(self, substsz):
        """The int8 instance is launched wherever its LDS fits 160 KiB.  Its four profile copies take
        4.5 KiB a letter: 32 letters fit beside the 5 rings of 4 strips and not beside the 9 of 8 strips;
        beside the staging 25 letters fit and 26 do not."""
        if self.family != "krow":
            return 0
        if self.staged_for(substsz):
            return 1 if substsz <= 25 else 0
        return 0 if substsz == 32 and self.ns == 8 else 1

    def accepts(self, case):
        if self.family == "lane":
            return True
        if self.family == "strip":
            return -32767 <= case.qmin and case.qmax <= 32767
        return case.int16

    def assert_ran(self, ll, case, npairs=1):
        assert ll["kind"] == self.kind, ll
        assert ll["k"] == self.k and (self.ns is None or ll["ns"] == self.ns), ll  # (the lane fill picks its strips)
        assert (ll["staged"], ll["mlsppt"], ll["npairs"]) == (self.staged_for(case.substsz), self.mlsppt, npairs), ll
        q8 = self.q8(case.substsz)
        assert ll["q8"] == q8, ll
        assert ll["q8_declined"] == (1 if q8 and not case.int8 else 0), (case, ll)


def _krow(ns, k):
    return {"GSA_SPARSE_KERNEL": "krow", "GSA_KROW_NS": str(ns), "GSA_KROW_K": str(k)}


SPARSE = [Inst("krow%d%d" % (ns, k), "krow", _krow(ns, k), "sparse_krow", ns, k)
          for ns, k in ((4, 4), (8, 4), (4, 2), (2, 4), (2, 2))]
SPARSE.append(Inst("strip", "strip", {"GSA_SPARSE_KERNEL": "strip"}, "sparse_strip", 4, 1))
MLSPPT = Inst("mlsppt", "krow", {}, "sparse_krow", 4, 4, mlsppt=1)
FULL = [Inst("fused", "krow", {"GSA_FULL_KERNEL": "twopass", "GSA_FULL_FUSED": "1", "GSA_FUSED_STAGED": "0"},
             "full_fused", 4, 4, full=True),
        Inst("fused_staged", "krow", {"GSA_FULL_KERNEL": "twopass", "GSA_FULL_FUSED": "1", "GSA_FUSED_STAGED": "1"},
             "full_fused", 4, 4, staged=1, full=True),
        Inst("two_launch", "krow", {"GSA_FULL_KERNEL": "twopass", "GSA_FULL_FUSED": "0"}, "full_two_launch", 4, 4,
             full=True),
        Inst("lane", "lane", {"GSA_FULL_KERNEL": "lane"}, "full_lane", None, 1, full=True)]
SINGLE = SPARSE + [MLSPPT] + FULL
# batches: the sparse one in the 4- and the 8-strip geometry (12 pairs of at most 3 tile rows fit the
# chip, so 4 strips is also the default), one full batch (two launches; its pass 1 the same kernel)
BATCH = [Inst("batch44", "krow", _krow(4, 4), "sparse_krow", 4, 4), Inst("batch84", "krow", _krow(8, 4), "sparse_krow", 8, 4),
         Inst("batch_full", "krow", {"GSA_FULL_KERNEL": "twopass"}, "full_two_launch", 4, 4, full=True)]


# -- on the device -------------------------------------------------------------------------------------

def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to("cuda:0")


def _kernel_failure(call):
    with pytest.raises(gsa.NwError) as ei:
        call()
    assert ei.value.stat == gsa.NwStat.errorKernelFailure, ei.value


def _invalid(call):
    with pytest.raises(gsa.NwError) as ei:
        call()
    assert ei.value.stat == gsa.NwStat.errorInvalidValue, ei.value


def _call_single(engine, inst, Y, X, sub, g, tBx):
    if inst.full:
        return engine.align_full(Y, X, sub, g)
    return engine.align_sparse(Y, X, sub, g, tileBx=tBx, overlap=bool(inst.mlsppt))


def _run_single(engine, inst, Y, X, sub, g, tBx, ref):
    """One fill through the host-buffer entry point of the instance, every word against ref."""
    r = _call_single(engine, inst, Y, X, sub, g, tBx)
    if inst.full:
        assert np.array_equal(r.score, ref.full), (inst, np.argwhere(r.score != ref.full)[:3])
    else:
        assert r.geom.tileBy == TBY
        assert np.array_equal(r.hrow, ref.hrow), (inst, np.flatnonzero(r.hrow != ref.hrow)[:3])
        assert np.array_equal(r.hcol, ref.hcol), (inst, np.flatnonzero(r.hcol != ref.hcol)[:3])
    assert r.align_cost == ref.cost


def _single(engine, knobs, inst, case):
    """The case on the instance: exact, with the launch record the edge asks for, or refused; then an
    ordinary fill on the same engine, which is exact and (a stale launch word) not declined."""
    inst.select(knobs)
    Y, X = case.pair()
    if inst.accepts(case):
        _run_single(engine, inst, Y, X, case.sub, case.g, case.shape[2], ref_single(case.name))
        inst.assert_ran(engine.last_launch(), case)
    else:
        _kernel_failure(lambda: _call_single(engine, inst, Y, X, case.sub, case.g, case.shape[2]))
    if not case.int8:
        plain = plain_case()
        _run_single(engine, inst, *plain.pair(), plain.sub, plain.g, FOLLOW_SHAPE[2], ref_single("plain"))
        inst.assert_ran(engine.last_launch(), plain)


@pytest.fixture(scope="module", autouse=True)
def _tile_height(engine):
    assert gsa.sparse_tile_by() == TBY


@pytest.mark.parametrize("inst", SINGLE, ids=repr)
@pytest.mark.parametrize("case", table_cases(), ids=repr)
def test_tables(engine, knobs, case, inst):
    """Asymmetric tables (a transposed read of the table changes every one of these), positive, zero
    and negative gap costs, 1, 2, 4 and 32 letters (letter 31 is the last of a table row in LDS)."""
    if case.substsz >= 2:
        Y, X = case.pair()
        n = min(len(Y), len(X))
        assert (Y[1:n] < X[1:n]).any() and (Y[1:n] > X[1:n]).any()  # letter pairs on both sides of the diagonal
        assert (Y == case.substsz - 1).any() and (X == case.substsz - 1).any()
    _single(engine, knobs, inst, case)


@pytest.mark.parametrize("inst", SINGLE, ids=repr)
@pytest.mark.parametrize("case", edge_cases(), ids=repr)
def test_profile_edges(engine, knobs, case, inst):
    """max(s - 2 g) at 127 / 128 / 32767 / 32768 and min(s - 2 g) at -128 / -129 / -32767 / -32768 /
    -32769, at g = 0 and at a negative g, on every instance."""
    _single(engine, knobs, inst, case)


def _batch_buffers(case, tBx, full):
    import torch
    pairs = case.batch()
    ins = [(_dev(Y), _dev(X)) for Y, X in pairs]
    if full:
        outs = [torch.full((len(Y) * len(X),), -7, dtype=torch.int32, device="cuda:0") for Y, X in pairs]
        descs = [(y.data_ptr(), y.numel(), x.data_ptr(), x.numel(), o.data_ptr()) for (y, x), o in zip(ins, outs)]
    else:
        geoms = [gsa.sparse_geometry(len(Y), len(X), tBx) for Y, X in pairs]
        outs = [(torch.full((g.hrowElems,), -7, dtype=torch.int32, device="cuda:0"),
                 torch.full((g.hcolElems,), -7, dtype=torch.int32, device="cuda:0")) for g in geoms]
        descs = [(y.data_ptr(), y.numel(), x.data_ptr(), x.numel(), (hr.data_ptr(), hc.data_ptr()))
                 for (y, x), (hr, hc) in zip(ins, outs)]
    return pairs, ins, outs, descs


def _run_batch(engine, inst, case, refs):
    pairs, ins, outs, descs = _batch_buffers(case, BATCH_TBX, inst.full)
    s = _dev(case.sub)
    engine.fill_batch_dev(descs, s.data_ptr(), case.substsz, case.g, mode="full" if inst.full else "sparse",
                          tileBx=BATCH_TBX)
    engine.sync()
    if refs is None:
        return
    for p, (out, ref) in enumerate(zip(outs, refs)):
        if inst.full:
            assert np.array_equal(out.cpu().numpy().reshape(ref.full.shape), ref.full), (inst, case, p)
        else:
            assert np.array_equal(out[0].cpu().numpy(), ref.hrow), (inst, case, p)
            assert np.array_equal(out[1].cpu().numpy(), ref.hcol), (inst, case, p)


@pytest.mark.parametrize("inst", BATCH, ids=repr)
@pytest.mark.parametrize("name", BATCH_CASES)
def test_batches(engine, knobs, name, inst):
    """12 pairs of 1 .. 2600 letters in one launch: tables and edges as above, every header word (every
    matrix word) of every pair.  The table is the launch's, so a table outside int16 refuses the whole
    call, and an ordinary batch behind it is exact."""
    case = case_named(name)
    inst.select(knobs)
    if inst.accepts(case):
        _run_batch(engine, inst, case, ref_batch(name))
        inst.assert_ran(engine.last_launch(), case, npairs=len(BATCH_LENS))
    else:
        _kernel_failure(lambda: _run_batch(engine, inst, case, None))
    if not case.int8:
        follow = case_named(BATCH_CASES[0])
        _run_batch(engine, inst, follow, ref_batch(follow.name))
        inst.assert_ran(engine.last_launch(), follow, npairs=len(BATCH_LENS))


def test_substsz_33_is_refused_everywhere(engine, knobs):
    """33 letters do not fit the LDS table rows: errorInvalidValue from every fill entry point, before
    anything is enqueued, and the context fills on."""
    import torch
    MLSPPT.select(knobs)
    t33 = np.zeros((33, 33), np.int32)
    Y, X = random_pair(300, 400, 20, 3)
    y, x, s = _dev(Y), _dev(X), _dev(t33)
    geom = gsa.sparse_geometry(len(Y), len(X), 64)
    hr = torch.empty(geom.hrowElems, dtype=torch.int32, device="cuda:0")
    hc = torch.empty(geom.hcolElems, dtype=torch.int32, device="cuda:0")
    ld = gsa.full_pitch(len(X))
    sc = torch.empty(len(Y) * ld + 64, dtype=torch.int32, device="cuda:0")
    seqs = (y.data_ptr(), len(Y), x.data_ptr(), len(X))
    _invalid(lambda: engine.fill_sparse_dev(*seqs, s.data_ptr(), 33, -11, 64, hr.data_ptr(), hc.data_ptr()))
    _invalid(lambda: engine.fill_full_dev(*seqs, s.data_ptr(), 33, -11, sc.data_ptr()))
    _invalid(lambda: engine.fill_full_dev(*seqs, s.data_ptr(), 33, -11, sc.data_ptr(), ld=ld))
    _invalid(lambda: engine.fill_batch_dev([seqs + ((hr.data_ptr(), hc.data_ptr()),)], s.data_ptr(), 33, -11, tileBx=64))
    _invalid(lambda: engine.fill_batch_dev([seqs + (sc.data_ptr(),)], s.data_ptr(), 33, -11, mode="full"))
    _invalid(lambda: engine.fill_batch_dev([seqs + (sc.data_ptr(),)], s.data_ptr(), 33, -11, mode="full", lds=[ld]))
    _invalid(lambda: engine.align_sparse(Y, X, t33, -11, tileBx=64))
    _invalid(lambda: engine.align_sparse(Y, X, t33, -11, tileBx=64, overlap=True))
    _invalid(lambda: engine.align_full(Y, X, t33, -11))
    engine.sync()
    plain = plain_case()
    for inst in (SPARSE[0], MLSPPT, FULL[0]):
        inst.select(knobs)
        _run_single(engine, inst, *plain.pair(), plain.sub, plain.g, FOLLOW_SHAPE[2], ref_single("plain"))
        inst.assert_ran(engine.last_launch(), plain)


# -- the shifted accumulator ------------------------------------------------------------------------------

def _acc_sparse(engine, R, C):
    """Two runs of letter 0 through gsa_fill_sparse_dev; the headers stay on the device."""
    import torch
    geom = gsa.sparse_geometry(R + 1, C + 1, ACC_TBX)
    y = torch.zeros(max(R, C) + 1, dtype=torch.int32, device="cuda:0")
    s = _dev(acc_table())
    hr = torch.full((geom.hrowElems,), -7, dtype=torch.int32, device="cuda:0")
    hc = torch.full((geom.hcolElems,), -7, dtype=torch.int32, device="cuda:0")
    engine.fill_sparse_dev(y.data_ptr(), R + 1, y.data_ptr(), C + 1, s.data_ptr(), 1, ACC_G, ACC_TBX, hr.data_ptr(),
                           hc.data_ptr())
    engine.sync()
    return hr, hc


def _acc_exact(engine, R, C):
    import torch
    hr, hc = _acc_sparse(engine, R, C)
    want_r, want_c = _exact.homopolymer_lg(R, C, ACC_V, ACC_G).headers(TBY, ACC_TBX)
    assert np.abs(want_r).max() < 2 ** 31 and np.abs(want_c).max() < 2 ** 31
    assert torch.equal(hr.cpu(), torch.from_numpy(want_r.astype(np.int32)))
    assert torch.equal(hc.cpu(), torch.from_numpy(want_c.astype(np.int32)))


ACC_INSTS = [SPARSE[0], SPARSE[1], SPARSE[5]]


@pytest.mark.parametrize("inst", ACC_INSTS, ids=repr)
def test_accumulator_inside(engine, knobs, inst):
    """q = 32767 on the whole diagonal of 65 537 letters: H' reaches 32767 x 65537 = 2 147 450 879 in the
    last real cell, under 2^31, and 32767 x 65536 in the largest header cell.  Exact, every header word."""
    inst.select(knobs)
    assert 32767 * ACC_INSIDE < 2 ** 31
    _acc_exact(engine, ACC_INSIDE, ACC_INSIDE)
    ll = engine.last_launch()
    assert (ll["kind"], ll["ns"], ll["k"], ll["q8_declined"]) == (inst.kind, inst.ns, inst.k, inst.q8(1)), ll


@pytest.mark.parametrize("R,C", [(ACC_PAST, ACC_PAST), ACC_RECT], ids=["65539x65539", "65539x70000"])
@pytest.mark.parametrize("inst", ACC_INSTS, ids=repr)
def test_accumulator_past(engine, knobs, inst, R, C):
    """Two letters more and H' passes 2^31 in the last real cells, while the reference's own H stays
    near 1.1e9.  The square pair has the headers of the 65 537 one, whose largest min(i, j) is 65 536:
    exact.  The rectangular one has header columns down to row 66 560 at columns up to 69 888:
    32767 x 66560 > 2^31, refused (error bit 2), never a wrong word; an inside fill follows, exact."""
    inst.select(knobs)
    assert 32767 * min(R, C) >= 2 ** 31 and abs(_exact.homopolymer_lg(R, C, ACC_V, ACC_G).cost()) < 2 ** 31
    if (R, C) == ACC_RECT:
        _kernel_failure(lambda: _acc_sparse(engine, R, C))
        _acc_exact(engine, 2049, 3001)
    else:
        _acc_exact(engine, R, C)


def test_accumulator_batch_one_pair_past(engine, knobs):
    """The bound is the launch's: the rectangular pair beside a short one refuses the whole batch, and the
    same batch with the square pair in its place is exact in both."""
    import torch
    SPARSE[0].select(knobs)
    s = _dev(acc_table())
    zeros = torch.zeros(ACC_RECT[1] + 1, dtype=torch.int32, device="cuda:0")

    def run(shapes):
        geoms = [gsa.sparse_geometry(R + 1, C + 1, ACC_TBX) for R, C in shapes]
        outs = [(torch.full((g.hrowElems,), -7, dtype=torch.int32, device="cuda:0"),
                 torch.full((g.hcolElems,), -7, dtype=torch.int32, device="cuda:0")) for g in geoms]
        engine.fill_batch_dev([(zeros.data_ptr(), R + 1, zeros.data_ptr(), C + 1, (hr.data_ptr(), hc.data_ptr()))
                               for (R, C), (hr, hc) in zip(shapes, outs)], s.data_ptr(), 1, ACC_G, tileBx=ACC_TBX)
        engine.sync()
        return outs

    _kernel_failure(lambda: run([(2049, 3001), ACC_RECT]))
    shapes = [(2049, 3001), (ACC_PAST, ACC_PAST)]
    outs = run(shapes)
    ll = engine.last_launch()
    assert (ll["kind"], ll["ns"], ll["k"], ll["npairs"], ll["q8_declined"]) == ("sparse_krow", 4, 4, 2, 1), ll
    for (R, C), (hr, hc) in zip(shapes, outs):
        want_r, want_c = _exact.homopolymer_lg(R, C, ACC_V, ACC_G).headers(TBY, ACC_TBX)
        assert torch.equal(hr.cpu(), torch.from_numpy(want_r.astype(np.int32)))
        assert torch.equal(hc.cpu(), torch.from_numpy(want_c.astype(np.int32)))


@pytest.mark.timeout(300)
def test_accumulator_full_fused(engine, knobs):
    """The fused full fill of the 65 537 pair, 17 GB: every word against the closed form, on the device,
    a gigabyte of rows at a time.  The 65 539 pair's last cells are past the bound: refused."""
    import torch
    FULL[1].select(knobs)
    knobs("GSA_FUSED_STAGED", None)  # the library's own choice at this size: staged
    n = ACC_INSIDE
    y = torch.zeros(ACC_PAST + 1, dtype=torch.int32, device="cuda:0")
    s = _dev(acc_table())
    buf = torch.empty((ACC_PAST + 1) * (ACC_PAST + 1), dtype=torch.int32, device="cuda:0")
    engine.fill_full_dev(y.data_ptr(), n + 1, y.data_ptr(), n + 1, s.data_ptr(), 1, ACC_G, buf.data_ptr())
    engine.sync()
    ll = engine.last_launch()
    assert (ll["kind"], ll["ns"], ll["k"], ll["staged"], ll["npairs"]) == ("full_fused", 4, 4, 1, 1), ll
    M = buf[:(n + 1) * (n + 1)].view(n + 1, n + 1)
    j = torch.arange(n + 1, dtype=torch.int64, device="cuda:0")[None, :]
    rows = (1 << 28) // (n + 1)
    for i0 in range(0, n + 1, rows):
        i = torch.arange(i0, min(i0 + rows, n + 1), dtype=torch.int64, device="cuda:0")[:, None]
        want = (ACC_V * torch.minimum(i, j) + ACC_G * (i - j).abs()).to(torch.int32)
        assert torch.equal(M[i0:i0 + rows], want), i0
        del want

    def past():
        engine.fill_full_dev(y.data_ptr(), ACC_PAST + 1, y.data_ptr(), ACC_PAST + 1, s.data_ptr(), 1, ACC_G, buf.data_ptr())
        engine.sync()

    _kernel_failure(past)
    del M, buf
    torch.cuda.empty_cache()


# -- the device check and trace on the same tables ---------------------------------------------------------

@pytest.mark.parametrize("name", CHECK_CASES)
def test_check_and_trace(engine, knobs, name):
    """gsa_check_sparse_dev and gsa_check_full_dev find nothing in the fills' output and find one planted
    wrong word; gsa_trace_sparse_dev equals the host trace, its cost the exact one."""
    import torch
    case = case_named(name)
    SPARSE[0].select(knobs)
    Y, X = case.pair()
    R1, C1, tBx = len(Y), len(X), case.shape[2]
    ref = ref_single(name)
    y, x, s = _dev(Y), _dev(X), _dev(case.sub)
    args = (y.data_ptr(), R1, x.data_ptr(), C1, s.data_ptr(), case.substsz, case.g)
    geom = gsa.sparse_geometry(R1, C1, tBx)
    hr = torch.full((geom.hrowElems,), -7, dtype=torch.int32, device="cuda:0")
    hc = torch.full((geom.hcolElems,), -7, dtype=torch.int32, device="cuda:0")
    engine.fill_sparse_dev(*args, tBx, hr.data_ptr(), hc.data_ptr())
    engine.sync()
    SPARSE[0].assert_ran(engine.last_launch(), case)
    r = engine.check_sparse_dev(*args, geom, hr.data_ptr(), hc.data_ptr())
    assert r["mismatches"] == 0 and r["first"] == -1, r
    res = gsa.SparseResult(hr.cpu().numpy(), hc.cpu().numpy(), geom, 0, {})
    assert np.array_equal(res.hrow, ref.hrow) and np.array_equal(res.hcol, ref.hcol)
    host = gsa.trace_sparse(res, Y, X, case.sub, case.g)
    assert engine.trace_sparse_dev(*args, geom, hr.data_ptr(), hc.data_ptr()) == host
    assert host[2] == ref.cost
    k = (geom.tileHdrMatCols + 1) * geom.tileHrowLen + 17  # tile (1, 1), an interior header row word
    hr[k] += 1
    r = engine.check_sparse_dev(*args, geom, hr.data_ptr(), hc.data_ptr())
    assert r["mismatches"] >= 1 and 0 <= r["first"] <= k, r
    FULL[0].select(knobs)
    sc = torch.full((R1 * C1,), -7, dtype=torch.int32, device="cuda:0")
    engine.fill_full_dev(*args, sc.data_ptr())
    engine.sync()
    FULL[0].assert_ran(engine.last_launch(), case)
    assert engine.check_full_dev(*args, sc.data_ptr()) == {"checked": R1 * C1, "mismatches": 0, "first": -1}
    assert np.array_equal(sc.cpu().numpy().reshape(R1, C1), ref.full)
    sc[1234 * C1 + 567] -= 1
    r = engine.check_full_dev(*args, sc.data_ptr())
    assert r["mismatches"] >= 1 and r["first"] == 1234 * C1 + 567, r
