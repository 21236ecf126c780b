"""One checked runner per entry-point family, for the tests that run the families against each other on
one context (tests/test_gpu_ctx_buffers.py, tests/test_gpu_ctx_sequences.py, tests/test_gpu_streams.py).
No fixtures and no GPU work at import; tests/test_families_inputs.py checks the inputs without a GPU.

A family has a `name`, deterministic host `inputs(size, decoy=False)`, the CPU reference's `want(size)`
(computed once per session) and `run(engine, size, stream=None, late=None)`, which uploads, calls,
asserts the result equal to `want` in every field and asserts the route that ran, from
gsa_last_launch's kind or the call's own info struct.  It returns the raw result, so that two runs can
be compared for identity.

The references, used directly and never through the library: tests/_exact.py (global and local
scores, the fills and their headers), tests/_align_oracle.py with every CIGAR also through
_exact.rescore (global and local alignments), tests/_semi_oracle.py, tests/_overlap_oracle.py, and
oracle.* for Trace1 / Trace2 and the hashes.

Two sizes.  SMALL is the smallest at which the shared state is really used: 300 x 250 for the fills and
the score calls; for the long pairs' align calls R just over one strip (600 rows where a strip is 512,
1100 where it is 1024, C = 0.8 R), so that two strips are filled and a checkpoint row is read back
from the granules; batches of three such pairs of different lengths; 9 subjects of 1 .. 80 letters and
a query under one sweep for the database calls, two queries for the multi calls.  LARGE is 3 x in
every length (a query over two sweeps, 150 subjects), so that every buffer regrows.

decoy=True: inputs of the same lengths and alphabet with other letters and another table (20 letters
below substsz = 25, values -4 .. 11).  `want` asserts that the decoy's result differs, so a call that
reads an input too early, on the wrong stream, gives a wrong answer and never an access out of range.
`late` (a Late) puts the decoy into the device tensors first and copies the true inputs over them on
the stream behind a delay.

DIRTY are predecessors that leave something behind on purpose: a rejected call, the int16 flag raised,
a status 1 hit, chunked and multi-round aligns, a short CIGAR buffer, a batch pair that goes alone."""
import ctypes
import os

import numpy as np

import gpuseqalign_amd as gsa
import oracle
from gpuseqalign_amd import formats as F
from tests import _align_oracle as ao
from tests import _exact
from tests import _overlap_oracle as oo
from tests import _semi_oracle as so
from tests._data import RESRC, random_pair
from tests._semi_pair import hdr, path_of, strip_rows

SMALL, LARGE = "small", "large"
SIZES = (SMALL, LARGE)
PAIR = {SMALL: (300, 250), LARGE: (3000, 2500)}
TRIPLE = {SMALL: [(300, 250), (250, 300), (120, 280)], LARGE: [(3000, 2500), (2500, 3000), (1200, 2800)]}
G = -11
TRACE_BX = 1024  # a tile too wide for its move codes to sit in LDS: they stay in global memory
K_LANE = 24      # query rows a lane of the database kernels holds; run_db compares with gsa_last_launch
SWEEP = 16 * K_LANE
BATCH_STRIP = 1024  # the batched align calls' strip height in every gap model
DECOY = 100003      # added to every seed
FIELDS = ("score", "i_start", "j_start", "i_end", "j_end", "cigar")
# one affine and one linear gap model, and local where the call has it
MODES3 = [(-11, -1, False), (-4, -4, False), (-11, -1, True)]
MODES2 = [(-11, -1), (-4, -4)]
DB_MODES = [(-11, -1, False), (-4, -4, True)]

_REF = {}


def _once(key, fn):
    """A reference computed once and shared by the tests."""
    if key not in _REF:
        _REF[key] = fn()
    return _REF[key]


def table(decoy=False):
    """The flat 25 x 25 table: blosum62, or the decoy's (values -4 .. 11)."""
    if decoy:
        return _once("decoy table", lambda: np.random.default_rng(4099).integers(-4, 12, 625).astype(np.int32))
    return _once("table", lambda: np.ascontiguousarray(
        F.read_subst_json(os.path.join(RESRC, "subst.json")).matrix("blosum62"), dtype=np.int32).ravel())


SUBSTSZ = 25


def _pair(R, C, decoy=False):
    return random_pair(R, C, 11 * R + C + (DECOY if decoy else 0))


def long_pair(R, C, seed):
    """Y: R - C random letters, then the subject X mutated: every alignment mode runs from about row
    R - C to the last row, across every strip boundary at a column well inside the matrix."""
    x = F.synthetic_seq(C, seed)
    m = F.mutate_seq(x, seed + 1)[1:]
    head = F.synthetic_seq(R, seed + 2)[1:]
    return hdr(np.concatenate([head[:max(R - len(m), 0)], m])[-R:]), x


def long_shape(size, tr):
    R = {512: 600, 1024: 1100}[tr] * (3 if size == LARGE else 1)
    return R, R * 4 // 5


def long_triple(size):
    R, C = long_shape(size, BATCH_STRIP)
    return [(R, C), (R + 130, C + 40), (R + 60, C + 90)]


def _n(x):
    """A result in plain values, so that == compares it."""
    if isinstance(x, np.ndarray):
        return (x.dtype.str, x.shape, x.tobytes())
    if isinstance(x, (list, tuple)):
        return tuple(_n(v) for v in x)
    if isinstance(x, dict):
        return tuple((k, _n(v)) for k, v in sorted(x.items()))
    if isinstance(x, (np.integer,)):
        return int(x)
    return x


def _i32(a):
    a = np.asarray(a)
    assert a.min() >= -(1 << 31) and a.max() < (1 << 31)
    return np.ascontiguousarray(a, dtype=np.int32)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to("cuda:0")


def _empty(n):
    """-7s, written on the default stream.  Nothing waits for them here (a wait for the default stream may
    wait for a side stream that shares its hardware queue, and with it for the late inputs): where a call
    on a side stream writes there, its kernels run behind Late's delay, or behind these in the same queue."""
    import torch
    return torch.full((int(n),), -7, dtype=torch.int32, device="cuda:0")


def _t3(r):
    return (r["score"], r["i_end"], r["j_end"])


def _t6(r):
    return tuple(r[f] for f in FIELDS)


class Late:
    """The decoy in the device tensors first; then, on `stream`, a delay of `cycles` and the copies of
    the true inputs from pinned memory, with an event behind them.  Nothing is synchronised: what the
    call under test issues anywhere but on `stream` sees the decoy."""

    def __init__(self, stream, cycles):
        self.stream, self.cycles, self.event, self.keep = stream, int(cycles), None, []

    def stage(self, true, decoy):
        import torch
        assert sorted(true) == sorted(decoy)
        dev = {k: _dev(decoy[k]) for k in true}
        pinned = {k: torch.from_numpy(np.ascontiguousarray(true[k], dtype=np.int32)).pin_memory() for k in true}
        for k in true:
            assert dev[k].shape == pinned[k].shape, k
        torch.cuda.synchronize()
        with torch.cuda.stream(self.stream):
            torch.cuda._sleep(self.cycles)
            for k in true:
                dev[k].copy_(pinned[k], non_blocking=True)
            self.event = torch.cuda.Event()
            self.event.record(self.stream)
        self.keep.append((dev, pinned))
        return dev

    def assert_pending(self, what):
        """Straight after an asynchronous call returned: the copies it depends on have not run yet."""
        assert self.event.query() is False, "%s: the late inputs had already arrived when the call returned" % what


class Family:
    """modes(size): what one run goes through; case(size, mode, decoy): {"dev": arrays that go to the
    device, ...host-side values}; ref(mode, case): the expected result; call(e, mode, case, t, stream,
    late): the result, with t the device tensors by name."""
    name = None
    takes_stream = True
    asynchronous = False
    krow_score = False  # a score call on the K-rows kernel: GSA_SCORE_K and GSA_KROW_Q8 apply
    knob = None

    def modes(self, size):
        return [None]

    def inputs(self, size, decoy=False):
        return [self.case(size, m, decoy) for m in self.modes(size)]

    def want(self, size):
        def make():
            true = [_n(self.ref(m, c)) for m, c in zip(self.modes(size), self.inputs(size))]
            for m, c, a in zip(self.modes(size), self.inputs(size, True), true):
                assert self.decoy_differs(m, c, a), (self.name, size, m, "the decoy's result equals the true one")
            return true
        return _once(("want", self.name, size), make)

    def decoy_differs(self, mode, decoy_case, true_result):
        return self.score_of(_n(self.ref(mode, decoy_case))) != self.score_of(true_result)

    def score_of(self, result):
        return result

    def run(self, e, size, stream=None, late=None, order=None):
        modes, want, got = self.modes(size), self.want(size), []
        assert stream is None or self.takes_stream
        if self.knob:
            e.set_knob(*self.knob)
        try:
            for k in (range(len(modes)) if order is None else order):
                c = self.case(size, modes[k], False)
                if late:
                    t = late.stage(c["dev"], self.case(size, modes[k], True)["dev"])
                else:
                    t = {n: _dev(a) for n, a in c["dev"].items()}
                    if stream is not None:  # the uploads ran on the default stream
                        import torch
                        torch.cuda.synchronize()
                g = _n(self.call(e, modes[k], c, t, stream, late))
                assert g == want[k], (self.name, size, modes[k], self.brief(g), self.brief(want[k]))
                got.append(g)
        finally:
            if self.knob:
                e.set_knob(self.knob[0], None)
        return got

    @staticmethod
    def brief(x):
        s = repr(x)
        return s if len(s) < 400 else s[:400] + " ..."


def _xy(t, k=""):
    return (t["y" + k].data_ptr(), t["y" + k].numel(), t["x" + k].data_ptr(), t["x" + k].numel())


# -- the fills ------------------------------------------------------------------------------------------

def headers(Y, X, sub, tBx):
    """(hrow, hcol, align_cost) of the NW-LG fill of the pair padded to whole tiles, from _exact."""
    tBy = gsa.sparse_tile_by()
    Yp, Xp, trows, tcols = _exact.pad_to_tiles(Y, X, tBy, tBx)
    H = _exact.fill_lg(Yp, Xp, sub, G)
    hr, hc = _exact.headers_of(H, trows, tcols, tBy, tBx)
    return _i32(hr), _i32(hc), int(H[len(Y) - 1, len(X) - 1])


def matrix(Y, X, sub):
    return _i32(_exact.fill_lg(Y, X, sub, G))


class _PairFamily(Family):
    def case(self, size, mode, decoy):
        Y, X = _pair(*PAIR[size], decoy)
        return {"dev": {"y": Y, "x": X, "sub": table(decoy)}}


class FillSparse(_PairFamily):
    name, asynchronous, tBx, kind = "fill_sparse", True, 64, "sparse_krow"

    def ref(self, mode, c):
        d = c["dev"]
        return headers(d["y"], d["x"], d["sub"], self.tBx)[:2]

    def launch(self, e, t, stream, late):
        geom = gsa.sparse_geometry(t["y"].numel(), t["x"].numel(), self.tBx)
        hr, hc = _empty(geom.hrowElems), _empty(geom.hcolElems)
        e.fill_sparse_dev(*_xy(t), t["sub"].data_ptr(), SUBSTSZ, G, self.tBx, hr.data_ptr(), hc.data_ptr(), stream)
        if late:
            late.assert_pending(self.name)
        return geom, hr, hc

    def call(self, e, mode, c, t, stream, late):
        _, hr, hc = self.launch(e, t, stream, late)
        e.sync(stream)
        assert e.last_launch()["kind"] == self.kind
        return hr.cpu().numpy(), hc.cpu().numpy()


class FillFull(_PairFamily):
    """A single pair: the fused two-pass fill."""
    name, asynchronous = "fill_full", True

    def ref(self, mode, c):
        d = c["dev"]
        return matrix(d["y"], d["x"], d["sub"])

    def launch(self, e, t, stream, late):
        out = _empty(t["y"].numel() * t["x"].numel())
        e.fill_full_dev(*_xy(t), t["sub"].data_ptr(), SUBSTSZ, G, out.data_ptr(), stream)
        if late:
            late.assert_pending(self.name)
        return out

    def call(self, e, mode, c, t, stream, late):
        out = self.launch(e, t, stream, late)
        e.sync(stream)
        assert e.last_launch()["kind"] == "full_fused"
        return out.cpu().numpy().reshape(t["y"].numel(), t["x"].numel())


class _TripleFamily(Family):
    def shapes(self, size):
        return TRIPLE[size]

    def pair(self, R, C, decoy):
        return _pair(R, C, decoy)

    def case(self, size, mode, decoy):
        dev = {"sub": table(decoy)}
        for k, (R, C) in enumerate(self.shapes(size)):
            dev["y%d" % k], dev["x%d" % k] = self.pair(R, C, decoy)
        return {"dev": dev}

    @staticmethod
    def pairs_of(c):
        return [(c["dev"]["y%d" % k], c["dev"]["x%d" % k]) for k in range(3)]

    @staticmethod
    def ptrs(t):
        return [_xy(t, str(k)) for k in range(3)]


class FillFullBatch(_TripleFamily):
    """Three pairs: the two-pass fill in two launches, its expansion scratch and staging."""
    name, asynchronous = "fill_full_batch", True

    def ref(self, mode, c):
        return [matrix(Y, X, c["dev"]["sub"]) for Y, X in self.pairs_of(c)]

    def call(self, e, mode, c, t, stream, late):
        outs = [_empty(p[1] * p[3]) for p in self.ptrs(t)]
        e.fill_batch_dev([p + (o.data_ptr(),) for p, o in zip(self.ptrs(t), outs)], t["sub"].data_ptr(), SUBSTSZ, G,
                         mode="full", stream=stream)
        if late:
            late.assert_pending(self.name)
        e.sync(stream)
        assert e.last_launch()["kind"] == "full_two_launch"
        return [o.cpu().numpy().reshape(p[1], p[3]) for p, o in zip(self.ptrs(t), outs)]


# -- global and local scores ------------------------------------------------------------------------------

class Score(_PairFamily):
    name, kind, both_ends, krow_score = "score", "score_krow", 0, True

    def modes(self, size):
        return MODES3

    def ref(self, mode, c):
        d = c["dev"]
        return _exact.score(d["y"], d["x"], d["sub"], *mode)

    def call(self, e, mode, c, t, stream, late):
        go, ge, local = mode
        r = e.score_dev(*_xy(t), t["sub"].data_ptr(), SUBSTSZ, go, ge, local, stream)
        ll = e.last_launch()
        assert ll["kind"] == self.kind, ll
        if not local:  # (a local pair may come back from both ends to one direction)
            assert ll["both_ends"] == self.both_ends, ll
        return _t3(r)


class ScoreBothEnds(Score):
    """GSA_SCORE_BIDI=2: from both ends at any size (the tap rows and reversed sequences' buffer)."""
    name, both_ends, knob = "score_both_ends", 1, ("GSA_SCORE_BIDI", "2")


class ScoreScan(Score):
    """GSA_SCORE_SCAN=1: the row scan and its boundary rows."""
    name, kind, knob, krow_score = "score_scan", "score_scan", ("GSA_SCORE_SCAN", "1"), False


class ScoreBatch(_TripleFamily):
    name, krow_score = "score_batch", True

    def modes(self, size):
        return MODES3

    def ref(self, mode, c):
        return [_exact.score(Y, X, c["dev"]["sub"], *mode) for Y, X in self.pairs_of(c)]

    def call(self, e, mode, c, t, stream, late):
        go, ge, local = mode
        res = e.score_batch_dev(self.ptrs(t), t["sub"].data_ptr(), SUBSTSZ, go, ge, local, stream)
        ll = e.last_launch()
        assert ll["kind"] == "score_krow" and ll["npairs"] == 3, ll
        return [_t3(r) for r in res]


# -- the database calls -----------------------------------------------------------------------------------

def db_pool(size, decoy=False):
    """(queries, subjects, hits): the small query fits one sweep (no boundary rows), the large one takes
    three; two different queries for the multi calls (the single-query calls take the first)."""
    R = {SMALL: SWEEP - 84, LARGE: 2 * SWEEP + 5}[size]
    n, lo, hi = {SMALL: (9, 1, 80), LARGE: (150, 200, 700)}[size]
    d = DECOY if decoy else 0
    lens = np.random.default_rng(R).integers(lo, hi + 1, n)
    queries = [F.synthetic_seq(R, 900 + R + d), F.synthetic_seq(R, 1900 + R + d)]
    subjects = [F.synthetic_seq(int(c), 1000 * R + i + d) for i, c in enumerate(lens)]
    return queries, subjects, list(range(0, n, max(1, n // 6)))


def _offsets(seqs):
    return np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.int64)


def _db_score(q, s, sub, go, ge, local, key):
    return _once(("dbs",) + key + (go, ge, local), lambda: _exact.score(q, s, sub, go, ge, local))


def _checked_align(q, s, sub, go, ge, local):
    """tests/_align_oracle.py's alignment, its CIGAR replayed by _exact.rescore."""
    w = ao.align(q, s, sub, go, ge, local)
    assert _exact.rescore(w[5], q, s, sub, go, ge, w[1], w[2], w[3], w[4]) == w[0], w[:5]
    return tuple(w)


class _DbFamily(Family):
    nq = 2

    def modes(self, size):
        return DB_MODES

    def case(self, size, mode, decoy):
        queries, subjects, hits = db_pool(size, decoy)
        queries = queries[:self.nq]
        return {"dev": {"q": np.concatenate(queries), "db": np.concatenate(subjects), "sub": table(decoy)},
                "queries": queries, "subjects": subjects, "hits": hits, "q_off": _offsets(queries),
                "off": _offsets(subjects), "key": (size, decoy)}

    @staticmethod
    def hit_pairs(c):
        """(query, subject) of the multi calls' hits: every chosen subject for query 0, then in reverse
        order for query 1."""
        return [(0, h) for h in c["hits"]] + [(1, h) for h in c["hits"][::-1]]

    def score_of(self, result):
        return result[0]


class _DbExactScores(_DbFamily):
    """The global and local score calls: _exact.score per pair is slow, so the decoy is compared on
    query 0 against the first five subjects."""

    def decoy_differs(self, mode, decoy_case, true_result):
        d, sub = decoy_case, decoy_case["dev"]["sub"]
        dec = [_db_score(d["queries"][0], d["subjects"][k], sub, *mode, d["key"] + (0, k))[0] for k in range(5)]
        first = true_result[0][0] if self.nq == 2 else true_result[0]
        return tuple(dec) != tuple(r if self.nq == 2 else r[0] for r in first[:5])


class Db(_DbExactScores):
    """score_db_dev and align_db_dev."""
    name, nq = "db", 1

    def ref(self, mode, c):
        q, sub = c["queries"][0], c["dev"]["sub"]
        scores = [_db_score(q, s, sub, *mode, c["key"] + (0, k)) for k, s in enumerate(c["subjects"])]
        return scores, [_checked_align(q, c["subjects"][h], sub, *mode) for h in c["hits"]]

    def call(self, e, mode, c, t, stream, late):
        go, ge, local = mode
        n = len(c["subjects"])
        res = e.score_db_dev(t["q"].data_ptr(), t["q"].numel(), t["db"].data_ptr(), c["off"], t["sub"].data_ptr(), SUBSTSZ,
                             go, ge, local, stream)
        ll = e.last_launch()
        assert ll["kind"] == "score_lanes" and ll["npairs"] == n and ll["k"] == K_LANE, ll
        al = e.align_db_dev(t["q"].data_ptr(), t["q"].numel(), t["db"].data_ptr(), c["off"], c["hits"], t["sub"].data_ptr(),
                            SUBSTSZ, go, ge, local, 0, stream)
        info = e.last_align_db_info()
        assert info["lane_hits"] == len(c["hits"]) and info["unsupported"] == 0 and info["chunks"] == 1, info
        assert all(r["status"] == 0 for r in al), al
        return [_t3(r) for r in res], [_t6(r) for r in al]


def _ranked(rows, top):
    """Per query the `top` best (subject, score, i_end, j_end) by (score descending, subject ascending)."""
    out = []
    for row in rows:
        order = sorted(range(len(row)), key=lambda s: (-row[s][0], s))[:top]
        out.append([(s,) + tuple(row[s]) for s in order])
    return out


TOP = 3


class ScoreDbMulti(_DbExactScores):
    name, entry = "score_db_multi", "score_db_multi_dev"

    def rows(self, mode, c):
        sub = c["dev"]["sub"]
        return [[_db_score(q, s, sub, *mode, c["key"] + (i, k)) for k, s in enumerate(c["subjects"])]
                for i, q in enumerate(c["queries"])]

    def ref(self, mode, c):
        rows = self.rows(mode, c)
        return [[r[0] for r in row] for row in rows], _ranked(rows, TOP)

    def info(self, e):
        return e.last_score_db_multi_info()

    def call(self, e, mode, c, t, stream, late):
        r = getattr(e, self.entry)(t["q"].data_ptr(), c["q_off"], t["db"].data_ptr(), c["off"], t["sub"].data_ptr(), SUBSTSZ,
                                   *mode, top=TOP, stream=stream)
        info = self.info(e)
        assert (info["lane_queries"], info["other_queries"]) == (2, 0), info
        assert info["lane_pairs"] == 2 * len(c["subjects"]), info
        hits = [[tuple(int(v) for v in h) for h in row] for row in r["hits"]]
        return r["scores"].tolist(), hits


class AlignDbMulti(_DbFamily):
    name, entry = "align_db_multi", "align_db_multi_dev"

    def ref(self, mode, c):
        sub = c["dev"]["sub"]
        al = [_checked_align(c["queries"][q], c["subjects"][s], sub, *mode) for q, s in self.hit_pairs(c)]
        return [a[0] for a in al], al

    def info(self, e):
        return e.last_align_db_multi_info()

    def call(self, e, mode, c, t, stream, late):
        hp = self.hit_pairs(c)
        al = getattr(e, self.entry)(t["q"].data_ptr(), c["q_off"], t["db"].data_ptr(), c["off"], [q for q, _ in hp],
                                    [s for _, s in hp], t["sub"].data_ptr(), SUBSTSZ, *mode, stream=stream)
        info = self.info(e)
        assert info["lane_hits"] == len(hp) and info["unsupported"] == 0, info
        assert all(r["status"] == 0 for r in al), al
        return [r["score"] for r in al], [_t6(r) for r in al]


class ScoreDbSemi(ScoreDbMulti):
    name, entry = "score_db_semi", "score_db_semi_dev"
    decoy_differs = Family.decoy_differs

    def modes(self, size):
        return MODES2

    def rows(self, mode, c):
        sub = c["dev"]["sub"]
        return [[so.score(q, s, sub, *mode) for s in c["subjects"]] for q in c["queries"]]

    def info(self, e):
        return e.last_score_db_semi_info()


class AlignDbSemi(AlignDbMulti):
    name, entry = "align_db_semi", "align_db_semi_dev"

    def modes(self, size):
        return MODES2

    def ref(self, mode, c):
        sub = c["dev"]["sub"]
        al = [tuple(so.align(c["queries"][q], c["subjects"][s], sub, *mode)) for q, s in self.hit_pairs(c)]
        return [a[0] for a in al], al

    def info(self, e):
        return e.last_align_db_semi_info()


# -- Trace2 on the device, the host-array calls, the verification calls -----------------------------------

class TraceSparse(FillSparse):
    """fill_sparse_dev and, behind it on the same stream, trace_sparse_dev."""
    name, asynchronous, tBx = "trace_sparse", True, TRACE_BX

    def ref(self, mode, c):
        d = c["dev"]
        hr, hc, _ = headers(d["y"], d["x"], d["sub"], self.tBx)
        tBy = gsa.sparse_tile_by()
        trows, tcols = oracle.sparse_geometry(len(d["y"]), len(d["x"]), tBy, self.tBx)
        return oracle.trace_sparse(hr, hc, trows, tcols, tBy, self.tBx, d["y"], d["x"], d["sub"], G)

    def call(self, e, mode, c, t, stream, late):
        geom, hr, hc = self.launch(e, t, stream, late)
        if stream is None:
            e.sync()
        got = e.trace_sparse_dev(*_xy(t), t["sub"].data_ptr(), SUBSTSZ, G, geom, hr.data_ptr(), hc.data_ptr(), stream)
        ll = e.last_launch()
        assert ll["kind"] == "trace_sparse", ll
        e.sync(stream)
        return got


class AlignSparse(_PairFamily):
    name, takes_stream, overlap = "align_sparse", False, False

    def ref(self, mode, c):
        d = c["dev"]
        return headers(d["y"], d["x"], d["sub"], 64)

    def call(self, e, mode, c, t, stream, late):
        d = c["dev"]
        r = e.align_sparse(d["y"], d["x"], d["sub"], G, tileBx=64, overlap=self.overlap)
        return r.hrow, r.hcol, r.align_cost


class AlignSparsePt(AlignSparse):
    name, overlap = "align_sparse_pt", True


def expected_sparse_checks(geom):
    tr, tc, W, H = geom.tileHdrMatRows, geom.tileHdrMatCols, geom.tileHrowLen, geom.tileHcolLen
    return tr * H + tc * W + tr * tc + (tr - 1) * tc * W + tr * (tc - 1) * H


class CheckSparse(_PairFamily):
    """check_sparse_dev over the reference's headers; the decoy's headers are all -7, which no pair
    gives: (values checked, clean)."""
    name, tBx = "check_sparse", 64

    def case(self, size, mode, decoy):
        c = super().case(size, mode, decoy)
        t = super().case(size, mode, False)["dev"]
        hr, hc = _once(("hdr", size, self.tBx), lambda: headers(t["y"], t["x"], t["sub"], self.tBx)[:2])
        if decoy:
            hr, hc = np.full_like(hr, -7), np.full_like(hc, -7)
        c["dev"]["hr"], c["dev"]["hc"] = hr, hc
        return c

    def ref(self, mode, c):
        d = c["dev"]
        geom = gsa.sparse_geometry(len(d["y"]), len(d["x"]), self.tBx)
        hr, hc, _ = headers(d["y"], d["x"], d["sub"], self.tBx)
        return expected_sparse_checks(geom), bool(np.array_equal(hr, d["hr"]) and np.array_equal(hc, d["hc"]))

    def call(self, e, mode, c, t, stream, late):
        geom = gsa.sparse_geometry(t["y"].numel(), t["x"].numel(), self.tBx)
        r = e.check_sparse_dev(*_xy(t), t["sub"].data_ptr(), SUBSTSZ, G, geom, t["hr"].data_ptr(), t["hc"].data_ptr(), stream)
        return r["checked"], r["mismatches"] == 0 and r["first"] == -1


class _MatrixFamily(_PairFamily):
    """The reference's full matrix among the inputs; the decoy's is the decoy pair's own."""

    def case(self, size, mode, decoy):
        c = super().case(size, mode, decoy)
        d = c["dev"]
        d["score"] = _once(("matrix", size, decoy), lambda: matrix(d["y"], d["x"], d["sub"])).ravel()
        return c

    @staticmethod
    def mat(c):
        d = c["dev"]
        return d["score"].reshape(len(d["y"]), len(d["x"]))


class CheckFull(_MatrixFamily):
    """check_full_dev; the decoy's matrix is all -7: (cells checked, clean)."""
    name = "check_full"

    def case(self, size, mode, decoy):
        c = super().case(size, mode, decoy)
        if decoy:
            c["dev"]["score"] = np.full_like(c["dev"]["score"], -7)
        return c

    def ref(self, mode, c):
        d = c["dev"]
        return d["score"].size, bool(np.array_equal(matrix(d["y"], d["x"], d["sub"]).ravel(), d["score"]))

    def call(self, e, mode, c, t, stream, late):
        r = e.check_full_dev(*_xy(t), t["sub"].data_ptr(), SUBSTSZ, G, t["score"].data_ptr(), stream)
        return r["checked"], r["mismatches"] == 0 and r["first"] == -1


class HashFull(_MatrixFamily):
    name = "hash_full"

    def ref(self, mode, c):
        return oracle.hash_full(self.mat(c))

    def call(self, e, mode, c, t, stream, late):
        return e.hash_full_dev(t["score"].data_ptr(), t["y"].numel(), t["x"].numel(), None, stream)


class TraceFull(_MatrixFamily):
    name = "trace_full"

    def ref(self, mode, c):
        d = c["dev"]
        h, s = oracle.trace_full(self.mat(c), d["y"], d["x"])
        return h, s, int(self.mat(c)[-1, -1])

    def call(self, e, mode, c, t, stream, late):
        return e.trace_full_dev(*_xy(t), t["score"].data_ptr(), None, stream)


# -- long pairs: alignments in the four modes, single and batched -----------------------------------------

def crosses(w, tr):
    """The strips an alignment w (score, i_start, j_start, i_end, j_end, cigar) makes a bottom-up trace
    fill when nothing limits it: those of the rows above the end cell down to the strip where the path
    stops or reaches column 0."""
    cells = path_of(w)  # last cell first
    if w[4] == 0 or w[3] == 0:
        return 0
    hi = -(-w[3] // tr) - 1
    lo = hi
    while lo > 0:
        at = [j for i, j in cells if i == lo * tr]
        if not at or at[0] == 0:
            break
        lo -= 1
    return hi - lo + 1


class _LongPair(Family):
    local_too = False

    def modes(self, size):
        return MODES3 if self.local_too else MODES2

    def tr(self, mode):
        return strip_rows(mode[0], mode[1])

    def case(self, size, mode, decoy):
        R, C = long_shape(size, self.tr(mode))
        Y, X = long_pair(R, C, 17 * R + C + (DECOY if decoy else 0))
        return {"dev": {"y": Y, "x": X, "sub": table(decoy)}}

    def score_of(self, result):
        return result[0]


class _LongBatch(_TripleFamily):
    local_too = False

    def modes(self, size):
        return MODES3 if self.local_too else MODES2

    def shapes(self, size):
        return long_triple(size)

    def pair(self, R, C, decoy):
        return long_pair(R, C, 17 * R + C + (DECOY if decoy else 0))

    def score_of(self, result):
        return tuple(r[0] for r in result)


def _align_glocal(Y, X, sub, go, ge, local):
    return _checked_align(Y, X, sub, go, ge, local)


class AlignPair(_LongPair):
    name, local_too = "align_pair", True

    def ref(self, mode, c):
        d = c["dev"]
        return _align_glocal(d["y"], d["x"], d["sub"], *mode)

    def call(self, e, mode, c, t, stream, late, limit=0):
        go, ge, local = mode
        r = e.align_pair_dev(*_xy(t), t["sub"].data_ptr(), SUBSTSZ, go, ge, local, limit, stream)
        info = e.last_align_pair_info()
        assert r["status"] == 0 and info["strip_rows"] == self.tr(mode) and info["strips_filled"] >= 2, (r["status"], info)
        assert (info["chunks"] == 1) == (limit == 0), info
        return _t6(r)


class AlignBatch(_LongBatch):
    name, local_too = "align_batch", True

    def ref(self, mode, c):
        return [_align_glocal(Y, X, c["dev"]["sub"], *mode) for Y, X in self.pairs_of(c)]

    def call(self, e, mode, c, t, stream, late, limit=0):
        go, ge, local = mode
        res = e.align_batch_dev(self.ptrs(t), t["sub"].data_ptr(), SUBSTSZ, go, ge, local, 0, limit, stream)
        info = e.last_align_batch_info()
        assert (info["batch_pairs"], info["alone_pairs"], info["host_pairs"]) == (3, 0, 0), info
        assert info["strip_rows"] == BATCH_STRIP and info["strips_filled"] >= 6, info
        assert (info["rounds"] == 1) == (limit == 0), info
        assert all(r["status"] == 0 for r in res), res
        return [_t6(r) for r in res]


class _ScorePair(_LongPair):
    krow_score = True

    def ref(self, mode, c):
        d = c["dev"]
        return tuple(self.oracle(d["y"], d["x"], d["sub"], *mode))

    def call(self, e, mode, c, t, stream, late):
        r = getattr(e, self.entry)(*_xy(t), t["sub"].data_ptr(), SUBSTSZ, *mode, stream)
        assert r["kernel_ms"] > 0, r  # (the call has one route and leaves no launch record)
        return _t3(r)


class ScoreSemi(_ScorePair):
    name, entry, oracle = "score_semi", "score_semi_dev", staticmethod(so.score)


class ScoreOverlap(_ScorePair):
    name, entry, oracle = "score_overlap", "score_overlap_dev", staticmethod(oo.score)


class _AlignPairMode(_LongPair):
    def ref(self, mode, c):
        d = c["dev"]
        return tuple(self.oracle(d["y"], d["x"], d["sub"], *mode))

    def call(self, e, mode, c, t, stream, late):
        r = getattr(e, self.entry)(*_xy(t), t["sub"].data_ptr(), SUBSTSZ, *mode, 0, stream)
        info = getattr(e, self.info)()
        assert r["status"] == 0 and info["strip_rows"] == self.tr(mode), (r["status"], info)
        assert info["strips_filled"] >= 2 and info["chunks"] == 1, info
        return _t6(r)


class AlignPairSemi(_AlignPairMode):
    name, entry, info, oracle = "align_pair_semi", "align_pair_semi_dev", "last_align_pair_semi_info", staticmethod(so.align)


class AlignPairOverlap(_AlignPairMode):
    name, entry, info, oracle = ("align_pair_overlap", "align_pair_overlap_dev", "last_align_pair_overlap_info",
                                 staticmethod(oo.align))


class _ScoreBatchMode(_LongBatch):
    krow_score = True

    def ref(self, mode, c):
        return [tuple(self.oracle(Y, X, c["dev"]["sub"], *mode)) for Y, X in self.pairs_of(c)]

    def call(self, e, mode, c, t, stream, late):
        res = getattr(e, self.entry)(self.ptrs(t), t["sub"].data_ptr(), SUBSTSZ, *mode, stream)
        assert res[0]["kernel_ms"] > 0, res  # (the call has one route and leaves no launch record)
        return [_t3(r) for r in res]


class ScoreSemiBatch(_ScoreBatchMode):
    name, entry, oracle = "score_semi_batch", "score_semi_batch_dev", staticmethod(so.score)


class ScoreOverlapBatch(_ScoreBatchMode):
    name, entry, oracle = "score_overlap_batch", "score_overlap_batch_dev", staticmethod(oo.score)


class _AlignBatchMode(_LongBatch):
    def ref(self, mode, c):
        return [tuple(self.oracle(Y, X, c["dev"]["sub"], *mode)) for Y, X in self.pairs_of(c)]

    def call(self, e, mode, c, t, stream, late):
        res = getattr(e, self.entry)(self.ptrs(t), t["sub"].data_ptr(), SUBSTSZ, *mode, 0, 0, stream)
        info = getattr(e, self.info)()
        assert (info["batch_pairs"], info["host_pairs"]) == (3, 0), info
        assert info["strip_rows"] == BATCH_STRIP and info["strips_filled"] >= 6 and info["rounds"] == 1, info
        assert all(r["status"] == 0 for r in res), res
        return [_t6(r) for r in res]


class AlignBatchSemi(_AlignBatchMode):
    name, entry, info, oracle = ("align_batch_semi", "align_batch_semi_dev", "last_align_batch_semi_info",
                                 staticmethod(so.align))


class AlignBatchOverlap(_AlignBatchMode):
    name, entry, info, oracle = ("align_batch_overlap", "align_batch_overlap_dev", "last_align_batch_overlap_info",
                                 staticmethod(oo.align))


FAMILIES = [FillSparse(), FillFull(), FillFullBatch(), Score(), ScoreBothEnds(), ScoreScan(), ScoreBatch(), Db(),
            TraceSparse(), AlignSparse(), AlignSparsePt(),
            ScoreDbMulti(), AlignDbMulti(), ScoreDbSemi(), AlignDbSemi(), AlignPair(), AlignBatch(), ScoreSemi(),
            AlignPairSemi(), ScoreSemiBatch(), AlignBatchSemi(), ScoreOverlap(), AlignPairOverlap(), ScoreOverlapBatch(),
            AlignBatchOverlap(),
            CheckSparse(), CheckFull(), HashFull(), TraceFull()]
BY_NAME = {f.name: f for f in FAMILIES}
assert len(BY_NAME) == len(FAMILIES) == 29


# -- dirty predecessors -----------------------------------------------------------------------------------
# Each has name, inputs() (host values, built without a GPU), guard() (asserts, without a GPU, that the
# inputs lie on the side of their guard they are meant to) and run(e), which checks what the call should
# itself return.

def _vr():
    from tests import test_gpu_value_ranges as vr  # its input builders; no GPU work at import
    return vr


class Rejected:
    """A global score one step past B + |go| < 2^29: errorInvalidValue before anything is enqueued."""
    name = "dirty_rejected"

    def inputs(self):
        vr = _vr()
        R, C = vr.SCAN_SHAPES[0]
        Y, X = vr.scan_pair(R, C)
        return Y, X, vr.table20(), vr.gaps_at(vr.GLOBAL_LIMIT, R, C, 11, True, 1, past=True)

    def guard(self):
        vr = _vr()
        Y, X, t, (go, ge) = self.inputs()
        assert np.abs(t).max() == 11
        assert vr.bound(len(Y) - 1, len(X) - 1, 11, go, ge, 1) >= vr.GLOBAL_LIMIT
        inside = vr.gaps_at(vr.GLOBAL_LIMIT, len(Y) - 1, len(X) - 1, 11, True, 1)
        assert vr.bound(len(Y) - 1, len(X) - 1, 11, *inside, 1) < vr.GLOBAL_LIMIT and inside[1] == ge + 1

    def run(self, e):
        Y, X, t, (go, ge) = self.inputs()
        y, x, s = _dev(Y), _dev(X), _dev(t)
        try:
            e.score_dev(y.data_ptr(), len(Y), x.data_ptr(), len(X), s.data_ptr(), 20, go, ge, False)
        except gsa.NwError as err:
            assert err.stat == gsa.NwStat.errorInvalidValue, err
        else:
            raise AssertionError("a global score past the bound was accepted")


class Int16Flag:
    """A table entry with s - go - ge = 32768: the K-rows kernel raises its flag, the row scan answers."""
    name = "dirty_int16_flag"

    def inputs(self):
        vr = _vr()
        Y, X = random_pair(*vr.EDGE_PAIR, 77)
        return Y, X, vr.edge_table(32756)

    def guard(self):
        Y, X, t = self.inputs()
        assert int(t.max()) + 11 + 1 == 32768 and int(t.max()) - 1 + 12 == 32767
        assert t[Y[1:, None], X[None, 1:]].max() == 32756, "the pair never reads the entry"

    def run(self, e):
        Y, X, t = self.inputs()
        y, x, s = _dev(Y), _dev(X), _dev(t)
        r = e.score_dev(y.data_ptr(), len(Y), x.data_ptr(), len(X), s.data_ptr(), 20, -11, -1, False)
        assert e.last_launch()["kind"] == "score_scan", e.last_launch()
        assert _t3(r) == _once("int16 flag", lambda: _exact.score(Y, X, t, -11, -1, False)), r


class Status1Hit:
    """align_db_dev with one hit at B >= 2^26: that hit comes back with status 1, the others traced."""
    name = "dirty_status1_hit"

    def inputs(self):
        vr = _vr()
        queries, subjects, t = vr.trace_pool(K_LANE)
        R = len(queries[0]) - 1
        return queries[0], subjects, t, vr.gaps_at(vr.TRACE_LIMIT, R, max(vr.TRACE_LENS), 11, True, 0, past=True)

    def guard(self):
        vr = _vr()
        q, subjects, t, (go, ge) = self.inputs()
        over = [vr.bound(len(q) - 1, len(s) - 1, 11, go, ge, 0) >= vr.TRACE_LIMIT for s in subjects]
        assert over == [False, False, True], over
        assert vr.bound(len(q) - 1, max(vr.TRACE_LENS), 11, go, ge, 1) < vr.GLOBAL_LIMIT

    def run(self, e):
        q, subjects, t, (go, ge) = self.inputs()
        dq, db, s = _dev(q), _dev(np.concatenate(subjects)), _dev(t)
        res = e.align_db_dev(dq.data_ptr(), len(q), db.data_ptr(), _offsets(subjects), [0, 1, 2], s.data_ptr(), 20, go, ge, False)
        info = e.last_align_db_info()
        assert (info["lane_hits"], info["unsupported"]) == (2, 1) and [r["status"] for r in res] == [0, 0, 1], (info, res)
        for k, (x, r) in enumerate(zip(subjects, res)):
            assert _t3(r) == _once(("status1", k), lambda: _exact.score(q, x, t, go, ge, False)), (k, r)
            if r["status"] == 0:
                assert _exact.rescore(r["cigar"], q, x, t, go, ge, 0, 0, r["i_end"], r["j_end"]) == r["score"], (k, r)


class _Limited:
    """An align family's SMALL linear-gap case under a scratch_limit of one strip's codes (+ 1 byte)."""
    mode = (-4, -4, False)

    def inputs(self):
        return self.family.case(SMALL, self.mode, False)

    def run(self, e):
        c = self.inputs()
        t = {n: _dev(a) for n, a in c["dev"].items()}
        got = _n(self.family.call(e, self.mode, c, t, None, None, limit=self.limit()))
        assert got == self.family.want(SMALL)[MODES3.index(self.mode)], (self.name, Family.brief(got))
        self.evidence(e)


class ChunkedPair(_Limited):
    """align_pair_dev in at least two chunks."""
    name, family = "dirty_chunked_pair", BY_NAME["align_pair"]

    def limit(self):
        d = self.inputs()["dev"]
        return (len(d["x"]) - 1) * strip_rows(*self.mode[:2]) // 2 + 1

    def guard(self):
        R = len(self.inputs()["dev"]["y"]) - 1
        tr = strip_rows(*self.mode[:2])
        assert -(-R // tr) == 2 and 2 * (self.limit() - 1) > self.limit(), "one strip fits, two do not"

    def evidence(self, e):
        assert e.last_align_pair_info()["chunks"] >= 2, e.last_align_pair_info()


class RoundsBatch(_Limited):
    """align_batch_dev in at least two rounds."""
    name, family = "dirty_rounds_batch", BY_NAME["align_batch"]

    def limit(self):
        d = self.inputs()["dev"]
        return max(len(d["x%d" % k]) - 1 for k in range(3)) * BATCH_STRIP // 2 + 1

    def guard(self):
        d = self.inputs()["dev"]
        strips = [(len(d["x%d" % k]) - 1) * BATCH_STRIP // 2 for k in range(3)]
        assert all(s <= self.limit() for s in strips) and sorted(strips)[0] + sorted(strips)[1] > self.limit()

    def evidence(self, e):
        assert e.last_align_batch_info()["rounds"] >= 2, e.last_align_batch_info()


class ShortCigar:
    """align_pair_dev with cigar_cap one byte short: status 2, the need reported, score and cells right."""
    name, family, mode = "dirty_short_cigar", BY_NAME["align_pair"], (-11, -1, False)

    def inputs(self):
        return self.family.case(SMALL, self.mode, False)

    def guard(self):
        assert len(self.family.want(SMALL)[0][5]) >= 2

    def run(self, e):
        c = self.inputs()
        t = {n: _dev(a) for n, a in c["dev"].items()}
        want = self.family.want(SMALL)[0]
        n = len(want[5])
        res, info = gsa.AlignDbResult(), gsa.AlignPairInfo()
        need, ms = ctypes.c_int64(-1), ctypes.c_float(0)
        buf = ctypes.create_string_buffer(n)
        st = gsa.lib().gsa_align_pair_dev(e._h, *_xy(t), t["sub"].data_ptr(), SUBSTSZ, -11, -1, 0, 0, ctypes.byref(res), buf, n,
                                          ctypes.byref(need), ctypes.byref(info), ctypes.byref(ms), None)
        assert st == 0 and res.status == 2 and need.value == n + 1, (st, res.status, need.value, n)
        assert (res.score, res.i_start, res.j_start, res.i_end, res.j_end) == want[:5]


class AlonePair:
    """An align_batch_dev list whose middle pair has B >= 2^26: it goes alone (align_pair_dev's path, which
    overwrites the granules and the pair slots) and comes back with status 1; its neighbours are traced."""
    name, mode = "dirty_alone_pair", (-11, -1, False)

    def inputs(self):
        t = table().reshape(25, 25).copy()
        t[np.diag_indices_from(t)] = 30000
        return [long_pair(700, 650, 41), long_pair(2400, 2300, 43), long_pair(1100, 300, 47)], t.ravel()

    def guard(self):
        pairs, t = self.inputs()
        bounds = [30000 * min(len(y), len(x)) - 30000 + 11 + (len(y) + len(x) - 2) for y, x in pairs]
        assert [b >= 1 << 26 for b in bounds] == [False, True, False], bounds
        assert max(bounds) + 11 < 1 << 29 and 30000 + 12 <= 32767

    def run(self, e):
        pairs, t = self.inputs()
        s = _dev(t)
        dev = [(_dev(y), _dev(x)) for y, x in pairs]
        res = e.align_batch_dev([(y.data_ptr(), y.numel(), x.data_ptr(), x.numel()) for y, x in dev], s.data_ptr(), SUBSTSZ,
                                *self.mode)
        info = e.last_align_batch_info()
        assert (info["batch_pairs"], info["alone_pairs"], info["host_pairs"]) == (2, 1, 0), info
        assert [r["status"] for r in res] == [0, 1, 0], res
        for k, ((y, x), r) in enumerate(zip(pairs, res)):
            w = _once(("alone", k), lambda: _checked_align(y, x, t, *self.mode))
            assert (_t6(r) == w) if k != 1 else (_t3(r) == (w[0], w[3], w[4]) and r["cigar"] == ""), (k, r)


DIRTY = [Rejected(), Int16Flag(), Status1Hit(), ChunkedPair(), RoundsBatch(), ShortCigar(), AlonePair()]
