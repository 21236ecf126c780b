"""The alignment of one long pair (gsa_align_pair_dev: the K-rows score kernel in one direction, then
the strip fill with 4-bit move codes seeded from its checkpoint rows and the walk over them,
nw_pair_trace.hip) against tests/_align_oracle.py, exactly: score, start cell, end cell
and CIGAR.  Every case asserts the status and, from gsa_align_pair_info, the strip height, the strips
filled and the chunks, so that no case passes through another route.  A strip is TR rows: 1024 for NW
with linear gaps, 512 in the other modes; a lane holds TR / 64 rows."""
import ctypes

import numpy as np
import pytest

import gpuseqalign_amd as gsa
from gpuseqalign_amd import formats as F
from tests import _align_oracle as ao
from tests.test_gpu_score import MODES

pytestmark = pytest.mark.gpu

# the issue's modes, and zero gap costs in the global modes
ALL_MODES = MODES + [(0, 0, False), (-7, 0, False)]
FIELDS = ("score", "i_start", "j_start", "i_end", "j_end", "cigar")
_REF = {}


def _tr(go, ge, local):
    return 1024 if (not local and go == ge) else 512


def _seq(n, seed, alphabet=20):
    return F.synthetic_seq(n, seed, alphabet)


def _hdr(a):
    return np.concatenate([[0], np.asarray(a)]).astype(np.int32)


def _related(R, C, seed):
    """Y of R letters, a mutated copy of X (C letters), cut or padded with random letters."""
    n = max(R, C)
    base = _seq(n, seed)
    mut = F.mutate_seq(base, seed + 1)[1:]
    mut = np.concatenate([mut, _seq(n, seed + 2)[1:]])[:R]
    return _hdr(mut), _hdr(base[1:C + 1])


class _Pair:
    """A pair and the table on the device."""

    def __init__(self, Y, X, sub):
        import torch
        dev = torch.device("cuda:0")
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)
        self.Y, self.X = np.asarray(Y, np.int32), np.asarray(X, np.int32)
        self.substsz = int(round(np.sqrt(np.asarray(sub).size)))
        self.subm = np.asarray(sub).reshape(self.substsz, self.substsz)
        self.y, self.x, self.sub = up(self.Y), up(self.X), up(self.subm.ravel())
        torch.cuda.synchronize(dev)

    def run(self, engine, go, ge, local, limit=0):
        r = engine.align_pair_dev(self.y.data_ptr(), self.y.numel(), self.x.data_ptr(), self.x.numel(),
                                  self.sub.data_ptr(), self.substsz, go, ge, local, scratch_limit=limit)
        return r, engine.last_align_pair_info()

    def score(self, engine, go, ge, local, swap=False):
        a, b = (self.x, self.y) if swap else (self.y, self.x)
        r = engine.score_dev(a.data_ptr(), a.numel(), b.data_ptr(), b.numel(), self.sub.data_ptr(), self.substsz, go,
                             ge, local)
        return r["score"], r["i_end"], r["j_end"]


def _want(key, p, go, ge, local):
    """The oracle's alignment and its path, computed once per (pair, mode) and shared by the cases."""
    k = (key, go, ge, local)
    if k not in _REF:
        res = ao.align(p.Y, p.X, p.subm, go, ge, local, want_path=True)
        _REF[k] = (res[:6], [(i, j) for i, j, _ in res[6]])
    return _REF[k]


def _t(r):
    return tuple(r[f] for f in FIELDS)


def _plan(path, tr, i_end, j_end, limit):
    """(chunks, strips filled, peak code bytes) of the bottom-up plan along the oracle's path: a chunk
    takes the strips that fit from the lowest one not yet filled, for the columns up to the cell where
    the path first reaches the chunk below's upper boundary; a path on column 0 needs no more codes."""
    strips = -(-i_end // tr)
    hi, J, chunks, filled, peak = strips - 1, j_end, 0, 0, 0
    while True:
        sb = J * tr // 2
        n = min(limit // sb, hi + 1)
        assert n >= 1
        chunks, filled, peak = chunks + 1, filled + n, max(peak, n * sb)
        lo = hi + 1 - n
        at = [j for i, j in path if i == lo * tr]
        if lo == 0 or not at or at[0] == 0:
            return chunks, filled, peak
        hi, J = lo - 1, at[0]


def _check(engine, p, key, go, ge, local, limit=0):
    """One call against the oracle: all six fields, status 0, and what the info says ran."""
    want, path = _want(key, p, go, ge, local)
    r, info = p.run(engine, go, ge, local, limit)
    tr = _tr(go, ge, local)
    print(key, (go, ge, local), limit, r["status"], _t(r)[:5], r["cigar"][:32], info)  # (shown with pytest -s)
    assert r["status"] == 0, (key, r, info)
    assert _t(r) == want, (key, len(p.Y) - 1, len(p.X) - 1, _t(r), want)
    assert info["strip_rows"] == tr, info
    if want[0] == 0 and local:
        assert (info["strips"], info["strips_filled"], info["chunks"]) == (0, 0, 0), info
        return r, info
    i_end, j_end = want[3], want[4]
    chunks, filled, peak = _plan(path, tr, i_end, j_end, limit if limit else 2 << 30)
    assert info["strips"] == -(-i_end // tr), info
    assert (info["chunks"], info["strips_filled"], info["code_bytes"]) == (chunks, filled, peak), (info, chunks, filled)
    if not limit:
        assert info["chunks"] == 1 and info["strips_filled"] == info["strips"], info
    return r, info


# -- 1. strip and lane edges ------------------------------------------------------------------------

_EDGE = {}
COLS = [1, 63, 64, 65, 300]


def _rows(tr):
    return [1, 7, 8, 9, 15, 16, 17, tr - 1, tr, tr + 1, 2 * tr, 2 * tr + 1, 3 * tr + 1]


@pytest.mark.parametrize("kind", ["random", "related"])
@pytest.mark.parametrize("go,ge,local", ALL_MODES)
def test_strip_and_lane_edges(engine, golden, go, ge, local, kind):
    """The last row on the first and last register row of a lane, on either side of a hand-off between
    two lanes and of a boundary between two strips; columns on either side of the wave's 64 lanes."""
    tr = _tr(go, ge, local)
    for R in _rows(tr):
        for C in COLS:
            k = (kind, R, C)
            if k not in _EDGE:
                Y, X = (_seq(R, 7 * R + C), _seq(C, 7 * R + C + 1)) if kind == "random" else _related(R, C, 3 * R + C)
                _EDGE[k] = _Pair(Y, X, golden.blosum62)
            _check(engine, _EDGE[k], ("edge",) + k, go, ge, local)


# -- 2. planted gaps --------------------------------------------------------------------------------

_PLANT = {}


def _plant(R, a, n, seed, inserted):
    """Y of R letters, and X: Y with the rows a ... a + n - 1 removed (a vertical gap there), or with n
    letters inserted behind row a - 1 (a horizontal gap on row a - 1).  The gap's letters are a letter
    the rest of the pair does not use, so that the gap cannot slide or split along equal letters."""
    y = _seq(R, seed, 19)
    if not inserted:
        y = y.copy()
        y[a:a + n] = 19
        return y, _hdr(np.concatenate([y[1:a], y[a + n:]]))
    return y, _hdr(np.concatenate([y[1:a], np.full(n, 19), y[a:]]))


def _gap_run(cigar, i0, j0, op):
    """(count, first row, first column) of the only run of `op` in a CIGAR; it must be the only gap."""
    i, j, found = i0, j0, []
    for count, o in ao.runs(cigar):
        if o == op:
            found.append((count, i + 1, j + 1))
        else:
            assert o in "=X", "another gap in %s" % cigar
        i += count if o != "D" else 0
        j += count if o != "I" else 0
    assert len(found) == 1, cigar
    return found[0]


@pytest.mark.parametrize("inserted", [False, True], ids=["removed", "inserted"])
@pytest.mark.parametrize("go,ge,local", MODES)
def test_planted_gaps(engine, golden, go, ge, local, inserted):
    """A 1-letter and a 30-letter gap across a hand-off between two lanes (rows 8/9 at 512, 16/17 at
    1024; local modes: the same hand-off 40 lanes further down, where the alignment reaches it) and
    across the strip boundaries TR / TR + 1 and 2 TR / 2 TR + 1.  The vertical 30-letter gap across a
    strip boundary in the affine modes is the walk in state F over a checkpoint row."""
    tr = _tr(go, ge, local)
    kr = tr // 64
    R = 2 * tr + 300
    for b in ([kr] if not local else []) + [41 * kr, tr, 2 * tr]:
        for n in (1, 30):
            a = max(b + 1 - (n + 1) // 2, 1)  # rows a ... a + n - 1 lie across the boundary b / b + 1
            k = (tr, b, n, inserted)
            if k not in _PLANT:
                _PLANT[k] = _Pair(*_plant(R, a, n, 31 * b + n, inserted), golden.blosum62)
            p = _PLANT[k]
            want, _ = _want(("plant",) + k, p, go, ge, local)
            count, row, col = _gap_run(want[5], want[1], want[2], "D" if inserted else "I")
            assert count == n and row == a, (count, row, a, n, b)
            assert a <= b + 1 <= a + n  # the gap's rows (inserted: the row it lies on) meet the boundary
            _check(engine, p, ("plant",) + k, go, ge, local)


# -- 3. local -----------------------------------------------------------------------------------------

LOCAL = [m for m in MODES if m[2]]
_LOC = {}


def _embed(R, a, b, C, at, seed):
    """Y of R random letters; X of C random letters with Y's rows a ... b copied in at column `at`."""
    y, x = _seq(R, seed), _seq(C, seed + 1, 19)
    x = x.copy()
    x[1:] = (x[1:] + 1) % 20  # (another stream than y's)
    x[at:at + b - a + 1] = y[a:b + 1]
    return y, x


@pytest.mark.parametrize("go,ge,local", LOCAL)
def test_local_over_three_strips(engine, golden, go, ge, local):
    """An alignment that starts in strip 0 and ends in strip 2."""
    if "three" not in _LOC:
        _LOC["three"] = _Pair(*_embed(1500, 200, 1200, 1300, 150, 5), golden.blosum62)
    r, info = _check(engine, _LOC["three"], "three", go, ge, local)
    assert r["i_start"] < 512 and r["i_end"] > 1024 and info["strips"] == 3


@pytest.mark.parametrize("go,ge,local", LOCAL)
def test_local_wholly_in_the_last_of_four_strips(engine, golden, go, ge, local):
    """With room for one strip's codes only the strips above the alignment are never filled."""
    if "last" not in _LOC:
        _LOC["last"] = _Pair(*_embed(2000, 1650, 1950, 500, 100, 9), golden.blosum62)
    p = _LOC["last"]
    want, _ = _want("last", p, go, ge, local)
    assert want[1] >= 3 * 512 and want[3] > want[1]
    r, info = _check(engine, p, "last", go, ge, local, limit=want[4] * 512 // 2)
    assert (info["strips"], info["chunks"], info["strips_filled"]) == (4, 1, 1), info


@pytest.mark.parametrize("go,ge,local", LOCAL)
def test_local_two_maximal_cells(engine, golden, go, ge, local):
    """The same motif twice down the rows, and twice along the columns: the first cell in row-major order."""
    if "twice" not in _LOC:
        m, junk = _seq(40, 3)[1:], _seq(530, 21)[1:]
        rows, cols = _hdr(np.concatenate([m, junk, m])), _hdr(m)
        _LOC["twice"] = (_Pair(rows, cols, golden.blosum62), _Pair(cols, rows, golden.blosum62))
    for n, p in enumerate(_LOC["twice"]):
        want, _ = _want(("twice", n), p, go, ge, local)
        H = ao.matrices(p.Y, p.X, p.subm, go, ge, local)[0]
        assert int((H == H.max()).sum()) >= 2
        _check(engine, p, ("twice", n), go, ge, local)


@pytest.mark.parametrize("go,ge,local", LOCAL)
def test_local_score_zero_and_homopolymers(engine, golden, go, ge, local):
    sub = np.asarray(golden.blosum62).reshape(25, 25)
    a, b = [(int(i), int(j)) for i, j in zip(*np.nonzero(sub[:20, :20] < 0))][0]
    if "zero" not in _LOC:
        _LOC["zero"] = _Pair(_hdr([a] * 700), _hdr([b] * 90), sub)
        _LOC["homo"] = _Pair(_hdr([a] * 700), _hdr([a] * 650), sub)
    r, _ = _check(engine, _LOC["zero"], "zero", go, ge, local)
    assert _t(r) == (0, 0, 0, 0, 0, "")
    r, _ = _check(engine, _LOC["homo"], "homo", go, ge, local)
    assert r["cigar"] == "650="


# -- 4. chunks ----------------------------------------------------------------------------------------

_CH = {}


@pytest.mark.parametrize("go,ge,local", MODES)
def test_chunks(engine, golden, go, ge, local):
    """A limit of exactly one strip's codes (a chunk per strip: at least three), of two strips' and a
    byte more, and a byte less than one strip's: the same alignment whatever the chunks (which are
    those of the plan along the oracle's path, _check), then status 1."""
    tr = _tr(go, ge, local)
    if tr not in _CH:
        _CH[tr] = _Pair(*_related(3 * tr + 100, 3 * tr, 17), golden.blosum62)
    p = _CH[tr]
    one, _ = _check(engine, p, ("chunks", tr), go, ge, local)
    strip = one["j_end"] * tr // 2
    r, info = _check(engine, p, ("chunks", tr), go, ge, local, limit=strip)
    assert _t(r) == _t(one) and info["chunks"] >= 3 and info["chunks"] == info["strips_filled"], info
    assert info["code_bytes"] == strip
    r, info = _check(engine, p, ("chunks", tr), go, ge, local, limit=2 * strip + 1)
    assert _t(r) == _t(one) and info["chunks"] >= 2 and info["code_bytes"] <= 2 * strip + 1, info
    r, info = p.run(engine, go, ge, local, strip - 1)
    assert r["status"] == 1 and r["cigar"] == "" and (r["i_start"], r["j_start"]) == (0, 0), r
    assert (info["strip_rows"], info["strips_filled"], info["chunks"], info["code_bytes"]) == (tr, 0, 0, 0), info
    assert (r["score"], r["i_end"], r["j_end"]) == p.score(engine, go, ge, local)


# -- 5. routing ---------------------------------------------------------------------------------------


def _status1(engine, p, go, ge, local):
    r, info = p.run(engine, go, ge, local)
    assert r["status"] == 1 and r["cigar"] == "", r
    assert (info["strips_filled"], info["chunks"], info["code_bytes"]) == (0, 0, 0), info
    assert (r["score"], r["i_end"], r["j_end"]) == p.score(engine, go, ge, local)
    return info


@pytest.mark.parametrize("go,ge,local", MODES)
def test_routing(engine, golden, knobs, go, ge, local):
    sub = np.asarray(golden.blosum62).reshape(25, 25).astype(np.int64)
    Y, X = _related(700, 650, 41)
    # a table outside int16 (after the shift): the score comes from the row scan
    wide = sub.copy()
    wide[np.diag_indices_from(wide)] = 40000
    info = _status1(engine, _Pair(Y, X, wide), go, ge, local)
    assert info["strip_rows"] == 0
    # the value bound B reaches 2^26: the 4 v + tag form's own limit
    big = sub.copy()
    big[np.diag_indices_from(big)] = 30000
    Yb, Xb = _related(2400, 2300, 43)
    assert 30000 * 2300 >= 1 << 26
    _status1(engine, _Pair(Yb, Xb, big), go, ge, local)
    # an asymmetric table and one of 4 letters: traced
    rng = np.random.default_rng(5)
    asym = rng.integers(-6, 9, (20, 20))
    assert (asym != asym.T).any()
    _check(engine, _Pair(Y, X, asym), "asym", go, ge, local)
    four = np.where(np.eye(4, dtype=bool), 5, -4)
    _check(engine, _Pair(_hdr(Y[1:] % 4), _hdr(X[1:] % 4), four), "four", go, ge, local)
    # the row scan by knob
    knobs("GSA_SCORE_SCAN", 1)
    info = _status1(engine, _Pair(Y, X, sub), go, ge, local)
    assert info["strip_rows"] == 0


# -- 6. one larger case per mode --------------------------------------------------------------------

_BIG = {}


@pytest.mark.parametrize("go,ge,local", MODES)
def test_related_3000(engine, golden, go, ge, local):
    if "p" not in _BIG:
        _BIG["p"] = _Pair(*_related(3000, 3000, 77), golden.blosum62)
    p = _BIG["p"]
    r, _ = _check(engine, p, "big", go, ge, local)
    assert ao.rescore(r["cigar"], p.Y, p.X, r["i_start"], r["j_start"], p.subm, go, ge) == \
        (r["score"], r["i_end"], r["j_end"])


# -- 7. around the call -------------------------------------------------------------------------------


def _raw(engine, p, go=-11, ge=-1, local=False, limit=0, cap=4096, null_out=False, null_cigar=False, null_y=False):
    res, info = gsa.AlignDbResult(), gsa.AlignPairInfo()
    need, ms = ctypes.c_int64(-1), ctypes.c_float(0)
    buf = ctypes.create_string_buffer(max(cap, 1))
    st = gsa.lib().gsa_align_pair_dev(engine._h, None if null_y else p.y.data_ptr(), p.y.numel(), p.x.data_ptr(),
                                      p.x.numel(), p.sub.data_ptr(), p.substsz, go, ge, int(local), limit,
                                      None if null_out else ctypes.byref(res), None if null_cigar else buf, cap,
                                      ctypes.byref(need), ctypes.byref(info), ctypes.byref(ms), None)
    return st, res, need.value, buf


@pytest.fixture(scope="module")
def small(engine, golden):
    return _Pair(*_related(700, 650, 91), golden.blosum62)


def test_short_cigar_buffer(engine, small):
    want, _ = _want("small", small, -11, -1, False)
    n = len(want[5])
    st, res, need, _ = _raw(engine, small, cap=n)
    assert st == 0 and res.status == 2 and need == n + 1
    assert (res.score, res.i_start, res.j_start, res.i_end, res.j_end) == want[:5]
    st, res, need, buf = _raw(engine, small, cap=n + 1)
    assert st == 0 and res.status == 0 and need == n + 1 and res.cigar_off == 0 and res.cigar_len == n
    assert buf.raw[:n + 1] == want[5].encode() + b"\0"
    st, res, need, _ = _raw(engine, small, cap=0, null_cigar=True)
    assert st == 0 and res.status == 2 and need == n + 1


@pytest.mark.parametrize("go,ge,local", [(-11, -1, False), (-11, -11, False), (-11, -1, True)])
def test_other_calls_before_and_after(engine, golden, small, go, ge, local):
    """score_dev in both directions, align_db_dev and score_db_multi_dev give the same before and
    after; gsa_last_launch's record is left as it was."""
    p = small
    off = np.array([0, p.x.numel()], np.int64)

    def others():
        db = engine.align_db_dev(p.y.data_ptr(), p.y.numel(), p.x.data_ptr(), off, [0], p.sub.data_ptr(), p.substsz,
                                 go, ge, local)
        multi = engine.score_db_multi_dev(p.y.data_ptr(), np.array([0, p.y.numel()], np.int64), p.x.data_ptr(), off,
                                          p.sub.data_ptr(), p.substsz, go, ge, local)
        return (p.score(engine, go, ge, local, swap=True), [_t(r) for r in db], np.asarray(multi["scores"]).tolist(),
                p.score(engine, go, ge, local))

    before = others()
    record = engine.last_launch()
    r, _ = _check(engine, p, "small", go, ge, local)
    assert engine.last_launch() == record
    assert others() == before
    assert (r["score"], r["i_end"], r["j_end"]) == before[3]
    assert _t(r) == tuple(before[1][0])


def test_scratch_is_counted_in_mem_stats(engine, small):
    engine.reset_mem_stats()
    _, info = small.run(engine, -11, -1, False)
    assert engine.mem_stats()["glmem_peak_allocs"] >= info["code_bytes"] > 0


def test_host_form_and_empty_sides(engine, golden, small):
    for go, ge, local in [(-11, -1, False), (-5, -2, True)]:
        r = engine.align_pair(small.Y, small.X, golden.blosum62, go, ge, local)
        assert r["status"] == 0 and _t(r) == _want("small", small, go, ge, local)[0]
    r = engine.align_pair(small.Y, small.X, golden.blosum62, -11)
    assert _t(r) == _want("small", small, -11, -11, False)[0]
    for Y, X in [(small.Y, small.X[:1]), (small.Y[:1], small.X), (small.Y[:1], small.X[:1])]:
        for go, ge, local in [(-11, -1, False), (-11, -1, True)]:
            r = engine.align_pair(Y, X, golden.blosum62, go, ge, local)
            assert r["status"] == 0 and _t(r) == ao.align(Y, X, golden.blosum62, go, ge, local), (len(Y), len(X), r)


def test_invalid_input(engine, small):
    p = small

    def good():
        _check(engine, p, "small", -11, -1, False)

    def bad(call):
        with pytest.raises(gsa.NwError) as ei:
            call()
        assert ei.value.stat == gsa.NwStat.errorInvalidValue
        good()

    def raw(**kw):
        engine._check(_raw(engine, p, **kw)[0], "gsa_align_pair_dev")

    good()
    bad(lambda: p.run(engine, -1, -11, False))            # go > ge
    bad(lambda: p.run(engine, -11, 1, False))             # ge > 0
    bad(lambda: p.run(engine, -2000010, -2000000, False)) # outside gsa_score_dev's value range
    bad(lambda: p.run(engine, -11, -1, False, limit=-1))  # negative scratch_limit
    bad(lambda: raw(cap=-1))
    bad(lambda: raw(null_out=True))
    bad(lambda: raw(null_cigar=True, cap=16))
    bad(lambda: raw(null_y=True))
    bad(lambda: engine.align_pair_dev(p.y.data_ptr(), 0, p.x.data_ptr(), p.x.numel(), p.sub.data_ptr(), p.substsz,
                                      -11, -1))
    bad(lambda: engine.align_pair_dev(p.y.data_ptr(), p.y.numel(), p.x.data_ptr(), p.x.numel(), p.sub.data_ptr(), 33,
                                      -11, -1))
