"""The alignments of a batch of long pairs in one call (gsa_align_batch_dev: the batched K-rows score
launch, then rounds of one fill launch over the strips of many pairs and one launch of the pairs'
walks, nw_pair_trace_batch.hip) against tests/_align_oracle.py, exactly: score, start
cell, end cell and CIGAR, and pair by pair against align_pair_dev.  Every case asserts the statuses
and, from gsa_align_batch_info, the strip height, the pairs per route, the strips filled and the
rounds, so that no case passes through another route.  A strip is 1024 rows in every mode (512 with
GSA_SCORE_K=2); a lane holds 16 (8) of them."""
import ctypes

import numpy as np
import pytest

import gpuseqalign_amd as gsa
from tests import _align_oracle as ao
from tests.test_gpu_align_pair import _embed, _gap_run, _hdr, _plan, _plant, _related, _seq
from tests.test_gpu_score import MODES

pytestmark = pytest.mark.gpu

ALL_MODES = MODES + [(0, 0, False), (-7, 0, False)]
FIELDS = ("score", "i_start", "j_start", "i_end", "j_end", "cigar")
TR = 1024
DEFAULT_LIMIT = 8 << 30
_REF = {}
_ALONE = {}
_BATCH = {}


def _t(r):
    return tuple(r[f] for f in FIELDS)


class _Batch:
    """Pairs (host arrays with the header element) and a table, on the device."""

    def __init__(self, key, pairs, sub):
        import torch
        dev = torch.device("cuda:0")
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)
        self.key = key
        self.pairs = [(np.asarray(y, np.int32), np.asarray(x, np.int32)) for y, x in pairs]
        self.substsz = int(round(np.sqrt(np.asarray(sub).size)))
        self.subm = np.asarray(sub).reshape(self.substsz, self.substsz)
        self.sub = up(self.subm.ravel())
        self.dev = [(up(y), up(x)) for y, x in self.pairs]
        torch.cuda.synchronize(dev)
        self.ptrs = [(y.data_ptr(), y.numel(), x.data_ptr(), x.numel()) for y, x in self.dev]

    def run(self, engine, go, ge, local, mwg=0, limit=0):
        r = engine.align_batch_dev(self.ptrs, self.sub.data_ptr(), self.substsz, go, ge, local, mwg, limit)
        return r, engine.last_align_batch_info()

    def want(self, k, go, ge, local):
        """The oracle's alignment of pair k and its path, computed once per mode."""
        key = (self.key, k, go, ge, local)
        if key not in _REF:
            y, x = self.pairs[k]
            if len(y) == 1 or len(x) == 1:
                _REF[key] = (ao.align(y, x, self.subm, go, ge, local), [])
            else:
                res = ao.align(y, x, self.subm, go, ge, local, want_path=True)
                _REF[key] = (res[:6], [(i, j) for i, j, _ in res[6]])
        return _REF[key]

    def alone(self, engine, k, go, ge, local):
        """align_pair_dev for pair k alone, once per mode."""
        key = (self.key, k, go, ge, local)
        if key not in _ALONE:
            yp, ar, xp, ac = self.ptrs[k]
            _ALONE[key] = engine.align_pair_dev(yp, ar, xp, ac, self.sub.data_ptr(), self.substsz, go, ge, local)
        return _ALONE[key]

    def empty(self, k):
        return len(self.pairs[k][0]) == 1 or len(self.pairs[k][1]) == 1


def _plan_batch(b, idx, go, ge, local, limit, tr=TR, log=None):
    """(rounds, strips filled, peak code bytes) of the batch plan over the pairs `idx`, restated along
    the oracle's paths: per round the active pairs by remaining code bytes descending (ties by index),
    each its lowest unfilled strip and as many above as still fit the round, for the columns up to
    where its path first reaches the boundary below; a path on column 0 needs no more codes.  `log`
    (a list) gets, per round, (the pairs that got a chunk, the active pairs that waited)."""
    st = {}
    for k in idx:
        want, path = b.want(k, go, ge, local)
        st[k] = [-(-want[3] // tr) - 1, want[4], path]
    rounds = filled = peak = 0
    while st:
        order = sorted(st, key=lambda k: (-(st[k][0] + 1) * st[k][1] * (tr // 2), k))
        used, got = 0, 0
        if log is not None:
            log.append(([], []))
        for k in order:
            hi, J, path = st[k]
            sb = J * (tr // 2)
            if sb > limit - used:
                if log is not None:
                    log[-1][1].append(k)
                continue
            n = min((limit - used) // sb, hi + 1)
            if log is not None:
                log[-1][0].append(k)
            used, got, filled = used + n * sb, got + 1, filled + n
            lo = hi + 1 - n
            at = [j for i, j in path if i == lo * tr]
            if lo == 0 or not at or at[0] == 0:
                del st[k]
            else:
                st[k][0], st[k][1] = lo - 1, at[0]
        assert got >= 1
        rounds, peak = rounds + 1, max(peak, used)
    return rounds, filled, peak


def _check(engine, b, go, ge, local, mwg=0, limit=0, tr=TR, single=True):
    """One call against the oracle (and align_pair_dev): all six fields and status 0 for every pair,
    and what the info says ran."""
    res, info = b.run(engine, go, ge, local, mwg, limit)
    print(b.key, (go, ge, local), mwg, limit, info)  # (shown with pytest -s)
    assert len(res) == len(b.pairs)
    traced = []
    for k, r in enumerate(res):
        want, _ = b.want(k, go, ge, local)
        assert r["status"] == 0, (b.key, k, r, info)
        assert _t(r) == want, (b.key, k, len(b.pairs[k][0]) - 1, len(b.pairs[k][1]) - 1, _t(r)[:5], want[:5])
        if single:
            one = b.alone(engine, k, go, ge, local)
            assert one["status"] == 0 and _t(r) == _t(one), (b.key, k)
        if not b.empty(k) and not (local and want[0] == 0):
            traced.append(k)
    host = len(b.pairs) - len(traced)
    assert info["strip_rows"] == tr, info
    assert (info["batch_pairs"], info["host_pairs"], info["alone_pairs"]) == (len(traced), host, 0), info
    assert info["strips"] == sum(-(-b.want(k, go, ge, local)[0][3] // tr) for k in traced), info
    rounds, filled, peak = _plan_batch(b, traced, go, ge, local, limit if limit else DEFAULT_LIMIT, tr)
    assert (info["rounds"], info["strips_filled"], info["code_bytes"]) == (rounds, filled, peak), (info, rounds, filled, peak)
    return res, info


def _first_letters_equal(y, x):
    """Y and X with X's first letter set to Y's: a positive cell (1, 1), so that no local score is 0."""
    x = x.copy()
    x[1] = y[1]
    return y, x


# -- 1. edges in one batch --------------------------------------------------------------------------

EDGE_SHAPES = [(1, 1), (1, 300), (15, 63), (16, 64), (17, 65), (1023, 1), (1023, 300), (1024, 63), (1024, 64),
               (1024, 300), (1025, 65), (1025, 300), (2048, 64), (2048, 300), (2049, 63), (2049, 300), (3073, 1),
               (3073, 65), (3073, 300), (17, 300), (16, 1), (15, 300)]


def _edge_batch(golden):
    if "edge" not in _BATCH:
        pairs = []
        for n, (R, C) in enumerate(EDGE_SHAPES):
            y, x = (_seq(R, 7 * R + C), _seq(C, 7 * R + C + 1)) if n % 2 else _related(R, C, 3 * R + C)
            pairs.append(_first_letters_equal(y, x))
        pairs.insert(3, (_hdr([]), _seq(40, 5)))     # an empty seqY
        pairs.insert(9, (_seq(1030, 6), _hdr([])))   # an empty seqX
        pairs.append(pairs[12])                      # one pair given twice
        _BATCH["edge"] = _Batch("edge", pairs, golden.blosum62)
    return _BATCH["edge"]


@pytest.mark.parametrize("mwg", [0, 1, 2])
@pytest.mark.parametrize("go,ge,local", ALL_MODES)
def test_edges_in_one_batch(engine, golden, go, ge, local, mwg):
    """The last row on either side of a hand-off between two lanes (16 / 17) and of the strip boundaries
    1024 / 1025 and 2048 / 2049, three strips and a row more, columns on either side of the wave's 64
    lanes; random and related pairs, two pairs with an empty side and one pair twice, in one call.
    With max_workgroups = 1 one workgroup runs every strip of every pair in turn."""
    b = _edge_batch(golden)
    res, info = _check(engine, b, go, ge, local, mwg, single=(mwg == 0))
    assert info["host_pairs"] == 2 and info["batch_pairs"] == len(b.pairs) - 2 and info["alone_pairs"] == 0, info
    assert info["rounds"] == 1 and info["strips_filled"] == info["strips"], info
    assert _t(res[12]) == _t(res[-1])


# -- 2. one pair --------------------------------------------------------------------------------------


@pytest.mark.parametrize("go,ge,local", MODES)
def test_one_pair_is_the_single_pair_plan(engine, golden, go, ge, local):
    """npairs = 1 (the score kernel's one-pair form): the result, and rounds, strips filled and peak
    bytes equal to the single-pair plan (tests/test_gpu_align_pair._plan) at TR = 1024."""
    if "one" not in _BATCH:
        _BATCH["one"] = _Batch("one", [_related(2 * TR + 60, 2 * TR + 40, 23)], golden.blosum62)
    b = _BATCH["one"]
    want, path = b.want(0, go, ge, local)
    strip = want[4] * TR // 2
    for limit in (0, strip, 2 * strip + 1):
        res, info = _check(engine, b, go, ge, local, limit=limit)
        chunks, filled, peak = _plan(path, TR, want[3], want[4], limit if limit else DEFAULT_LIMIT)
        assert (info["rounds"], info["strips_filled"], info["code_bytes"]) == (chunks, filled, peak), info
    assert local or info["strips"] == 3


# -- 3. planted gaps across strip boundaries --------------------------------------------------------


@pytest.mark.parametrize("go,ge,local", MODES)
def test_planted_gaps_and_local_over_three_strips(engine, golden, go, ge, local):
    """Vertical gaps of 1 and 30 rows across the rows 1024 / 1025 and 2048 / 2049 -- in the affine modes
    the walk in state F over a checkpoint row, in the local ones the F' floor at 1024-row strips -- and
    a local alignment from strip 0 to strip 2.  Each gap is found as one run in the oracle's CIGAR
    first."""
    if "plant" not in _BATCH:
        pairs, where = [], []
        for bnd in (TR, 2 * TR):
            for n in (1, 30):
                a = bnd + 1 - (n + 1) // 2  # rows a ... a + n - 1 lie across the boundary bnd / bnd + 1
                pairs.append(_plant(2 * TR + 300, a, n, 31 * bnd + n, False))
                where.append((a, n, bnd))
        pairs.append(_embed(2500, 200, 2300, 2400, 150, 5))
        _BATCH["plant"] = (_Batch("plant", pairs, golden.blosum62), where)
    b, where = _BATCH["plant"]
    for k, (a, n, bnd) in enumerate(where):
        want, _ = b.want(k, go, ge, local)
        count, row, _ = _gap_run(want[5], want[1], want[2], "I")
        assert count == n and row == a and a <= bnd + 1 <= a + n, (count, row, a, n, bnd)
    res, info = _check(engine, b, go, ge, local)
    if local:
        r = res[len(where)]
        assert r["i_start"] < TR and r["i_end"] > 2 * TR, r


# -- 4. rounds ----------------------------------------------------------------------------------------


def _rounds_batch(golden):
    if "rounds" not in _BATCH:
        x = _seq(700, 61)
        # rows of junk in front of a copy of X: the global path runs up column 0 from row 2200, in the
        # pair's strip 2 of three
        col0 = (_hdr(np.concatenate([(_seq(2200, 62)[1:] + 7) % 20, x[1:]])), x)
        # the last pair is related over all its rows: its local alignments span three strips too
        pairs = [_related(3 * TR + 100, 900, 17), _related(2 * TR + 5, 1000, 19), _related(TR + 9, 400, 29), col0,
                 _related(300, 1000, 37), _related(2 * TR + 200, 2 * TR + 100, 71)]
        _BATCH["rounds"] = _Batch("rounds", pairs, golden.blosum62)
    return _BATCH["rounds"]


@pytest.mark.parametrize("go,ge,local", MODES)
def test_rounds(engine, golden, go, ge, local):
    """A limit of twice the largest strip: at least three rounds, a pair split over rounds while another
    waits, and (global) a pair that finishes on column 0 below its strip 0.  The results are the
    default limit's; rounds, strips filled and peak bytes are those of the plan restated along the
    oracle's paths (_check).  At exactly the largest strip every pair is traced; a byte below, exactly
    the pairs whose strip exceeds the limit get status 1, with the oracle's score and end cell."""
    b = _rounds_batch(golden)
    base, info0 = _check(engine, b, go, ge, local)
    assert info0["rounds"] == 1 and info0["strips_filled"] == info0["strips"]
    sb = [b.want(k, go, ge, local)[0][4] * TR // 2 for k in range(len(b.pairs))]
    big = max(sb)
    res, info = _check(engine, b, go, ge, local, limit=2 * big, single=False)
    assert [_t(r) for r in res] == [_t(r) for r in base]
    assert info["rounds"] >= 3 and info["code_bytes"] <= 2 * big, info
    # in the plan just asserted, some pair has chunks in two rounds, in the later of which another pair waits
    log = []
    _plan_batch(b, list(range(len(b.pairs))), go, ge, local, 2 * big, log=log)
    assert any(k in log[m][0] and log[n][1] for k in range(len(b.pairs)) for m in range(len(log))
               for n in range(m + 1, len(log)) if k in log[n][0]), log
    if not local:
        want, path = b.want(3, go, ge, local)
        assert (2 * TR, 0) in path  # on column 0 at the boundary above its strip 2
        # its turn comes with room for one strip only: the strips above are never filled
        assert info["strips_filled"] < info["strips"], info
    res, info = _check(engine, b, go, ge, local, limit=big, single=False)
    assert [_t(r) for r in res] == [_t(r) for r in base] and info["code_bytes"] <= big
    res, info = b.run(engine, go, ge, local, limit=big - 1)
    over = [k for k in range(len(b.pairs)) if sb[k] > big - 1]
    assert over and len(over) < len(b.pairs)
    for k, r in enumerate(res):
        want = b.want(k, go, ge, local)[0]
        if k in over:
            assert r["status"] == 1 and r["cigar"] == "" and (r["i_start"], r["j_start"]) == (0, 0), (k, r)
            assert (r["score"], r["i_end"], r["j_end"]) == (want[0], want[3], want[4]), (k, r)
        else:
            assert r["status"] == 0 and _t(r) == want, (k, r)
    assert info["batch_pairs"] == len(b.pairs) - len(over) and info["alone_pairs"] == 0, info


# -- 5. other routes ----------------------------------------------------------------------------------


@pytest.mark.parametrize("go,ge,local", MODES)
def test_other_routes(engine, golden, knobs, go, ge, local):
    sub = np.asarray(golden.blosum62).reshape(25, 25).astype(np.int64)
    small = [_related(700, 650, 41), _related(1030, 300, 47)]
    # the value bound B reaches 2^26 for one pair (the 4 v + tag form's own limit): it goes alone and gets
    # status 1 with an exact score; its neighbours are traced
    big = sub.copy()
    big[np.diag_indices_from(big)] = 30000
    assert 30000 * 2300 >= 1 << 26 > 30000 * 650 + 11 + 2 * (1030 + 700)
    b = _Batch(("route", "big"), [small[0], _related(2400, 2300, 43), small[1]], big)
    res, info = b.run(engine, go, ge, local)
    assert [r["status"] for r in res] == [0, 1, 0], res
    assert (info["batch_pairs"], info["alone_pairs"], info["host_pairs"], info["strip_rows"]) == (2, 1, 0, TR), info
    for k in (0, 2):
        assert _t(res[k]) == b.want(k, go, ge, local)[0]
    want = ao.align(*b.pairs[1], b.subm, go, ge, local)
    assert res[1]["cigar"] == "" and (res[1]["score"], res[1]["i_end"], res[1]["j_end"]) == (want[0], want[3], want[4])
    # a table outside int16 (after the shift): every pair alone, as align_pair_dev answers it
    wide = sub.copy()
    wide[np.diag_indices_from(wide)] = 40000
    b = _Batch(("route", "wide"), small, wide)
    res, info = b.run(engine, go, ge, local)
    assert (info["batch_pairs"], info["alone_pairs"], info["strip_rows"]) == (0, 2, 0), info
    for k, r in enumerate(res):
        one = b.alone(engine, k, go, ge, local)
        assert (r["status"], _t(r)) == (one["status"], _t(one)) and r["status"] == 1
    # 2 rows per lane by knob: strips of 512 rows, the same alignments
    b = _Batch(("route", "k2"), small + [_related(1500, 400, 53)], sub)
    base, _ = _check(engine, b, go, ge, local)
    knobs("GSA_SCORE_K", 2)
    res, info = _check(engine, b, go, ge, local, tr=512, single=False)
    assert info["strip_rows"] == 512 and [_t(r) for r in res] == [_t(r) for r in base]


# -- 6. the raw ABI -----------------------------------------------------------------------------------


def _raw(engine, b, go=-11, ge=-1, local=False, mwg=0, limit=0, cap=1 << 16, npairs=None, null_out=False,
         null_cigar=False, null_pairs=False, null_subst=False, patch=None):
    n = len(b.ptrs) if npairs is None else npairs
    arr = (gsa.PairDev * max(len(b.ptrs), 1))()
    for k, (yp, ar, xp, ac) in enumerate(b.ptrs):
        arr[k].seqY, arr[k].adjrows, arr[k].seqX, arr[k].adjcols = yp, ar, xp, ac
    if patch:
        patch(arr)
    res, info = (gsa.AlignDbResult * max(len(b.ptrs), 1))(), gsa.AlignBatchInfo()
    need, ms = ctypes.c_int64(-1), ctypes.c_float(0)
    buf = ctypes.create_string_buffer(max(cap, 1))
    st = gsa.lib().gsa_align_batch_dev(engine._h, n, None if null_pairs else arr, None if null_subst else b.sub.data_ptr(),
                                       b.substsz, go, ge, int(local), mwg, limit, None if null_out else res,
                                       None if null_cigar else buf, cap, ctypes.byref(need), ctypes.byref(info),
                                       ctypes.byref(ms), None)
    return st, res, need.value, buf


@pytest.fixture(scope="module")
def few(engine, golden):
    return _Batch("few", [_related(700, 650, 91), _related(1100, 200, 93), (_seq(30, 3), _hdr([])),
                          _related(90, 1500, 95)], golden.blosum62)


def test_short_cigar_buffer(engine, few):
    cigs = [few.want(k, -11, -1, False)[0][5] for k in range(len(few.pairs))]
    total = sum(len(c) + 1 for c in cigs)
    offs = np.cumsum([0] + [len(c) + 1 for c in cigs])
    st, res, need, buf = _raw(engine, few, cap=total)
    assert st == 0 and need == total
    for k, c in enumerate(cigs):
        assert (res[k].status, res[k].cigar_off, res[k].cigar_len) == (0, offs[k], len(c))
        assert buf.raw[offs[k]:offs[k] + len(c) + 1] == c.encode() + b"\0"
    # room for the first two strings and all of the third but its NUL: the fourth does not fit either
    cap = int(offs[2]) + len(cigs[2])
    st, res, need, buf = _raw(engine, few, cap=cap)
    assert st == 0 and need == total
    assert [res[k].status for k in range(4)] == [0, 0, 2, 2]
    for k in (0, 1):
        assert (res[k].cigar_off, res[k].cigar_len) == (offs[k], len(cigs[k]))
    for k in range(4):
        want = few.want(k, -11, -1, False)[0]
        assert (res[k].score, res[k].i_start, res[k].j_start, res[k].i_end, res[k].j_end) == want[:5]
    st, res, need, _ = _raw(engine, few, cap=0, null_cigar=True)
    assert st == 0 and need == total and [res[k].status for k in range(4)] == [2, 2, 2, 2]


def test_invalid_input(engine, few):
    def good():
        st, res, _, _ = _raw(engine, few)
        assert st == 0 and [res[k].status for k in range(4)] == [0, 0, 0, 0]

    def bad(**kw):
        st = _raw(engine, few, **kw)[0]
        assert st == gsa.NwStat.errorInvalidValue, kw
        good()

    def set_field(k, name, value):
        return lambda arr: setattr(arr[k], name, value)

    good()
    bad(go=-1, ge=-11)                         # go > ge
    bad(ge=1)                                  # ge > 0
    bad(go=-2000010, ge=-2000000)              # outside gsa_score_batch_dev's value range
    bad(npairs=0)
    bad(npairs=-1)
    bad(null_pairs=True)
    bad(null_subst=True)
    bad(patch=set_field(1, "adjrows", 0))
    bad(patch=set_field(2, "adjcols", 0))
    bad(patch=set_field(1, "seqY", None))
    bad(patch=set_field(3, "seqX", None))
    bad(limit=-1)
    bad(cap=-1)
    bad(mwg=-1)
    bad(null_out=True)
    bad(null_cigar=True, cap=16)
    st = gsa.lib().gsa_align_batch_dev(engine._h, 1, (gsa.PairDev * 1)(), few.sub.data_ptr(), 33, -11, -1, 0, 0, 0,
                                       (gsa.AlignDbResult * 1)(), None, 0, None, None, None, None)
    assert st == gsa.NwStat.errorInvalidValue


@pytest.mark.parametrize("go,ge,local", [(-11, -1, False), (-11, -11, False), (-11, -1, True)])
def test_other_calls_before_and_after(engine, few, go, ge, local):
    """align_pair_dev and score_batch_dev give the same before and after a batch call, and
    gsa_last_launch's record is left as it was."""
    def others():
        yp, ar, xp, ac = few.ptrs[1]
        one = engine.align_pair_dev(yp, ar, xp, ac, few.sub.data_ptr(), few.substsz, go, ge, local)
        sc = engine.score_batch_dev(few.ptrs, few.sub.data_ptr(), few.substsz, go, ge, local)
        return _t(one), [(r["score"], r["i_end"], r["j_end"]) for r in sc]

    before = others()
    record = engine.last_launch()
    res, _ = _check(engine, few, go, ge, local)
    assert engine.last_launch() == record
    assert others() == before
    assert _t(res[1]) == before[0]
    assert [(r["score"], r["i_end"], r["j_end"]) for r in res] == before[1]


def test_scratch_is_counted_in_mem_stats(engine, few):
    engine.reset_mem_stats()
    _, info = few.run(engine, -11, -1, False)
    moves = sum(len(y) - 1 + len(x) - 1 for k, (y, x) in enumerate(few.pairs) if not few.empty(k))
    # the codes, the move bytes, and the two new slots (tables and records, 4 KiB at the least each)
    assert engine.mem_stats()["glmem_peak_allocs"] >= info["code_bytes"] + moves + 2 * 4096 > 2 * 4096


def test_host_form(engine, golden, few):
    for go, ge, local in [(-11, -1, False), (-5, -2, True)]:
        res = engine.align_batch(few.pairs, golden.blosum62, go, ge, local)
        assert [r["status"] for r in res] == [0] * 4
        assert [_t(r) for r in res] == [few.want(k, go, ge, local)[0] for k in range(4)]
    res = engine.align_batch(few.pairs[:2], golden.blosum62, -11)
    assert [_t(r) for r in res] == [few.want(k, -11, -11, False)[0] for k in range(2)]
    assert engine.last_align_batch_info()["batch_pairs"] == 2
