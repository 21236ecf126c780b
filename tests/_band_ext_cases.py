"""What the GPU tests of the banded extension calls share (tests/test_gpu_score_band_ext.py,
tests/test_gpu_align_pair_band_ext.py and the two batch files): the pairs with a planted end cell, and
`check`, which runs both calls on a pair and asserts everything they return against
tests/_band_ext_oracle.py and the formulas of gpuseqalign_amd/csrc/nw_band_ext_plan.h as DESIGN.md 2.2r
states them.  The gap models, tables and random pairs are tests/_band_cases.py's; the geometry (TR, KR,
NWV) is read from the info struct and the width limit, not assumed."""
import numpy as np

import gpuseqalign_amd as gsa
from tests import _align_oracle as ao
from tests import _band_ext_oracle as eo
from tests._band_cases import GAP_IDS, GAPS, blosum_like, random_seq, related, table  # noqa: F401

FIELDS = ("score", "i_start", "j_start", "i_end", "j_end", "cigar")
UNIT = table(4, 1, -1)  # match 1, mismatch -1


def geometry(info):
    """(TR, KR, lag, NWV) from the info struct and the width limit: max_width = 64 NWV lag - TR + 1 - 63."""
    TR = info["strip_rows"]
    assert TR % 64 == 0
    KR = TR // 64
    lag = KR + 2
    nwv, rem = divmod(gsa.band_max_width() + TR - 1 + 63, 64 * lag)
    assert rem == 0
    return TR, KR, lag, nwv


def plan_of(TR, lag, nwv, R, C, lo, hi):
    """The info fields the plan's formulas give for a pair with R, C >= 1: those of the trimmed pair."""
    Ru, Cu = eo.trim(R, C, lo, hi)
    clo, chi = eo.clamp(R, C, lo, hi)
    W = chi - clo + 1
    strips = -(-Ru // TR)
    nq = -(-(W + TR - 1 + 63) // 64)
    return dict(strip_rows=TR, strips=strips, waves=min(nwv, strips), supersteps=(strips - 1) * lag + nq,
                band_lo=clo, band_hi=chi, code_bytes=strips * (W + TR - 1) * TR // 2, rows_used=Ru, cols_used=Cu)


def want_info(info, R, C, lo, hi):
    TR, _, lag, nwv = geometry(info)
    return plan_of(TR, lag, nwv, R, C, lo, hi)


def planted(rng, p, R, C, n=4):
    """x = y up to p; behind p, y is all letter 0 and x all letter 1.  Under UNIT no cell behind (p, p) in
    row-major order exceeds p and none before it reaches p: the extension ends at (p, p) with "p="."""
    head = rng.integers(0, n, size=p)
    y = np.concatenate([[0], head, np.zeros(R - p, np.int64)]).astype(np.int32)
    x = np.concatenate([[0], head, np.ones(C - p, np.int64)]).astype(np.int32)
    return y, x


def planted_want(p):
    return (p, 0, 0, p, p, "%d=" % p if p else "")


def tied(rng, p, R, C, n=4):
    """planted(p) with one mismatch and one match behind the peak: under UNIT the value p stands at
    (p, p) and again at (p + 2, p + 2)."""
    y, x = planted(rng, p, R, C, n)
    y[p + 1], x[p + 1] = 2, 3
    y[p + 2] = x[p + 2] = 2
    return y, x


def check(engine, y, x, sub, go, ge, lo, hi, want=None, wide=False):
    """Both calls on one pair: the score call, all six fields, the CIGAR, status and every info field
    against the oracle (or `want`), and the CIGAR replayed on the host.  Returns (result, info)."""
    R, C = len(y) - 1, len(x) - 1
    if want is None:
        want = eo.align(y, x, sub, go, ge, lo, hi, wide=wide)
    s = engine.score_band_ext(y, x, sub, go, ge, band_lo=lo, band_hi=hi)
    assert (s["score"], s["i_end"], s["j_end"]) == (want[0], want[3], want[4]), (R, C, lo, hi, go, ge)
    assert s["kernel_ms"] > 0
    a = engine.align_pair_band_ext(y, x, sub, go, ge, band_lo=lo, band_hi=hi)
    assert a["status"] == 0
    assert tuple(a[k] for k in FIELDS) == tuple(want), (R, C, lo, hi, go, ge)
    assert ao.rescore(a["cigar"], y, x, 0, 0, sub, go, ge) == (a["score"], a["i_end"], a["j_end"])
    info = engine.last_align_pair_band_ext_info()
    for k, v in want_info(info, R, C, lo, hi).items():
        assert info[k] == v, (k, info[k], v)
    assert info["proved_optimal"] == eo.certificate(R, C, lo, hi, sub, go, ge, a["score"])
    assert info["score_ms"] > 0 and info["walk_ms"] > 0
    assert abs(a["kernel_ms"] - (info["score_ms"] + info["walk_ms"])) < 1e-3
    return a, info


# -- the batch calls --

PAIR_INFO = ("band_lo", "band_hi", "code_bytes", "rows_used", "cols_used", "strips", "supersteps", "proved_optimal")


def singles(engine, pairs, bands, sub, go, ge, scratch_limit=0):
    """Per pair what align_pair_band_ext and score_band_ext return for it alone, and the single call's info."""
    out = []
    for (y, x), (lo, hi) in zip(pairs, bands):
        a = engine.align_pair_band_ext(y, x, sub, go, ge, band_lo=lo, band_hi=hi, scratch_limit=scratch_limit)
        info = engine.last_align_pair_band_ext_info()
        s = engine.score_band_ext(y, x, sub, go, ge, band_lo=lo, band_hi=hi)
        out.append((a, info, s))
    return out


def against_single(batch, pinfo, sbatch, want, pairs, sub, go, ge):
    """batch / sbatch: the alignment and the score call's lists; pinfo: the info dict's "pairs"; want:
    singles()'s list.  Status 2 cannot occur: the Python forms size the buffer."""
    assert len(batch) == len(pinfo) == len(sbatch) == len(want) == len(pairs)
    for p, ((a, info, s), (y, x)) in enumerate(zip(want, pairs)):
        b = batch[p]
        assert b["status"] == a["status"], (p, b, a)
        assert tuple(b[k] for k in FIELDS) == tuple(a[k] for k in FIELDS), (p, b, a)
        assert {k: pinfo[p][k] for k in PAIR_INFO} == {k: info[k] for k in PAIR_INFO}, (p, pinfo[p], info)
        assert (sbatch[p]["score"], sbatch[p]["i_end"], sbatch[p]["j_end"]) == (s["score"], s["i_end"], s["j_end"]), p
        if b["status"] == 0:
            assert ao.rescore(b["cigar"], y, x, 0, 0, sub, go, ge) == (b["score"], b["i_end"], b["j_end"]), p
        host = len(y) == 1 or len(x) == 1
        want_round = -1 if host else (-2 if b["status"] == 1 else None)
        assert pinfo[p]["round"] == want_round if want_round is not None else pinfo[p]["round"] >= 0, (p, pinfo[p])


def against_oracle(batch, pinfo, pairs, bands, sub, go, ge, max_cells=400000):
    """The pairs small enough, against tests/_band_ext_oracle.py directly."""
    for p, ((y, x), (lo, hi)) in enumerate(zip(pairs, bands)):
        R, C = len(y) - 1, len(x) - 1
        if R * C > max_cells or batch[p]["status"] != 0:
            continue
        want = eo.align(y, x, sub, go, ge, lo, hi)
        assert tuple(batch[p][k] for k in FIELDS) == tuple(want), (p, R, C, lo, hi)
        assert pinfo[p]["proved_optimal"] == (1 if R == 0 or C == 0 else eo.certificate(R, C, lo, hi, sub, go, ge, want[0]))
        assert (pinfo[p]["band_lo"], pinfo[p]["band_hi"]) == eo.clamp(R, C, lo, hi)
        assert (pinfo[p]["rows_used"], pinfo[p]["cols_used"]) == eo.trim(R, C, lo, hi)


class DevBatch:
    """Pairs and table on the device: seqs are uploaded once per array object, so that two entries that
    name the same arrays name the same buffers."""

    def __init__(self, engine, pairs, sub):
        import torch
        self.engine = engine
        dev = torch.device("cuda", engine.device)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)
        sub = np.asarray(sub)
        self.substsz = len(sub)
        self.dS = up(sub.ravel())
        self._keep = {}
        self.ptrs = []
        for y, x in pairs:
            t = []
            for a in (y, x):
                if id(a) not in self._keep:
                    self._keep[id(a)] = (a, up(a))
                t.append(self._keep[id(a)][1])
            self.ptrs.append((t[0].data_ptr(), t[0].numel(), t[1].data_ptr(), t[1].numel()))
        torch.cuda.synchronize(dev)

    @staticmethod
    def _strip(results):
        return [{k: v for k, v in r.items() if k != "kernel_ms"} for r in results]

    def align(self, go, ge, bands, order=None, **kw):
        """(results, info) of align_batch_band_ext_dev, in the list's own order whatever `order` ran."""
        order = list(range(len(self.ptrs))) if order is None else list(order)
        r = self.engine.align_batch_band_ext_dev([self.ptrs[p] for p in order], self.dS.data_ptr(), self.substsz, go, ge,
                                                 kw.pop("max_workgroups", 0), kw.pop("scratch_limit", 0),
                                                 kw.pop("stream", None), bands=[bands[p] for p in order], **kw)
        info = self.engine.last_align_batch_band_ext_info()
        back = [0] * len(order)
        for k, p in enumerate(order):
            back[p] = k
        info["pairs"] = [info["pairs"][back[p]] for p in range(len(order))]
        return self._strip([r[back[p]] for p in range(len(order))]), info

    def score(self, go, ge, bands, order=None, **kw):
        order = list(range(len(self.ptrs))) if order is None else list(order)
        r = self.engine.score_band_ext_batch_dev([self.ptrs[p] for p in order], self.dS.data_ptr(), self.substsz, go, ge,
                                                 kw.pop("stream", None), bands=[bands[p] for p in order], **kw)
        back = [0] * len(order)
        for k, p in enumerate(order):
            back[p] = k
        return self._strip([r[back[p]] for p in range(len(order))])

    def _tables(self, bands):
        import ctypes
        m = max(len(self.ptrs), 1)
        arr = (gsa.PairDev * m)()
        lo, hi = (ctypes.c_int64 * m)(), (ctypes.c_int64 * m)()
        for k, (yp, ar, xp, ac) in enumerate(self.ptrs):
            arr[k].seqY, arr[k].adjrows, arr[k].seqX, arr[k].adjcols = yp, ar, xp, ac
            lo[k], hi[k] = bands[k]
        return m, arr, lo, hi

    def raw_align(self, go, ge, bands, cap, scratch_limit=0, waves=0, max_workgroups=0, null_cigar=False, null_out=False,
                  npairs=None, fill=None):
        """gsa_align_batch_band_ext_dev through ctypes: (status, results, buffer, need, pair info, info)."""
        import ctypes
        n = len(self.ptrs) if npairs is None else npairs
        m, arr, lo, hi = self._tables(bands)
        res, pinfo, info = (gsa.AlignDbResult * m)(), (gsa.AlignBatchBandExtPair * m)(), gsa.AlignBatchBandExtInfo()
        if fill is not None:
            for r in res:
                r.score, r.status, r.i_end, r.cigar_off = fill, fill, fill, fill
        need, ms = ctypes.c_int64(-1), ctypes.c_float(-1.0)
        buf = ctypes.create_string_buffer(max(cap, 1))
        st = gsa.lib().gsa_align_batch_band_ext_dev(self.engine._h, n, arr, self.dS.data_ptr(), self.substsz, go, ge, lo, hi,
                                                    waves, max_workgroups, scratch_limit, None if null_out else res,
                                                    None if null_cigar else buf, cap, ctypes.byref(need), pinfo,
                                                    ctypes.byref(info), ctypes.byref(ms), None)
        return st, res, buf, need.value, pinfo, info

    def raw_score(self, go, ge, bands, waves=0, max_workgroups=0, npairs=None, fill=None):
        import ctypes
        n = len(self.ptrs) if npairs is None else npairs
        m, arr, lo, hi = self._tables(bands)
        res = (gsa.ScoreResult * m)()
        if fill is not None:
            for r in res:
                r.score, r.i_end, r.j_end = fill, fill, fill
        ms = ctypes.c_float(-1.0)
        st = gsa.lib().gsa_score_band_ext_batch_dev(self.engine._h, n, arr, self.dS.data_ptr(), self.substsz, go, ge, lo, hi,
                                                    waves, max_workgroups, res, ctypes.byref(ms), None)
        return st, res, ms.value
