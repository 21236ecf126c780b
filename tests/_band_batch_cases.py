"""What the tests of the banded batch calls share (tests/test_align_batch_band_plan.py,
tests/test_gpu_score_band_batch.py, tests/test_gpu_align_batch_band.py): the waves rule and the round plan
of gpuseqalign_amd/csrc/nw_band_batch_plan.h restated in Python (the plan test checks the restatement
against the header through its driver), and `against_single`, which runs the single-pair calls on every
pair of a batch -- the yardstick DESIGN.md 2.2q names -- and asserts the batch's answers against them
field for field, per-pair info included, with every CIGAR replayed."""
import numpy as np

from tests import _align_oracle as ao
from tests import _band_oracle as bo
from tests._band_cases import FIELDS

WAVES = (4, 8, 16)
PAIR_INFO = ("band_lo", "band_hi", "code_bytes", "strips", "supersteps", "proved_optimal")


def waves_ok(nwv, strips, nq, lag=6):
    return strips <= nwv or nq <= nwv * lag


def pick_waves(forced, pairs, lag=6):
    """pairs: (strips, nq).  0: refused."""
    if forced == 0:
        return next((w for w in WAVES if all(waves_ok(w, s, n, lag) for s, n in pairs)), 16)
    if forced not in WAVES or not all(waves_ok(forced, s, n, lag) for s, n in pairs):
        return 0
    return forced


def plan_rounds(code_bytes, limit):
    """(rounds, round_of, peak): code bytes descending, ties by index; a round takes every pair that still
    fits the bytes left.  Negative bytes: the pair takes no part (-3); over the limit: -2."""
    round_of = [-3] * len(code_bytes)
    todo = []
    for p, b in enumerate(code_bytes):
        if b < 0:
            continue
        if b > limit:
            round_of[p] = -2
        else:
            todo.append(p)
    todo.sort(key=lambda p: (-code_bytes[p], p))
    rounds, peak = [], 0
    while todo:
        left, take, rest = limit, [], []
        for p in todo:
            if code_bytes[p] <= left:
                left -= code_bytes[p]
                round_of[p] = len(rounds)
                take.append(p)
            else:
                rest.append(p)
        peak = max(peak, limit - left)
        rounds.append(take)
        todo = rest
    return rounds, round_of, peak


def singles(engine, pairs, bands, sub, go, ge, scratch_limit=0):
    """Per pair what align_pair_band and score_band return for it alone, and the single call's info."""
    out = []
    for (y, x), (lo, hi) in zip(pairs, bands):
        a = engine.align_pair_band(y, x, sub, go, ge, band_lo=lo, band_hi=hi, scratch_limit=scratch_limit)
        info = engine.last_align_pair_band_info()
        s = engine.score_band(y, x, sub, go, ge, band_lo=lo, band_hi=hi)
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
        R, C = len(y) - 1, len(x) - 1
        if b["status"] == 0:
            assert ao.rescore(b["cigar"], y, x, 0, 0, sub, go, ge) == (b["score"], R, C), p
        want_round = -1 if R == 0 or C == 0 else (-2 if b["status"] == 1 else None)
        assert pinfo[p]["round"] == want_round if want_round is not None else pinfo[p]["round"] >= 0, (p, pinfo[p])


def against_oracle(batch, pinfo, pairs, bands, sub, go, ge, max_cells=400000):
    """The pairs small enough, against tests/_band_oracle.py directly."""
    for p, ((y, x), (lo, hi)) in enumerate(zip(pairs, bands)):
        R, C = len(y) - 1, len(x) - 1
        if R == 0 or C == 0 or R * C > max_cells or batch[p]["status"] != 0:
            continue
        want = bo.align(y, x, sub, go, ge, lo, hi)
        assert tuple(batch[p][k] for k in FIELDS) == tuple(want), (p, R, C, lo, hi)
        assert pinfo[p]["proved_optimal"] == bo.certificate(R, C, lo, hi, sub, go, ge, batch[p]["score"])
        assert (pinfo[p]["band_lo"], pinfo[p]["band_hi"]) == bo.clamp(R, C, lo, hi)


def strip_ms(results):
    return [{k: v for k, v in r.items() if k != "kernel_ms"} for r in results]


def nq_of(W, TR=256):
    return -(-(W + TR - 1 + 63) // 64)


def np_seq(a):
    return np.ascontiguousarray(a, dtype=np.int32)


class DevBatch:
    """Pairs and table on the device: seqs are uploaded once per array object, so that two entries that
    name the same arrays name the same buffers."""

    def __init__(self, engine, pairs, sub):
        import torch
        self.engine = engine
        dev = torch.device("cuda", engine.device)
        up = lambda a: torch.from_numpy(np_seq(a)).to(dev)
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

    def align(self, go, ge, bands, order=None, **kw):
        """(results, info) of align_batch_band_dev, in the list's own order whatever `order` ran."""
        order = list(range(len(self.ptrs))) if order is None else list(order)
        r = self.engine.align_batch_band_dev([self.ptrs[p] for p in order], self.dS.data_ptr(), self.substsz, go, ge,
                                             kw.pop("max_workgroups", 0), kw.pop("scratch_limit", 0), kw.pop("stream", None),
                                             bands=[bands[p] for p in order], **kw)
        info = self.engine.last_align_batch_band_info()
        back = [0] * len(order)
        for k, p in enumerate(order):
            back[p] = k
        info["pairs"] = [info["pairs"][back[p]] for p in range(len(order))]
        return strip_ms([r[back[p]] for p in range(len(order))]), info

    def score(self, go, ge, bands, order=None, **kw):
        order = list(range(len(self.ptrs))) if order is None else list(order)
        r = self.engine.score_band_batch_dev([self.ptrs[p] for p in order], self.dS.data_ptr(), self.substsz, go, ge,
                                             kw.pop("stream", None), bands=[bands[p] for p in order], **kw)
        back = [0] * len(order)
        for k, p in enumerate(order):
            back[p] = k
        return strip_ms([r[back[p]] for p in range(len(order))])

    def raw_align(self, go, ge, bands, cap, scratch_limit=0, waves=0, max_workgroups=0, null_cigar=False, null_out=False,
                  npairs=None, fill=None):
        """gsa_align_batch_band_dev through ctypes: (status, results, buffer, need, pair info, info)."""
        import ctypes

        import gpuseqalign_amd as gsa
        n = len(self.ptrs) if npairs is None else npairs
        m = max(len(self.ptrs), 1)
        arr = (gsa.PairDev * m)()
        lo, hi = (ctypes.c_int64 * m)(), (ctypes.c_int64 * m)()
        for k, (yp, ar, xp, ac) in enumerate(self.ptrs):
            arr[k].seqY, arr[k].adjrows, arr[k].seqX, arr[k].adjcols = yp, ar, xp, ac
            lo[k], hi[k] = bands[k]
        res, pinfo, info = (gsa.AlignDbResult * m)(), (gsa.AlignBatchBandPair * m)(), gsa.AlignBatchBandInfo()
        if fill is not None:
            for r in res:
                r.score, r.status, r.i_end, r.cigar_off = fill, fill, fill, fill
        need, ms = ctypes.c_int64(-1), ctypes.c_float(-1.0)
        buf = ctypes.create_string_buffer(max(cap, 1))
        st = gsa.lib().gsa_align_batch_band_dev(self.engine._h, n, arr, self.dS.data_ptr(), self.substsz, go, ge, lo, hi, waves,
                                                max_workgroups, scratch_limit, None if null_out else res,
                                                None if null_cigar else buf, cap, ctypes.byref(need), pinfo, ctypes.byref(info),
                                                ctypes.byref(ms), None)
        return st, res, buf, need.value, pinfo, info

    def raw_score(self, go, ge, bands, waves=0, max_workgroups=0, npairs=None, fill=None):
        import ctypes

        import gpuseqalign_amd as gsa
        n = len(self.ptrs) if npairs is None else npairs
        m = max(len(self.ptrs), 1)
        arr = (gsa.PairDev * m)()
        lo, hi = (ctypes.c_int64 * m)(), (ctypes.c_int64 * m)()
        for k, (yp, ar, xp, ac) in enumerate(self.ptrs):
            arr[k].seqY, arr[k].adjrows, arr[k].seqX, arr[k].adjcols = yp, ar, xp, ac
            lo[k], hi[k] = bands[k]
        res = (gsa.ScoreResult * m)()
        if fill is not None:
            for r in res:
                r.score, r.i_end, r.j_end = fill, fill, fill
        ms = ctypes.c_float(-1.0)
        st = gsa.lib().gsa_score_band_batch_dev(self.engine._h, n, arr, self.dS.data_ptr(), self.substsz, go, ge, lo, hi, waves,
                                                max_workgroups, res, ctypes.byref(ms), None)
        return st, res, ms.value
