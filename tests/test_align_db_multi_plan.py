"""The host plan of gsa_align_db_multi_dev (gpuseqalign_amd/csrc/nw_lanes_trace_multi_plan.h; DESIGN.md
2.2g), checked on the CPU: tests/align_db_multi_plan_driver.cpp, a stand-alone program over the header,
is compiled once with the host compiler and run as a child process on seeded cases; the properties the
kernels rely on are asserted on the plans it prints.  No GPU and no library needed."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWEEP, TASK, COL = 384, 4, 192
_EXE = {}


def _driver():
    if "exe" not in _EXE:
        d = tempfile.mkdtemp(prefix="dba_plan_")
        exe = os.path.join(d, "plan_driver")
        cc = os.environ.get("CC")
        cmd = [cc] if cc else ["c++"]
        subprocess.check_call(cmd + ["-std=c++17", "-O1", "-x", "c++", "-I", os.path.join(ROOT, "gpuseqalign_amd", "csrc"),
                                     os.path.join(ROOT, "tests", "align_db_multi_plan_driver.cpp"), "-o", exe, "-lstdc++"])
        _EXE["exe"] = exe
    return _EXE["exe"]


def _passes(R):
    return -(-R // SWEEP)


def _code_bytes(R, C):
    return _passes(R) * (C + 1) * COL


class Case:
    def __init__(self, qlen, slen, hits, unit, limit):
        self.qlen, self.slen, self.hits, self.unit, self.limit = list(qlen), list(slen), list(hits), unit, limit
        self.qoff = np.concatenate([[0], np.cumsum([n + 1 for n in self.qlen])])
        self.off = np.concatenate([[0], np.cumsum([n + 1 for n in self.slen])])
        # the route of a pair: both sides have letters and its codes alone fit the limit
        self.lane = [int(self.qlen[q] > 0 and self.slen[s] > 0 and _code_bytes(self.qlen[q], self.slen[s]) <= limit)
                     for q, s in self.hits]

    def text(self):
        out = ["%d %d %d %d %d" % (len(self.qlen), len(self.slen), len(self.hits), self.unit, self.limit)]
        out.append(" ".join(map(str, self.qlen)))
        out.append(" ".join(map(str, self.slen)))
        out += ["%d %d %d" % (q, s, l) for (q, s), l in zip(self.hits, self.lane)]
        return "\n".join(out) + "\n"


def _run(cases):
    """The plans of `cases`: per case a list of chunks, a chunk a dict of its header and record lists."""
    p = subprocess.run([_driver()], input="".join(c.text() for c in cases), capture_output=True, text=True, check=True)
    plans, plan, chunk = [], None, None
    for line in p.stdout.split("\n"):
        f = line.split()
        if not f:
            continue
        if f[0] == "plan":
            plan = []
            want = int(f[1])
        elif f[0] == "chunk":
            chunk = {"codeBytes": int(f[1]), "moveBytes": int(f[2]), "cmax": int(f[3]), "H": [], "Q": [], "T": [], "U": [], "L": []}
            plan.append(chunk)
        elif f[0] == "end":
            assert len(plan) == want
            plans.append(plan)
        else:
            chunk[f[0]].append(tuple(int(v) for v in f[1:]))
    assert len(plans) == len(cases), p.stderr
    return plans


def _check(case, plan):
    """Every property the issue lists, on one plan; returns the chunk count."""
    seen, order = [], []
    for ci, ch in enumerate(plan):
        H, Q, T, U, L = ch["H"], ch["Q"], ch["T"], ch["U"], ch["L"]
        assert H and Q and T and U and L
        for hit, qi, R, C, qOff, dbOff, cOff, cLen, mOff, mLen in H:
            q, s = case.hits[hit]
            assert case.lane[hit] == 1
            assert (R, C) == (case.qlen[q], case.slen[s]) and R >= 1 and C >= 1
            assert (qOff, dbOff) == (case.qoff[q], case.off[s])
            assert Q[qi] == (case.qoff[q], R, q)
            assert cLen == _code_bytes(R, C) and mLen == R + C
            seen.append(hit)
            order.append((-R, q, -C, hit))
        assert len({q[2] for q in Q}) == len(Q), "a query twice in a chunk"
        # code and move ranges: disjoint, back to back, their sum the chunk's and within the limit
        for off, ln, total in ((6, 7, ch["codeBytes"]), (8, 9, ch["moveBytes"])):
            at = 0
            for h in sorted(H, key=lambda h: h[off]):
                assert h[off] == at
                at += h[ln]
            assert at == total
        assert ch["codeBytes"] <= case.limit
        assert ch["cmax"] == max(h[3] for h in H)
        # every hit in exactly one task slot; no task mixes queries
        slots = []
        for first, n in T:
            assert 1 <= n <= TASK and first + n <= len(H)
            assert len({H[k][1] for k in range(first, first + n)}) == 1
            slots += list(range(first, first + n))
        assert slots == list(range(len(H)))
        for (f0, n0), (f1, _) in zip(T, T[1:]):
            if H[f0][1] == H[f1][1]:
                assert n0 == TASK  # only a query's last task is short
        # a unit's tasks are consecutive and of one query; only a query's last unit is short
        tasks = []
        for qi, ft, nt in U:
            assert 1 <= nt <= case.unit and ft + nt <= len(T)
            assert all(H[T[t][0]][1] == qi for t in range(ft, ft + nt))
            tasks += list(range(ft, ft + nt))
        assert tasks == list(range(len(T)))
        for (q0, _, n0), (q1, _, _) in zip(U, U[1:]):
            if q0 == q1:
                assert n0 == case.unit
        # launches: a partition of the units, queries and tasks; one sweep class each, classes distinct
        units, queries, tks = [], [], []
        for passes, fu, nu, fq, nqq, ft, nt in L:
            assert nu >= 1 and nqq >= 1 and nt >= 1
            units += list(range(fu, fu + nu))
            queries += list(range(fq, fq + nqq))
            tks += list(range(ft, ft + nt))
            for qi, uft, unt in U[fu:fu + nu]:
                assert fq <= qi < fq + nqq and ft <= uft and uft + unt <= ft + nt
                assert _passes(Q[qi][1]) == passes
        assert units == list(range(len(U))) and queries == list(range(len(Q))) and tks == list(range(len(T)))
        assert len({l[0] for l in L}) == len(L)
        # greedy: the next chunk's first hit did not fit this one
        if ci + 1 < len(plan):
            assert ch["codeBytes"] + plan[ci + 1]["H"][0][7] > case.limit
    assert sorted(seen) == [h for h, l in enumerate(case.lane) if l], "every lane hit exactly once"
    assert order == sorted(order), "sweep class, query (longest first), subject (longest first)"
    return len(plan)


def _hits(rng, qlen, slen, counts):
    """counts[q] hits of query q, interleaved by query; some pairs repeated."""
    per = [[(q, int(s)) for s in rng.integers(0, len(slen), n)] for q, n in enumerate(counts)]
    for row in per:
        if len(row) >= 3:
            row[2] = row[0]  # the same pair twice
    hits = []
    for k in range(max(counts) if counts else 0):
        hits += [row[k] for row in per if k < len(row)]
    return hits


def _seeded(nq, unit, seed):
    rng = np.random.default_rng(seed)
    edge = [1, 384, 385, 769]
    qlen = [edge[q % 4] if q % 3 == 0 else int(rng.integers(1, 900)) for q in range(nq)]
    if nq >= 5:
        qlen[4] = 0  # an empty query: its hits are not the plan's
    slen = [int(c) for c in rng.integers(0, 301, 40)]
    slen[0], slen[1], slen[2] = 300, 1, 0
    sizes = [0, 1, 3, 4, 5, 4 * unit - 1, 4 * unit, 4 * unit + 1]
    counts = [sizes[(q + seed) % len(sizes)] for q in range(nq)]
    if nq == 1:
        counts = [sizes[seed % len(sizes)]]
    return qlen, slen, _hits(rng, qlen, slen, counts)


@pytest.mark.parametrize("unit", [1, 4, 8])
@pytest.mark.parametrize("nq", [1, 2, 5, 33])
def test_seeded_plans(nq, unit):
    cases, want = [], []
    for seed in range(8):
        qlen, slen, hits = _seeded(nq, unit, seed)
        need = [_code_bytes(qlen[q], slen[s]) for q, s in hits if qlen[q] > 0 and slen[s] > 0]
        total, largest = sum(need), max(need, default=0)
        cases.append(Case(qlen, slen, hits, unit, max(total, 1)))
        want.append((1, 1) if need else (0, 0))
        if need:
            cases.append(Case(qlen, slen, hits, unit, max(largest, total // 3)))
            want.append((3 if largest <= total // 3 else 1, len(need)))
            cases.append(Case(qlen, slen, hits, unit, largest))  # many chunks
            want.append((-(-total // largest), len(need)))
            cases.append(Case(qlen, slen, hits, unit, max(largest // 2, 1)))  # the largest hits are not lane hits
            want.append((0, len(need)))
    for case, plan, (lo, hi) in zip(cases, _run(cases), want):
        n = _check(case, plan)
        assert lo <= n <= hi, (n, lo, hi, case.limit)


def test_exact_chunk_counts_and_hand_checked_plan():
    """Six equal hits of one query: a limit of two hits' codes gives exactly three chunks, a limit of all
    six one.  A hand-checked plan: 9 hits of a 385-letter query and 1 of a 5-letter one, unit 2."""
    one = _code_bytes(100, 50)
    a = Case([100], [50], [(0, 0)] * 6, 4, 2 * one)
    b = Case([100], [50], [(0, 0)] * 6, 4, 6 * one)
    c = Case([5, 385], [10, 20, 0], [(1, 0)] * 4 + [(0, 1)] + [(1, 1)] * 5 + [(0, 2), (1, 2)], 2, 1 << 40)
    pa, pb, pc = _run([a, b, c])
    assert _check(a, pa) == 3 and _check(b, pb) == 1 and _check(c, pc) == 1
    assert [len(ch["H"]) for ch in pa] == [2, 2, 2] and [ch["codeBytes"] for ch in pa] == [2 * one] * 3
    ch = pc[0]
    assert [h[0] for h in ch["H"]] == [5, 6, 7, 8, 9, 0, 1, 2, 3, 4]  # 385 x 20 first, then 385 x 10, then 5 x 20
    assert ch["T"] == [(0, 4), (4, 4), (8, 1), (9, 1)]
    assert ch["U"] == [(0, 0, 2), (0, 2, 1), (1, 3, 1)]
    assert ch["L"] == [(2, 0, 2, 0, 1, 0, 3), (1, 2, 1, 1, 1, 3, 1)]
    assert ch["Q"] == [(c.qoff[1], 385, 1), (c.qoff[0], 5, 0)]
    assert ch["codeBytes"] == 5 * 2 * 21 * COL + 4 * 2 * 11 * COL + 21 * COL and ch["cmax"] == 20


def test_no_lane_hits_is_an_empty_plan():
    c = Case([0, 7], [0, 9], [(0, 1), (1, 0), (0, 0)], 4, 1 << 30)
    assert _run([c]) == [[]]
    assert _run([Case([7], [9], [], 4, 1 << 30)]) == [[]]
