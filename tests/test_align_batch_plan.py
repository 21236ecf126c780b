"""The host plan of gsa_align_batch_dev (gpuseqalign_amd/csrc/nw_pair_trace_batch_plan.h; DESIGN.md
2.2j), checked on the CPU: tests/align_batch_plan_driver.cpp, a stand-alone program over the header, is
compiled once with the host compiler and run as a child process on seeded cases.  The driver checks the
plan's properties itself and fails on a violation; the rounds it prints are checked again here: every
round within the limit, code ranges disjoint, every pair's strips covered bottom-up, contiguously and
once, every round at least one strip, one pair's rounds equal to pair_plan_chunk's chunks (restated in
Python).  No GPU and no library needed."""
import os
import random
import subprocess
import tempfile


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_EXE = {}


def _driver():
    if "exe" not in _EXE:
        d = tempfile.mkdtemp(prefix="batch_plan_")
        exe = os.path.join(d, "plan_driver")
        cc = os.environ.get("CC")
        cmd = [cc] if cc else ["c++"]
        subprocess.check_call(cmd + ["-std=c++17", "-O1", "-x", "c++", "-I", os.path.join(ROOT, "gpuseqalign_amd", "csrc"),
                                     os.path.join(ROOT, "tests", "align_batch_plan_driver.cpp"), "-o", exe, "-lstdc++"])
        _EXE["exe"] = exe
    return _EXE["exe"]


def _text(cases):
    """Cases (TR, limit, seed, [(iEnd, jEnd), ...]) as the driver reads them."""
    return "".join("%d %d %d %d\n" % (tr, limit, seed, len(pairs)) + "".join("%d %d\n" % p for p in pairs)
                   for tr, limit, seed, pairs in cases)


def _run(cases):
    """Per case: the rounds, each (bytes, [chunk dicts], [pairs done in it])."""
    p = subprocess.run([_driver()], input=_text(cases), capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    plans, cur = [], None
    for line in p.stdout.split("\n"):
        f = line.split()
        if not f:
            continue
        v = [int(x) for x in f[1:]]
        if f[0] == "case":
            cur = []
        elif f[0] == "round":
            cur.append((v[0], [], []))
        elif f[0] == "chunk":
            cur[-1][1].append(dict(zip(("pair", "tLo", "tHi", "J", "stripBytes", "codeBytes", "codeOff"), v)))
        elif f[0] == "done":
            cur[-1][2].append(v[0])
        elif f[0] == "end":
            assert v[0] == len(cur)
            plans.append(cur)
        else:
            assert f[0] == "ok" and v[0] == len(cases)
    assert len(plans) == len(cases)
    return plans


def _verify(case, rounds):
    tr, limit, _, pairs = case
    nxt = [-(-i // tr) - 1 for i, _ in pairs]  # the strip each pair's next chunk ends on
    cols = [j for _, j in pairs]
    done = [False] * len(pairs)
    filled = [0] * len(pairs)
    for used, chunks, fin in rounds:
        assert chunks and 0 < used <= limit and used == sum(c["codeBytes"] for c in chunks)
        spans = []
        for c in chunks:
            p = c["pair"]
            assert not done[p] and c["tHi"] == nxt[p] and 0 <= c["tLo"] <= c["tHi"]
            assert 1 <= c["J"] <= cols[p] and c["stripBytes"] == c["J"] * (tr // 2)
            n = c["tHi"] - c["tLo"] + 1
            assert c["codeBytes"] == n * c["stripBytes"]
            spans.append((c["codeOff"], c["codeOff"] + c["codeBytes"]))
            filled[p] += n
            nxt[p], cols[p] = c["tLo"] - 1, c["J"]
        assert len({c["pair"] for c in chunks}) == len(chunks)
        spans.sort()
        assert spans[0][0] >= 0 and spans[-1][1] <= limit and all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))
        for p in fin:
            done[p] = True
        # a pair that reached strip 0 is done
        assert all(done[c["pair"]] for c in chunks if c["tLo"] == 0)
    assert all(done)
    return len(rounds), sum(filled)


def _pair_chunks(tr, i_end, j_end, limit, cols):
    """nw_pair_trace_plan.h's chunks of one pair, with the walk leaving chunk k at column cols[k]."""
    out, hi, J = [], -(-i_end // tr) - 1, j_end
    while True:
        sb = J * (tr // 2)
        n = min(limit // sb, hi + 1)
        out.append((hi + 1 - n, hi, J))
        if len(out) > len(cols):
            return out
        hi, J = hi - n, cols[len(out) - 1]


def test_one_pair_is_the_single_pair_plan():
    rng = random.Random(3)
    cases = []
    for k in range(300):
        tr = rng.choice((512, 1024))
        i_end, j_end = rng.randint(1, 70000), rng.randint(1, 70000)
        sb = j_end * (tr // 2)
        cases.append((tr, rng.randint(sb, 12 * sb), k, [(i_end, j_end)]))
    many = 0
    for case, rounds in zip(cases, _run(cases)):
        _verify(case, rounds)
        tr, limit, _, [(i_end, j_end)] = case
        got = [(c["tLo"], c["tHi"], c["J"]) for _, [c], _ in rounds]
        assert all(c["codeOff"] == 0 for _, [c], _ in rounds)
        assert got == _pair_chunks(tr, i_end, j_end, limit, [c[2] for c in got[1:]])
        many += len(rounds) >= 3
    assert many >= 20


def test_fixed_order_and_waiting():
    """Three pairs, a limit of two of the largest strips: the pair with the most bytes left goes first,
    and a pair for which nothing is left in a round waits for the next."""
    tr = 1024
    pairs = [(3 * tr, 1000), (5 * tr, 1000), (tr, 400)]
    sb = 1000 * tr // 2
    [rounds] = _run([(tr, 2 * sb, 1, pairs)])
    _verify((tr, 2 * sb, 1, pairs), rounds)
    first = rounds[0][1]
    assert [c["pair"] for c in first] == [1] and (first[0]["tLo"], first[0]["tHi"]) == (3, 4)
    assert len(rounds) >= 3


def test_many_seeded_batches():
    rng = random.Random(11)
    cases = []
    for k in range(1500):
        tr = rng.choice((512, 1024))
        n = rng.randint(1, 40)
        top = rng.choice((300, 3000, 70000))
        pairs = [(rng.randint(1, top), rng.randint(1, top)) for _ in range(n)]
        sb = max(j for _, j in pairs) * (tr // 2)
        limit = rng.choice((sb, sb + 1, 2 * sb, rng.randint(sb, 40 * sb), 8 << 30))
        cases.append((tr, limit, k, pairs))
    stats = [_verify(c, r) for c, r in zip(cases, _run(cases))]
    assert min(s[0] for s in stats) == 1 and max(s[0] for s in stats) >= 10
