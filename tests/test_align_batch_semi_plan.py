"""The host plan of gsa_align_batch_semi_dev (gpuseqalign_amd/csrc/nw_pair_semi_trace_batch_plan.h;
DESIGN.md 2.2l), checked on the CPU: tests/align_batch_semi_plan_driver.cpp, a stand-alone program over
the header, is compiled once with the host compiler and run as a child process on seeded cases.  The
driver checks the plan's properties itself and fails on a violation; the rounds it prints are checked
again here: every round within the limit, code ranges disjoint, every pair's strips covered bottom-up,
contiguously, once and up to strip 0, every round at least one strip, the fixed order, one pair's rounds
equal to semi_plan_chunk's chunks (restated in Python), and hand-computed cases.  No GPU and no library
needed."""
import os
import random
import subprocess
import tempfile


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_EXE = {}


def _driver():
    if "exe" not in _EXE:
        d = tempfile.mkdtemp(prefix="batch_semi_plan_")
        exe = os.path.join(d, "plan_driver")
        cc = os.environ.get("CC")
        cmd = [cc] if cc else ["c++"]
        subprocess.check_call(cmd + ["-std=c++17", "-O1", "-x", "c++", "-I", os.path.join(ROOT, "gpuseqalign_amd", "csrc"),
                                     os.path.join(ROOT, "tests", "align_batch_semi_plan_driver.cpp"), "-o", exe, "-lstdc++"])
        _EXE["exe"] = exe
    return _EXE["exe"]


def _text(cases):
    """Cases (TR, limit, seed, [(R, jEnd, jW), ...]) as the driver reads them."""
    return "".join("%d %d %d %d\n" % (tr, limit, seed, len(pairs)) + "".join("%d %d %d\n" % p for p in pairs)
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
            cur[-1][1].append(dict(zip(("pair", "tLo", "tHi", "W", "stripBytes", "codeBytes", "codeOff"), v)))
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
    nxt = [-(-r // tr) - 1 for r, _, _ in pairs]  # the strip each pair's next chunk ends on
    width = [j - w for _, j, w in pairs]
    done = [False] * len(pairs)
    filled = [0] * len(pairs)
    for used, chunks, fin in rounds:
        assert chunks and 0 < used <= limit and used == sum(c["codeBytes"] for c in chunks)
        spans = []
        for c in chunks:
            p = c["pair"]
            assert not done[p] and c["tHi"] == nxt[p] and 0 <= c["tLo"] <= c["tHi"]
            assert 1 <= c["W"] <= width[p] and c["stripBytes"] == c["W"] * (tr // 2)
            n = c["tHi"] - c["tLo"] + 1
            assert c["codeBytes"] == n * c["stripBytes"]
            spans.append((c["codeOff"], c["codeOff"] + c["codeBytes"]))
            filled[p] += n
            nxt[p], width[p] = c["tLo"] - 1, c["W"]
        assert len({c["pair"] for c in chunks}) == len(chunks)
        spans.sort()
        assert spans[0][0] >= 0 and spans[-1][1] <= limit and all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))
        for p in fin:
            done[p] = True
        # done exactly when the chunk holds strip 0: a semi-global path always reaches row 0
        assert sorted(fin) == sorted(c["pair"] for c in chunks if c["tLo"] == 0)
    assert all(done)
    assert filled == [-(-r // tr) for r, _, _ in pairs]  # every strip, once
    return len(rounds), sum(filled)


def _check_order(case, rounds):
    """The pairs that got a chunk in a round, by remaining code bytes descending (the strips left times
    the chunk's strip bytes), ties by index."""
    tr, _, _, pairs = case
    nxt = [-(-r // tr) - 1 for r, _, _ in pairs]
    for _, chunks, _ in rounds:
        keys = [(-(nxt[c["pair"]] + 1) * c["stripBytes"], c["pair"]) for c in chunks]
        assert keys == sorted(keys), keys
        for c in chunks:
            nxt[c["pair"]] = c["tLo"] - 1


def _semi_chunks(tr, R, j_end, jW, limit, cols):
    """nw_pair_semi_plan.h's chunks of one pair, with the walk leaving chunk k at column cols[k]."""
    out, hi, J = [], -(-R // tr) - 1, j_end
    while True:
        sb = (J - jW) * (tr // 2)
        n = min(limit // sb, hi + 1)
        out.append((hi + 1 - n, hi, J - jW))
        if hi + 1 - n == 0:
            return out
        hi, J = hi - n, cols[len(out) - 1]


def test_one_pair_is_the_single_pair_plan():
    rng = random.Random(3)
    cases = []
    for k in range(300):
        tr = rng.choice((512, 1024))
        R, j_end = rng.randint(1, 70000), rng.randint(1, 70000)
        jW = rng.choice((0, rng.randint(0, j_end - 1)))
        sb = (j_end - jW) * (tr // 2)
        cases.append((tr, rng.randint(sb, 12 * sb), k, [(R, j_end, jW)]))
    many = 0
    for case, rounds in zip(cases, _run(cases)):
        _verify(case, rounds)
        tr, limit, _, [(R, j_end, jW)] = case
        got = [(c["tLo"], c["tHi"], c["W"]) for _, [c], _ in rounds]
        assert all(c["codeOff"] == 0 for _, [c], _ in rounds)
        assert got == _semi_chunks(tr, R, j_end, jW, limit, [jW + c[2] for c in got[1:]])
        many += len(rounds) >= 3
    assert many >= 20


def test_hand_computed_rounds():
    """Three pairs at TR = 1024 (512 bytes a column and strip), a limit of two of the widest strips.
    Pair 1 (5 strips of 1000 columns behind jW = 2000) has the most bytes left and takes the whole first
    round with its strips 3 and 4; pair 0 (3 strips, 1000 columns from column 1) and pair 2 (1 strip of
    400) wait."""
    tr = 1024
    pairs = [(3 * tr, 1000, 0), (5 * tr, 3000, 2000), (tr, 2400, 2000)]
    sb = 1000 * tr // 2
    case = (tr, 2 * sb, 1, pairs)
    [rounds] = _run([case])
    _verify(case, rounds)
    _check_order(case, rounds)
    first = rounds[0]
    assert first[0] == 2 * sb and first[2] == []
    assert [(c["pair"], c["tLo"], c["tHi"], c["W"], c["codeOff"]) for c in first[1]] == [(1, 3, 4, 1000, 0)]
    # the last strip to be filled anywhere is a strip 0, and pair 2's only chunk is (0, 0, 400 columns)
    two = [c for _, chunks, _ in rounds for c in chunks if c["pair"] == 2]
    assert [(c["tLo"], c["tHi"], c["W"], c["codeBytes"]) for c in two] == [(0, 0, 400, 400 * 512)]
    assert len(rounds) >= 3
    # one strip exactly: the first chunk is the lowest strip alone, over the whole window
    case = (512, 700 * 256, 5, [(3 * 512 + 1, 900, 200)])
    [rounds] = _run([case])
    _verify(case, rounds)
    c = rounds[0][1][0]
    assert (c["tLo"], c["tHi"], c["W"], c["codeBytes"]) == (3, 3, 700, 700 * 256) and len(rounds) >= 2
    # the default limit: everything in one round, in the fixed order, back to back
    case = (1024, 8 << 30, 7, [(2048, 500, 100), (1024, 9000, 0), (3000, 800, 0)])
    [rounds] = _run([case])
    assert len(rounds) == 1
    assert [(c["pair"], c["tLo"], c["tHi"], c["W"], c["codeOff"]) for c in rounds[0][1]] == [
        (1, 0, 0, 9000, 0), (2, 0, 2, 800, 9000 * 512), (0, 0, 1, 400, 9000 * 512 + 3 * 800 * 512)]
    assert sorted(rounds[0][2]) == [0, 1, 2]


def test_many_seeded_batches():
    rng = random.Random(11)
    cases = []
    for k in range(1500):
        tr = rng.choice((512, 1024))
        n = rng.randint(1, 40)
        top = rng.choice((300, 3000, 70000))
        pairs = []
        for _ in range(n):
            j_end = rng.randint(1, top)
            jW = rng.choice((0, 0, rng.randint(0, j_end - 1), (j_end - 1) * 9 // 10))  # from 0 to most of the subject
            pairs.append((rng.randint(1, top), j_end, jW))
        sb = max(j - w for _, j, w in pairs) * (tr // 2)
        limit = rng.choice((sb, sb + 1, 2 * sb, rng.randint(sb, 40 * sb), 8 << 30))
        cases.append((tr, limit, k, pairs))
    plans = _run(cases)
    stats = [_verify(c, r) for c, r in zip(cases, plans)]
    for c, r in zip(cases, plans):
        _check_order(c, r)
    assert min(s[0] for s in stats) == 1 and max(s[0] for s in stats) >= 10
