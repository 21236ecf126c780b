"""The host plan of gsa_align_batch_overlap_dev (gpuseqalign_amd/csrc/nw_pair_overlap_trace_batch_plan.h;
DESIGN.md 2.2n), checked on the CPU: tests/align_batch_overlap_plan_driver.cpp, a stand-alone program over
the header, is compiled once with the host compiler and run as a child process on hand-computed and seeded
cases.  The driver checks the plan's properties itself and fails on a violation; the rounds it prints are
checked again here: every round within the limit, code ranges disjoint, every pair's strips covered
bottom-up and contiguously from i_end's strip up to where its walk ends, nothing planned below i_end's
strip or above a walk that reached column 0, every round at least one strip, the fixed order, one pair's
rounds equal to overlap_plan_chunk's chunks, and the whole again against the plan restated in
tests/_overlap_batch.py along the same paths.  No GPU and no library needed."""
import os
import random
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_EXE = {}


def _driver():
    if "exe" not in _EXE:
        d = tempfile.mkdtemp(prefix="batch_overlap_plan_")
        exe = os.path.join(d, "plan_driver")
        cc = os.environ.get("CC")
        cmd = [cc] if cc else ["c++"]
        subprocess.check_call(cmd + ["-std=c++17", "-O1", "-x", "c++", "-I", os.path.join(ROOT, "gpuseqalign_amd", "csrc"),
                                     os.path.join(ROOT, "tests", "align_batch_overlap_plan_driver.cpp"), "-o", exe, "-lstdc++"])
        _EXE["exe"] = exe
    return _EXE["exe"]


def _text(cases):
    """Cases (TR, limit, seed, [(iEnd, jEnd, iStart, jStart), ...]) as the driver reads them."""
    return "".join("%d %d %d %d\n" % (tr, limit, seed, len(pairs)) + "".join("%d %d %d %d\n" % p for p in pairs)
                   for tr, limit, seed, pairs in cases)


def _run(cases):
    """Per case: the rounds, each (bytes, [chunk dicts], {pair done in it: the cell its walk ended on})."""
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
            cur.append((v[0], [], {}))
        elif f[0] == "chunk":
            cur[-1][1].append(dict(zip(("pair", "tLo", "tHi", "J", "stripBytes", "codeBytes", "codeOff"), v)))
        elif f[0] == "done":
            cur[-1][2][v[0]] = (v[1], v[2])
        elif f[0] == "end":
            assert v[0] == len(cur)
            plans.append(cur)
        else:
            assert f[0] == "ok" and v[0] == len(cases)
    assert len(plans) == len(cases)
    return plans


def _verify(case, rounds):
    tr, limit, _, pairs = case
    end = [(ie - 1) // tr for ie, _, _, _ in pairs]
    nxt = list(end)  # the strip each pair's next chunk ends on
    width = [je for _, je, _, _ in pairs]
    done = [False] * len(pairs)
    filled = [0] * len(pairs)
    top = [None] * len(pairs)  # the highest strip filled
    for used, chunks, fin in rounds:
        assert chunks and 0 < used <= limit and used == sum(c["codeBytes"] for c in chunks)
        spans = []
        for c in chunks:
            p = c["pair"]
            assert not done[p] and c["tHi"] == nxt[p] <= end[p] and 0 <= c["tLo"] <= c["tHi"]
            assert 1 <= c["J"] <= width[p] and c["stripBytes"] == c["J"] * (tr // 2)
            n = c["tHi"] - c["tLo"] + 1
            assert c["codeBytes"] == n * c["stripBytes"]
            spans.append((c["codeOff"], c["codeOff"] + c["codeBytes"]))
            filled[p] += n
            nxt[p], width[p], top[p] = c["tLo"] - 1, c["J"], c["tLo"]
        assert len({c["pair"] for c in chunks}) == len(chunks)
        spans.sort()
        assert spans[0][0] >= 0 and spans[-1][1] <= limit and all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))
        for p, cell in fin.items():
            ie, je, i0, j0 = pairs[p]
            assert cell == (i0, j0) or (cell[1] == 0 and i0 == 0)  # on a free border
            done[p] = True
            # the chunk in which the walk ended holds the row it ended on; nothing above it is filled
            assert top[p] * tr <= cell[0] or cell[0] == 0
        # a pair not done goes on: its chunk did not hold strip 0
        for c in chunks:
            assert (c["pair"] in fin) or c["tLo"] > 0
    assert all(done)
    for p, (ie, je, i0, j0) in enumerate(pairs):
        assert filled[p] == end[p] - top[p] + 1 <= end[p] + 1  # contiguous, bottom-up, from i_end's strip
        assert top[p] * tr <= i0  # the last chunk reaches the row the walk ended on; none was planned after it
    return len(rounds), sum(filled), sum(e + 1 for e in end)


def _check_order(case, rounds):
    """The pairs that got a chunk in a round, by remaining code bytes descending (the strips left times
    the chunk's strip bytes), ties by index."""
    tr, _, _, pairs = case
    nxt = [(ie - 1) // tr for ie, _, _, _ in pairs]
    for _, chunks, _ in rounds:
        keys = [(-(nxt[c["pair"]] + 1) * c["stripBytes"], c["pair"]) for c in chunks]
        assert keys == sorted(keys), keys
        for c in chunks:
            nxt[c["pair"]] = c["tLo"] - 1


def _restated(case, rounds):
    """tests/_overlap_batch.py's plan_rounds along the columns the driver's walks took: a path per pair
    made of its cells on the chunk boundaries."""
    from tests._overlap_batch import plan_rounds
    tr, limit, _, pairs = case
    cells = [[] for _ in pairs]
    # the boundary cells: where each pair's next chunk starts (its J on row tLo TR of the chunk before)
    seen = [None] * len(pairs)
    for _, chunks, fin in rounds:
        for c in chunks:
            p = c["pair"]
            if seen[p] is not None:
                cells[p].append((seen[p] * tr, c["J"]))
            seen[p] = c["tLo"]
        for p, cell in fin.items():
            if cell[0] == seen[p] * tr and seen[p] > 0:
                cells[p].append(cell)  # ended on the boundary itself, on column 0
    items = [(ie, je, cells[p]) for p, (ie, je, _, _) in enumerate(pairs)]
    got = plan_rounds(tr, limit, items)
    assert got == (len(rounds), sum(c["tHi"] - c["tLo"] + 1 for _, ch, _ in rounds for c in ch), max(u for u, _, _ in rounds))


def test_hand_computed_rounds():
    """TR = 1024 (512 bytes a column and strip).  Pair 0 ends on column C at row 900 of a long Y: one strip,
    whatever R is.  Pair 1 ends on row 5 TR and starts on column 0 at row 3 TR + 7: strips 4 and 3 are
    filled, strips 0 ... 2 never.  Pair 2 is a containment from row 0 to row 2 TR."""
    tr = 1024
    pairs = [(900, 1000, 0, 100), (5 * tr, 1000, 3 * tr + 7, 0), (2 * tr, 600, 0, 10)]
    sb = 1000 * 512
    case = (tr, sb, 1, pairs)  # one strip of the widest pairs per round
    [rounds] = _run([case])
    _verify(case, rounds)
    _check_order(case, rounds)
    first = rounds[0]
    assert [(c["pair"], c["tLo"], c["tHi"], c["J"], c["codeOff"]) for c in first[1]] == [(1, 4, 4, 1000, 0)]
    by = {p: [(c["tLo"], c["tHi"]) for _, ch, _ in rounds for c in ch if c["pair"] == p] for p in range(3)}
    assert by[0] == [(0, 0)] and by[1] == [(4, 4), (3, 3)] and by[2][0] == (1, 1) and by[2][-1] == (0, 0)
    assert [f[1] for _, _, f in rounds if 1 in f] == [(3 * tr + 7, 0)]
    # the default limit: everything in one round, in the fixed order, back to back; pair 1 fills all five strips
    case = (tr, 8 << 30, 2, pairs)
    [rounds] = _run([case])
    _verify(case, rounds)
    assert len(rounds) == 1 and sorted(rounds[0][2]) == [0, 1, 2]
    assert [(c["pair"], c["tLo"], c["tHi"], c["J"], c["codeOff"]) for c in rounds[0][1]] == [
        (1, 0, 4, 1000, 0), (2, 0, 1, 600, 5 * sb), (0, 0, 0, 1000, 5 * sb + 2 * 600 * 512)]


def _chunks_of_one(tr, i_end, j_end, limit, cols):
    """nw_pair_overlap_plan.h's chunks of one pair, with the walk leaving chunk k at column cols[k]."""
    out, hi, J, k = [], (i_end - 1) // tr, j_end, 0
    while True:
        sb = J * (tr // 2)
        n = min(limit // sb, hi + 1)
        out.append((hi + 1 - n, hi, J))
        if k >= len(cols):
            return out
        hi, J, k = hi - n, cols[k], k + 1


def test_one_pair_is_the_single_pair_plan():
    rng = random.Random(3)
    cases = []
    for k in range(300):
        tr = rng.choice((512, 1024))
        i_end, j_end = rng.randint(1, 70000), rng.randint(1, 70000)
        start = (0, rng.randint(0, j_end - 1)) if rng.random() < 0.5 else (rng.randint(0, i_end - 1), 0)
        sb = j_end * (tr // 2)
        cases.append((tr, rng.randint(sb, 12 * sb), k, [(i_end, j_end) + start]))
    many = 0
    for case, rounds in zip(cases, _run(cases)):
        _verify(case, rounds)
        _restated(case, rounds)
        tr, limit, _, [(i_end, j_end, _, _)] = case
        got = [(c["tLo"], c["tHi"], c["J"]) for _, [c], _ in rounds]
        assert all(c["codeOff"] == 0 for _, [c], _ in rounds)
        assert got == _chunks_of_one(tr, i_end, j_end, limit, [c[2] for c in got[1:]])
        many += len(rounds) >= 3
    assert many >= 20


def test_many_seeded_batches():
    rng = random.Random(11)
    cases = []
    for k in range(1500):
        tr = rng.choice((512, 1024))
        n = rng.randint(1, 40)
        top = rng.choice((300, 3000, 70000))
        pairs = []
        for _ in range(n):
            i_end, j_end = rng.randint(1, top), rng.randint(1, top)
            # start cells on row 0 and on column 0 at random heights
            start = (0, rng.randint(0, j_end - 1)) if rng.random() < 0.5 else (rng.randint(0, i_end - 1), 0)
            pairs.append((i_end, j_end) + start)
        sb = max(j for _, j, _, _ in pairs) * (tr // 2)
        limit = rng.choice((sb, sb + 1, 2 * sb, rng.randint(sb, 40 * sb), 8 << 30))
        cases.append((tr, limit, k, pairs))
    plans = _run(cases)
    stats = [_verify(c, r) for c, r in zip(cases, plans)]
    for c, r in zip(cases, plans):
        _check_order(c, r)
        _restated(c, r)
    assert min(s[0] for s in stats) == 1 and max(s[0] for s in stats) >= 10
    assert sum(s[1] < s[2] for s in stats) >= 100  # strips above a walk that reached column 0 are never filled
