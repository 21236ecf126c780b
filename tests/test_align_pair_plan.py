"""The host plan of gsa_align_pair_dev (gpuseqalign_amd/csrc/nw_pair_trace_plan.h),
checked on the CPU: tests/align_pair_plan_driver.cpp, a stand-alone program over the header, is compiled
once with the host compiler and run as a child process on seeded cases; the properties the fill and the
walk rely on are asserted on the plans it prints.  No GPU and no library needed."""
import os
import subprocess
import tempfile


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_EXE = {}


def _driver():
    if "exe" not in _EXE:
        d = tempfile.mkdtemp(prefix="pair_plan_")
        exe = os.path.join(d, "plan_driver")
        cc = os.environ.get("CC")
        cmd = [cc] if cc else ["c++"]
        subprocess.check_call(cmd + ["-std=c++17", "-O1", "-x", "c++", "-I", os.path.join(ROOT, "gpuseqalign_amd", "csrc"),
                                     os.path.join(ROOT, "tests", "align_pair_plan_driver.cpp"), "-o", exe, "-lstdc++"])
        _EXE["exe"] = exe
    return _EXE["exe"]


def _run(cases):
    """Per case (TR, iEnd, jEnd, limit, seed): (strips, [chunk dicts], nofit or None)."""
    text = "".join("%d %d %d %d %d\n" % c for c in cases)
    p = subprocess.run([_driver()], input=text, capture_output=True, text=True, check=True)
    plans, cur = [], None
    for line in p.stdout.split("\n"):
        f = line.split()
        if not f:
            continue
        v = [int(x) for x in f[1:]]
        if f[0] == "plan":
            cur = {"strips": v[0], "chunks": [], "nofit": None}
        elif f[0] == "chunk":
            cur["chunks"].append(dict(zip(("tLo", "tHi", "J", "stripBytes", "codeBytes", "stop"), v), off={}))
        elif f[0] == "strip":
            cur["chunks"][-1]["off"][v[0]] = v[1]
        elif f[0] == "nofit":
            cur["nofit"] = tuple(v)
        else:
            plans.append(cur)
    assert len(plans) == len(cases), p.stderr
    return plans


def _verify(case, plan):
    tr, i_end, j_end, limit, _ = case
    strips = -(-i_end // tr)
    assert plan["strips"] == strips
    chunks = plan["chunks"]
    if j_end * (tr // 2) > limit:
        # one strip alone does not fit: nothing is planned
        assert chunks == [] and plan["nofit"] == (strips - 1, j_end * (tr // 2))
        return 0
    assert plan["nofit"] is None and chunks
    rows, hi, J = [], strips - 1, j_end
    for c in chunks:
        # bottom-up and consecutive; the column bound never grows
        assert c["tHi"] == hi and 0 <= c["tLo"] <= c["tHi"]
        assert 1 <= c["J"] <= J
        if c is chunks[0]:
            assert c["J"] == j_end
        n = c["tHi"] - c["tLo"] + 1
        assert c["stripBytes"] == c["J"] * (tr // 2) and c["codeBytes"] == n * c["stripBytes"] <= limit
        # greedy: one more strip would not fit, or there is none
        assert c["tLo"] == 0 or (n + 1) * c["stripBytes"] > limit
        # the strips' code ranges: disjoint, inside the chunk's codes
        spans = sorted((c["off"][s], c["off"][s] + c["stripBytes"]) for s in range(c["tLo"], c["tHi"] + 1))
        assert len(c["off"]) == n and spans[0][0] == 0 and spans[-1][1] == c["codeBytes"]
        assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))
        assert c["stop"] == c["tLo"] * tr
        for s in range(c["tLo"], c["tHi"] + 1):
            rows += list(range(s * tr + 1, min((s + 1) * tr, i_end) + 1))
        hi, J = c["tLo"] - 1, c["J"]
    # every row 1 ... iEnd in exactly one strip of exactly one chunk
    assert hi == -1 and sorted(rows) == list(range(1, i_end + 1))
    return len(chunks)


def _cases():
    out, seed = [], 1
    for tr in (512, 1024):
        for i_end in (1, tr - 1, tr, tr + 1, 3 * tr + 1, 9 * tr + 5):
            for j_end in (1, 65, 700):
                sb = j_end * (tr // 2)
                strips = -(-i_end // tr)
                # one chunk, about three chunks, a chunk per strip, a byte more than that, below one strip, the default
                for limit in (strips * sb, max(sb, -(-strips // 3) * sb), sb, sb + 1, 2 * sb - 1, sb - 1, 2 << 30):
                    if limit >= 1:
                        seed += 1
                        out.append((tr, i_end, j_end, limit, seed))
    return out


def test_plan_properties():
    cases = _cases()
    counts = [_verify(c, p) for c, p in zip(cases, _run(cases))]
    assert 0 in counts and 1 in counts and 3 in counts and max(counts) >= 10


def test_limits_for_one_three_and_many_chunks():
    tr, i_end, j_end = 512, 9 * 512 + 5, 700
    sb = j_end * tr // 2
    cases = [(tr, i_end, j_end, 10 * sb, 7), (tr, i_end, 1, 4 * (tr // 2), 7), (tr, i_end, j_end, sb, 7),
             (tr, i_end, j_end, sb - 1, 7)]
    plans = _run(cases)
    got = [_verify(c, p) for c, p in zip(cases, plans)]
    # all ten strips at once; J = 1 keeps every chunk at four strips: 4 + 4 + 2; one strip's codes: the
    # first chunk is one strip, the later ones as many as their fewer columns let in; no fit
    assert got[:2] == [1, 3] and 2 <= got[2] <= 10 and got[3] == 0
    assert [c["tHi"] - c["tLo"] + 1 for c in plans[1]["chunks"]] == [4, 4, 2]
    assert plans[2]["chunks"][0]["tLo"] == plans[2]["chunks"][0]["tHi"] == 9


def test_many_seeded_plans():
    import random
    rng = random.Random(5)
    cases = []
    for k in range(2000):
        tr = rng.choice((512, 1024))
        i_end, j_end = rng.randint(1, 40 * tr), rng.randint(1, 5000)
        sb = j_end * (tr // 2)
        cases.append((tr, i_end, j_end, rng.randint(max(1, sb // 2), 12 * sb), k))
    for c, p in zip(cases, _run(cases)):
        _verify(c, p)
