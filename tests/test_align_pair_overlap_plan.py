"""The host plan of gsa_align_pair_overlap_dev (gpuseqalign_amd/csrc/nw_pair_overlap_plan.h; DESIGN.md
2.2m), checked on the CPU.  tests/align_pair_overlap_plan_driver.cpp, a stand-alone program over the
header, is compiled once with the host compiler and run as a child process: the strips of an end cell and
the chunks on hand-computed cases, then the plan's properties on seeded cases -- bottom-up from i_end's
strip, greedy under the limit, each chunk no wider than the column where the walk left the one below,
nothing planned once the walk stands on a border."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_EXE = {}
BIG = 2 << 30


def _driver():
    if "exe" not in _EXE:
        d = tempfile.mkdtemp(prefix="pair_overlap_plan_")
        exe = os.path.join(d, "plan_driver")
        cc = os.environ.get("CC")
        cmd = [cc] if cc else ["c++"]
        subprocess.check_call(cmd + ["-std=c++17", "-O1", "-x", "c++", "-I", os.path.join(ROOT, "gpuseqalign_amd", "csrc"),
                                     os.path.join(ROOT, "tests", "align_pair_overlap_plan_driver.cpp"), "-o", exe, "-lstdc++"])
        _EXE["exe"] = exe
    return _EXE["exe"]


def _run(cases):
    """Per case (TR, iEnd, jEnd, limit, seed): {"strips", "end_strip", "chunks", "walks", "nofit"}."""
    text = "".join("%d %d %d %d %d\n" % c for c in cases)
    p = subprocess.run([_driver()], input=text, capture_output=True, text=True, check=True)
    plans, cur = [], None
    for line in p.stdout.split("\n"):
        f = line.split()
        if not f:
            continue
        v = [int(x) for x in f[1:]]
        if f[0] == "plan":
            cur = {"strips": v[0], "end_strip": v[1], "chunks": [], "walks": [], "nofit": None}
        elif f[0] == "chunk":
            cur["chunks"].append(dict(zip(("tLo", "tHi", "J", "stripBytes", "codeBytes", "stop"), v)))
        elif f[0] == "walk":
            cur["walks"].append(tuple(v))
        elif f[0] == "nofit":
            cur["nofit"] = tuple(v)
        else:
            plans.append(cur)
    assert len(plans) == len(cases), p.stderr
    return plans


def test_hand_computed_cases():
    cases = [
        # an end cell on row 1300 at column 700, TR = 512: rows 1 ... 1300 lie in 3 strips; all fit one chunk
        (512, 1300, 700, BIG, 1),
        # the same under a limit of one strip's codes, 700 x 256 bytes: the first chunk is strip 2 alone
        (512, 1300, 700, 700 * 256, 1),
        # two strips' codes and one byte: strips 1 and 2
        (512, 1300, 700, 2 * 700 * 256 + 1, 1),
        # one byte short of a strip
        (512, 1300, 700, 700 * 256 - 1, 1),
        # an end cell on column C above row R: row 512 is the last row of strip 0, row 513 the first of strip 1
        (512, 512, 90, BIG, 1),
        (512, 513, 90, BIG, 1),
        (1024, 1, 1, 512, 1),
    ]
    plans = _run(cases)
    assert [(p["strips"], p["end_strip"]) for p in plans] == [(3, 2), (3, 2), (3, 2), (3, 2), (1, 0), (2, 1), (1, 0)]
    first = [p["chunks"][0] if p["chunks"] else None for p in plans]
    assert first[0] == dict(tLo=0, tHi=2, J=700, stripBytes=179200, codeBytes=537600, stop=0)
    assert first[1] == dict(tLo=2, tHi=2, J=700, stripBytes=179200, codeBytes=179200, stop=1024)
    assert first[2] == dict(tLo=1, tHi=2, J=700, stripBytes=179200, codeBytes=358400, stop=512)
    assert first[3] is None and plans[3]["nofit"] == (2, 179200)
    assert first[4] == dict(tLo=0, tHi=0, J=90, stripBytes=23040, codeBytes=23040, stop=0)
    assert first[5] == dict(tLo=0, tHi=1, J=90, stripBytes=23040, codeBytes=46080, stop=0)
    assert first[6] == dict(tLo=0, tHi=0, J=1, stripBytes=512, codeBytes=512, stop=0)
    # a chunk that reaches strip 0 is the last one whatever the walk does
    for p in (plans[0], plans[4], plans[5], plans[6]):
        assert len(p["chunks"]) == 1 and p["nofit"] is None


def _verify(case, plan):
    tr, i_end, j_end, limit, _ = case
    assert plan["strips"] == -(-i_end // tr) and plan["end_strip"] == plan["strips"] - 1
    if j_end * (tr // 2) > limit:
        assert plan["chunks"] == [] and plan["nofit"] == (plan["end_strip"], j_end * (tr // 2))
        return 0, False
    assert plan["nofit"] is None and len(plan["walks"]) == len(plan["chunks"]) >= 1
    hi, J = plan["end_strip"], j_end
    stopped_early = False
    for n, (c, (wi, wj)) in enumerate(zip(plan["chunks"], plan["walks"])):
        assert c["tHi"] == hi and 0 <= c["tLo"] <= c["tHi"] and c["J"] == J >= 1
        k = c["tHi"] - c["tLo"] + 1
        assert c["stripBytes"] == J * (tr // 2) and c["codeBytes"] == k * c["stripBytes"] <= limit
        assert c["tLo"] == 0 or (k + 1) * c["stripBytes"] > limit  # greedy
        assert c["stop"] == c["tLo"] * tr
        last = n == len(plan["chunks"]) - 1
        goes_on = c["tLo"] > 0 and wi == c["stop"] and wj >= 1
        assert goes_on == (not last)
        if last and c["tLo"] > 0:
            stopped_early = True  # the walk reached column 0: the strips above are never planned
            assert wj == 0
        hi, J = c["tLo"] - 1, wj
    return len(plan["chunks"]), stopped_early


def test_seeded_plans():
    import random
    rng = random.Random(9)
    cases = []
    for k in range(1500):
        tr = rng.choice((512, 1024))
        i_end, j_end = rng.randint(1, 12 * tr), rng.randint(1, 200000)
        sb = j_end * (tr // 2)
        cases.append((tr, i_end, j_end, rng.choice((BIG, rng.randint(max(1, sb // 2), 6 * sb))), k))
    out = [_verify(c, p) for c, p in zip(cases, _run(cases))]
    counts = [n for n, _ in out]
    assert 0 in counts and 1 in counts and max(counts) >= 4
    assert sum(1 for _, early in out if early) >= 50
