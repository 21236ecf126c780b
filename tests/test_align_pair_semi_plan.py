"""The host plan of gsa_align_pair_semi_dev (gpuseqalign_amd/csrc/nw_pair_semi_plan.h),
checked on the CPU.  tests/align_pair_semi_plan_driver.cpp, a stand-alone program over the header, is
compiled once with the host compiler and run as a child process: the window jW on hand-computed cases
and the chunks' widths.  Then the window's exactness, with no GPU and no library: on a few hundred
random pairs the matrices are filled again with column jW forced to minus infinity below row 0, and
the walk over them must give tests/_semi_oracle.py's alignment, with j_start > jW whenever jW > 0."""
import os
import subprocess
import tempfile

import numpy as np

from tests import _semi_oracle as so

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_EXE = {}


def _driver():
    if "exe" not in _EXE:
        d = tempfile.mkdtemp(prefix="pair_semi_plan_")
        exe = os.path.join(d, "plan_driver")
        cc = os.environ.get("CC")
        cmd = [cc] if cc else ["c++"]
        subprocess.check_call(cmd + ["-std=c++17", "-O1", "-x", "c++", "-I", os.path.join(ROOT, "gpuseqalign_amd", "csrc"),
                                     os.path.join(ROOT, "tests", "align_pair_semi_plan_driver.cpp"), "-o", exe, "-lstdc++"])
        _EXE["exe"] = exe
    return _EXE["exe"]


def _run(cases):
    """Per case (TR, R, jEnd, S, pmax, gape, limit, seed): {"strips", "jW", "chunks", "nofit"}."""
    text = "".join("%d %d %d %d %d %d %d %d\n" % c for c in cases)
    p = subprocess.run([_driver()], input=text, capture_output=True, text=True, check=True)
    plans, cur = [], None
    for line in p.stdout.split("\n"):
        f = line.split()
        if not f:
            continue
        v = [int(x) for x in f[1:]]
        if f[0] == "plan":
            cur = {"strips": v[0], "jW": v[1], "chunks": [], "nofit": None}
        elif f[0] == "chunk":
            cur["chunks"].append(dict(zip(("tLo", "tHi", "W", "stripBytes", "codeBytes", "stop"), v)))
        elif f[0] == "nofit":
            cur["nofit"] = tuple(v)
        else:
            plans.append(cur)
    assert len(plans) == len(cases), p.stderr
    return plans


BIG = 2 << 30


def test_window_on_hand_computed_cases():
    # (TR, R, jEnd, S, pmax, gape, limit, seed) -> jW
    cases = [
        # a perfect 300-letter match at 11 a letter: S = 3300, no room for a 'D': jW = 5000 - 300 - 0 - 1
        ((512, 300, 5000, 3300, 11, -1, BIG, 1), 4699),
        # 100 below the best possible at -1 a letter: dmax = 100
        ((512, 300, 5000, 3200, 11, -1, BIG, 1), 4599),
        # the same at -2: dmax = 50; at -3: floor(100 / 3) = 33
        ((512, 300, 5000, 3200, 11, -2, BIG, 1), 4649),
        ((512, 300, 5000, 3200, 11, -3, BIG, 1), 4666),
        # gape = 0: no bound on the 'D' letters
        ((512, 300, 5000, 3300, 11, 0, BIG, 1), 0),
        # S < 0: dmax = (3300 + 40) / 1 = 3340, jW = 5000 - 300 - 3340 - 1
        ((512, 300, 5000, -40, 11, -1, BIG, 1), 1359),
        # a window that would begin left of column 0
        ((512, 300, 250, 3300, 11, -1, BIG, 1), 0),
        ((512, 300, 301, 3300, 11, -1, BIG, 1), 0),
        ((512, 300, 302, 3300, 11, -1, BIG, 1), 1),
        # an all-negative table: pmax = 0, S = -500: dmax = 500 / 4 = 125
        ((1024, 100, 9000, -500, 0, -4, BIG, 1), 8774),
        # a score too low to bound anything within the subject
        ((1024, 100, 9000, -40000, 0, -4, BIG, 1), 0),
    ]
    plans = _run([c for c, _ in cases])
    assert [p["jW"] for p in plans] == [w for _, w in cases]
    for (c, w), p in zip(cases, plans):
        # one chunk of every strip, its width j_end - jW
        assert p["nofit"] is None and len(p["chunks"]) == 1 and p["chunks"][0]["W"] == c[2] - w
        assert p["chunks"][0]["stripBytes"] == (c[2] - w) * c[0] // 2


def _verify(case, plan):
    tr, R, j_end, S, pmax, ge, limit, _ = case
    strips = -(-R // tr)
    jW = plan["jW"]
    dmax = (pmax * R - S) // -ge if ge < 0 else None
    assert jW == (0 if ge == 0 else max(0, j_end - R - dmax - 1)) and 0 <= jW < j_end
    assert plan["strips"] == strips
    if (j_end - jW) * (tr // 2) > limit:
        assert plan["chunks"] == [] and plan["nofit"] == (strips - 1, (j_end - jW) * (tr // 2))
        return 0
    hi, W = strips - 1, j_end - jW
    for c in plan["chunks"]:
        assert c["tHi"] == hi and 0 <= c["tLo"] <= c["tHi"] and 1 <= c["W"] <= W
        n = c["tHi"] - c["tLo"] + 1
        assert c["stripBytes"] == c["W"] * (tr // 2) and c["codeBytes"] == n * c["stripBytes"] <= limit
        assert c["tLo"] == 0 or (n + 1) * c["stripBytes"] > limit  # greedy
        assert c["stop"] == c["tLo"] * tr
        hi, W = c["tLo"] - 1, c["W"]
    assert hi == -1  # every strip up to strip 0: the path always reaches row 0
    assert plan["chunks"][0]["W"] == j_end - jW
    return len(plan["chunks"])


def test_chunk_widths_on_seeded_plans():
    import random
    rng = random.Random(9)
    cases = []
    for k in range(1500):
        tr = rng.choice((512, 1024))
        R, j_end = rng.randint(1, 12 * tr), rng.randint(1, 200000)
        pmax, ge = rng.choice((0, 5, 11)), rng.choice((0, -1, -2, -11))
        S = rng.randint(-3 * R, pmax * R)
        jW = 0 if ge == 0 else max(0, j_end - R - (pmax * R - S) // -ge - 1)
        sb = (j_end - jW) * (tr // 2)
        cases.append((tr, R, j_end, S, pmax, ge, rng.choice((BIG, rng.randint(max(1, sb // 2), 6 * sb))), k))
    counts = [_verify(c, p) for c, p in zip(cases, _run(cases))]
    assert 0 in counts and 1 in counts and max(counts) >= 4


# -- the window is exact ------------------------------------------------------------------------------

NEG = so.NEG


def _fill_windowed(y, x, sub, go, ge, jW):
    """The oracle's matrices for the columns jW ... C with column jW minus infinity below row 0."""
    R, C = len(y) - 1, len(x) - 1
    H = np.full((R + 1, C + 1), NEG, np.int64)
    E = np.full((R + 1, C + 1), NEG, np.int64)
    F = np.full((R + 1, C + 1), NEG, np.int64)
    H[0, :] = 0
    for i in range(1, R + 1):
        if jW == 0:
            H[i, 0] = F[i, 0] = go + (i - 1) * ge
        for j in range(jW + 1, C + 1):
            E[i, j] = max(E[i, j - 1] + ge, H[i, j - 1] + go)
            F[i, j] = max(F[i - 1, j] + ge, H[i - 1, j] + go)
            H[i, j] = max(H[i - 1, j - 1] + sub[y[i], x[j]], E[i, j], F[i, j])
    return H, E, F


def _walk(y, x, sub, go, ge, H, E, F, j_end, jW):
    """The oracle's walk from (R, j_end); it must never stand on column jW > 0 below row 0."""
    i, j, state, ops = len(y) - 1, j_end, "H", []
    while i > 0:
        assert not (jW > 0 and j <= jW), (i, j, jW)
        if state == "H":
            h = int(H[i, j])
            if j > 0 and h == int(H[i - 1, j - 1]) + int(sub[y[i], x[j]]):
                ops.append("=" if y[i] == x[j] else "X")
                i, j = i - 1, j - 1
            elif h == int(F[i, j]):
                state = "F"
            else:
                assert j > 0 and h == int(E[i, j]), (i, j, h)
                state = "E"
        elif state == "F":
            ops.append("I")
            state = "F" if int(F[i - 1, j]) + ge > int(H[i - 1, j]) + go else "H"
            i -= 1
        else:
            ops.append("D")
            state = "E" if int(E[i, j - 1]) + ge > int(H[i, j - 1]) + go else "H"
            j -= 1
    return j, so._fold(ops[::-1])


def test_window_is_exact_on_random_pairs():
    rng = np.random.default_rng(11)
    tables = {2: [np.array([[2, -3], [-3, 2]]), np.array([[1, -1], [-1, 1]]), np.array([[3, 0], [-2, 1]])],
              4: [np.where(np.eye(4, dtype=bool), 5, -4), rng.integers(-3, 4, (4, 4)), np.full((4, 4), -2)]}
    windows = 0
    for n in range(300):
        alpha = (2, 4)[n % 2]
        sub = tables[alpha][(n // 2) % 3]
        go, ge = [(-11, -1), (-4, -4), (-5, -2), (0, 0), (-7, 0)][n % 5]
        R, C = int(rng.integers(1, 41)), int(rng.integers(1, 151))
        y = np.concatenate([[0], rng.integers(0, alpha, R)]).astype(np.int32)
        x = np.concatenate([[0], rng.integers(0, alpha, C)]).astype(np.int32)
        if n % 3 and C > R:  # the query planted, lightly mutated, so that the score is high and the window narrow
            at = int(rng.integers(0, C - R + 1))
            y[1:] = x[1 + at:1 + at + R]
            flip = rng.random(R) < 0.1
            y[1:][flip] = rng.integers(0, alpha, int(flip.sum()))
        want = so.align(y, x, sub, go, ge)
        S, j_end = want[0], want[4]
        pmax = max(0, int(sub.max()))
        jW = 0 if ge == 0 else max(0, j_end - R - (pmax * R - S) // -ge - 1)
        if j_end == 0:
            continue
        H, E, F = _fill_windowed(y, x, sub, go, ge, jW)
        assert int(H[R, j_end]) == S
        j_start, cigar = _walk(y, x, sub, go, ge, H, E, F, j_end, jW)
        assert (S, 0, j_start, R, j_end, cigar) == want, (n, jW, want)
        if jW > 0:
            windows += 1
            assert j_start > jW
    assert windows >= 40
