"""The host plan of the banded extension calls (gpuseqalign_amd/csrc/nw_band_ext_plan.h),
checked on the CPU.  tests/band_ext_plan_driver.cpp, a stand-alone program over the header, is compiled
with the host compiler and run as a child process.  Its `check` mode checks validity, the trim, the plan
of the trimmed pair and the certificate on hand-computed cases and the trim's properties over every band
of every pair up to 24 x 24; `plan` and `cert` are compared here with Python restatements
(tests/_band_ext_oracle.py and the formulas DESIGN.md 2.2p states for the strips).  The same program is
built once more with the host sanitizers, as its own program."""
import os
import subprocess
import tempfile

import numpy as np

from tests import _band_ext_oracle as eo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_EXE = {}
KR, TR, NWV, LAG = 4, 256, 16, 6
LIMIT = 64 * NWV * LAG - TR + 1 - 63


def _driver(sanitize=False):
    key = "san" if sanitize else "exe"
    if key not in _EXE:
        d = tempfile.mkdtemp(prefix="band_ext_plan_")
        exe = os.path.join(d, "plan_driver")
        cc = os.environ.get("CC")
        cmd = [cc] if cc else ["c++"]
        flags = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else []
        subprocess.check_call(cmd + ["-std=c++17", "-O1", "-x", "c++"] + flags +
                              ["-I", os.path.join(ROOT, "gpuseqalign_amd", "csrc"),
                               os.path.join(ROOT, "tests", "band_ext_plan_driver.cpp"), "-o", exe, "-lstdc++"])
        _EXE[key] = exe
    return _EXE[key]


def _check(sanitize):
    p = subprocess.run([_driver(sanitize), "check"], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    f = p.stdout.split()
    assert f[:2] == ["check", "ok"], p.stdout
    return dict(zip(f[2::2], (int(v) for v in f[3::2])))


def test_self_checks():
    out = _check(False)
    # seven checks on each of the (R + 3) (C + 3) bands of every pair with R, C <= 24, and the hand-computed ones
    assert out["max_width"] == LIMIT and out["checks"] > 7 * sum(R + 3 for R in range(1, 25)) ** 2


def test_self_checks_under_the_host_sanitizers():
    assert _check(True) == _check(False)


def _plan(R, C, lo, hi):
    p = subprocess.run([_driver(), "plan", str(R), str(C), str(lo), str(hi)], capture_output=True, text=True, check=True)
    f = p.stdout.split()
    if f[0] == "refused":
        return {"valid": int(f[2])}
    return dict(zip(("Ru", "Cu", "lo", "hi", "W", "Wc", "strips", "waves", "nq", "T", "stripBytes", "codeBytes"),
                    (int(v) for v in f[1:])))


def _want(R, C, lo, hi):
    Ru, Cu = eo.trim(R, C, lo, hi)
    clo, chi = eo.clamp(R, C, lo, hi)
    W = chi - clo + 1
    strips = -(-Ru // TR)
    nq = -(-(W + TR - 1 + 63) // 64)
    return dict(Ru=Ru, Cu=Cu, lo=clo, hi=chi, W=W, Wc=W + TR - 1, strips=strips, waves=min(NWV, strips), nq=nq,
                T=(strips - 1) * LAG + nq, stripBytes=(W + TR - 1) * TR // 2, codeBytes=strips * (W + TR - 1) * TR // 2)


def test_plans_against_the_stated_formulas():
    rng = np.random.default_rng(21)
    seen = {"trimR": 0, "trimC": 0, "wide": 0, "invalid": 0}
    for k in range(80):
        R, C = int(rng.integers(1, 40000)), int(rng.integers(1, 40000))
        lo, hi = -int(rng.integers(0, 3000)), int(rng.integers(0, 3000))
        if k % 10 == 0:
            lo, hi = [(1, 5), (-5, -1), (3, 2)][(k // 10) % 3]
        if k % 10 == 5:  # wider than the limit, on a pair that does not clamp it
            R, C, lo, hi = R + 4000, C + 4000, -int(rng.integers(2900, 3200)), int(rng.integers(2927, 3200))
        p = _plan(R, C, lo, hi)
        if not eo.valid(lo, hi):
            assert p == {"valid": 0}
            seen["invalid"] += 1
            continue
        w = _want(R, C, lo, hi)
        if w["W"] > LIMIT:
            assert p == {"valid": 1}
            seen["wide"] += 1
            continue
        assert p == w, (R, C, lo, hi)
        seen["trimR"] += w["Ru"] < R
        seen["trimC"] += w["Cu"] < C
    assert min(seen.values()) >= 3, seen
    # the issue's trimming case: one strip of 120 rows
    assert _plan(3 * TR, 100, -20, 5) == _want(3 * TR, 100, -20, 5)
    assert _plan(3 * TR, 100, -20, 5)["strips"] == 1 and _plan(3 * TR, 100, -20, 5)["Ru"] == 120
    # far outside: clamped
    assert _plan(300, 200, -10 ** 12, 10 ** 12) == _want(300, 200, -300, 200)
    # an empty side is the host's
    assert _plan(0, 5, 0, 3) == {"valid": 1} and _plan(5, 0, -3, 0) == {"valid": 1}


def test_certificate_agrees_with_the_oracle_restatement():
    rng = np.random.default_rng(22)
    ones = 0
    for _ in range(60):
        R, C = int(rng.integers(1, 300)), int(rng.integers(1, 300))
        lo, hi = eo.clamp(R, C, -int(rng.integers(0, 40)), int(rng.integers(0, 40)))
        pmax, go = int(rng.integers(0, 6)), -int(rng.integers(0, 12))
        ge = -int(rng.integers(0, -go + 1))
        for S in (int(rng.integers(0, 600)), 0, 10 ** 6):
            p = subprocess.run([_driver(), "cert"] + [str(v) for v in (R, C, lo, hi, pmax, go, ge, S)],
                               capture_output=True, text=True, check=True)
            sub = np.array([[pmax, -1], [-1, -3]])
            want = eo.certificate(R, C, lo, hi, sub, go, ge, S)
            ones += want
            assert p.stdout.split() == ["cert", str(want)]
    assert 30 < ones < 170
