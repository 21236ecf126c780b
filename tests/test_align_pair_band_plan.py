"""The host plan of gsa_score_band_dev / gsa_align_pair_band_dev (gpuseqalign_amd/csrc/nw_band_plan.h;
DESIGN.md 2.2p), checked on the CPU.  tests/band_plan_driver.cpp, a stand-alone program over the header,
is compiled with the host compiler and run as a child process.  Its `schedule` mode simulates the
workgroup's lockstep super-steps for every band width whose chain length falls on either side of a
multiple of 64 and for 1, 2, NWV, NWV + 1 and 3 NWV + 1 strips, and checks itself that every column a
consumer reads was written in a strictly earlier super-step and still stands in its ring, that no wave
holds two strips at once, and that T and the bytes of codes are as stated; it also checks validity,
clamping and the certificate on hand-computed cases.  The same program is built once more with the
host sanitizers, as its own program."""
import os
import subprocess
import tempfile

import numpy as np

from tests import _band_oracle as bo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_EXE = {}
KR, TR, NWV, LAG = 4, 256, 16, 6


def _driver(sanitize=False):
    key = "san" if sanitize else "exe"
    if key not in _EXE:
        d = tempfile.mkdtemp(prefix="band_plan_")
        exe = os.path.join(d, "plan_driver")
        cc = os.environ.get("CC")
        cmd = [cc] if cc else ["c++"]
        flags = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else []
        subprocess.check_call(cmd + ["-std=c++17", "-O1", "-x", "c++"] + flags +
                              ["-I", os.path.join(ROOT, "gpuseqalign_amd", "csrc"),
                               os.path.join(ROOT, "tests", "band_plan_driver.cpp"), "-o", exe, "-lstdc++"])
        _EXE[key] = exe
    return _EXE[key]


def _schedule(sanitize):
    p = subprocess.run([_driver(sanitize), "schedule"], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    f = p.stdout.split()
    assert f[:2] == ["schedule", "ok"], p.stdout
    return dict(zip(f[2::2], (int(v) for v in f[3::2])))


def test_schedule_simulation():
    out = _schedule(False)
    # three residues of 64 over the widths up to the limit, and the few extra ones
    assert out["max_width"] == 64 * NWV * LAG - TR + 1 - 63 >= 4096
    assert out["widths"] >= 3 * (out["max_width"] // 64) and out["checks"] > 10 ** 8


def test_schedule_simulation_under_the_host_sanitizers():
    assert _schedule(True) == _schedule(False)


def _plan(R, C, lo, hi):
    p = subprocess.run([_driver(), "plan", str(R), str(C), str(lo), str(hi)], capture_output=True, text=True, check=True)
    f = p.stdout.split()
    if f == ["refused"]:
        return None
    return dict(zip(("lo", "hi", "W", "Wc", "strips", "waves", "nq", "T", "stripBytes", "codeBytes"), (int(v) for v in f[1:])))


def test_plans_against_the_stated_formulas():
    rng = np.random.default_rng(4)
    limit = 64 * NWV * LAG - TR + 1 - 63
    for _ in range(60):
        R, C = int(rng.integers(1, 40000)), int(rng.integers(1, 40000))
        k = int(rng.integers(0, 3000))
        lo, hi = min(0, C - R) - k, max(0, C - R) + int(rng.integers(0, 3000))
        p = _plan(R, C, lo, hi)
        clo, chi = bo.clamp(R, C, lo, hi)
        W = chi - clo + 1
        if W > limit:
            assert p is None
            continue
        strips = -(-R // TR)
        nq = -(-(W + TR - 1 + 63) // 64)
        assert p == dict(lo=clo, hi=chi, W=W, Wc=W + TR - 1, strips=strips, waves=min(NWV, strips), nq=nq,
                         T=(strips - 1) * LAG + nq, stripBytes=(W + TR - 1) * TR // 2,
                         codeBytes=strips * (W + TR - 1) * TR // 2)
    assert _plan(700, 1000, 0, 299) is None and _plan(700, 1000, 1, 300) is None and _plan(1000, 700, -299, 0) is None
    assert _plan(20000, 20000, -((limit - 1) // 2), limit // 2)["W"] == limit
    assert _plan(20000, 20000, -((limit - 1) // 2) - 1, limit // 2) is None
    # 32 MB of codes at 50k with 1025 diagonals
    assert _plan(50000, 50000, -512, 512)["codeBytes"] == 196 * 1280 * 128 == 32112640


def test_certificate_agrees_with_the_oracle_restatement():
    rng = np.random.default_rng(6)
    for _ in range(40):
        R, C = int(rng.integers(1, 300)), int(rng.integers(1, 300))
        k = int(rng.integers(0, 30))
        lo, hi = bo.clamp(R, C, min(0, C - R) - k, max(0, C - R) + int(rng.integers(0, 30)))
        pmax, go, ge = int(rng.integers(0, 6)), -int(rng.integers(0, 12)), 0
        ge = -int(rng.integers(0, -go + 1))
        for S in (int(rng.integers(-400, 400)), -10 ** 6, 10 ** 6):
            p = subprocess.run([_driver(), "cert"] + [str(v) for v in (R, C, lo, hi, pmax, go, ge, S)],
                               capture_output=True, text=True, check=True)
            sub = np.array([[pmax, -1], [-1, -3]])
            assert p.stdout.split() == ["cert", str(bo.certificate(R, C, lo, hi, sub, go, ge, S))]
