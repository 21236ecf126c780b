"""The host plan of gsa_score_band_batch_dev / gsa_align_batch_band_dev (gpuseqalign_amd/csrc/
nw_band_batch_plan.h), checked on the CPU.  tests/band_batch_plan_driver.cpp, a stand-alone
program over the header, is compiled with the host compiler and run as a child process.  Its `schedule`
mode simulates a pair's lockstep super-steps on workgroups of 4, 8 and 16 waves at each count's width
limit, one diagonal below it and one above (refused with more strips than waves), at the widths whose chain
length sits on either side of a multiple of 64, for 1, 2, nwv, nwv + 1 and 3 nwv + 1 strips, and checks
itself that every ring entry a consumer reads unmasked -- the diagonal's cell included -- was written by
the producer strip in a strictly earlier super-step, that no wave holds two strips at once and that T ends
with the last strip; then the waves rule, the claim order and the round plan.  The same program is built
once more with the host sanitizers, as its own program.  The Python restatement the GPU tests use
(tests/_band_batch_cases.py) is checked against the header through the driver's other modes."""
import os
import subprocess
import tempfile

import numpy as np

from tests import _band_batch_cases as bc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_EXE = {}
TR, LAG = 256, 6


def _driver(sanitize=False):
    key = "san" if sanitize else "exe"
    if key not in _EXE:
        d = tempfile.mkdtemp(prefix="band_batch_plan_")
        exe = os.path.join(d, "plan_driver")
        cc = os.environ.get("CC")
        cmd = [cc] if cc else ["c++"]
        flags = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else []
        subprocess.check_call(cmd + ["-std=c++17", "-O1", "-x", "c++"] + flags +
                              ["-I", os.path.join(ROOT, "gpuseqalign_amd", "csrc"),
                               os.path.join(ROOT, "tests", "band_batch_plan_driver.cpp"), "-o", exe, "-lstdc++"])
        _EXE[key] = exe
    return _EXE[key]


def _schedule(sanitize):
    p = subprocess.run([_driver(sanitize), "schedule"], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    f = p.stdout.split()
    assert f[:2] == ["schedule", "ok"], p.stdout
    return dict(zip(f[2::2], (int(v) for v in f[3::2])))


def test_schedule_simulation_on_4_8_and_16_waves():
    out = _schedule(False)
    # per count: three residues of 64 over the widths up to its limit, five strip counts each
    want = sum(3 * ((64 * w * LAG - TR - 62) // 64) for w in bc.WAVES) * 5
    assert out["sims"] >= want and out["checks"] > 10 ** 7


def test_schedule_simulation_under_the_host_sanitizers():
    assert _schedule(True) == _schedule(False)


def _rounds(limit, code_bytes):
    p = subprocess.run([_driver(), "rounds", str(limit)] + [str(b) for b in code_bytes], capture_output=True, text=True,
                       check=True)
    f = p.stdout.split()
    assert f[0] == "rounds" and f[2] == "peak" and f[4] == "of"
    return int(f[1]), int(f[3]), [int(v) for v in f[5:]]


def test_round_plan_restatement_agrees_with_the_header():
    rng = np.random.default_rng(5)
    for _ in range(60):
        n = int(rng.integers(0, 14))
        limit = int(rng.integers(1, 5000))
        code_bytes = [int(v) for v in rng.integers(-300, 5200, size=n)]
        if n > 2:
            code_bytes[0], code_bytes[1] = limit, limit + 1
        rounds, round_of, peak = bc.plan_rounds(code_bytes, limit)
        assert _rounds(limit, code_bytes) == (len(rounds), peak, round_of)
        # every pair in exactly one place, no round over the limit
        assert sorted(p for r in rounds for p in r) == [p for p, b in enumerate(code_bytes) if 0 <= b <= limit]
        assert all(sum(code_bytes[p] for p in r) <= limit for r in rounds)
    # one pair: the single call's plan
    assert _rounds(4096, [4096]) == (1, 4096, [0]) and _rounds(4095, [4096]) == (0, 0, [-2])
    # the limit the sum of all: one round; the largest pair's bytes exactly: every pair in some round
    assert _rounds(60, [10, 20, 30]) == (1, 60, [0, 0, 0])
    assert _rounds(30, [10, 20, 30]) == (2, 30, [1, 1, 0])
    assert _rounds(29, [10, 20, 30]) == (2, 20, [1, 0, -2])


def _waves(forced, pairs):
    args = [str(v) for sn in pairs for v in sn]
    p = subprocess.run([_driver(), "waves", str(forced)] + args, capture_output=True, text=True, check=True)
    f = p.stdout.split()
    assert f[0] == "waves"
    return int(f[1])


def test_waves_rule_restatement_agrees_with_the_header():
    rng = np.random.default_rng(6)
    limits = {w: 64 * w * LAG - TR + 1 - 63 for w in bc.WAVES}
    assert limits == {4: 1218, 8: 2754, 16: 5826}
    for w, lim in limits.items():
        assert bc.nq_of(lim) == w * LAG and bc.nq_of(lim + 1) == w * LAG + 1
        # at the limit the count serves any number of strips; one diagonal more only pairs of no more strips than waves
        assert _waves(0, [(w + 1, bc.nq_of(lim))]) == w == _waves(w, [(3 * w + 1, bc.nq_of(lim))])
        assert _waves(w, [(w + 1, bc.nq_of(lim + 1))]) == 0 and _waves(w, [(w, bc.nq_of(lim + 1))]) == w
    for _ in range(60):
        pairs = [(int(rng.integers(1, 40)), bc.nq_of(int(rng.integers(1, 5827)))) for _ in range(int(rng.integers(0, 5)))]
        for forced in (0, 4, 8, 16, 5, -1):
            assert _waves(forced, pairs) == bc.pick_waves(forced, pairs), (forced, pairs)
