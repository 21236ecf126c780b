"""bench.py as the driver runs it, on the GPU: a plain run reports the headline alone and
`--steps` timed steps, `--dump-outputs` writes the headers of the last timed fill.  Two short
runs with the same arguments must dump identical arrays."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ("align_costs", "golden_match", "fill_10k_full", "fill_100k_full", "config4", "config4_rank_share",
             "full_batch", "config5", "cpu_baseline")


def _bench(args):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "GSA_BENCH_REHEARSE")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])


@pytest.mark.gpu
def test_plain_run_is_the_headline_alone_and_dumps_its_outputs(tmp_path):
    d1, d2 = str(tmp_path / "d1"), str(tmp_path / "d2")
    j = _bench(["--gpus", "1", "--steps", "2", "--warmup", "1", "--dump-outputs", d1])
    assert j["steps"] == 2 and j["warmup"] == 1 and j["unit"] == "GCUPS" and j["dtype"] == "int32"
    assert j["higher_is_better"] is True and j["ms_per_step"] > 0
    cells = j["config"]["R"] * j["config"]["C"]
    assert j["value"] == pytest.approx(cells / (j["ms_per_step"] * 1e-3) / 1e9, rel=1e-3)
    assert not [k for k in FULL_ONLY if k in j]
    _bench(["--gpus", "1", "--steps", "3", "--warmup", "0", "--dump-outputs", d2])
    total = 0
    for name in ("hrow", "hcol"):
        a, b = np.load(os.path.join(d1, name + ".npy")), np.load(os.path.join(d2, name + ".npy"))
        total += os.path.getsize(os.path.join(d1, name + ".npy"))
        assert a.dtype == np.float64 and a.size > 0 and np.array_equal(a, b)
        assert np.count_nonzero(a) > 0.99 * a.size  # scores, not an untouched buffer
    assert sorted(os.listdir(d1)) == ["hcol.npy", "hrow.npy"] and total <= 64 * 10**6
