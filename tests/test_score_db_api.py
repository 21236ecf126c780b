"""Database search (gsa_score_db_dev), the parts that need no GPU: the entry point in the header, the
library and the ctypes bindings, its argument check without a context, the Python entry points and
the launch kind.  The kernel is checked in tests/test_gpu_score_db.py."""
import ctypes
import inspect
import os
import re

import gpuseqalign_amd as gsa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_point_declared_exported_bound():
    text = open(os.path.join(ROOT, "include", "gsa.h")).read()
    assert re.search(r"\bint\s+gsa_score_db_dev\s*\(", text)
    assert re.search(r"\bGSA_LAUNCH_SCORE_LANES\s*=\s*10\b", text)
    assert hasattr(gsa.lib(), "gsa_score_db_dev")
    res, args = gsa.SIGNATURES["gsa_score_db_dev"]
    assert res is ctypes.c_int and len(args) == 14


def test_null_context_is_invalid_value():
    off = (ctypes.c_int64 * 2)(0, 5)
    out = (gsa.ScoreResult * 1)()
    ms = ctypes.c_float(0.0)
    st = gsa.lib().gsa_score_db_dev(None, None, 10, None, off, 1, None, 25, -11, -1, 0, out, ctypes.byref(ms), None)
    assert st == gsa.NwStat.errorInvalidValue


def test_python_entry_points_exist():
    for name, params in [("score_db", ["query", "subjects", "subst", "gapo", "gape", "local"]),
                         ("score_db_dev", ["query_ptr", "adjq", "db_ptr", "db_off", "subst_ptr", "substsz", "gapo",
                                           "gape", "local", "stream"])]:
        sig = inspect.signature(getattr(gsa.Engine, name))
        assert list(sig.parameters)[1:1 + len(params)] == params, name


def test_launch_kind_and_knobs():
    assert gsa.LAUNCH_KINDS[-1] == "score_lanes" and gsa.LAUNCH_KINDS.index("score_lanes") == 10
    assert gsa.KNOB_NAMES[-2:] == ("GSA_DB_LANES", "GSA_DB_MAXC")
