"""Many queries against one database (gsa_score_db_multi_dev), the parts that need no GPU: the entry
point in the header, the library and the ctypes bindings, its argument check without a context, the
Python entry points, and that it adds no launch kind and no knob.  The kernel is checked in
tests/test_gpu_score_db_multi.py."""
import ctypes
import inspect
import os
import re

import numpy as np

import gpuseqalign_amd as gsa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_point_declared_exported_bound():
    text = open(os.path.join(ROOT, "include", "gsa.h")).read()
    assert re.search(r"\bint\s+gsa_score_db_multi_dev\s*\(", text)
    assert hasattr(gsa.lib(), "gsa_score_db_multi_dev")
    res, args = gsa.SIGNATURES["gsa_score_db_multi_dev"]
    assert res is ctypes.c_int and len(args) == 20
    decl = re.search(r"int\s+gsa_score_db_multi_dev\s*\((.*?)\)\s*;", text, re.S).group(1)
    assert len(decl.split(",")) == 20


def test_structures_match_the_header():
    assert ctypes.sizeof(gsa.DbHit) == 16
    assert [n for n, _ in gsa.DbHit._fields_] == ["subject", "score", "i_end", "j_end"]
    assert gsa.DB_HIT_DTYPE.itemsize == 16 and list(gsa.DB_HIT_DTYPE.names) == [n for n, _ in gsa.DbHit._fields_]
    text = open(os.path.join(ROOT, "include", "gsa.h")).read()
    body = re.search(r"typedef struct gsa_score_db_multi_info\s*\{(.*?)\}\s*gsa_score_db_multi_info;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    ctype = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "float": ctypes.c_float}
    fields = []
    for t, names in re.findall(r"\b(int32_t|int64_t|float)\s+([^;]+);", body):
        fields += [(n.strip(), ctype[t]) for n in names.split(",")]
    assert fields == list(gsa.ScoreDbMultiInfo._fields_)


def test_null_context_is_invalid_value():
    off = (ctypes.c_int64 * 2)(0, 5)
    scores = (ctypes.c_int32 * 1)()
    info = gsa.ScoreDbMultiInfo()
    ms = ctypes.c_float(0.0)
    st = gsa.lib().gsa_score_db_multi_dev(None, None, off, 1, None, off, 1, None, 25, -11, -1, 0, 0, 0, 0, scores, None,
                                          ctypes.byref(info), ctypes.byref(ms), None)
    assert st == gsa.NwStat.errorInvalidValue


def test_python_entry_points_exist():
    want = [("score_db_multi_dev", ["queries_ptr", "q_off", "db_ptr", "db_off", "subst_ptr", "substsz", "gapo", "gape",
                                    "local", "top", "want_scores", "max_workgroups", "scratch_limit", "stream"]),
            ("score_db_multi", ["queries", "subjects", "subst", "gapo", "gape", "local", "top"]),
            ("search_db_multi", ["queries", "subjects", "subst", "gapo", "gape", "local", "top"]),
            ("last_score_db_multi_info", [])]
    for name, params in want:
        sig = inspect.signature(getattr(gsa.Engine, name))
        assert list(sig.parameters)[1:] == params, name
    d = {k: p.default for k, p in inspect.signature(gsa.Engine.score_db_multi_dev).parameters.items()}
    assert (d["gape"], d["local"], d["top"], d["want_scores"], d["max_workgroups"], d["scratch_limit"], d["stream"]) == \
        (None, False, 0, True, 0, 0, None)
    assert inspect.signature(gsa.Engine.score_db_multi).parameters["top"].default == 0
    assert inspect.signature(gsa.Engine.search_db_multi).parameters["top"].default == 10


def test_unit_size_is_exposed():
    assert gsa.score_db_multi_unit() >= 1
    assert isinstance(np.int32(gsa.score_db_multi_unit()).item(), int)


def test_no_new_launch_kind_and_no_new_knob():
    assert len(gsa.LAUNCH_KINDS) == 11 and gsa.LAUNCH_KINDS[-1] == "score_lanes"
    assert gsa.KNOB_NAMES[-2:] == ("GSA_DB_LANES", "GSA_DB_MAXC") and len(gsa.KNOB_NAMES) == 27
