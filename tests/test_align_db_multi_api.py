"""The alignments of many queries' hits in one call (gsa_align_db_multi_dev), the parts that need no
GPU: the entry points in the header, the library and the ctypes bindings, the info struct against the
header, the argument check without a context, the Python entry points, and that the call adds no launch
kind and no knob.  The plan is checked in tests/test_align_db_multi_plan.py, the kernels in
tests/test_gpu_align_db_multi.py."""
import ctypes
import inspect
import os
import re

import gpuseqalign_amd as gsa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CTYPES = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "float": ctypes.c_float}


def _header():
    return open(os.path.join(ROOT, "include", "gsa.h")).read()


def _struct_fields(name):
    body = re.search(r"typedef struct %s\s*\{(.*?)\}\s*%s;" % (name, name), _header(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for ctype, names in re.findall(r"\b(int32_t|int64_t|float)\s+([^;]+);", body):
        fields += [(n.strip(), _CTYPES[ctype]) for n in names.split(",")]
    return fields


def test_entry_points_declared_exported_bound():
    decl = re.search(r"\bint\s+gsa_align_db_multi_dev\s*\((.*?)\)\s*;", _header(), re.S)
    assert decl
    nargs = len(decl.group(1).split(","))
    assert nargs == 24
    assert hasattr(gsa.lib(), "gsa_align_db_multi_dev")
    res, args = gsa.SIGNATURES["gsa_align_db_multi_dev"]
    assert res is ctypes.c_int and len(args) == nargs
    assert re.search(r"\bint32_t\s+gsa_align_db_multi_unit\s*\(\s*void\s*\)\s*;", _header())
    assert hasattr(gsa.lib(), "gsa_align_db_multi_unit")
    assert gsa.SIGNATURES["gsa_align_db_multi_unit"] == (ctypes.c_int32, [])
    assert "align_db_multi_dev" in dir(gsa.Engine)


def test_info_matches_header():
    info = _struct_fields("gsa_align_db_multi_info")
    assert info == list(gsa.AlignDbMultiInfo._fields_)
    assert [n for n, _ in info] == ["lane_hits", "unsupported", "chunks", "launches", "workgroups", "lane_queries",
                                    "tasks", "units", "profile_builds", "code_bytes", "fill_ms", "walk_ms"]
    # gsa_align_db_info keeps its fields: lane_queries lives in the new struct only
    assert "lane_queries" not in [n for n, _ in _struct_fields("gsa_align_db_info")]


def test_null_context_is_invalid_value():
    off = (ctypes.c_int64 * 2)(0, 5)
    hq = (ctypes.c_int32 * 1)(0)
    hs = (ctypes.c_int32 * 1)(0)
    out = (gsa.AlignDbResult * 1)()
    info = gsa.AlignDbMultiInfo()
    ms = ctypes.c_float(0.0)
    need = ctypes.c_int64(0)
    buf = ctypes.create_string_buffer(64)
    st = gsa.lib().gsa_align_db_multi_dev(None, None, off, 1, None, off, 1, hq, hs, 1, None, 25, -11, -1, 0, 0, 0, out,
                                          buf, 64, ctypes.byref(need), ctypes.byref(info), ctypes.byref(ms), None)
    assert st == gsa.NwStat.errorInvalidValue


def test_python_entry_points_and_defaults():
    want = [("align_db_multi_dev", ["queries_ptr", "q_off", "db_ptr", "db_off", "hit_query", "hit_subject", "subst_ptr",
                                    "substsz", "gapo", "gape", "local", "max_workgroups", "scratch_limit", "stream"]),
            ("align_db_multi", ["queries", "subjects", "hit_query", "hit_subject", "subst", "gapo", "gape", "local"]),
            ("search_db_multi", ["queries", "subjects", "subst", "gapo", "gape", "local", "top"]),
            ("last_align_db_multi_info", [])]
    for name, params in want:
        sig = inspect.signature(getattr(gsa.Engine, name))
        assert list(sig.parameters)[1:] == params, name
    d = {k: p.default for k, p in inspect.signature(gsa.Engine.align_db_multi_dev).parameters.items()}
    assert (d["gape"], d["local"], d["max_workgroups"], d["scratch_limit"], d["stream"]) == (None, False, 0, 0, None)
    d = {k: p.default for k, p in inspect.signature(gsa.Engine.align_db_multi).parameters.items()}
    assert (d["gape"], d["local"]) == (None, False)
    assert inspect.signature(gsa.Engine.search_db_multi).parameters["top"].default == 10


def test_unit_size_is_exposed():
    assert gsa.align_db_multi_unit() >= 1
    assert isinstance(gsa.align_db_multi_unit(), int)


def test_no_launch_kind_and_no_knob_added():
    assert gsa.LAUNCH_KINDS[-1] == "score_lanes" and len(gsa.LAUNCH_KINDS) == 11
    assert gsa.KNOB_NAMES[-2:] == ("GSA_DB_LANES", "GSA_DB_MAXC") and len(gsa.KNOB_NAMES) == 27
