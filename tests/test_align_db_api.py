"""Alignments of database hits (gsa_align_db_dev), the parts that need no GPU: the entry point in the
header, the library and the ctypes bindings, the structs against the header, its argument check without
a context, the Python entry points.  The kernels are checked in tests/test_gpu_align_db.py."""
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


def test_entry_point_declared_exported_bound():
    decl = re.search(r"\bint\s+gsa_align_db_dev\s*\((.*?)\)\s*;", _header(), re.S)
    assert decl
    nargs = len(decl.group(1).split(","))
    assert nargs == 21
    assert hasattr(gsa.lib(), "gsa_align_db_dev")
    res, args = gsa.SIGNATURES["gsa_align_db_dev"]
    assert res is ctypes.c_int and len(args) == nargs


def test_structs_match_header():
    want = [("score", ctypes.c_int32), ("status", ctypes.c_int32), ("i_start", ctypes.c_int64),
            ("j_start", ctypes.c_int64), ("i_end", ctypes.c_int64), ("j_end", ctypes.c_int64),
            ("cigar_off", ctypes.c_int64), ("cigar_len", ctypes.c_int64)]
    assert _struct_fields("gsa_align_db_result") == want == list(gsa.AlignDbResult._fields_)
    info = _struct_fields("gsa_align_db_info")
    assert info == list(gsa.AlignDbInfo._fields_)
    assert [n for n, _ in info][:5] == ["lane_hits", "unsupported", "chunks", "tasks", "code_bytes"]
    assert ctypes.sizeof(gsa.AlignDbResult) == 56


def test_null_context_is_invalid_value():
    off = (ctypes.c_int64 * 2)(0, 5)
    hits = (ctypes.c_int32 * 1)(0)
    out = (gsa.AlignDbResult * 1)()
    info = gsa.AlignDbInfo()
    ms = ctypes.c_float(0.0)
    need = ctypes.c_int64(0)
    buf = ctypes.create_string_buffer(64)
    st = gsa.lib().gsa_align_db_dev(None, None, 10, None, off, 1, hits, 1, None, 25, -11, -1, 0, 0, out, buf, 64,
                                    ctypes.byref(need), ctypes.byref(info), ctypes.byref(ms), None)
    assert st == gsa.NwStat.errorInvalidValue


def test_python_entry_points_exist():
    for name, params in [("align_db_dev", ["query_ptr", "adjq", "db_ptr", "db_off", "hits", "subst_ptr", "substsz",
                                           "gapo", "gape", "local", "scratch_limit", "stream"]),
                         ("align_db", ["query", "subjects", "hits", "subst", "gapo", "gape", "local"]),
                         ("search_db", ["query", "subjects", "subst", "gapo", "gape", "local", "top"]),
                         ("last_align_db_info", [])]:
        sig = inspect.signature(getattr(gsa.Engine, name))
        assert list(sig.parameters)[1:] == params, name
    assert inspect.signature(gsa.Engine.search_db).parameters["top"].default == 10
    assert inspect.signature(gsa.Engine.align_db_dev).parameters["scratch_limit"].default == 0


def test_no_launch_kind_and_no_knob_added():
    assert gsa.LAUNCH_KINDS[-1] == "score_lanes" and len(gsa.LAUNCH_KINDS) == 11
    assert gsa.KNOB_NAMES[-2:] == ("GSA_DB_LANES", "GSA_DB_MAXC")
