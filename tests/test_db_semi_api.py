"""The semi-global database search (gsa_score_db_multi_semi_dev, gsa_align_db_multi_semi_dev), the parts
that need no GPU: the entry points in the header, the library and the ctypes bindings, their argument
check without a context, the Python entry points, and that they add no launch kind and no knob.  The
kernels are checked in tests/test_gpu_score_db_semi.py and tests/test_gpu_align_db_semi.py."""
import ctypes
import inspect
import os
import re

import pytest

import gpuseqalign_amd as gsa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name,nargs,old", [("gsa_score_db_multi_semi_dev", 19, "gsa_score_db_multi_dev"),
                                            ("gsa_align_db_multi_semi_dev", 23, "gsa_align_db_multi_dev")])
def test_entry_points_declared_exported_bound(name, nargs, old):
    text = open(os.path.join(ROOT, "include", "gsa.h")).read()
    assert re.search(r"\bint\s+%s\s*\(" % name, text)
    assert hasattr(gsa.lib(), name)
    res, args = gsa.SIGNATURES[name]
    assert res is ctypes.c_int and len(args) == nargs
    decl = re.search(r"int\s+%s\s*\((.*?)\)\s*;" % name, text, re.S).group(1)
    assert len(decl.split(",")) == nargs
    # the old call's arguments without `local`
    old_decl = re.search(r"int\s+%s\s*\((.*?)\)\s*;" % old, text, re.S).group(1)
    norm = lambda d: [" ".join(a.split()) for a in d.split(",")]
    assert norm(decl) == [a for a in norm(old_decl) if a != "int32_t local"]
    old_args = list(gsa.SIGNATURES[old][1])
    at = norm(old_decl).index("int32_t local")
    assert list(args) == old_args[:at] + old_args[at + 1:]


def test_null_context_is_invalid_value():
    off = (ctypes.c_int64 * 2)(0, 5)
    scores = (ctypes.c_int32 * 1)()
    info = gsa.ScoreDbMultiInfo()
    ms = ctypes.c_float(0.0)
    st = gsa.lib().gsa_score_db_multi_semi_dev(None, None, off, 1, None, off, 1, None, 25, -11, -1, 0, 0, 0, scores, None,
                                               ctypes.byref(info), ctypes.byref(ms), None)
    assert st == gsa.NwStat.errorInvalidValue
    hit = (ctypes.c_int32 * 1)(0)
    out = (gsa.AlignDbResult * 1)()
    ainfo = gsa.AlignDbMultiInfo()
    need = ctypes.c_int64(0)
    st = gsa.lib().gsa_align_db_multi_semi_dev(None, None, off, 1, None, off, 1, hit, hit, 1, None, 25, -11, -1, 0, 0, out,
                                               None, 0, ctypes.byref(need), ctypes.byref(ainfo), ctypes.byref(ms), None)
    assert st == gsa.NwStat.errorInvalidValue


def test_python_entry_points_exist():
    want = [("score_db_semi_dev", ["queries_ptr", "q_off", "db_ptr", "db_off", "subst_ptr", "substsz", "gapo", "gape", "top",
                                   "want_scores", "max_workgroups", "scratch_limit", "stream"]),
            ("score_db_semi", ["queries", "subjects", "subst", "gapo", "gape", "top"]),
            ("last_score_db_semi_info", []),
            ("align_db_semi_dev", ["queries_ptr", "q_off", "db_ptr", "db_off", "hit_query", "hit_subject", "subst_ptr",
                                   "substsz", "gapo", "gape", "max_workgroups", "scratch_limit", "stream"]),
            ("align_db_semi", ["queries", "subjects", "hit_query", "hit_subject", "subst", "gapo", "gape"]),
            ("last_align_db_semi_info", []),
            ("search_db_semi", ["queries", "subjects", "subst", "gapo", "gape", "top"])]
    for name, params in want:
        sig = inspect.signature(getattr(gsa.Engine, name))
        assert list(sig.parameters)[1:] == params, name
        # the *_multi form without `local`, defaults included
        multi = inspect.signature(getattr(gsa.Engine, name.replace("_semi", "_multi")))
        assert [(k, p.default) for k, p in multi.parameters.items() if k != "local"] == \
            [(k, p.default) for k, p in sig.parameters.items()], name


def test_new_instances_have_no_scratch_and_no_spills():
    """The build's resource reports of the two new translation units: every kernel named, none with
    scratch or a spilled register."""
    want = {"nw_lanes_semi": ["nw_dbsemi_kernelILb1E", "nw_dbsemi_kernelILb0E"],
            "nw_lanes_semi_trace": ["nw_dbsemi_fill_kernelILb1E", "nw_dbsemi_fill_kernelILb0E", "nw_dbsemi_walk_kernel"]}
    for unit, kernels in want.items():
        text = open(os.path.join(ROOT, "gpuseqalign_amd", "csrc", "build", unit + ".resources.txt")).read()
        names = re.findall(r"Function Name: (\S+)", text)
        assert len(names) == len(kernels) and all(any(k in n for n in names) for k in kernels), names
        for field in ("ScratchSize \\[bytes/lane\\]", "SGPRs Spill", "VGPRs Spill"):
            assert re.findall(field + r": (\d+)", text) == ["0"] * len(kernels), (unit, field)


def test_no_new_launch_kind_and_no_new_knob():
    assert len(gsa.LAUNCH_KINDS) == 11 and gsa.LAUNCH_KINDS[-1] == "score_lanes"
    assert gsa.KNOB_NAMES[-2:] == ("GSA_DB_LANES", "GSA_DB_MAXC") and len(gsa.KNOB_NAMES) == 27
