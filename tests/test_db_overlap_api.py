"""The overlap (dovetail) database search (gsa_score_db_multi_overlap_dev, gsa_align_db_multi_overlap_dev;
DESIGN.md 2.2o), the parts that need no GPU: the entry points in the header, the library and the ctypes
bindings, their argument check without a context, the Python entry points, the build's resource reports
of the two new units, and that the calls add no launch kind and no knob.  The kernels are checked in
tests/test_gpu_score_db_overlap.py and tests/test_gpu_align_db_overlap.py."""
import ctypes
import inspect
import os
import re

import pytest

import gpuseqalign_amd as gsa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gpuseqalign_amd", "csrc")


@pytest.mark.parametrize("name,nargs,semi", [("gsa_score_db_multi_overlap_dev", 19, "gsa_score_db_multi_semi_dev"),
                                             ("gsa_align_db_multi_overlap_dev", 23, "gsa_align_db_multi_semi_dev")])
def test_entry_points_declared_exported_bound(name, nargs, semi):
    text = open(os.path.join(ROOT, "include", "gsa.h")).read()
    assert re.search(r"\bint\s+%s\s*\(" % name, text)
    assert hasattr(gsa.lib(), name)
    res, args = gsa.SIGNATURES[name]
    assert res is ctypes.c_int and len(args) == nargs
    # the semi-global call's arguments, one for one
    norm = lambda d: [" ".join(a.split()) for a in d.split(",")]
    decl = re.search(r"int\s+%s\s*\((.*?)\)\s*;" % name, text, re.S).group(1)
    semi_decl = re.search(r"int\s+%s\s*\((.*?)\)\s*;" % semi, text, re.S).group(1)
    assert norm(decl) == norm(semi_decl) and len(norm(decl)) == nargs
    assert list(args) == list(gsa.SIGNATURES[semi][1])


def _score_status(*args):
    info, ms = gsa.ScoreDbMultiInfo(), ctypes.c_float(0.0)
    return gsa.lib().gsa_score_db_multi_overlap_dev(*args, ctypes.byref(info), ctypes.byref(ms), None)


def _align_status(*args):
    info, ms, need = gsa.AlignDbMultiInfo(), ctypes.c_float(0.0), ctypes.c_int64(0)
    return gsa.lib().gsa_align_db_multi_overlap_dev(*args, ctypes.byref(need), ctypes.byref(info), ctypes.byref(ms), None)


def test_null_context_or_bad_arguments_are_invalid_value():
    """Without a context every call is errorInvalidValue, whatever else is wrong with it: good-looking
    arguments, a gap model out of order, a table size out of range, negative counts and limits."""
    off = (ctypes.c_int64 * 2)(0, 5)
    scores = (ctypes.c_int32 * 1)()
    hit = (ctypes.c_int32 * 1)(0)
    out = (gsa.AlignDbResult * 1)()
    bad = gsa.NwStat.errorInvalidValue
    for substsz, go, ge, top, wgs, limit in [(25, -11, -1, 0, 0, 0), (25, -1, -11, 0, 0, 0), (25, -11, 1, 0, 0, 0),
                                             (0, -11, -1, 0, 0, 0), (33, -11, -1, 0, 0, 0), (25, -11, -1, -1, 0, 0),
                                             (25, -11, -1, 0, -1, 0), (25, -11, -1, 0, 0, -1)]:
        assert _score_status(None, None, off, 1, None, off, 1, None, substsz, go, ge, top, wgs, limit, scores, None) == bad
        assert _align_status(None, None, off, 1, None, off, 1, hit, hit, 1, None, substsz, go, ge, wgs, limit, out,
                             None, 0) == bad
    assert _score_status(None, None, off, 0, None, off, 1, None, 25, -11, -1, 0, 0, 0, scores, None) == bad   # nq = 0
    assert _score_status(None, None, off, 1, None, off, 1, None, 25, -11, -1, 0, 0, 0, None, None) == bad     # no output
    assert _align_status(None, None, off, 1, None, off, 1, hit, hit, -1, None, 25, -11, -1, 0, 0, out, None, 0) == bad
    assert _align_status(None, None, off, 1, None, off, 1, hit, hit, 1, None, 25, -11, -1, 0, 0, None, None, 0) == bad


def test_python_entry_points_exist():
    names = ["score_db_%s_dev", "score_db_%s", "last_score_db_%s_info", "align_db_%s_dev", "align_db_%s",
             "last_align_db_%s_info", "search_db_%s"]
    for name in names:
        sig = inspect.signature(getattr(gsa.Engine, name % "overlap"))
        semi = inspect.signature(getattr(gsa.Engine, name % "semi"))
        # the *_semi form's parameters, defaults included
        assert [(k, p.default) for k, p in sig.parameters.items()] == \
            [(k, p.default) for k, p in semi.parameters.items()], name


def test_last_info_before_any_call_is_an_error():
    e = gsa.Engine.__new__(gsa.Engine)  # no context: the info calls read attributes only
    for name in ("last_score_db_overlap_info", "last_align_db_overlap_info"):
        with pytest.raises(gsa.NwError) as ei:
            getattr(e, name)()
        assert ei.value.stat == gsa.NwStat.errorInvalidValue


def test_new_instances_have_no_scratch_and_no_spills():
    """The build's resource reports of the two new translation units: every kernel named, none with
    scratch or a spilled register."""
    want = {"nw_lanes_overlap": ["nw_dboverlap_kernelILb1E", "nw_dboverlap_kernelILb0E"],
            "nw_lanes_overlap_trace": ["nw_dboverlap_fill_kernelILb1E", "nw_dboverlap_fill_kernelILb0E",
                                       "nw_dboverlap_walk_kernel"]}
    for unit, kernels in want.items():
        text = open(os.path.join(CSRC, "build", unit + ".resources.txt")).read()
        names = re.findall(r"Function Name: (\S+)", text)
        assert len(names) == len(kernels) and all(any(k in n for n in names) for k in kernels), names
        for field in ("ScratchSize \\[bytes/lane\\]", "SGPRs Spill", "VGPRs Spill"):
            assert re.findall(field + r": (\d+)", text) == ["0"] * len(kernels), (unit, field)


def test_makefile_rules_carry_the_report_flag():
    text = open(os.path.join(CSRC, "Makefile")).read()
    for unit, defs in (("nw_lanes_overlap", ["$(DBM_DEF)"]), ("nw_lanes_overlap_trace", ["$(DBM_DEF)", "$(DBA_DEF)"])):
        rule = re.search(r"^build/%s\.o:.*\n\t(.*)$" % unit, text, re.M)
        assert rule, unit
        cmd = rule.group(1)
        assert "-Rpass-analysis=kernel-resource-usage" in cmd and "build/%s.resources.txt" % unit in cmd, cmd
        assert all(d in cmd for d in defs), cmd
        assert "build/%s.o" % unit in re.search(r"^OBJS = (.*)$", text, re.M).group(1)


def test_no_new_launch_kind_and_no_new_knob():
    assert len(gsa.LAUNCH_KINDS) == 11 and gsa.LAUNCH_KINDS[-1] == "score_lanes"
    assert gsa.KNOB_NAMES[-2:] == ("GSA_DB_LANES", "GSA_DB_MAXC") and len(gsa.KNOB_NAMES) == 27
