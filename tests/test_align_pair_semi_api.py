"""The long pairs' semi-global mode (gsa_score_semi_dev, gsa_align_pair_semi_dev), the parts that need
no GPU: the entry points in the header, the library and the ctypes bindings, the info struct's layout,
the argument check without a context, the Python entry points, the Makefile's rules and the resource
reports of the two new translation units, and that the calls add no launch kind and no knob.  The
kernels are checked in tests/test_gpu_score_semi_pair.py and tests/test_gpu_align_pair_semi.py."""
import ctypes
import inspect
import os
import re

import gpuseqalign_amd as gsa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gpuseqalign_amd", "csrc")


def _args(text, name):
    decl = re.search(r"int\s+%s\s*\((.*?)\)\s*;" % name, text, re.S).group(1)
    return [" ".join(a.split()) for a in decl.split(",")]


def test_entry_points_declared_exported_bound():
    """Both argument lists are the global calls' without `local`."""
    text = open(os.path.join(ROOT, "include", "gsa.h")).read()
    for semi, glob, n in (("gsa_score_semi_dev", "gsa_score_dev", 11), ("gsa_align_pair_semi_dev", "gsa_align_pair_dev", 17)):
        assert hasattr(gsa.lib(), semi)
        res, args = gsa.SIGNATURES[semi]
        want = [a.replace("gsa_align_pair_info", "gsa_align_pair_semi_info") for a in _args(text, glob) if a != "int32_t local"]
        assert res is ctypes.c_int and len(args) == len(want) == n
        assert _args(text, semi) == want
        gres, gargs = gsa.SIGNATURES[glob]
        assert [a for a in args if a is not ctypes.POINTER(gsa.AlignPairSemiInfo)] == \
            [a for k, a in enumerate(gargs) if k != 9 and a is not ctypes.POINTER(gsa.AlignPairInfo)]
    assert gsa.SIGNATURES["gsa_align_pair_semi_dev"][1][14] == ctypes.POINTER(gsa.AlignPairSemiInfo)


def test_info_struct_layout():
    text = open(os.path.join(ROOT, "include", "gsa.h")).read()
    body = re.search(r"typedef struct gsa_align_pair_semi_info \{(.*?)\} gsa_align_pair_semi_info;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n.strip() for decl in body.split(";") if decl.strip() for n in decl.split(None, 1)[1].split(",")]
    assert names == [f[0] for f in gsa.AlignPairSemiInfo._fields_]
    I = gsa.AlignPairSemiInfo
    assert ctypes.sizeof(I) == 48
    assert [(f, getattr(I, f).offset) for f, _ in I._fields_] == [
        ("strip_rows", 0), ("strips", 4), ("strips_filled", 8), ("chunks", 12), ("code_bytes", 16), ("j_window", 24),
        ("score_ms", 32), ("fill_ms", 36), ("walk_ms", 40), ("pad0", 44)]


def test_null_context_is_invalid_value():
    out, info, sr = gsa.AlignDbResult(), gsa.AlignPairSemiInfo(), gsa.ScoreResult()
    need, ms = ctypes.c_int64(0), ctypes.c_float(0.0)
    st = gsa.lib().gsa_align_pair_semi_dev(None, None, 5, None, 5, None, 25, -11, -1, 0, ctypes.byref(out), None, 0,
                                           ctypes.byref(need), ctypes.byref(info), ctypes.byref(ms), None)
    assert st == gsa.NwStat.errorInvalidValue
    st = gsa.lib().gsa_score_semi_dev(None, None, 5, None, 5, None, 25, -11, -1, ctypes.byref(sr), None)
    assert st == gsa.NwStat.errorInvalidValue


def test_python_entry_points():
    dev = ["seqY_ptr", "adjrows", "seqX_ptr", "adjcols", "subst_ptr", "substsz", "gapo", "gape"]
    want = [("score_semi_dev", dev + ["stream"]),
            ("score_semi", ["seqY", "seqX", "subst", "gapo", "gape"]),
            ("align_pair_semi_dev", dev + ["scratch_limit", "stream"]),
            ("align_pair_semi", ["seqY", "seqX", "subst", "gapo", "gape", "scratch_limit"]),
            ("last_align_pair_semi_info", [])]
    for name, params in want:
        sig = inspect.signature(getattr(gsa.Engine, name))
        assert list(sig.parameters)[1:] == params, name
    for name in ("score_semi_dev", "score_semi", "align_pair_semi_dev", "align_pair_semi"):
        sig = inspect.signature(getattr(gsa.Engine, name))
        assert sig.parameters["gape"].default is None
        if "stream" in sig.parameters:
            assert sig.parameters["stream"].default is None
        if "scratch_limit" in sig.parameters:
            assert sig.parameters["scratch_limit"].default == 0


def test_makefile_builds_both_units_with_reports():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    objs = re.search(r"^OBJS = (.*)$", mk, re.M).group(1).split()
    for unit in ("nw_kscore_semi", "nw_pair_semi_trace"):
        assert "build/%s.o" % unit in objs
        rule = re.search(r"^build/%s\.o:.*\n\t(.*)$" % unit, mk, re.M).group(1)
        assert "-Rpass-analysis=kernel-resource-usage" in rule and "build/%s.resources.txt" % unit in rule
        assert "_SCHED" not in rule  # the default scheduler
        assert os.path.exists(os.path.join(CSRC, "build", unit + ".resources.txt"))
    # the trace unit is a translation unit of its own; the score unit is nw_krow.hip under two defines
    src = open(os.path.join(CSRC, "nw_pair_semi_trace.hip")).read()
    assert not re.search(r'#include\s+"[^"]*\.hip"', src)
    src = open(os.path.join(CSRC, "nw_kscore_semi.hip")).read()
    code = [l.strip() for l in src.split("\n") if l.strip() and not l.startswith("//")]
    assert code == ["#define GSA_KROW_SCORE", "#define GSA_KSCORE_SEMI", '#include "nw_krow.hip"']


def _report(unit):
    text = open(os.path.join(CSRC, "build", unit + ".resources.txt")).read()
    out = {}
    for block in text.split("Function Name: ")[1:]:
        name = block.split()[0]
        out[name] = tuple(int(re.search(f + r": (\d+)", block).group(1))
                          for f in ("ScratchSize \\[bytes/lane\\]", "SGPRs Spill", "VGPRs Spill"))
    return out


def test_trace_instances_have_no_scratch_and_no_spills():
    """The four fill instances (affine or linear, 8 or 16 rows per lane) and the walk."""
    kernels = ["nw_semi_fill_kernelILb%dELi%dE" % (a, k) for a in (0, 1) for k in (8, 16)] + ["nw_semi_walk_kernel"]
    rep = _report("nw_pair_semi_trace")
    assert len(rep) == len(kernels) and all(any(k in n for n in rep) for k in kernels), list(rep)
    assert set(rep.values()) == {(0, 0, 0)}, rep


# (scratch bytes per lane, spilled SGPRs, spilled VGPRs) of the global single-pair instances of
# nw_kscore_kernel, by (linear, int8 profile, K): from the resource reports of nw_kscore.hip (default
# scheduler) and nw_kscore_ag.hip (iterative ILP scheduler) built with the Makefile's flags at the
# commit before this mode was added, in a scratch directory (-Rpass-analysis=kernel-resource-usage)
GLOBAL_INSTANCES = {
    (True, False, 2): (0, 20, 0), (True, True, 2): (0, 18, 0), (True, False, 4): (0, 20, 0), (True, True, 4): (0, 18, 0),
    (False, False, 2): (0, 30, 0), (False, True, 2): (0, 34, 0), (False, False, 4): (0, 30, 0), (False, True, 4): (0, 34, 0),
}


def test_score_instances_use_no_more_scratch_or_spills_than_the_global_ones():
    """The report lists the 8 semi-global instances (affine mode 7 and linear mode 8, int16 and int8
    profile, K = 2 and 4, single pair) and the row maximum's kernel; none has more scratch or more
    spilled registers than the global instance of the same gap model, profile and K."""
    rep = _report("nw_kscore_semi")
    score = {n: v for n, v in rep.items() if "nw_kscore_kernel" in n}
    assert len(score) == 8 and len(rep) == 9 and any("nw_semi_rowmax_kernel" in n for n in rep)
    for (lin, q8, k), glob in GLOBAL_INSTANCES.items():
        name = "nw_kscore_kernelILi%dELb%dELi%dELb0EE" % (8 if lin else 7, q8, k)
        got = [v for n, v in score.items() if name in n]
        assert len(got) == 1, name
        assert all(g <= w for g, w in zip(got[0], glob)), (name, got[0], glob)
    assert [v for n, v in rep.items() if "rowmax" in n] == [(0, 0, 0)]


def test_no_new_launch_kind_and_no_new_knob():
    assert len(gsa.LAUNCH_KINDS) == 11 and gsa.LAUNCH_KINDS[-1] == "score_lanes"
    assert gsa.KNOB_NAMES[-2:] == ("GSA_DB_LANES", "GSA_DB_MAXC") and len(gsa.KNOB_NAMES) == 27
