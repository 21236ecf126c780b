"""The long pairs' batched semi-global calls (gsa_score_semi_batch_dev, gsa_align_batch_semi_dev), the
parts that need no GPU: the entry points in the header, the library and the ctypes bindings, the info
struct's layout, the argument check without a context, the Python entry points, the Makefile's rules and
the resource reports of the two new translation units, that the reports of the neighbouring units still
list the kernels they listed before, and that the calls add no launch kind and no knob.  The kernels are
checked in tests/test_gpu_score_semi_batch.py and tests/test_gpu_align_batch_semi.py."""
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
    """Both argument lists are the global batch calls' without `local`."""
    text = open(os.path.join(ROOT, "include", "gsa.h")).read()
    for semi, glob, n in (("gsa_score_semi_batch_dev", "gsa_score_batch_dev", 10),
                          ("gsa_align_batch_semi_dev", "gsa_align_batch_dev", 16)):
        assert hasattr(gsa.lib(), semi)
        res, args = gsa.SIGNATURES[semi]
        want = [a.replace("gsa_align_batch_info", "gsa_align_batch_semi_info") for a in _args(text, glob) if a != "int32_t local"]
        assert res is ctypes.c_int and len(args) == len(want) == n
        assert _args(text, semi) == want
        gres, gargs = gsa.SIGNATURES[glob]
        assert [a for a in args if a is not ctypes.POINTER(gsa.AlignBatchSemiInfo)] == \
            [a for k, a in enumerate(gargs) if k != 7 and a is not ctypes.POINTER(gsa.AlignBatchInfo)]
    assert gsa.SIGNATURES["gsa_align_batch_semi_dev"][1][13] == ctypes.POINTER(gsa.AlignBatchSemiInfo)


def test_info_struct_layout():
    text = open(os.path.join(ROOT, "include", "gsa.h")).read()
    body = re.search(r"typedef struct gsa_align_batch_semi_info \{(.*?)\} gsa_align_batch_semi_info;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n.strip() for decl in body.split(";") if decl.strip() for n in decl.split(None, 1)[1].split(",")]
    assert names == [f[0] for f in gsa.AlignBatchSemiInfo._fields_]
    I = gsa.AlignBatchSemiInfo
    assert ctypes.sizeof(I) == 64 and ctypes.sizeof(I) % 8 == 0
    assert [(f, getattr(I, f).offset) for f, _ in I._fields_] == [
        ("batch_pairs", 0), ("host_pairs", 4), ("strip_rows", 8), ("strips", 12), ("strips_filled", 16), ("rounds", 20),
        ("code_bytes", 24), ("window_cols", 32), ("gran_bytes", 40), ("score_ms", 48), ("fill_ms", 52), ("walk_ms", 56),
        ("pad0", 60)]
    assert [t for f, t in I._fields_ if f in ("code_bytes", "window_cols", "gran_bytes")] == [ctypes.c_int64] * 3


def test_null_context_is_invalid_value():
    out, info, sr = gsa.AlignDbResult(), gsa.AlignBatchSemiInfo(), gsa.ScoreResult()
    need, ms = ctypes.c_int64(0), ctypes.c_float(0.0)
    pairs = (gsa.PairDev * 1)()
    st = gsa.lib().gsa_align_batch_semi_dev(None, 1, pairs, None, 25, -11, -1, 0, 0, ctypes.byref(out), None, 0,
                                            ctypes.byref(need), ctypes.byref(info), ctypes.byref(ms), None)
    assert st == gsa.NwStat.errorInvalidValue
    st = gsa.lib().gsa_score_semi_batch_dev(None, 1, pairs, None, 25, -11, -1, ctypes.byref(sr), ctypes.byref(ms), None)
    assert st == gsa.NwStat.errorInvalidValue


def test_python_entry_points():
    dev = ["pairs", "subst_ptr", "substsz", "gapo", "gape"]
    want = [("score_semi_batch_dev", dev + ["stream"]),
            ("score_semi_batch", ["pairs", "subst", "gapo", "gape"]),
            ("align_batch_semi_dev", dev + ["max_workgroups", "scratch_limit", "stream"]),
            ("align_batch_semi", ["pairs", "subst", "gapo", "gape", "scratch_limit"]),
            ("last_align_batch_semi_info", [])]
    for name, params in want:
        sig = inspect.signature(getattr(gsa.Engine, name))
        assert list(sig.parameters)[1:] == params, name
    for name, _ in want[:4]:
        sig = inspect.signature(getattr(gsa.Engine, name))
        assert sig.parameters["gape"].default is None
        for opt, dflt in (("stream", None), ("scratch_limit", 0), ("max_workgroups", 0)):
            if opt in sig.parameters:
                assert sig.parameters[opt].default == dflt or sig.parameters[opt].default is dflt
    # the batch calls' argument lists without `local`
    for semi, glob in (("score_semi_batch_dev", "score_batch_dev"), ("align_batch_semi_dev", "align_batch_dev"),
                       ("score_semi_batch", "score_batch"), ("align_batch_semi", "align_batch")):
        g = [p for p in inspect.signature(getattr(gsa.Engine, glob)).parameters if p != "local"]
        assert list(inspect.signature(getattr(gsa.Engine, semi)).parameters) == g


def test_makefile_builds_both_units_with_reports():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    objs = re.search(r"^OBJS = (.*)$", mk, re.M).group(1).split()
    for unit in ("nw_kscore_semi_batch", "nw_pair_semi_trace_batch"):
        assert "build/%s.o" % unit in objs
        rule = re.search(r"^build/%s\.o:.*\n\t(.*)$" % unit, mk, re.M).group(1)
        assert "-Rpass-analysis=kernel-resource-usage" in rule and "build/%s.resources.txt" % unit in rule
        assert "_SCHED" not in rule  # the default scheduler
        assert os.path.exists(os.path.join(CSRC, "build", unit + ".resources.txt"))
    # the trace unit is a translation unit of its own; the score unit is nw_krow.hip under two defines
    src = open(os.path.join(CSRC, "nw_pair_semi_trace_batch.hip")).read()
    assert not re.search(r'#include\s+"[^"]*\.hip"', src)
    src = open(os.path.join(CSRC, "nw_kscore_semi_batch.hip")).read()
    code = [l.strip() for l in src.split("\n") if l.strip() and not l.startswith("//")]
    assert code == ["#define GSA_KROW_SCORE", "#define GSA_KSCORE_SEMI_BATCH", '#include "nw_krow.hip"']
    # the plan is free of HIP
    plan = open(os.path.join(CSRC, "nw_pair_semi_trace_batch_plan.h")).read()
    assert "hip" not in re.sub(r"//.*", "", plan).lower()


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
    kernels = ["nw_semi_batch_fill_kernelILb%dELi%dE" % (a, k) for a in (0, 1) for k in (8, 16)] + ["nw_semi_batch_walk_kernel"]
    rep = _report("nw_pair_semi_trace_batch")
    assert len(rep) == len(kernels) and all(any(k in n for n in rep) for k in kernels), list(rep)
    assert set(rep.values()) == {(0, 0, 0)}, rep


def test_score_instances_use_no_more_scratch_or_spills_than_the_single_pair_ones():
    """The report lists the 8 batched semi-global instances (affine mode 7 and linear mode 8, int16 and
    int8 profile, K = 2 and 4, BATCH) and the batched row maximum's kernel; none has more scratch or more
    spilled registers than nw_kscore_semi's single-pair instance of the same gap model, profile and K."""
    rep = _report("nw_kscore_semi_batch")
    single = _report("nw_kscore_semi")
    score = {n: v for n, v in rep.items() if "nw_kscore_kernel" in n}
    assert len(score) == 8 and len(rep) == 9 and any("nw_semi_rowmax_batch_kernel" in n for n in rep)
    for mode in (7, 8):
        for q8 in (0, 1):
            for k in (2, 4):
                got = [v for n, v in score.items() if "nw_kscore_kernelILi%dELb%dELi%dELb1EE" % (mode, q8, k) in n]
                one = [v for n, v in single.items() if "nw_kscore_kernelILi%dELb%dELi%dELb0EE" % (mode, q8, k) in n]
                assert len(got) == 1 and len(one) == 1, (mode, q8, k)
                assert all(g <= w for g, w in zip(got[0], one[0])), (mode, q8, k, got[0], one[0])
    assert [v for n, v in rep.items() if "rowmax" in n] == [(0, 0, 0)]


def test_neighbouring_reports_list_the_kernels_they_listed():
    """nw_kscore_semi: 8 single-pair score instances and the row maximum; nw_pair_semi_trace: 4 fills and
    the walk; nw_pair_trace_batch: 8 fills and the walk."""
    rep = _report("nw_kscore_semi")
    want = ["nw_kscore_kernelILi%dELb%dELi%dELb0EE" % (m, q, k) for m in (7, 8) for q in (0, 1) for k in (2, 4)]
    assert len(rep) == 9 and all(any(w in n for n in rep) for w in want + ["nw_semi_rowmax_kernel"]), list(rep)
    rep = _report("nw_pair_semi_trace")
    want = ["nw_semi_fill_kernelILb%dELi%dE" % (a, k) for a in (0, 1) for k in (8, 16)] + ["nw_semi_walk_kernel"]
    assert len(rep) == 5 and all(any(w in n for n in rep) for w in want), list(rep)
    rep = _report("nw_pair_trace_batch")
    want = ["nw_pair_batch_fill_kernelILb%dELb%dELi%dE" % (l, a, k) for l in (0, 1) for a in (0, 1) for k in (8, 16)]
    assert len(rep) == 9 and all(any(w in n for n in rep) for w in want + ["nw_pair_batch_walk_kernel"]), list(rep)


def test_no_new_launch_kind_and_no_new_knob():
    assert len(gsa.LAUNCH_KINDS) == 11 and gsa.LAUNCH_KINDS[-1] == "score_lanes"
    assert gsa.KNOB_NAMES[-2:] == ("GSA_DB_LANES", "GSA_DB_MAXC") and len(gsa.KNOB_NAMES) == 27
