"""The long pairs' overlap mode (gsa_score_overlap_dev, gsa_align_pair_overlap_dev), the parts that need
no GPU: the entry points in the header, the library and the ctypes bindings, the info struct's layout,
the argument check without a context, the Python entry points, the Makefile's rules and the resource
reports of the two new translation units, and that the calls add no launch kind and no knob.  The
kernels are checked in tests/test_gpu_score_overlap_pair.py and tests/test_gpu_align_pair_overlap.py."""
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
    """Both argument lists are the semi-global calls', with the overlap info struct."""
    text = open(os.path.join(ROOT, "include", "gsa.h")).read()
    for ov, semi, n in (("gsa_score_overlap_dev", "gsa_score_semi_dev", 11),
                        ("gsa_align_pair_overlap_dev", "gsa_align_pair_semi_dev", 17)):
        assert hasattr(gsa.lib(), ov)
        res, args = gsa.SIGNATURES[ov]
        want = [a.replace("gsa_align_pair_semi_info", "gsa_align_pair_overlap_info") for a in _args(text, semi)]
        assert res is ctypes.c_int and len(args) == len(want) == n
        assert _args(text, ov) == want
        sres, sargs = gsa.SIGNATURES[semi]
        assert [a for a in args if a is not ctypes.POINTER(gsa.AlignPairOverlapInfo)] == \
            [a for a in sargs if a is not ctypes.POINTER(gsa.AlignPairSemiInfo)]
    assert gsa.SIGNATURES["gsa_align_pair_overlap_dev"][1][14] == ctypes.POINTER(gsa.AlignPairOverlapInfo)


def test_semantics_are_stated_in_the_header():
    text = " ".join(open(os.path.join(ROOT, "include", "gsa.h")).read().replace("*", " ").split())
    for phrase in ("row 0 is free: H(0, j) = 0, E = F = minus infinity, j = 0 ... C",
                   "column 0 is free: H(i, 0) = 0, E = F = minus infinity, i = 0 ... R",
                   "so score >= 0 always",
                   "A score of 0 therefore always ends at (R, 0)",
                   "stops as soon as i = 0 or j = 0",
                   "No gap letters are emitted along either border"):
        assert phrase in text, phrase


def test_info_struct_layout():
    text = open(os.path.join(ROOT, "include", "gsa.h")).read()
    body = re.search(r"typedef struct gsa_align_pair_overlap_info \{(.*?)\} gsa_align_pair_overlap_info;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n.strip() for decl in body.split(";") if decl.strip() for n in decl.split(None, 1)[1].split(",")]
    assert names == [f[0] for f in gsa.AlignPairOverlapInfo._fields_]
    I = gsa.AlignPairOverlapInfo
    assert ctypes.sizeof(I) == 40 and ctypes.sizeof(I) % 8 == 0
    assert [(f, getattr(I, f).offset) for f, _ in I._fields_] == [
        ("strip_rows", 0), ("strips", 4), ("strips_filled", 8), ("chunks", 12), ("code_bytes", 16),
        ("score_ms", 24), ("fill_ms", 28), ("walk_ms", 32), ("pad0", 36)]


def test_null_context_is_invalid_value():
    out, info, sr = gsa.AlignDbResult(), gsa.AlignPairOverlapInfo(), gsa.ScoreResult()
    need, ms = ctypes.c_int64(0), ctypes.c_float(0.0)
    st = gsa.lib().gsa_align_pair_overlap_dev(None, None, 5, None, 5, None, 25, -11, -1, 0, ctypes.byref(out), None, 0,
                                              ctypes.byref(need), ctypes.byref(info), ctypes.byref(ms), None)
    assert st == gsa.NwStat.errorInvalidValue
    st = gsa.lib().gsa_score_overlap_dev(None, None, 5, None, 5, None, 25, -11, -1, ctypes.byref(sr), None)
    assert st == gsa.NwStat.errorInvalidValue


def test_python_entry_points():
    dev = ["seqY_ptr", "adjrows", "seqX_ptr", "adjcols", "subst_ptr", "substsz", "gapo", "gape"]
    want = [("score_overlap_dev", dev + ["stream"]),
            ("score_overlap", ["seqY", "seqX", "subst", "gapo", "gape"]),
            ("align_pair_overlap_dev", dev + ["scratch_limit", "stream"]),
            ("align_pair_overlap", ["seqY", "seqX", "subst", "gapo", "gape", "scratch_limit"]),
            ("last_align_pair_overlap_info", [])]
    for name, params in want:
        sig = inspect.signature(getattr(gsa.Engine, name))
        assert list(sig.parameters)[1:] == params, name
        semi = inspect.signature(getattr(gsa.Engine, name.replace("overlap", "semi")))
        assert list(sig.parameters) == list(semi.parameters), name
    for name in ("score_overlap_dev", "score_overlap", "align_pair_overlap_dev", "align_pair_overlap"):
        sig = inspect.signature(getattr(gsa.Engine, name))
        assert sig.parameters["gape"].default is None
        if "stream" in sig.parameters:
            assert sig.parameters["stream"].default is None
        if "scratch_limit" in sig.parameters:
            assert sig.parameters["scratch_limit"].default == 0


def test_makefile_builds_both_units_with_reports():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    objs = re.search(r"^OBJS = (.*)$", mk, re.M).group(1).split()
    for unit in ("nw_kscore_overlap", "nw_pair_overlap_trace"):
        assert "build/%s.o" % unit in objs
        rule = re.search(r"^build/%s\.o:.*\n\t(.*)$" % unit, mk, re.M).group(1)
        assert "-Rpass-analysis=kernel-resource-usage" in rule and "build/%s.resources.txt" % unit in rule
        assert "_SCHED" not in rule  # the default scheduler
        assert os.path.exists(os.path.join(CSRC, "build", unit + ".resources.txt"))
    # the trace unit is a translation unit of its own; the score unit is nw_krow.hip under two defines
    src = open(os.path.join(CSRC, "nw_pair_overlap_trace.hip")).read()
    assert not re.search(r'#include\s+"[^"]*\.hip"', src)
    src = open(os.path.join(CSRC, "nw_kscore_overlap.hip")).read()
    code = [l.strip() for l in src.split("\n") if l.strip() and not l.startswith("//")]
    assert code == ["#define GSA_KROW_SCORE", "#define GSA_KSCORE_OVERLAP", '#include "nw_krow.hip"']
    # and the overlap instances live nowhere else
    for other in ("nw_kscore_semi.hip", "nw_kscore_semi_batch.hip", "nw_kscore.hip", "nw_kscore_ag.hip"):
        assert "OVERLAP" not in open(os.path.join(CSRC, other)).read()


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
    kernels = ["nw_overlap_fill_kernelILb%dELi%dE" % (a, k) for a in (0, 1) for k in (8, 16)] + ["nw_overlap_walk_kernel"]
    rep = _report("nw_pair_overlap_trace")
    assert len(rep) == len(kernels) and all(any(k in n for n in rep) for k in kernels), list(rep)
    assert set(rep.values()) == {(0, 0, 0)}, rep


def _score_reports():
    rep = _report("nw_kscore_overlap")
    semi = _report("nw_kscore_semi")
    out = {}
    for lin in (False, True):
        for q8 in (0, 1):
            for k in (2, 4):
                name = "nw_kscore_kernelILi%dELb%dELi%dELb0EE" % (10 if lin else 9, q8, k)
                sname = "nw_kscore_kernelILi%dELb%dELi%dELb0EE" % (8 if lin else 7, q8, k)
                got = [v for n, v in rep.items() if name in n]
                ref = [v for n, v in semi.items() if sname in n]
                assert len(got) == 1 and len(ref) == 1, name
                out[name] = (got[0], ref[0])
    return rep, out


def test_score_report_lists_the_instances_and_none_has_scratch():
    """The report lists the 8 overlap instances (affine mode 9 and linear mode 10, int16 and int8
    profile, K = 2 and 4, single pair) and the finishing kernel; none has scratch or a spilled VGPR."""
    rep, pairs = _score_reports()
    score = {n: v for n, v in rep.items() if "nw_kscore_kernel" in n}
    assert len(score) == 8 and len(rep) == 9 and any("nw_overlap_max_kernel" in n for n in rep)
    for name, (got, _) in pairs.items():
        assert got[0] == 0 and got[2] == 0, (name, got)
    assert [v for n, v in rep.items() if "overlap_max" in n] == [(0, 0, 0)]


def test_score_instances_spill_no_more_than_the_semi_global_ones():
    """No overlap instance has more spilled registers than the semi-global instance of the same gap
    model, profile and K, read from that unit's own report."""
    _, pairs = _score_reports()
    for name, (got, ref) in pairs.items():
        assert got[1] <= ref[1] and got[2] <= ref[2], (name, got, ref)


def test_no_new_launch_kind_and_no_new_knob():
    assert len(gsa.LAUNCH_KINDS) == 11 and gsa.LAUNCH_KINDS[-1] == "score_lanes"
    assert gsa.KNOB_NAMES[-2:] == ("GSA_DB_LANES", "GSA_DB_MAXC") and len(gsa.KNOB_NAMES) == 27
