"""The long pairs' batched overlap calls (gsa_score_overlap_batch_dev, gsa_align_batch_overlap_dev), the
parts that need no GPU: the entry points in the header, the library and the ctypes bindings, the header's
wording of the semantics, the info struct's layout, the argument check without a context, the Python entry
points, the Makefile's rules and the resource reports of the two new translation units, that the reports
of the neighbouring units still list the kernels they listed before, and that the calls add no launch kind
and no knob.  The kernels are checked in tests/test_gpu_score_overlap_batch.py and
tests/test_gpu_align_batch_overlap.py."""
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


def _header():
    return open(os.path.join(ROOT, "include", "gsa.h")).read()


def test_entry_points_declared_exported_bound():
    """Both argument lists are the batched semi-global calls'."""
    text = _header()
    for ov, semi, n in (("gsa_score_overlap_batch_dev", "gsa_score_semi_batch_dev", 10),
                        ("gsa_align_batch_overlap_dev", "gsa_align_batch_semi_dev", 16)):
        assert hasattr(gsa.lib(), ov)
        res, args = gsa.SIGNATURES[ov]
        want = [a.replace("gsa_align_batch_semi_info", "gsa_align_batch_overlap_info") for a in _args(text, semi)]
        assert res is ctypes.c_int and len(args) == len(want) == n
        assert _args(text, ov) == want
        sres, sargs = gsa.SIGNATURES[semi]
        assert [a for a in args if a is not ctypes.POINTER(gsa.AlignBatchOverlapInfo)] == \
            [a for a in sargs if a is not ctypes.POINTER(gsa.AlignBatchSemiInfo)]
    assert gsa.SIGNATURES["gsa_align_batch_overlap_dev"][1][13] == ctypes.POINTER(gsa.AlignBatchOverlapInfo)


def test_header_states_the_semantics():
    text = " ".join(re.sub(r"^\s*\*", "", l) for l in _header().split("\n"))
    text = " ".join(text.split())
    for phrase in (
            "out[p] is exactly what gsa_score_overlap_dev returns for pair p alone, with calc_kernel_ms 0",
            "whatever the pair's position or neighbours in the list, the rows per lane and the profile width",
            "two entries may name the same buffers",
            "out[p] is, field for field, what gsa_align_pair_overlap_dev returns for pair p alone",
            "whatever the strip height, the round, the pair's position or neighbours in the list and max_workgroups",
            "a pair's offset independent of cigar_cap, status 2 for a string that does not fit",
            "Status 1 -- score and end cell valid, start cell 0, an empty CIGAR -- for a pair one strip of whose codes "
            "(j_end TR / 2 bytes) exceeds scratch_limit",
            "here the other pairs are unaffected",
            "0 is the default, 8 GiB",
            "the rows past R are stored too",
            "adds no launch kind and no knob"):
        assert phrase in text, phrase


def test_info_struct_layout():
    text = _header()
    body = re.search(r"typedef struct gsa_align_batch_overlap_info \{(.*?)\} gsa_align_batch_overlap_info;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n.strip() for decl in body.split(";") if decl.strip() for n in decl.split(None, 1)[1].split(",")]
    assert names == [f[0] for f in gsa.AlignBatchOverlapInfo._fields_]
    I = gsa.AlignBatchOverlapInfo
    assert ctypes.sizeof(I) == 56 and ctypes.sizeof(I) % 8 == 0 and ctypes.alignment(I) == 8
    assert [(f, getattr(I, f).offset) for f, _ in I._fields_] == [
        ("batch_pairs", 0), ("host_pairs", 4), ("strip_rows", 8), ("strips", 12), ("strips_filled", 16), ("rounds", 20),
        ("code_bytes", 24), ("gran_bytes", 32), ("score_ms", 40), ("fill_ms", 44), ("walk_ms", 48), ("pad0", 52)]
    assert [t for f, t in I._fields_ if f in ("code_bytes", "gran_bytes")] == [ctypes.c_int64] * 2


def test_null_context_is_invalid_value():
    out, info, sr = gsa.AlignDbResult(), gsa.AlignBatchOverlapInfo(), gsa.ScoreResult()
    need, ms = ctypes.c_int64(0), ctypes.c_float(0.0)
    pairs = (gsa.PairDev * 1)()
    st = gsa.lib().gsa_align_batch_overlap_dev(None, 1, pairs, None, 25, -11, -1, 0, 0, ctypes.byref(out), None, 0,
                                               ctypes.byref(need), ctypes.byref(info), ctypes.byref(ms), None)
    assert st == gsa.NwStat.errorInvalidValue
    st = gsa.lib().gsa_score_overlap_batch_dev(None, 1, pairs, None, 25, -11, -1, ctypes.byref(sr), ctypes.byref(ms), None)
    assert st == gsa.NwStat.errorInvalidValue


def test_python_entry_points():
    """Shaped like the batched semi-global methods, defaults included."""
    for ov, semi in (("score_overlap_batch_dev", "score_semi_batch_dev"), ("score_overlap_batch", "score_semi_batch"),
                     ("align_batch_overlap_dev", "align_batch_semi_dev"), ("align_batch_overlap", "align_batch_semi"),
                     ("last_align_batch_overlap_info", "last_align_batch_semi_info")):
        a, b = inspect.signature(getattr(gsa.Engine, ov)), inspect.signature(getattr(gsa.Engine, semi))
        assert [(p.name, p.default) for p in a.parameters.values()] == [(p.name, p.default) for p in b.parameters.values()], ov
    sig = inspect.signature(gsa.Engine.align_batch_overlap_dev)
    assert (sig.parameters["max_workgroups"].default, sig.parameters["scratch_limit"].default) == (0, 0)
    src = inspect.getsource(gsa.Engine.align_batch_overlap) + inspect.getsource(gsa.Engine.score_overlap_batch)
    assert src.count("self._upload_pairs(pairs, subst)") == 2


def test_makefile_builds_both_units_with_reports():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    objs = re.search(r"^OBJS = (.*)$", mk, re.M).group(1).split()
    for unit in ("nw_kscore_overlap_batch", "nw_pair_overlap_trace_batch"):
        assert "build/%s.o" % unit in objs
        rule = re.search(r"^build/%s\.o:.*\n\t(.*)$" % unit, mk, re.M).group(1)
        assert "-Rpass-analysis=kernel-resource-usage" in rule and "build/%s.resources.txt" % unit in rule
        assert "_SCHED" not in rule  # the default scheduler
        assert os.path.exists(os.path.join(CSRC, "build", unit + ".resources.txt"))
    # the trace unit is a translation unit of its own; the score unit is nw_krow.hip under two defines
    src = open(os.path.join(CSRC, "nw_pair_overlap_trace_batch.hip")).read()
    assert not re.search(r'#include\s+"[^"]*\.hip"', src)
    src = open(os.path.join(CSRC, "nw_kscore_overlap_batch.hip")).read()
    code = [l.strip() for l in src.split("\n") if l.strip() and not l.startswith("//")]
    assert code == ["#define GSA_KROW_SCORE", "#define GSA_KSCORE_OVERLAP_BATCH", '#include "nw_krow.hip"']
    # the plan is free of HIP
    plan = open(os.path.join(CSRC, "nw_pair_overlap_trace_batch_plan.h")).read()
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
    kernels = ["nw_overlap_batch_fill_kernelILb%dELi%dE" % (a, k) for a in (0, 1) for k in (8, 16)] + ["nw_overlap_batch_walk_kernel"]
    rep = _report("nw_pair_overlap_trace_batch")
    assert len(rep) == len(kernels) and all(any(k in n for n in rep) for k in kernels), list(rep)
    assert set(rep.values()) == {(0, 0, 0)}, rep


def test_score_instances_have_no_scratch_and_spill_no_more_than_the_single_pair_ones():
    """The report lists the 8 batched overlap instances (affine mode 9 and linear mode 10, int16 and int8
    profile, K = 2 and 4, BATCH) and the finishing kernel, 9 in all; none has scratch or a spilled VGPR,
    and none spills more SGPRs than nw_kscore_overlap's single-pair instance of the same gap model,
    profile and K."""
    rep = _report("nw_kscore_overlap_batch")
    single = _report("nw_kscore_overlap")
    score = {n: v for n, v in rep.items() if "nw_kscore_kernel" in n}
    assert len(score) == 8 and len(rep) == 9 and any("nw_overlap_max_batch_kernel" in n for n in rep)
    for mode in (9, 10):
        for q8 in (0, 1):
            for k in (2, 4):
                got = [v for n, v in score.items() if "nw_kscore_kernelILi%dELb%dELi%dELb1EE" % (mode, q8, k) in n]
                one = [v for n, v in single.items() if "nw_kscore_kernelILi%dELb%dELi%dELb0EE" % (mode, q8, k) in n]
                assert len(got) == 1 and len(one) == 1, (mode, q8, k)
                assert got[0][0] == 0 and got[0][2] == 0, (mode, q8, k, got[0])
                assert got[0][1] <= one[0][1], (mode, q8, k, got[0], one[0])
    assert [v for n, v in rep.items() if "nw_overlap_max_batch_kernel" in n] == [(0, 0, 0)]


def test_neighbouring_reports_list_the_kernels_they_listed():
    """nw_kscore_overlap: 8 single-pair score instances and the maximum's kernel; nw_pair_overlap_trace:
    4 fills and the walk; nw_kscore_semi_batch: 8 batched instances and the row maximum."""
    rep = _report("nw_kscore_overlap")
    want = ["nw_kscore_kernelILi%dELb%dELi%dELb0EE" % (m, q, k) for m in (9, 10) for q in (0, 1) for k in (2, 4)]
    assert len(rep) == 9 and all(any(w in n for n in rep) for w in want + ["nw_overlap_max_kernel"]), list(rep)
    rep = _report("nw_pair_overlap_trace")
    want = ["nw_overlap_fill_kernelILb%dELi%dE" % (a, k) for a in (0, 1) for k in (8, 16)] + ["nw_overlap_walk_kernel"]
    assert len(rep) == 5 and all(any(w in n for n in rep) for w in want), list(rep)
    rep = _report("nw_kscore_semi_batch")
    want = ["nw_kscore_kernelILi%dELb%dELi%dELb1EE" % (m, q, k) for m in (7, 8) for q in (0, 1) for k in (2, 4)]
    assert len(rep) == 9 and all(any(w in n for n in rep) for w in want + ["nw_semi_rowmax_batch_kernel"]), list(rep)


def test_no_new_launch_kind_and_no_new_knob():
    assert len(gsa.LAUNCH_KINDS) == 11 and gsa.LAUNCH_KINDS[-1] == "score_lanes"
    assert gsa.KNOB_NAMES[-2:] == ("GSA_DB_LANES", "GSA_DB_MAXC") and len(gsa.KNOB_NAMES) == 27
