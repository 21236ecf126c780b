"""The alignments of a batch of long pairs (gsa_align_batch_dev), the parts that need no GPU: the entry
point in the header, the library and the ctypes bindings, the info struct's layout, its argument check
without a context, the Python entry points, the new translation unit's resource report, that the
single-pair unit's report kept every number, and that the call adds no launch kind and no knob.  The
kernels are checked in tests/test_gpu_align_batch.py, the plan in tests/test_align_batch_plan.py."""
import ctypes
import inspect
import os
import re

import gpuseqalign_amd as gsa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gpuseqalign_amd", "csrc")


def _args(text, name):
    return [" ".join(a.split()) for a in re.search(r"int\s+%s\s*\((.*?)\)\s*;" % name, text, re.S).group(1).split(",")]


def test_entry_point_declared_exported_bound():
    text = open(os.path.join(ROOT, "include", "gsa.h")).read()
    assert hasattr(gsa.lib(), "gsa_align_batch_dev")
    res, args = gsa.SIGNATURES["gsa_align_batch_dev"]
    norm = _args(text, "gsa_align_batch_dev")
    assert res is ctypes.c_int and len(args) == len(norm) == 17
    # gsa_score_batch_dev's arguments up to `local`, then gsa_align_db_multi_dev's from max_workgroups on,
    # with the batch's info
    score = _args(text, "gsa_score_batch_dev")
    multi = _args(text, "gsa_align_db_multi_dev")
    assert norm[:8] == score[:8]
    assert norm[8:] == [a.replace("gsa_align_db_multi_info", "gsa_align_batch_info")
                        for a in multi[multi.index("int32_t max_workgroups"):]]
    assert args[2] == ctypes.POINTER(gsa.PairDev) and args[10] == ctypes.POINTER(gsa.AlignDbResult)
    assert args[14] == ctypes.POINTER(gsa.AlignBatchInfo)


def test_info_struct_layout():
    text = open(os.path.join(ROOT, "include", "gsa.h")).read()
    body = re.search(r"typedef struct gsa_align_batch_info \{(.*?)\} gsa_align_batch_info;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n.strip() for decl in body.split(";") if decl.strip() for n in decl.split(None, 1)[1].split(",")]
    assert names == [f[0] for f in gsa.AlignBatchInfo._fields_]
    I = gsa.AlignBatchInfo
    assert ctypes.sizeof(I) == 56 and ctypes.sizeof(I) % 8 == 0
    assert [(f, getattr(I, f).offset) for f, _ in I._fields_] == [
        ("batch_pairs", 0), ("alone_pairs", 4), ("host_pairs", 8), ("strip_rows", 12), ("strips", 16),
        ("strips_filled", 20), ("rounds", 24), ("pad0", 28), ("code_bytes", 32), ("score_ms", 40), ("fill_ms", 44),
        ("walk_ms", 48), ("pad1", 52)]


def test_null_context_is_invalid_value():
    pairs, out, info = (gsa.PairDev * 1)(), (gsa.AlignDbResult * 1)(), gsa.AlignBatchInfo()
    need, ms = ctypes.c_int64(0), ctypes.c_float(0.0)
    st = gsa.lib().gsa_align_batch_dev(None, 1, pairs, None, 25, -11, -1, 0, 0, 0, out, None, 0, ctypes.byref(need),
                                       ctypes.byref(info), ctypes.byref(ms), None)
    assert st == gsa.NwStat.errorInvalidValue


def test_python_entry_points():
    want = [("align_batch_dev", ["pairs", "subst_ptr", "substsz", "gapo", "gape", "local", "max_workgroups",
                                 "scratch_limit", "stream"]),
            ("align_batch", ["pairs", "subst", "gapo", "gape", "local", "scratch_limit"]),
            ("last_align_batch_info", [])]
    for name, params in want:
        sig = inspect.signature(getattr(gsa.Engine, name))
        assert list(sig.parameters)[1:] == params, name
    sig = inspect.signature(gsa.Engine.align_batch_dev)
    assert [sig.parameters[k].default for k in ("gape", "local", "max_workgroups", "scratch_limit", "stream")] == \
        [None, False, 0, 0, None]
    sig = inspect.signature(gsa.Engine.align_batch)
    assert [sig.parameters[k].default for k in ("gape", "local", "scratch_limit")] == [None, False, 0]


def _report(unit):
    """{kernel name: {field: value}} of a unit's resource report."""
    text = open(os.path.join(CSRC, "build", unit + ".resources.txt")).read()
    out = {}
    for block in text.split("Function Name: ")[1:]:
        out[block.split()[0]] = {k.strip(): int(v) for k, v in re.findall(r"remark:\s+([A-Za-z \[\]/]+): (\d+)", block)}
    return out


def test_new_instances_have_no_scratch_and_no_spills():
    """The build's resource report of the new translation unit: the eight fill instances (local or
    global, affine or linear, 8 or 16 rows per lane) and the walk, none with scratch or a spilled
    register."""
    kernels = ["nw_pair_batch_fill_kernelILb%dELb%dELi%dE" % (l, a, k) for l in (0, 1) for a in (0, 1) for k in (8, 16)]
    kernels.append("nw_pair_batch_walk_kernel")
    rep = _report("nw_pair_trace_batch")
    assert len(rep) == len(kernels) and all(any(k in n for n in rep) for k in kernels), list(rep)
    for name, f in rep.items():
        assert (f["ScratchSize [bytes/lane]"], f["SGPRs Spill"], f["VGPRs Spill"]) == (0, 0, 0), (name, f)
        assert f["LDS Size [bytes/block]"] == (4096 if "fill" in name else 0), (name, f)


# nw_pair_trace.resources.txt as the commit before this unit was added builds it: (instance, SGPRs, VGPRs,
# AGPRs, scratch, occupancy, SGPR spills, VGPR spills, LDS)
PAIR_TRACE_ROWS = [
    ("nw_pair_walk_kernel", 50, 7, 0, 0, 8, 0, 0, 0),
    ("nw_pair_fill_kernelILb1ELb1ELi8E", 59, 63, 0, 0, 8, 0, 0, 4096),
    ("nw_pair_fill_kernelILb1ELb0ELi8E", 57, 54, 0, 0, 8, 0, 0, 4096),
    ("nw_pair_fill_kernelILb0ELb1ELi8E", 59, 65, 0, 0, 7, 0, 0, 4096),
    ("nw_pair_fill_kernelILb0ELb0ELi8E", 57, 54, 0, 0, 8, 0, 0, 4096),
    ("nw_pair_fill_kernelILb1ELb1ELi16E", 59, 100, 0, 0, 4, 0, 0, 4096),
    ("nw_pair_fill_kernelILb1ELb0ELi16E", 57, 55, 0, 0, 8, 0, 0, 4096),
    ("nw_pair_fill_kernelILb0ELb1ELi16E", 59, 89, 0, 0, 5, 0, 0, 4096),
    ("nw_pair_fill_kernelILb0ELb0ELi16E", 57, 66, 0, 0, 7, 0, 0, 4096),
]


def test_single_pair_unit_keeps_its_nine_kernels_and_numbers():
    """nw_pair_trace.hip is not touched by the batch (the new unit carries its own copy of the body): it
    includes no .hip file, and its nine kernels keep every numeric field of the resource report."""
    src = open(os.path.join(CSRC, "nw_pair_trace.hip")).read()
    assert not re.search(r'#include\s+"[^"]*\.hip"', src) and "nw_pair_trace_batch" not in src
    rep = _report("nw_pair_trace")
    assert len(rep) == 9
    fields = ("TotalSGPRs", "VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "SGPRs Spill",
              "VGPRs Spill", "LDS Size [bytes/block]")
    for row in PAIR_TRACE_ROWS:
        [name] = [n for n in rep if row[0] in n]
        assert tuple(rep[name][f] for f in fields) == row[1:], (name, rep[name])


def test_makefile_builds_the_unit_with_its_report():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "build/nw_pair_trace_batch.o" in re.search(r"^OBJS = (.*)$", mk, re.M).group(1)
    rule = re.search(r"^build/nw_pair_trace_batch\.o:(.*)\n\t(.*)$", mk, re.M)
    assert "nw_pair_trace_batch.hip" in rule.group(1) and "nw_krow" not in rule.group(1)
    assert "build/nw_pair_trace_batch.resources.txt" in rule.group(2) and "sched-strategy" not in rule.group(2)
    assert "_SCHED" not in rule.group(2)  # the default scheduler
    score = re.search(r"^build/gsa_score\.o:(.*)$", mk, re.M).group(1)
    assert "nw_pair_trace_batch.h" in score and "nw_pair_trace_batch_plan.h" in score
    for unit in ("nw_lanes", "nw_lanes_trace", "nw_lanes_multi", "nw_lanes_trace_multi", "nw_lanes_semi",
                 "nw_lanes_semi_trace", "nw_pair_trace", "nw_pair_trace_batch"):
        assert os.path.exists(os.path.join(CSRC, "build", unit + ".resources.txt"))


def test_no_new_launch_kind_and_no_new_knob():
    assert len(gsa.LAUNCH_KINDS) == 11 and gsa.LAUNCH_KINDS[-1] == "score_lanes"
    assert gsa.KNOB_NAMES[-2:] == ("GSA_DB_LANES", "GSA_DB_MAXC") and len(gsa.KNOB_NAMES) == 27
