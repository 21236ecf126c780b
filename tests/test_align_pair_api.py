"""The alignment of one long pair (gsa_align_pair_dev), the parts that need no GPU: the entry point in
the header, the library and the ctypes bindings, the info struct's layout, its argument check without a
context, the Python entry points, the new translation unit's resource report, and that the call adds
no launch kind and no knob.  The kernels are checked in tests/test_gpu_align_pair.py."""
import ctypes
import inspect
import os
import re

import gpuseqalign_amd as gsa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gpuseqalign_amd", "csrc")


def test_entry_point_declared_exported_bound():
    text = open(os.path.join(ROOT, "include", "gsa.h")).read()
    assert hasattr(gsa.lib(), "gsa_align_pair_dev")
    res, args = gsa.SIGNATURES["gsa_align_pair_dev"]
    decl = re.search(r"int\s+gsa_align_pair_dev\s*\((.*?)\)\s*;", text, re.S).group(1)
    norm = [" ".join(a.split()) for a in decl.split(",")]
    assert res is ctypes.c_int and len(args) == len(norm) == 18
    # gsa_score_dev's arguments up to `local`, then gsa_align_db_dev's from scratch_limit on, with the pair's info
    score = [" ".join(a.split()) for a in re.search(r"int\s+gsa_score_dev\s*\((.*?)\)\s*;", text, re.S).group(1).split(",")]
    db = [" ".join(a.split()) for a in re.search(r"int\s+gsa_align_db_dev\s*\((.*?)\)\s*;", text, re.S).group(1).split(",")]
    assert norm[:10] == score[:10]
    assert norm[10:] == [a.replace("gsa_align_db_info", "gsa_align_pair_info") for a in db[db.index("int64_t scratch_limit"):]]
    assert args[11] == ctypes.POINTER(gsa.AlignDbResult) and args[15] == ctypes.POINTER(gsa.AlignPairInfo)


def test_info_struct_layout():
    text = open(os.path.join(ROOT, "include", "gsa.h")).read()
    body = re.search(r"typedef struct gsa_align_pair_info \{(.*?)\} gsa_align_pair_info;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n.strip() for decl in body.split(";") if decl.strip() for n in decl.split(None, 1)[1].split(",")]
    assert names == [f[0] for f in gsa.AlignPairInfo._fields_]
    I = gsa.AlignPairInfo
    assert ctypes.sizeof(I) == 40
    assert [(f, getattr(I, f).offset) for f, _ in I._fields_] == [
        ("strip_rows", 0), ("strips", 4), ("strips_filled", 8), ("chunks", 12), ("code_bytes", 16), ("score_ms", 24),
        ("fill_ms", 28), ("walk_ms", 32), ("pad0", 36)]
    assert ctypes.sizeof(gsa.AlignDbResult) == 56


def test_null_context_is_invalid_value():
    out, info = gsa.AlignDbResult(), gsa.AlignPairInfo()
    need, ms = ctypes.c_int64(0), ctypes.c_float(0.0)
    st = gsa.lib().gsa_align_pair_dev(None, None, 5, None, 5, None, 25, -11, -1, 0, 0, ctypes.byref(out), None, 0,
                                      ctypes.byref(need), ctypes.byref(info), ctypes.byref(ms), None)
    assert st == gsa.NwStat.errorInvalidValue


def test_python_entry_points():
    want = [("align_pair_dev", ["seqY_ptr", "adjrows", "seqX_ptr", "adjcols", "subst_ptr", "substsz", "gapo", "gape",
                                "local", "scratch_limit", "stream"]),
            ("align_pair", ["seqY", "seqX", "subst", "gapo", "gape", "local", "scratch_limit"]),
            ("last_align_pair_info", [])]
    for name, params in want:
        sig = inspect.signature(getattr(gsa.Engine, name))
        assert list(sig.parameters)[1:] == params, name
    sig = inspect.signature(gsa.Engine.align_pair)
    assert [sig.parameters[k].default for k in ("gape", "local", "scratch_limit")] == [None, False, 0]


def test_new_instances_have_no_scratch_and_no_spills():
    """The build's resource report of the new translation unit: the eight fill instances (local or
    global, affine or linear, 8 or 16 rows per lane) and the walk, none with scratch or a spilled
    register."""
    kernels = ["nw_pair_fill_kernelILb%dELb%dELi%dE" % (l, a, k) for l in (0, 1) for a in (0, 1) for k in (8, 16)]
    kernels.append("nw_pair_walk_kernel")
    text = open(os.path.join(CSRC, "build", "nw_pair_trace.resources.txt")).read()
    names = re.findall(r"Function Name: (\S+)", text)
    assert len(names) == len(kernels) and all(any(k in n for n in names) for k in kernels), names
    for field in ("ScratchSize \\[bytes/lane\\]", "SGPRs Spill", "VGPRs Spill"):
        assert re.findall(field + r": (\d+)", text) == ["0"] * len(kernels), field


def test_existing_lane_units_are_not_touched():
    """The new fill is a translation unit of its own: it includes none of the lane kernels' sources and
    the Makefile builds those as before, each with its report."""
    src = open(os.path.join(CSRC, "nw_pair_trace.hip")).read()
    assert not re.search(r'#include\s+"[^"]*\.hip"', src)
    mk = open(os.path.join(CSRC, "Makefile")).read()
    for unit in ("nw_lanes", "nw_lanes_trace", "nw_lanes_multi", "nw_lanes_trace_multi", "nw_lanes_semi",
                 "nw_lanes_semi_trace", "nw_pair_trace"):
        assert "build/%s.resources.txt" % unit in mk
        assert os.path.exists(os.path.join(CSRC, "build", unit + ".resources.txt"))
    rule = re.search(r"^build/nw_pair_trace\.o:(.*)$", mk, re.M).group(1)
    assert "nw_krow" not in rule and "nw_kscore" not in rule


def test_no_new_launch_kind_and_no_new_knob():
    assert len(gsa.LAUNCH_KINDS) == 11 and gsa.LAUNCH_KINDS[-1] == "score_lanes"
    assert gsa.KNOB_NAMES[-2:] == ("GSA_DB_LANES", "GSA_DB_MAXC") and len(gsa.KNOB_NAMES) == 27
