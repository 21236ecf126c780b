"""The banded batch calls (gsa_score_band_batch_dev, gsa_align_batch_band_dev), the parts that need no GPU:
the entry points in the header, the library and the ctypes bindings, the two structs' layouts against the
header text, the argument check without a context, the Python entry points and their band forms, the
Makefile's rule and the resource report of the new translation unit, the banded single-pair unit's
report next to it, and that the calls add no launch kind and no knob.  The kernels are checked in
tests/test_gpu_score_band_batch.py and tests/test_gpu_align_batch_band.py."""
import ctypes
import inspect
import os
import re

import pytest

import gpuseqalign_amd as gsa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gpuseqalign_amd", "csrc")


def _args(text, name):
    decl = re.search(r"int\s+%s\s*\((.*?)\)\s*;" % name, text, re.S).group(1)
    return [" ".join(a.split()) for a in decl.split(",")]


def test_entry_points_declared_exported_bound():
    """The argument lists are the semi-global batch calls' with the bands, the waves and (score call) the
    grid cap behind gape, and the per-pair info in front of the info struct."""
    text = open(os.path.join(ROOT, "include", "gsa.h")).read()
    i32, i64p = ctypes.c_int32, ctypes.POINTER(ctypes.c_int64)
    want = _args(text, "gsa_score_semi_batch_dev")
    want[7:7] = ["const int64_t* band_lo", "const int64_t* band_hi", "int32_t waves", "int32_t max_workgroups"]
    assert _args(text, "gsa_score_band_batch_dev") == want and len(want) == 14
    res, args = gsa.SIGNATURES["gsa_score_band_batch_dev"]
    sargs = list(gsa.SIGNATURES["gsa_score_semi_batch_dev"][1])
    sargs[7:7] = [i64p, i64p, i32, i32]
    assert res is ctypes.c_int and args == sargs

    want = [a.replace("gsa_align_batch_semi_info", "gsa_align_batch_band_info") for a in _args(text, "gsa_align_batch_semi_dev")]
    assert want[7] == "int32_t max_workgroups"
    want[7:7] = ["const int64_t* band_lo", "const int64_t* band_hi", "int32_t waves"]
    k = want.index("gsa_align_batch_band_info* info")
    want[k:k] = ["gsa_align_batch_band_pair* pair_info"]
    assert _args(text, "gsa_align_batch_band_dev") == want and len(want) == 20
    res, args = gsa.SIGNATURES["gsa_align_batch_band_dev"]
    sargs = [ctypes.POINTER(gsa.AlignBatchBandInfo) if a is ctypes.POINTER(gsa.AlignBatchSemiInfo) else a
             for a in gsa.SIGNATURES["gsa_align_batch_semi_dev"][1]]
    sargs[7:7] = [i64p, i64p, i32]
    sargs[k:k] = [ctypes.POINTER(gsa.AlignBatchBandPair)]
    assert res is ctypes.c_int and args == sargs
    for name in ("gsa_score_band_batch_dev", "gsa_align_batch_band_dev"):
        assert hasattr(gsa.lib(), name)


def test_semantics_are_stated_in_the_header():
    text = " ".join(open(os.path.join(ROOT, "include", "gsa.h")).read().replace("*", " ").split())
    for phrase in ("out[p] is exactly what gsa_score_band_dev returns for pair p alone with band_lo[p], band_hi[p]",
                   "out[p] is, field for field, what gsa_align_pair_band_dev returns for pair p alone with band_lo[p], band_hi[p]",
                   "whatever the pair's position or neighbours in the list, the waves per workgroup, max_workgroups, "
                   "the round it lands in, or whether two entries name the same buffers",
                   "W <= 1218 at 4 waves, 2754 at 8 and 5826 at 16",
                   "It is an argument and no knob: no result depends on it",
                   "taken by code bytes descending, ties by index; a round takes every pair that still fits the bytes left",
                   "0 is the default, 8 GiB",
                   "a pair's offset independent of cigar_cap, status 2 for a string that does not fit",
                   "npairs = 0 succeeds with nothing launched",
                   "Nothing polls memory and no workgroup waits for another"):
        assert phrase in text, phrase


def _struct(text, name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    decls = [d.split(None, 1) for d in body.split(";") if d.strip()]
    assert {t for t, _ in decls} <= {"int32_t", "int64_t", "float"}
    ctype = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "float": ctypes.c_float}
    return [(n.strip(), ctype[t]) for t, rest in decls for n in rest.split(",")]


def test_struct_layouts():
    text = open(os.path.join(ROOT, "include", "gsa.h")).read()
    P, I = gsa.AlignBatchBandPair, gsa.AlignBatchBandInfo
    assert _struct(text, "gsa_align_batch_band_pair") == list(P._fields_)
    assert _struct(text, "gsa_align_batch_band_info") == list(I._fields_)
    assert ctypes.sizeof(P) == 40 and ctypes.sizeof(I) == 48 and ctypes.sizeof(P) % 8 == 0 == ctypes.sizeof(I) % 8
    assert [(f, getattr(P, f).offset) for f, _ in P._fields_] == [
        ("band_lo", 0), ("band_hi", 8), ("code_bytes", 16), ("strips", 24), ("supersteps", 28), ("proved_optimal", 32),
        ("round", 36)]
    assert [(f, getattr(I, f).offset) for f, _ in I._fields_] == [
        ("batch_pairs", 0), ("host_pairs", 4), ("nocode_pairs", 8), ("rounds", 12), ("waves", 16), ("strip_rows", 20),
        ("code_bytes", 24), ("fill_ms", 32), ("nocode_ms", 36), ("walk_ms", 40), ("pad0", 44)]


def test_null_context_is_invalid_value():
    n = 2
    pairs = (gsa.PairDev * n)()
    lo, hi = (ctypes.c_int64 * n)(-2, -2), (ctypes.c_int64 * n)(2, 2)
    out, sr = (gsa.AlignDbResult * n)(), (gsa.ScoreResult * n)()
    pinfo, info = (gsa.AlignBatchBandPair * n)(), gsa.AlignBatchBandInfo()
    need, ms = ctypes.c_int64(0), ctypes.c_float(0.0)
    st = gsa.lib().gsa_align_batch_band_dev(None, n, pairs, None, 5, -11, -1, lo, hi, 0, 0, 0, out, None, 0,
                                            ctypes.byref(need), pinfo, ctypes.byref(info), ctypes.byref(ms), None)
    assert st == gsa.NwStat.errorInvalidValue
    st = gsa.lib().gsa_score_band_batch_dev(None, n, pairs, None, 5, -11, -1, lo, hi, 0, 0, sr, ctypes.byref(ms), None)
    assert st == gsa.NwStat.errorInvalidValue


def test_python_entry_points():
    """The semi-global batch calls' shapes; bands, waves and (where the semi-global call has none) the grid
    cap are keyword arguments behind them."""
    kw = inspect.Parameter.KEYWORD_ONLY
    want = [("score_band_batch_dev", "score_semi_batch_dev", ["bands", "waves", "max_workgroups"]),
            ("score_band_batch", "score_semi_batch", ["bands", "band", "waves", "max_workgroups"]),
            ("align_batch_band_dev", "align_batch_semi_dev", ["bands", "waves"]),
            ("align_batch_band", "align_batch_semi", ["bands", "band", "waves", "max_workgroups"])]
    for name, semi, extra in want:
        sig = inspect.signature(getattr(gsa.Engine, name))
        ssig = inspect.signature(getattr(gsa.Engine, semi))
        assert list(sig.parameters) == list(ssig.parameters) + extra, name
        for p in ssig.parameters:
            assert sig.parameters[p].default == ssig.parameters[p].default and sig.parameters[p].kind == ssig.parameters[p].kind
        assert all(sig.parameters[p].kind == kw for p in extra), name
        assert sig.parameters["waves"].default == 0
        assert inspect.signature(getattr(gsa.Engine, name)).parameters.get("max_workgroups").default == 0
    for name in ("score_band_batch_dev", "align_batch_band_dev"):
        assert inspect.signature(getattr(gsa.Engine, name)).parameters["bands"].default is inspect.Parameter.empty
    for name in ("score_band_batch", "align_batch_band"):
        sig = inspect.signature(getattr(gsa.Engine, name))
        assert sig.parameters["bands"].default is None and sig.parameters["band"].default is None
    assert list(inspect.signature(gsa.Engine.last_align_batch_band_info).parameters) == ["self"]


def test_host_forms_take_exactly_one_band_form():
    """The check comes before anything touches the device or the engine."""
    e = object.__new__(gsa.Engine)
    pairs, sub = [([0, 1, 1, 0], [0, 1, 0]), ([0, 1], [0, 1, 1, 1])], [[1, -1], [-1, 1]]
    for fn in (gsa.Engine.score_band_batch, gsa.Engine.align_batch_band):
        for kw in ({}, {"bands": [(-1, 0), (0, 2)], "band": 2}):
            with pytest.raises(ValueError):
                fn(e, pairs, sub, -2, -1, **kw)
    # band=k: Engine._band_of per pair
    assert gsa.Engine._bands_of(pairs, None, 4) == [(-5, 4), (-4, 6)] == [gsa.Engine._band_of(3, 2, None, None, 4),
                                                                           gsa.Engine._band_of(1, 3, None, None, 4)]
    assert gsa.Engine._bands_of(pairs, [(-7, 1), (0, 2)], None) == [(-7, 1), (0, 2)]
    # the _dev forms: one band per pair
    for fn in (gsa.Engine.score_band_batch_dev, gsa.Engine.align_batch_band_dev):
        with pytest.raises(ValueError):
            fn(e, [(1, 2, 3, 4)], 0, 2, -2, -1, bands=[])


def test_makefile_builds_the_unit_with_its_report():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    objs = re.search(r"^OBJS = (.*)$", mk, re.M).group(1).split()
    assert "build/nw_band_batch.o" in objs and "build/nw_band.o" in objs
    rule = re.search(r"^build/nw_band_batch\.o:(.*)\n\t(.*)$", mk, re.M)
    assert "-Rpass-analysis=kernel-resource-usage" in rule.group(2) and "build/nw_band_batch.resources.txt" in rule.group(2)
    assert "_SCHED" not in rule.group(2)  # the default scheduler
    for dep in ("nw_band_batch.h", "nw_band_batch_plan.h", "nw_band_dev.h", "nw_band_plan.h"):
        assert dep in rule.group(1), dep
    assert "nw_band_dev.h" in re.search(r"^build/nw_band\.o:(.*)$", mk, re.M).group(1)
    assert os.path.exists(os.path.join(CSRC, "build", "nw_band_batch.resources.txt"))
    # a translation unit of its own that shares the pair's body through a header, and a plan header without HIP
    src = open(os.path.join(CSRC, "nw_band_batch.hip")).read()
    assert not re.search(r'#include\s+"[^"]*\.hip"', src) and '#include "nw_band_dev.h"' in src
    assert '#include "nw_band_dev.h"' in open(os.path.join(CSRC, "nw_band.hip")).read()
    assert src.count("band_pair_fill<") == 1 and "band_dev::band_walk(" in src
    plan = open(os.path.join(CSRC, "nw_band_batch_plan.h")).read()
    assert "hip" not in "".join(l for l in plan.split("\n") if l.startswith("#include"))
    # no spin loop: the fill's loops are counted, in the unit and in the shared body
    dev = open(os.path.join(CSRC, "nw_band_dev.h")).read()
    assert "while (" not in src and "for (;;)" not in src
    assert "while (" not in dev.split("void band_walk")[0] and "for (;;)" not in dev


def _report(unit):
    text = open(os.path.join(CSRC, "build", unit + ".resources.txt")).read()
    out = {}
    for block in text.split("Function Name: ")[1:]:
        name = block.split()[0]
        out[name] = tuple(int(re.search(f + r": (\d+)", block).group(1))
                          for f in ("ScratchSize \\[bytes/lane\\]", "SGPRs Spill", "VGPRs Spill", " VGPRs"))
    return out


def test_instances_have_no_scratch_and_no_spills():
    """The four fill instances (affine or linear, with or without codes) and the walk."""
    kernels = ["nw_band_batch_kernelILb%dELb%dEE" % (a, c) for a in (0, 1) for c in (0, 1)] + ["nw_band_batch_walk_kernel"]
    rep = _report("nw_band_batch")
    assert len(rep) == len(kernels) and all(any(k in n for n in rep) for k in kernels), list(rep)
    assert {v[:3] for v in rep.values()} == {(0, 0, 0)}, rep


def test_the_single_pair_unit_keeps_its_five_kernels_and_registers():
    """nw_band.hip shares its body with the new unit through nw_band_dev.h: the same five kernels, no
    scratch, no spills, and the VGPR counts it had with the body in the unit itself."""
    rep = _report("nw_band")
    want = {"nw_band_kernelILb1ELb1EE": 68, "nw_band_kernelILb0ELb1EE": 56, "nw_band_kernelILb1ELb0EE": 54,
            "nw_band_kernelILb0ELb0EE": 48, "nw_band_walk_kernel": 6}
    assert len(rep) == 5
    for k, vgprs in want.items():
        (name,) = [n for n in rep if k in n]
        assert rep[name] == (0, 0, 0, vgprs), (name, rep[name])


def test_no_new_launch_kind_and_no_new_knob():
    assert len(gsa.LAUNCH_KINDS) == 11 and gsa.LAUNCH_KINDS[-1] == "score_lanes"
    assert gsa.KNOB_NAMES[-2:] == ("GSA_DB_LANES", "GSA_DB_MAXC") and len(gsa.KNOB_NAMES) == 27
