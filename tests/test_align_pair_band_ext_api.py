"""The banded extension calls of one pair (gsa_score_band_ext_dev, gsa_align_pair_band_ext_dev;
DESIGN.md 2.2r), the parts that need no GPU: the entry points in the header, the library and the ctypes
bindings, the info struct's layout, the argument check without a context, the Python entry points and
their band forms, the Makefile's rule and the resource report of the new translation unit, and that the
global banded kernels kept the registers, LDS and occupancy they had before the body got its extension
mode.  The kernels are checked in tests/test_gpu_score_band_ext.py and
tests/test_gpu_align_pair_band_ext.py."""
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
    """The argument lists are the global banded calls', with the extension's info struct."""
    text = open(os.path.join(ROOT, "include", "gsa.h")).read()
    for ext, band, n in (("gsa_score_band_ext_dev", "gsa_score_band_dev", 13),
                         ("gsa_align_pair_band_ext_dev", "gsa_align_pair_band_dev", 19)):
        assert hasattr(gsa.lib(), ext)
        res, args = gsa.SIGNATURES[ext]
        want = [a.replace("gsa_align_pair_band_info", "gsa_align_pair_band_ext_info") for a in _args(text, band)]
        assert res is ctypes.c_int and len(args) == len(want) == n
        assert _args(text, ext) == want
        assert [a for a in args if a is not ctypes.POINTER(gsa.AlignPairBandExtInfo)] == \
            [a for a in gsa.SIGNATURES[band][1] if a is not ctypes.POINTER(gsa.AlignPairBandInfo)]
    assert gsa.SIGNATURES["gsa_align_pair_band_ext_dev"][1][16] == ctypes.POINTER(gsa.AlignPairBandExtInfo)


def test_semantics_are_stated_in_the_header():
    text = " ".join(open(os.path.join(ROOT, "include", "gsa.h")).read().replace("*", " ").split())
    for phrase in ("the band must hold (0, 0): band_lo <= 0 <= band_hi, else errorInvalidValue",
                   "It need not hold (R, C)",
                   "Score: the maximum of H over all cells of the band",
                   "the first maximal cell in row-major order (smallest i, then smallest j)",
                   "A score of 0 therefore ends at (0, 0) with an empty CIGAR and status 0",
                   "diagonal before F before E; a gap is extended only when that is strictly better than opening",
                   "consumes exactly i_end letters of seqY and j_end letters of seqX",
                   "R = 0 or C = 0 is answered on the host: score 0, end (0, 0), an empty CIGAR, status 0, proved_optimal 1",
                   "R' = min(R, C - band_lo), C' = min(C, R + band_hi)",
                   "U_hi = pmax min(R, C - band_hi - 1) + gapo + band_hi gape",
                   "U_lo = pmax min(C, R - a) + gapo + (a - 1) gape",
                   "proved_optimal = 1 iff S is strictly greater than every bound that applies",
                   "Nothing polls memory and the reduction uses no atomics"):
        assert phrase in text, phrase


def test_info_struct_layout():
    text = open(os.path.join(ROOT, "include", "gsa.h")).read()
    body = re.search(r"typedef struct gsa_align_pair_band_ext_info \{(.*?)\} gsa_align_pair_band_ext_info;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    decls = [d.split(None, 1) for d in body.split(";") if d.strip()]
    assert {t for t, _ in decls} <= {"int32_t", "int64_t", "float"}
    names = [n.strip() for _, rest in decls for n in rest.split(",")]
    I = gsa.AlignPairBandExtInfo
    assert names == [f[0] for f in I._fields_]
    # the band info's fields, then the trimmed pair
    assert list(I._fields_[:len(gsa.AlignPairBandInfo._fields_)]) == list(gsa.AlignPairBandInfo._fields_)
    assert ctypes.sizeof(I) == 72 and ctypes.sizeof(I) % 8 == 0
    assert [(f, getattr(I, f).offset) for f, _ in I._fields_] == [
        ("strip_rows", 0), ("strips", 4), ("waves", 8), ("supersteps", 12), ("proved_optimal", 16), ("pad0", 20),
        ("band_lo", 24), ("band_hi", 32), ("code_bytes", 40), ("score_ms", 48), ("walk_ms", 52), ("rows_used", 56),
        ("cols_used", 64)]


def test_null_context_is_invalid_value():
    out, info, sr = gsa.AlignDbResult(), gsa.AlignPairBandExtInfo(), gsa.ScoreResult()
    need, ms = ctypes.c_int64(0), ctypes.c_float(0.0)
    st = gsa.lib().gsa_align_pair_band_ext_dev(None, None, 5, None, 5, None, 25, -11, -1, -2, 2, 0, ctypes.byref(out), None,
                                               0, ctypes.byref(need), ctypes.byref(info), ctypes.byref(ms), None)
    assert st == gsa.NwStat.errorInvalidValue
    st = gsa.lib().gsa_score_band_ext_dev(None, None, 5, None, 5, None, 25, -11, -1, -2, 2, ctypes.byref(sr), None)
    assert st == gsa.NwStat.errorInvalidValue


def test_python_entry_points():
    """The shape of the global banded wrappers."""
    for name in ("score_band_dev", "score_band", "align_pair_band_dev", "align_pair_band", "last_align_pair_band_info"):
        ext = name.replace("band", "band_ext")
        sig, bsig = inspect.signature(getattr(gsa.Engine, ext)), inspect.signature(getattr(gsa.Engine, name))
        assert list(sig.parameters) == list(bsig.parameters), ext
        for p in sig.parameters:
            assert sig.parameters[p].default == bsig.parameters[p].default and sig.parameters[p].kind == bsig.parameters[p].kind


def test_host_forms_take_exactly_one_band_form():
    """The check comes before anything touches the device or the engine; band=w means (-w, w)."""
    e = object.__new__(gsa.Engine)
    y, x, sub = [0, 1, 1, 0], [0, 1, 0], [[1, -1], [-1, 1]]
    for fn in (gsa.Engine.score_band_ext, gsa.Engine.align_pair_band_ext):
        for kw in ({}, {"band_lo": -1}, {"band_hi": 1}, {"band_lo": -1, "band_hi": 0, "band": 2}, {"band_lo": -1, "band": 2}):
            with pytest.raises(ValueError):
                fn(e, y, x, sub, -2, -1, **kw)
    assert gsa.Engine._band_ext_of(None, None, 4) == (-4, 4) and gsa.Engine._band_ext_of(None, None, 0) == (0, 0)
    assert gsa.Engine._band_ext_of(-7, 1, None) == (-7, 1)


def test_no_info_before_the_first_call():
    e = object.__new__(gsa.Engine)
    with pytest.raises(gsa.NwError):
        e.last_align_pair_band_ext_info()


def test_makefile_builds_the_unit_with_its_report():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    objs = re.search(r"^OBJS = (.*)$", mk, re.M).group(1).split()
    assert "build/nw_band_ext.o" in objs and "build/nw_band.o" in objs
    rule = re.search(r"^build/nw_band_ext\.o:(.*)\n\t(.*)$", mk, re.M)
    assert "-Rpass-analysis=kernel-resource-usage" in rule.group(2) and "build/nw_band_ext.resources.txt" in rule.group(2)
    assert "_SCHED" not in rule.group(2)  # the default scheduler
    for dep in ("nw_band_ext.h", "nw_band_ext_plan.h", "nw_band_dev.h", "nw_band_plan.h", "nw_band.h"):
        assert dep in rule.group(1), dep
    assert os.path.exists(os.path.join(CSRC, "build", "nw_band_ext.resources.txt"))
    # a translation unit of its own that shares the pair's body through the header, and a plan header without HIP
    src = open(os.path.join(CSRC, "nw_band_ext.hip")).read()
    assert not re.search(r'#include\s+"[^"]*\.hip"', src) and '#include "nw_band_dev.h"' in src
    assert src.count("band_pair_fill<AFFINE, CODES, true>") == 1 and "band_dev::band_walk_from_start(" in src
    plan = open(os.path.join(CSRC, "nw_band_ext_plan.h")).read()
    assert "hip" not in "".join(l for l in plan.split("\n") if l.startswith("#include"))
    # the global units keep their instances of the body, without the extension mode
    for unit in ("nw_band.hip", "nw_band_batch.hip"):
        assert open(os.path.join(CSRC, unit)).read().count("band_pair_fill<AFFINE, CODES>(") == 1
    # barriers only: no spin loop and no atomics in the unit or in the shared body's fill
    dev = open(os.path.join(CSRC, "nw_band_dev.h")).read().split("void band_walk")[0]
    for text in (src, dev):
        code = "\n".join(l.split("//")[0] for l in text.split("\n"))
        assert "while (" not in code and "for (;;)" not in code and "atomic" not in code.lower()


def _report(unit):
    text = open(os.path.join(CSRC, "build", unit + ".resources.txt")).read()
    out = {}
    for block in text.split("Function Name: ")[1:]:
        name = block.split()[0]
        out[name] = tuple(int(re.search(f + r": (\d+)", block).group(1))
                          for f in ("ScratchSize \\[bytes/lane\\]", "SGPRs Spill", "VGPRs Spill", " VGPRs", "TotalSGPRs",
                                    "Occupancy \\[waves/SIMD\\]", "LDS Size \\[bytes/block\\]"))
    return out


def test_instances_have_no_scratch_and_no_spills():
    """The four fill instances (affine or linear, with or without codes) and the walk."""
    kernels = ["nw_band_ext_kernelILb%dELb%dEE" % (a, c) for a in (0, 1) for c in (0, 1)] + ["nw_band_ext_walk_kernel"]
    rep = _report("nw_band_ext")
    assert len(rep) == len(kernels) and all(any(k in n for n in rep) for k in kernels), list(rep)
    assert {v[:3] for v in rep.values()} == {(0, 0, 0)}, rep
    # the ring and the table of nw_band.hip and 16 slots of 16 bytes; 16 waves stay resident (4 per SIMD)
    fills = [v for n, v in rep.items() if "walk" not in n]
    assert {v[6] for v in fills} == {28672 + 16 * 16} and min(v[5] for v in fills) >= 4


def test_the_global_fill_instances_are_what_they_were():
    """VGPRs, SGPRs, occupancy and LDS of the eight global banded fill instances, as the reports stated
    them before band_pair_fill got its EXT parameter: with EXT == false it compiles to what it was."""
    want = {"nw_band": {"nw_band_kernelILb1ELb1EE": (68, 62, 7, 28672), "nw_band_kernelILb0ELb1EE": (56, 55, 8, 28672),
                        "nw_band_kernelILb1ELb0EE": (54, 46, 8, 28672), "nw_band_kernelILb0ELb0EE": (48, 46, 8, 28672)},
            "nw_band_batch": {"nw_band_batch_kernelILb1ELb1EE": (72, 74, 7, 4104), "nw_band_batch_kernelILb0ELb1EE": (64, 67, 8, 4104),
                              "nw_band_batch_kernelILb1ELb0EE": (62, 58, 8, 4104), "nw_band_batch_kernelILb0ELb0EE": (56, 58, 8, 4104)}}
    for unit, kernels in want.items():
        rep = _report(unit)
        assert len(rep) == 5
        for k, nums in kernels.items():
            (name,) = [n for n in rep if k in n]
            assert rep[name] == (0, 0, 0) + nums, (name, rep[name])


def test_no_new_launch_kind_and_no_new_knob():
    assert len(gsa.LAUNCH_KINDS) == 11 and gsa.LAUNCH_KINDS[-1] == "score_lanes"
    assert gsa.KNOB_NAMES[-2:] == ("GSA_DB_LANES", "GSA_DB_MAXC") and len(gsa.KNOB_NAMES) == 27
