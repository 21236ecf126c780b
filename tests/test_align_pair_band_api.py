"""The long pairs' banded calls (gsa_score_band_dev, gsa_align_pair_band_dev), the parts that need no GPU:
the entry points in the header, the library and the ctypes bindings, the info struct's layout, the
argument check without a context, the Python entry points, the Makefile's rule and the resource report of
the new translation unit, and that the calls add no launch kind and no knob.  The kernels are checked in
tests/test_gpu_score_band.py and tests/test_gpu_align_pair_band.py."""
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
    """The argument lists are the semi-global calls' with the band behind gape and the band's info struct."""
    text = open(os.path.join(ROOT, "include", "gsa.h")).read()
    for band, semi, n in (("gsa_score_band_dev", "gsa_score_semi_dev", 13),
                          ("gsa_align_pair_band_dev", "gsa_align_pair_semi_dev", 19)):
        assert hasattr(gsa.lib(), band)
        res, args = gsa.SIGNATURES[band]
        want = [a.replace("gsa_align_pair_semi_info", "gsa_align_pair_band_info") for a in _args(text, semi)]
        want[9:9] = ["int64_t band_lo", "int64_t band_hi"]
        assert res is ctypes.c_int and len(args) == len(want) == n
        assert _args(text, band) == want
        sargs = list(gsa.SIGNATURES[semi][1])
        sargs[9:9] = [ctypes.c_int64, ctypes.c_int64]
        assert [a for a in args if a is not ctypes.POINTER(gsa.AlignPairBandInfo)] == \
            [a for a in sargs if a is not ctypes.POINTER(gsa.AlignPairSemiInfo)]
    assert gsa.SIGNATURES["gsa_align_pair_band_dev"][1][16] == ctypes.POINTER(gsa.AlignPairBandInfo)
    assert re.search(r"int64_t\s+gsa_band_max_width\s*\(\s*void\s*\)\s*;", text)
    assert gsa.SIGNATURES["gsa_band_max_width"] == (ctypes.c_int64, [])
    # no context is needed: the limit is a compile-time constant of the library
    assert gsa.band_max_width() == gsa.lib().gsa_band_max_width() == 64 * 16 * 6 - 256 + 1 - 63 >= 4096


def test_semantics_are_stated_in_the_header():
    text = " ".join(open(os.path.join(ROOT, "include", "gsa.h")).read().replace("*", " ").split())
    for phrase in ("is in the band iff band_lo <= j - i <= band_hi",
                   "Every cell outside the band has H = E = F = minus infinity, border cells included",
                   "Row 0: H = E = go + (j - 1) ge, F = minus infinity",
                   "Column 0: H = F = go + (i - 1) ge, E = minus infinity",
                   "Walk from (R, C) in state H: diagonal before F before E",
                   "A gap is extended only when that is strictly better than opening",
                   "band_lo <= min(0, C - R) and band_hi >= max(0, C - R), else errorInvalidValue",
                   "The call clamps band_lo to -R and band_hi to C",
                   "U_hi = pmax (C - band_hi - 1) + 2 gapo + band_hi gape + (band_hi - D) gape",
                   "U_lo = pmax (R - a) + 2 gapo + (a - 1) gape + (a + D - 1) gape",
                   "proved_optimal = 1 iff S is strictly greater than every bound that applies"):
        assert phrase in text, phrase


def test_info_struct_layout():
    text = open(os.path.join(ROOT, "include", "gsa.h")).read()
    body = re.search(r"typedef struct gsa_align_pair_band_info \{(.*?)\} gsa_align_pair_band_info;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    decls = [d.split(None, 1) for d in body.split(";") if d.strip()]
    assert {t for t, _ in decls} <= {"int32_t", "int64_t", "float"}
    names = [n.strip() for _, rest in decls for n in rest.split(",")]
    assert names == [f[0] for f in gsa.AlignPairBandInfo._fields_]
    I = gsa.AlignPairBandInfo
    assert ctypes.sizeof(I) == 56 and ctypes.sizeof(I) % 8 == 0
    assert [(f, getattr(I, f).offset) for f, _ in I._fields_] == [
        ("strip_rows", 0), ("strips", 4), ("waves", 8), ("supersteps", 12), ("proved_optimal", 16), ("pad0", 20),
        ("band_lo", 24), ("band_hi", 32), ("code_bytes", 40), ("score_ms", 48), ("walk_ms", 52)]


def test_null_context_is_invalid_value():
    out, info, sr = gsa.AlignDbResult(), gsa.AlignPairBandInfo(), gsa.ScoreResult()
    need, ms = ctypes.c_int64(0), ctypes.c_float(0.0)
    st = gsa.lib().gsa_align_pair_band_dev(None, None, 5, None, 5, None, 25, -11, -1, -2, 2, 0, ctypes.byref(out), None, 0,
                                           ctypes.byref(need), ctypes.byref(info), ctypes.byref(ms), None)
    assert st == gsa.NwStat.errorInvalidValue
    st = gsa.lib().gsa_score_band_dev(None, None, 5, None, 5, None, 25, -11, -1, -2, 2, ctypes.byref(sr), None)
    assert st == gsa.NwStat.errorInvalidValue


def test_python_entry_points():
    dev = ["seqY_ptr", "adjrows", "seqX_ptr", "adjcols", "subst_ptr", "substsz", "gapo", "gape", "band_lo", "band_hi"]
    host = ["seqY", "seqX", "subst", "gapo", "gape", "band_lo", "band_hi", "band"]
    want = [("score_band_dev", dev + ["stream"]),
            ("score_band", host),
            ("align_pair_band_dev", dev + ["scratch_limit", "stream"]),
            ("align_pair_band", host + ["scratch_limit"]),
            ("last_align_pair_band_info", [])]
    for name, params in want:
        sig = inspect.signature(getattr(gsa.Engine, name))
        assert list(sig.parameters)[1:] == params, name
        # the semi-global call's shape, with the band behind gape
        semi = list(inspect.signature(getattr(gsa.Engine, name.replace("band", "semi"))).parameters)
        assert [p for p in sig.parameters if p not in ("band_lo", "band_hi", "band")] == semi, name
    for name in ("score_band", "align_pair_band"):
        sig = inspect.signature(getattr(gsa.Engine, name))
        assert all(sig.parameters[p].default is None for p in ("gape", "band_lo", "band_hi", "band"))
    for name in ("score_band_dev", "align_pair_band_dev"):
        assert inspect.signature(getattr(gsa.Engine, name)).parameters["stream"].default is None
    for name in ("align_pair_band_dev", "align_pair_band"):
        assert inspect.signature(getattr(gsa.Engine, name)).parameters["scratch_limit"].default == 0


def test_host_forms_take_exactly_one_band_form():
    """The check comes before anything touches the device or the engine."""
    e = object.__new__(gsa.Engine)
    y, x, sub = [0, 1, 1, 0], [0, 1, 0], [[1, -1], [-1, 1]]
    for fn in (gsa.Engine.score_band, gsa.Engine.align_pair_band):
        for kw in ({}, {"band_lo": -1}, {"band_hi": 1}, {"band_lo": -1, "band_hi": 0, "band": 2}, {"band_lo": -1, "band": 2}):
            with pytest.raises(ValueError):
                fn(e, y, x, sub, -2, -1, **kw)
    # band=k: k diagonals beyond the ones (0, 0) and (R, C) need
    assert gsa.Engine._band_of(3, 2, None, None, 4) == (-5, 4) and gsa.Engine._band_of(2, 9, None, None, 0) == (0, 7)
    assert gsa.Engine._band_of(3, 2, -7, 1, None) == (-7, 1)


def test_makefile_builds_the_unit_with_its_report():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    objs = re.search(r"^OBJS = (.*)$", mk, re.M).group(1).split()
    assert "build/nw_band.o" in objs
    rule = re.search(r"^build/nw_band\.o:(.*)\n\t(.*)$", mk, re.M)
    assert "-Rpass-analysis=kernel-resource-usage" in rule.group(2) and "build/nw_band.resources.txt" in rule.group(2)
    assert "_SCHED" not in rule.group(2)  # the default scheduler
    assert "nw_band_plan.h" in rule.group(1) and "nw_band.h" in rule.group(1)
    assert os.path.exists(os.path.join(CSRC, "build", "nw_band.resources.txt"))
    # a translation unit of its own, and a plan header without HIP
    src = open(os.path.join(CSRC, "nw_band.hip")).read()
    assert not re.search(r'#include\s+"[^"]*\.hip"', src)
    plan = open(os.path.join(CSRC, "nw_band_plan.h")).read()
    assert "hip" not in "".join(l for l in plan.split("\n") if l.startswith("#include"))
    # no spin loop: the kernels' only loops are counted
    assert "while (" not in src.split("nw_band_walk_kernel")[0]


def _report(unit):
    text = open(os.path.join(CSRC, "build", unit + ".resources.txt")).read()
    out = {}
    for block in text.split("Function Name: ")[1:]:
        name = block.split()[0]
        out[name] = tuple(int(re.search(f + r": (\d+)", block).group(1))
                          for f in ("ScratchSize \\[bytes/lane\\]", "SGPRs Spill", "VGPRs Spill"))
    return out


def test_instances_have_no_scratch_and_no_spills():
    """The four fill instances (affine or linear, with or without codes) and the walk."""
    kernels = ["nw_band_kernelILb%dELb%dEE" % (a, c) for a in (0, 1) for c in (0, 1)] + ["nw_band_walk_kernel"]
    rep = _report("nw_band")
    assert len(rep) == len(kernels) and all(any(k in n for n in rep) for k in kernels), list(rep)
    assert set(rep.values()) == {(0, 0, 0)}, rep


def test_no_new_launch_kind_and_no_new_knob():
    assert len(gsa.LAUNCH_KINDS) == 11 and gsa.LAUNCH_KINDS[-1] == "score_lanes"
    assert gsa.KNOB_NAMES[-2:] == ("GSA_DB_LANES", "GSA_DB_MAXC") and len(gsa.KNOB_NAMES) == 27
