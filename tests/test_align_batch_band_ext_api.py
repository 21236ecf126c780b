"""The banded extension batch calls (gsa_score_band_ext_batch_dev, gsa_align_batch_band_ext_dev;
DESIGN.md 2.2r), the parts that need no GPU: the entry points in the header, the library and the ctypes
bindings, the two structs' layouts against the header text, the argument check without a context, the
Python entry points and their band forms, the Makefile's rule and the resource report of the new
translation unit.  The kernels are checked in tests/test_gpu_score_band_ext_batch.py and
tests/test_gpu_align_batch_band_ext.py."""
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
    """The argument lists are the global banded batch calls', with the extension's structs."""
    text = open(os.path.join(ROOT, "include", "gsa.h")).read()
    assert _args(text, "gsa_score_band_ext_batch_dev") == _args(text, "gsa_score_band_batch_dev")
    assert gsa.SIGNATURES["gsa_score_band_ext_batch_dev"] == gsa.SIGNATURES["gsa_score_band_batch_dev"]
    want = [a.replace("gsa_align_batch_band_pair", "gsa_align_batch_band_ext_pair")
             .replace("gsa_align_batch_band_info", "gsa_align_batch_band_ext_info")
            for a in _args(text, "gsa_align_batch_band_dev")]
    assert _args(text, "gsa_align_batch_band_ext_dev") == want and len(want) == 20
    res, args = gsa.SIGNATURES["gsa_align_batch_band_ext_dev"]
    swap = {ctypes.POINTER(gsa.AlignBatchBandPair): ctypes.POINTER(gsa.AlignBatchBandExtPair),
            ctypes.POINTER(gsa.AlignBatchBandInfo): ctypes.POINTER(gsa.AlignBatchBandExtInfo)}
    assert res is ctypes.c_int and args == [swap.get(a, a) for a in gsa.SIGNATURES["gsa_align_batch_band_dev"][1]]
    for name in ("gsa_score_band_ext_batch_dev", "gsa_align_batch_band_ext_dev"):
        assert hasattr(gsa.lib(), name)


def test_semantics_are_stated_in_the_header():
    text = " ".join(open(os.path.join(ROOT, "include", "gsa.h")).read().replace("*", " ").split())
    for phrase in ("out[p] is exactly what gsa_score_band_ext_dev returns for pair p alone",
                   "out[p] is, field for field, what gsa_align_pair_band_ext_dev returns for pair p alone",
                   "whatever the pair's position, its neighbours, the waves, the grid or the round",
                   "Nothing is enqueued before every pair has passed its checks"):
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
    P, I = gsa.AlignBatchBandExtPair, gsa.AlignBatchBandExtInfo
    assert _struct(text, "gsa_align_batch_band_ext_pair") == list(P._fields_)
    assert _struct(text, "gsa_align_batch_band_ext_info") == list(I._fields_)
    # the band structs' fields plus the trimmed pair
    assert {f for f, _ in P._fields_} == {f for f, _ in gsa.AlignBatchBandPair._fields_} | {"rows_used", "cols_used"}
    assert list(I._fields_[:-2]) == list(gsa.AlignBatchBandInfo._fields_)
    assert ctypes.sizeof(P) == 56 and ctypes.sizeof(I) == 64 and ctypes.sizeof(P) % 8 == 0 == ctypes.sizeof(I) % 8
    assert [(f, getattr(P, f).offset) for f, _ in P._fields_] == [
        ("band_lo", 0), ("band_hi", 8), ("code_bytes", 16), ("rows_used", 24), ("cols_used", 32), ("strips", 40),
        ("supersteps", 44), ("proved_optimal", 48), ("round", 52)]
    assert [(f, getattr(I, f).offset) for f, _ in I._fields_] == [
        ("batch_pairs", 0), ("host_pairs", 4), ("nocode_pairs", 8), ("rounds", 12), ("waves", 16), ("strip_rows", 20),
        ("code_bytes", 24), ("fill_ms", 32), ("nocode_ms", 36), ("walk_ms", 40), ("pad0", 44), ("rows_used", 48),
        ("cols_used", 56)]


def test_null_context_is_invalid_value():
    n = 2
    pairs = (gsa.PairDev * n)()
    lo, hi = (ctypes.c_int64 * n)(-2, -2), (ctypes.c_int64 * n)(2, 2)
    out, sr = (gsa.AlignDbResult * n)(), (gsa.ScoreResult * n)()
    pinfo, info = (gsa.AlignBatchBandExtPair * n)(), gsa.AlignBatchBandExtInfo()
    need, ms = ctypes.c_int64(0), ctypes.c_float(0.0)
    st = gsa.lib().gsa_align_batch_band_ext_dev(None, n, pairs, None, 5, -11, -1, lo, hi, 0, 0, 0, out, None, 0,
                                                ctypes.byref(need), pinfo, ctypes.byref(info), ctypes.byref(ms), None)
    assert st == gsa.NwStat.errorInvalidValue
    st = gsa.lib().gsa_score_band_ext_batch_dev(None, n, pairs, None, 5, -11, -1, lo, hi, 0, 0, sr, ctypes.byref(ms), None)
    assert st == gsa.NwStat.errorInvalidValue


def test_python_entry_points():
    """The shape of the global banded batch wrappers."""
    for name in ("score_band_batch_dev", "score_band_batch", "align_batch_band_dev", "align_batch_band",
                 "last_align_batch_band_info"):
        ext = name.replace("band", "band_ext")
        sig, bsig = inspect.signature(getattr(gsa.Engine, ext)), inspect.signature(getattr(gsa.Engine, name))
        assert list(sig.parameters) == list(bsig.parameters), ext
        for p in sig.parameters:
            assert sig.parameters[p].default == bsig.parameters[p].default and sig.parameters[p].kind == bsig.parameters[p].kind


def test_host_forms_take_exactly_one_band_form():
    """The check comes before anything touches the device or the engine; band=w means (-w, w) per pair."""
    e = object.__new__(gsa.Engine)
    pairs, sub = [([0, 1, 1, 0], [0, 1, 0]), ([0, 1], [0, 1, 1, 1])], [[1, -1], [-1, 1]]
    for fn in (gsa.Engine.score_band_ext_batch, gsa.Engine.align_batch_band_ext):
        for kw in ({}, {"bands": [(-1, 0), (0, 2)], "band": 2}):
            with pytest.raises(ValueError):
                fn(e, pairs, sub, -2, -1, **kw)
    assert gsa.Engine._bands_ext_of(pairs, None, 4) == [(-4, 4), (-4, 4)]
    assert gsa.Engine._bands_ext_of(pairs, [(-7, 1), (0, 2)], None) == [(-7, 1), (0, 2)]
    for fn in (gsa.Engine.score_band_ext_batch_dev, gsa.Engine.align_batch_band_ext_dev):
        with pytest.raises(ValueError):
            fn(e, [(1, 2, 3, 4)], 0, 2, -2, -1, bands=[])
    with pytest.raises(gsa.NwError):
        e.last_align_batch_band_ext_info()


def test_makefile_builds_the_unit_with_its_report():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    objs = re.search(r"^OBJS = (.*)$", mk, re.M).group(1).split()
    assert "build/nw_band_ext_batch.o" in objs and "build/nw_band_batch.o" in objs
    rule = re.search(r"^build/nw_band_ext_batch\.o:(.*)\n\t(.*)$", mk, re.M)
    assert "-Rpass-analysis=kernel-resource-usage" in rule.group(2) and "build/nw_band_ext_batch.resources.txt" in rule.group(2)
    assert "_SCHED" not in rule.group(2)  # the default scheduler
    for dep in ("nw_band_ext_batch.h", "nw_band_ext_plan.h", "nw_band_batch_plan.h", "nw_band_dev.h", "nw_band_plan.h"):
        assert dep in rule.group(1), dep
    assert os.path.exists(os.path.join(CSRC, "build", "nw_band_ext_batch.resources.txt"))
    src = open(os.path.join(CSRC, "nw_band_ext_batch.hip")).read()
    assert not re.search(r'#include\s+"[^"]*\.hip"', src) and '#include "nw_band_dev.h"' in src
    assert src.count("band_pair_fill<AFFINE, CODES, true>") == 1 and "band_dev::band_walk_from_start(" in src
    # no spin loop; the claim is the unit's only atomic
    code = "\n".join(l.split("//")[0] for l in src.split("\n"))
    assert "while (" not in code and "for (;;)" not in code
    assert len(re.findall(r"atomic\w*\(", code)) == 1 and "claim = atomicAdd(counter, 1u)" in code


def _report(unit):
    text = open(os.path.join(CSRC, "build", unit + ".resources.txt")).read()
    out = {}
    for block in text.split("Function Name: ")[1:]:
        name = block.split()[0]
        out[name] = tuple(int(re.search(f + r": (\d+)", block).group(1))
                          for f in ("ScratchSize \\[bytes/lane\\]", "SGPRs Spill", "VGPRs Spill",
                                    "Occupancy \\[waves/SIMD\\]", "LDS Size \\[bytes/block\\]"))
    return out


def test_instances_have_no_scratch_and_no_spills():
    """The four fill instances (affine or linear, with or without codes) and the walk."""
    kernels = ["nw_band_ext_batch_kernelILb%dELb%dEE" % (a, c) for a in (0, 1) for c in (0, 1)] + ["nw_band_ext_batch_walk_kernel"]
    rep = _report("nw_band_ext_batch")
    assert len(rep) == len(kernels) and all(any(k in n for n in rep) for k in kernels), list(rep)
    assert {v[:3] for v in rep.values()} == {(0, 0, 0)}, rep
    # the table and the claim word of nw_band_batch.hip and 16 slots of 16 bytes (the ring is dynamic);
    # a workgroup of 16 waves stays resident (4 per SIMD)
    fills = [v for n, v in rep.items() if "walk" not in n]
    assert {v[4] for v in fills} == {4104 + 16 * 16} and min(v[3] for v in fills) >= 4
