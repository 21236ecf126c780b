"""The C-ABI library: loads, exports every symbol include/gsa.h declares, and its host-side
consumers (Trace1/Hash1/Trace2/Hash2, src/nwtrace1_plain.cpp / src/nwtrace2_sparse.cpp)
agree with the oracle; and loading it before PyTorch leaves one HIP runtime in the process.  No GPU
compute here."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import gpuseqalign_amd as gsa
import oracle
from tests._data import random_pair

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    text = open(os.path.join(ROOT, "include", "gsa.h")).read()
    return sorted(set(re.findall(r"\b(gsa_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_header():
    L = gsa.lib()
    decl = declared_symbols()
    assert len(decl) >= 15
    for name in decl:
        assert hasattr(L, name), name
        assert name in gsa.SIGNATURES, name


def test_last_launch_binding_matches_header():
    """gsa_launch_info / enum gsa_launch_kind in gsa.h against the ctypes mirror: the same fields in
    the same order (int32_t / int64_t only), the same kinds by value; no context: errorInvalidValue."""
    text = open(os.path.join(ROOT, "include", "gsa.h")).read()
    body = re.search(r"typedef struct gsa_launch_info\s*\{(.*?)\}\s*gsa_launch_info;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for ctype, names in re.findall(r"\b(int32_t|int64_t)\s+([^;]+);", body):
        fields += [(n.strip(), ctypes.c_int32 if ctype == "int32_t" else ctypes.c_int64) for n in names.split(",")]
    assert fields == list(gsa.LaunchInfo._fields_)
    enum = re.search(r"enum gsa_launch_kind\s*\{(.*?)\};", text, re.S).group(1)
    kinds = re.findall(r"GSA_LAUNCH_([A-Z_]+)\s*=\s*(\d+)", enum)
    assert [int(v) for _, v in kinds] == list(range(len(kinds)))
    assert tuple(n.lower() for n, _ in kinds) == gsa.LAUNCH_KINDS
    li = gsa.LaunchInfo()
    assert gsa.lib().gsa_last_launch(None, ctypes.byref(li)) == gsa.NwStat.errorInvalidValue


def test_geometry():
    g = gsa.sparse_geometry(10001, 10001, 256)
    assert g.tileBy == gsa.sparse_tile_by() == 1024
    assert g.tileHdrMatRows == -(-10000 // 1024) and g.tileHdrMatCols == -(-10000 // 256)
    assert g.hrowElems == g.tileHdrMatRows * g.tileHdrMatCols * 257
    e = gsa.sparse_geometry(1, 1, 64)  # empty sequences -> one tile (gpu9 host :419-426)
    assert (e.tileHdrMatRows, e.tileHdrMatCols) == (1, 1)
    with pytest.raises(gsa.NwError):
        gsa.sparse_geometry(10, 10, 50)


def test_host_trace_hash_match_oracle(golden):
    for p, Y, X in golden.pairs("pair_debug.txt")[::5]:
        S, _ = oracle.fill_full(Y, X, golden.blosum62, -11)
        assert gsa.hash_full(S) == oracle.hash_full(S)
        assert gsa.trace_full(S, Y, X) == oracle.trace_full(S, Y, X)


@pytest.mark.parametrize("tBx", [64, 256])
def test_host_sparse_consumers_match_oracle(golden, tBx):
    tBy = gsa.sparse_tile_by()
    cases = [golden.pair("len64 len728"), golden.pair("len728 len728"), random_pair(600, 333, 7),
             golden.pair("len1 len1")]
    for Y, X in cases:
        hr, hc, tr, tc, cost = oracle.sparse_headers(Y, X, golden.blosum62, -11, tBy, tBx)
        geom = gsa.sparse_geometry(len(Y), len(X), tBx)
        assert (geom.tileHdrMatRows, geom.tileHdrMatCols) == (tr, tc)
        res = gsa.SparseResult(hr, hc, geom, cost, {})
        th, ed, c = gsa.trace_sparse(res, Y, X, golden.blosum62, -11)
        oth, oed, oc = oracle.trace_sparse(hr, hc, tr, tc, tBy, tBx, Y, X, golden.blosum62, -11)
        assert (th, ed, c) == (oth, oed, oc)
        assert gsa.sparse_align_cost(res, Y, X, golden.blosum62, -11) == cost
        assert gsa.hash_sparse(res, Y, X, golden.blosum62, -11) == oracle.hash_stream(Y, X, golden.blosum62, -11)[0]


def test_registry_names():
    m = gsa.get_nw_algorithm_map()
    assert m["NwAlign_Gpu9_Mlsp_DiagDiagDiag"].trace is m["NwAlign_Amd_Strip_Mlsp"].trace
    assert m["NwAlign_Gpu3_Ml_DiagDiag"].hash is m["NwAlign_Amd_Strip_Full"].hash


_ORDER = """
import gpuseqalign_amd as gsa
gsa.lib()                     # the library first ...
import torch                  # ... then PyTorch, which may bring a HIP runtime of its own
names = {l.split()[-1] for l in open('/proc/self/maps') if 'libamdhip64' in l}
%s
print('runtimes', len(names))
"""


def test_library_before_torch_is_one_hip_runtime():
    """gsa.lib() in a fresh process that has not imported torch yet: one libamdhip64 in the process
    afterwards, not the system's beside PyTorch's (whichever of two initialises second finds no device)."""
    out = subprocess.run([sys.executable, "-c", _ORDER % ""], cwd=ROOT, capture_output=True, text=True, check=True).stdout
    assert out.split()[-2:] == ["runtimes", "1"], out


@pytest.mark.gpu
def test_library_before_torch_still_opens_the_device(engine):
    """The same order on a GPU: both PyTorch and a context of ours find the device."""
    body = "assert torch.cuda.is_available(); torch.zeros(1, device='cuda:0'); gsa.Engine(0).close()"
    out = subprocess.run([sys.executable, "-c", _ORDER % body], cwd=ROOT, capture_output=True, text=True, check=True).stdout
    assert out.split()[-2:] == ["runtimes", "1"], out
