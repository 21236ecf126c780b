"""The six long-pair trace units (nw_pair_trace, nw_pair_semi_trace, nw_pair_overlap_trace and their _batch
units) share one strip fill, one walk per shape and one piece of launch glue, nw_pair_trace_dev.h: each of
them is defined there and nowhere else, and every kernel of the six units keeps every numeric field of
the build's resource report.  No GPU is needed; the kernels are checked in tests/test_gpu_align_*.py."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gpuseqalign_amd", "csrc")
HEADER = "nw_pair_trace_dev.h"
UNITS = ("nw_pair_trace", "nw_pair_trace_batch", "nw_pair_semi_trace", "nw_pair_semi_trace_batch",
         "nw_pair_overlap_trace", "nw_pair_overlap_trace_batch")


def _code(name):
    """A source file without its comments."""
    text = open(os.path.join(CSRC, name)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return re.sub(r"//[^\n]*", "", text)


def test_body_preamble_walk_and_glue_are_defined_once():
    """The lane shift, the affine flip of the packed codes, the walk's gap-extension test and the
    occupancy query each stand in the header and in none of the six units."""
    header = _code(HEADER)
    for token in ("__builtin_amdgcn_update_dpp", "0xccccccccu", "kDbTraceFExt",
                  "hipOccupancyMaxActiveBlocksPerMultiprocessor"):
        assert header.count(token) >= 1, token
        for unit in UNITS:
            assert _code(unit + ".hip").count(token) == 0, (unit, token)


def test_units_include_the_header_and_no_source_file():
    for unit in UNITS:
        src = _code(unit + ".hip")
        assert re.search(r'#include\s+"%s"' % re.escape(HEADER), src), unit
        assert not re.search(r'#include\s+"[^"]*\.hip"', src), unit


def test_header_has_no_kernel_and_the_fill_body_no_atomic_and_no_open_loop():
    header = _code(HEADER)
    assert "__global__" not in header and "__shared__" not in header
    fill = re.search(r"#define GSA_PAIR_STRIP_FILL\(.*?\n(.*?)\n\s*\} while \(0\)\n", header, re.S).group(1)
    assert "CodesN<NW>" in fill and "from_lane_above" in fill  # the body, whole
    for word in ("atomic", "for (;;)", "while (", "__syncthreads", "__builtin_amdgcn_s_barrier"):
        assert word not in fill, word
    # the ticket counter stays in the kernels: one atomic per unit, and nothing in them polls
    for unit in UNITS:
        src = _code(unit + ".hip")
        assert re.findall(r"atomic\w*\(", src) == ["atomicAdd("], unit
        assert "while (" not in src and src.count("for (;;)") == 1, unit


def test_makefile_rules_depend_on_the_header():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    for unit in UNITS:
        rule = re.search(r"^build/%s\.o:(.*)\n\t(.*)$" % unit, mk, re.M)
        assert HEADER in rule.group(1).split(), unit
        assert "build/%s.resources.txt" % unit in rule.group(2) and "_SCHED" not in rule.group(2), unit


# The resource reports of the six units as the commit before this change builds them, every unit with the
# strip fill and the walk written out in its own kernels: (instance, SGPRs, VGPRs, AGPRs, scratch, occupancy,
# SGPR spills, VGPR spills, LDS).  nw_pair_trace's nine are those of tests/test_align_batch_api.py.
PARENT_ROWS = {
    "nw_pair_trace": [
        ("nw_pair_walk_kernel", 50, 7, 0, 0, 8, 0, 0, 0),
        ("nw_pair_fill_kernelILb1ELb1ELi8E", 59, 63, 0, 0, 8, 0, 0, 4096),
        ("nw_pair_fill_kernelILb1ELb0ELi8E", 57, 54, 0, 0, 8, 0, 0, 4096),
        ("nw_pair_fill_kernelILb0ELb1ELi8E", 59, 65, 0, 0, 7, 0, 0, 4096),
        ("nw_pair_fill_kernelILb0ELb0ELi8E", 57, 54, 0, 0, 8, 0, 0, 4096),
        ("nw_pair_fill_kernelILb1ELb1ELi16E", 59, 100, 0, 0, 4, 0, 0, 4096),
        ("nw_pair_fill_kernelILb1ELb0ELi16E", 57, 55, 0, 0, 8, 0, 0, 4096),
        ("nw_pair_fill_kernelILb0ELb1ELi16E", 59, 89, 0, 0, 5, 0, 0, 4096),
        ("nw_pair_fill_kernelILb0ELb0ELi16E", 57, 66, 0, 0, 7, 0, 0, 4096),
    ],
    "nw_pair_trace_batch": [
        ("nw_pair_batch_walk_kernel", 48, 30, 0, 0, 8, 0, 0, 0),
        ("nw_pair_batch_fill_kernelILb1ELb1ELi8E", 52, 65, 0, 0, 7, 0, 0, 4096),
        ("nw_pair_batch_fill_kernelILb1ELb0ELi8E", 48, 54, 0, 0, 8, 0, 0, 4096),
        ("nw_pair_batch_fill_kernelILb0ELb1ELi8E", 52, 67, 0, 0, 7, 0, 0, 4096),
        ("nw_pair_batch_fill_kernelILb0ELb0ELi8E", 48, 54, 0, 0, 8, 0, 0, 4096),
        ("nw_pair_batch_fill_kernelILb1ELb1ELi16E", 52, 102, 0, 0, 4, 0, 0, 4096),
        ("nw_pair_batch_fill_kernelILb1ELb0ELi16E", 48, 68, 0, 0, 7, 0, 0, 4096),
        ("nw_pair_batch_fill_kernelILb0ELb1ELi16E", 52, 91, 0, 0, 5, 0, 0, 4096),
        ("nw_pair_batch_fill_kernelILb0ELb0ELi16E", 48, 72, 0, 0, 7, 0, 0, 4096),
    ],
    "nw_pair_semi_trace": [
        ("nw_semi_walk_kernel", 52, 8, 0, 0, 8, 0, 0, 0),
        ("nw_semi_fill_kernelILb1ELi8E", 59, 64, 0, 0, 8, 0, 0, 4096),
        ("nw_semi_fill_kernelILb0ELi8E", 57, 54, 0, 0, 8, 0, 0, 4096),
        ("nw_semi_fill_kernelILb1ELi16E", 59, 87, 0, 0, 5, 0, 0, 4096),
        ("nw_semi_fill_kernelILb0ELi16E", 57, 65, 0, 0, 7, 0, 0, 4096),
    ],
    "nw_pair_semi_trace_batch": [
        ("nw_semi_batch_walk_kernel", 52, 30, 0, 0, 8, 0, 0, 0),
        ("nw_semi_batch_fill_kernelILb1ELi8E", 52, 65, 0, 0, 7, 0, 0, 4096),
        ("nw_semi_batch_fill_kernelILb0ELi8E", 48, 54, 0, 0, 8, 0, 0, 4096),
        ("nw_semi_batch_fill_kernelILb1ELi16E", 52, 89, 0, 0, 5, 0, 0, 4096),
        ("nw_semi_batch_fill_kernelILb0ELi16E", 48, 70, 0, 0, 7, 0, 0, 4096),
    ],
    "nw_pair_overlap_trace": [
        ("nw_overlap_walk_kernel", 46, 6, 0, 0, 8, 0, 0, 0),
        ("nw_overlap_fill_kernelILb1ELi8E", 58, 63, 0, 0, 8, 0, 0, 4096),
        ("nw_overlap_fill_kernelILb0ELi8E", 56, 54, 0, 0, 8, 0, 0, 4096),
        ("nw_overlap_fill_kernelILb1ELi16E", 58, 100, 0, 0, 4, 0, 0, 4096),
        ("nw_overlap_fill_kernelILb0ELi16E", 56, 55, 0, 0, 8, 0, 0, 4096),
    ],
    "nw_pair_overlap_trace_batch": [
        ("nw_overlap_batch_walk_kernel", 40, 32, 0, 0, 8, 0, 0, 0),
        ("nw_overlap_batch_fill_kernelILb1ELi8E", 52, 65, 0, 0, 7, 0, 0, 4096),
        ("nw_overlap_batch_fill_kernelILb0ELi8E", 48, 54, 0, 0, 8, 0, 0, 4096),
        ("nw_overlap_batch_fill_kernelILb1ELi16E", 52, 102, 0, 0, 4, 0, 0, 4096),
        ("nw_overlap_batch_fill_kernelILb0ELi16E", 48, 68, 0, 0, 7, 0, 0, 4096),
    ],
}

FIELDS = ("TotalSGPRs", "VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "SGPRs Spill",
          "VGPRs Spill", "LDS Size [bytes/block]")


def _report(unit):
    text = open(os.path.join(CSRC, "build", unit + ".resources.txt")).read()
    out = {}
    for block in text.split("Function Name: ")[1:]:
        out[block.split()[0]] = tuple(int(re.search(re.escape(f) + r": (\d+)", block).group(1)) for f in FIELDS)
    return out


def test_all_38_kernels_keep_their_numbers():
    assert sum(len(rows) for rows in PARENT_ROWS.values()) == 38 and set(PARENT_ROWS) == set(UNITS)
    for unit, rows in PARENT_ROWS.items():
        rep = _report(unit)
        assert len(rep) == len(rows), (unit, list(rep))
        for row in rows:
            [name] = [n for n in rep if row[0] in n]
            assert rep[name] == row[1:], (unit, name, rep[name], row[1:])
