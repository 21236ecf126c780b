"""The host side of the six long-pair trace units in gsa_score.hip: one chunk loop (trace_pair) drives the
three single-pair alignments, one round loop (trace_batch) the three batch alignments, one plan
(nw_pair_trace_batch_plan.h) spreads the batches' strips over rounds, one function scores a semi-global
or an overlap batch, and one helper packs the CIGARs of every alignment call.  Each of these stands once.
No GPU is needed; what the calls compute is checked in tests/test_gpu_align_*.py."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gpuseqalign_amd", "csrc")


def _code(path):
    """A source file without its comments."""
    text = open(path).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return re.sub(r"//[^\n]*", "", text)


HOST = _code(os.path.join(CSRC, "gsa_score.hip"))


def test_every_trace_launcher_is_called_once():
    for call in ("launch_pair_trace(", "launch_semi_trace(", "launch_overlap_trace(", "launch_pair_batch_trace(",
                 "launch_semi_batch_trace(", "launch_overlap_batch_trace("):
        assert HOST.count(call) == 1, call
    # and each from its mode's struct, which the one loop of its shape is instantiated with
    for loop, modes in (("trace_pair", ("GlobalTrace", "SemiTrace", "OverlapTrace")),
                        ("trace_batch", ("GlobalBatchTrace", "SemiBatchTrace", "OverlapBatchTrace"))):
        assert len(re.findall(r"\bint %s\(" % loop, HOST)) == 1, loop
        for mode in modes:
            assert HOST.count("%s<%s>(" % (loop, mode)) == 1, (loop, mode)
            assert len(re.findall(r"\bstruct %s\b" % mode, HOST)) == 1, mode


def test_one_batch_plan():
    assert HOST.count("batch_plan_round(") == 1
    sources = [p for pat in ("*.h", "*.hip", "*.cpp", "Makefile") for p in glob.glob(os.path.join(CSRC, pat))]
    assert len(sources) > 50
    for path in sources:
        text = open(path).read()
        for gone in ("semi_batch_plan_round", "overlap_batch_plan_round"):
            assert gone not in text, (path, gone)
    plan = _code(os.path.join(CSRC, "nw_pair_trace_batch_plan.h"))
    assert len(re.findall(r"\bstruct BatchPairState\b", plan)) == 1 and re.search(r"long long jW = 0;", plan)
    assert "semi_plan_chunk(" in plan
    # the mode headers keep what is theirs, without HIP and without a plan of their own
    for name in ("nw_pair_trace_batch_plan.h", "nw_pair_semi_trace_batch_plan.h", "nw_pair_overlap_trace_batch_plan.h"):
        head = _code(os.path.join(CSRC, name))
        assert "hip" not in head.lower(), name
        assert len(re.findall(r"\binline bool \w+_batch_advance\(", head)) == 1, name
    for name in ("nw_pair_semi_trace_batch_plan.h", "nw_pair_overlap_trace_batch_plan.h"):
        head = _code(os.path.join(CSRC, name))
        assert "struct" not in head and "stable_sort" not in head, name
        assert '#include "nw_pair_trace_batch_plan.h"' in head, name


def test_the_three_plan_drivers_use_the_one_state():
    for name in ("align_batch_plan_driver.cpp", "align_batch_semi_plan_driver.cpp", "align_batch_overlap_plan_driver.cpp"):
        src = _code(os.path.join(ROOT, "tests", name))
        assert "gsa::BatchPairState" in src and "gsa::batch_plan_round(" in src, name
        assert not re.search(r"\b(Semi|Overlap)Batch(PairState|Chunk)\b", src), name


def test_task_sort_blob_layout_and_cigar_packer_stand_once():
    assert HOST.count("std::stable_sort(tasks.begin(), tasks.end()") == 1
    for token in ("oTask = 64", "oDesc = oTask +", "oWalk = oDesc +"):
        assert HOST.count(token) == 1, token
    # the packer: one loop that copies a string to its offset; no call copies to the buffer's start itself
    assert HOST.count("std::memcpy(cigar + at,") == 1
    assert "std::memcpy(cigar," not in HOST
    assert len(re.findall(r"\bint64_t pack_cigars\(", HOST)) == 1
    # the three batch calls and the three single-pair calls through their shared ends, the database calls
    # and the banded calls directly
    assert HOST.count("pack_cigars(") == 1 + 2 + 2 + 2
    assert HOST.count("finish_pair(") == 1 + 3 and HOST.count("finish_batch(") == 1 + 3


def test_events_times_and_shift_are_shared():
    assert HOST.count("for (hipEvent_t& ev : ctx->adbev)") == 1
    assert HOST.count("KR == 8 ? 3 : 4") == 1
    assert HOST.count("ctx->adbev[1], ctx->adbev[2]") == 1 + 2  # add_trace_ms, and the banded calls' conditional walk time


def test_one_batched_semi_overlap_score():
    assert "score_overlap_batch_impl" not in HOST and "OverlapBatchRoute" not in HOST
    assert len(re.findall(r"\bint score_semi_batch_impl\(", HOST)) == 1
    assert len(re.findall(r"\bstruct SemiBatchRoute\b", HOST)) == 1
    for call in ("launch_krow_score_semi_batch(", "launch_krow_score_overlap_batch(", "launch_semi_rowmax_batch(",
                 "launch_overlap_max_batch("):
        assert HOST.count(call) == 1, call
