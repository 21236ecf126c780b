"""gpuseqalign_amd -- MI355X-native NW-LG engine (drop-in for GpuSeqAlign's align path).

Python host side over the C ABI of ``libgsa.so`` (include/gsa.h).  The compute path is the
hand-written gfx950 HIP kernels in ``csrc/`` (``nw_krow.hip`` sparse fills, ``nw_lane.hip`` full
fills, ``nw_strip.hip`` score-only fills); there is no CPU fallback: if the library is missing or
no GPU is visible, GPU entry points raise.

Mirrors the reference's registry (src/nw_algorithm.cpp:48-69): an ``NwAlgorithm`` is an
{align, trace, hash} triple; the plain family pairs with Trace1/Hash1, the sparse (mlsp)
family with Trace2/Hash2.
"""
from __future__ import annotations

import ctypes
import dataclasses
import os
from typing import Callable, Dict, Optional, Sequence, Tuple

import numpy as np

__all__ = [
    "NwStat", "NwError", "lib", "Engine", "AlignResult", "SparseResult", "PairDev",
    "NwAlgorithm", "get_nw_algorithm_map", "hash_full", "trace_full", "trace_sparse", "hash_sparse",
    "sparse_align_cost", "sparse_tile_by", "KNOB_NAMES", "LAUNCH_KINDS",
]

_PKG = os.path.dirname(os.path.abspath(__file__))
_SO = os.environ.get("GSA_LIB") or os.path.join(_PKG, "libgsa.so")  # GSA_LIB: diagnostic builds only
_LIB = None


class NwStat:
    """NwStat (src/run_types.hpp:12-24)."""
    success = 0
    helpMenuRequested = 1
    errorCudaGeneral = 2
    errorMemoryAllocation = 3
    errorMemoryTransfer = 4
    errorKernelFailure = 5
    errorIoStream = 6
    errorInvalidFormat = 7
    errorInvalidValue = 8
    errorInvalidResult = 9
    names = {0: "success", 1: "helpMenuRequested", 2: "errorCudaGeneral", 3: "errorMemoryAllocation",
             4: "errorMemoryTransfer", 5: "errorKernelFailure", 6: "errorIoStream", 7: "errorInvalidFormat",
             8: "errorInvalidValue", 9: "errorInvalidResult"}


class NwError(RuntimeError):
    def __init__(self, stat: int, where: str, hip_error: int = 0):
        self.stat = stat
        self.hip_error = hip_error
        super().__init__(f"{where}: {NwStat.names.get(stat, stat)} (hipError {hip_error})")


class _Laps(ctypes.Structure):
    _fields_ = [("alloc", ctypes.c_float), ("cpy_dev", ctypes.c_float), ("init_hdr", ctypes.c_float),
                ("calc", ctypes.c_float), ("cpy_host", ctypes.c_float), ("calc_kernel_ms", ctypes.c_float)]

    def as_dict(self):
        return {"align.alloc": self.alloc, "align.cpy_dev": self.cpy_dev, "align.init_hdr": self.init_hdr,
                "align.calc": self.calc, "align.cpy_host": self.cpy_host, "calc_kernel_ms": self.calc_kernel_ms}


class SparseGeom(ctypes.Structure):
    _fields_ = [("tileBx", ctypes.c_int32), ("tileBy", ctypes.c_int32), ("tileHdrMatRows", ctypes.c_int32),
                ("tileHdrMatCols", ctypes.c_int32), ("tileHrowLen", ctypes.c_int32), ("tileHcolLen", ctypes.c_int32),
                ("hrowElems", ctypes.c_int64), ("hcolElems", ctypes.c_int64)]


class PairDev(ctypes.Structure):
    """gsa_pair_dev (include/gsa.h): device pointers of one pair of a batched fill."""
    _fields_ = [("seqY", ctypes.c_void_p), ("adjrows", ctypes.c_int32), ("seqX", ctypes.c_void_p),
                ("adjcols", ctypes.c_int32), ("score", ctypes.c_void_p), ("tileHrowMat", ctypes.c_void_p),
                ("tileHcolMat", ctypes.c_void_p)]


class CheckResult(ctypes.Structure):
    """gsa_check_result (include/gsa.h): outcome of a device-side verification."""
    _fields_ = [("checked", ctypes.c_int64), ("mismatches", ctypes.c_int64), ("first", ctypes.c_int64)]

    def as_dict(self):
        return {"checked": int(self.checked), "mismatches": int(self.mismatches), "first": int(self.first)}


class MemStats(ctypes.Structure):
    """gsa_mem_stats: the reference's NwAlgResult peak-alloc columns (nwalign_shared.cpp:5-25)."""
    _fields_ = [("glmem_peak_allocs", ctypes.c_int64), ("shmem_peak_allocs", ctypes.c_int64),
                ("locmem_peak_allocs", ctypes.c_int64), ("regmem_peak_allocs", ctypes.c_int64)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class FullTiming(ctypes.Structure):
    """gsa_full_timing (include/gsa.h): pass times and pass 2's effective shader clock."""
    _fields_ = [("pass1_ms", ctypes.c_float), ("pass2_ms", ctypes.c_float),
                ("clock_ghz_median", ctypes.c_float), ("clock_ghz_mean", ctypes.c_float),
                ("workgroups", ctypes.c_int64), ("fused", ctypes.c_int32), ("groups", ctypes.c_int32)]


class LaunchInfo(ctypes.Structure):
    """gsa_launch_info (include/gsa.h): the instance the last call on a context ran."""
    _fields_ = [("kind", ctypes.c_int32), ("ns", ctypes.c_int32), ("k", ctypes.c_int32), ("q8", ctypes.c_int32),
                ("q8_declined", ctypes.c_int32), ("staged", ctypes.c_int32), ("mlsppt", ctypes.c_int32),
                ("both_ends", ctypes.c_int32), ("npairs", ctypes.c_int32), ("pair_major", ctypes.c_int32),
                ("trace_band", ctypes.c_int32),
                ("tickets", ctypes.c_int64), ("band_tiles", ctypes.c_int64)]


# enum gsa_launch_kind (include/gsa.h), by value
LAUNCH_KINDS = ("none", "full_lane", "full_fused", "full_two_launch", "sparse_krow", "sparse_strip", "score_krow",
                "score_strip", "score_scan", "trace_sparse", "score_lanes")


class ScoreResult(ctypes.Structure):
    """gsa_score_result (include/gsa.h)."""
    _fields_ = [("score", ctypes.c_int32), ("i_end", ctypes.c_int64), ("j_end", ctypes.c_int64),
                ("calc_kernel_ms", ctypes.c_float)]


class AlignDbResult(ctypes.Structure):
    """gsa_align_db_result (include/gsa.h)."""
    _fields_ = [("score", ctypes.c_int32), ("status", ctypes.c_int32), ("i_start", ctypes.c_int64),
                ("j_start", ctypes.c_int64), ("i_end", ctypes.c_int64), ("j_end", ctypes.c_int64),
                ("cigar_off", ctypes.c_int64), ("cigar_len", ctypes.c_int64)]


class AlignDbInfo(ctypes.Structure):
    """gsa_align_db_info (include/gsa.h): what the last gsa_align_db_dev call ran."""
    _fields_ = [("lane_hits", ctypes.c_int32), ("unsupported", ctypes.c_int32), ("chunks", ctypes.c_int32),
                ("tasks", ctypes.c_int64), ("code_bytes", ctypes.c_int64), ("fill_ms", ctypes.c_float),
                ("walk_ms", ctypes.c_float)]


class AlignPairInfo(ctypes.Structure):
    """gsa_align_pair_info (include/gsa.h): what the last gsa_align_pair_dev call ran."""
    _fields_ = [("strip_rows", ctypes.c_int32), ("strips", ctypes.c_int32), ("strips_filled", ctypes.c_int32),
                ("chunks", ctypes.c_int32), ("code_bytes", ctypes.c_int64), ("score_ms", ctypes.c_float),
                ("fill_ms", ctypes.c_float), ("walk_ms", ctypes.c_float), ("pad0", ctypes.c_int32)]


class AlignPairSemiInfo(ctypes.Structure):
    """gsa_align_pair_semi_info (include/gsa.h): what the last gsa_align_pair_semi_dev call ran."""
    _fields_ = [("strip_rows", ctypes.c_int32), ("strips", ctypes.c_int32), ("strips_filled", ctypes.c_int32),
                ("chunks", ctypes.c_int32), ("code_bytes", ctypes.c_int64), ("j_window", ctypes.c_int64),
                ("score_ms", ctypes.c_float), ("fill_ms", ctypes.c_float), ("walk_ms", ctypes.c_float),
                ("pad0", ctypes.c_int32)]


class AlignPairOverlapInfo(ctypes.Structure):
    """gsa_align_pair_overlap_info (include/gsa.h): what the last gsa_align_pair_overlap_dev call ran."""
    _fields_ = [("strip_rows", ctypes.c_int32), ("strips", ctypes.c_int32), ("strips_filled", ctypes.c_int32),
                ("chunks", ctypes.c_int32), ("code_bytes", ctypes.c_int64),
                ("score_ms", ctypes.c_float), ("fill_ms", ctypes.c_float), ("walk_ms", ctypes.c_float),
                ("pad0", ctypes.c_int32)]


class AlignPairBandInfo(ctypes.Structure):
    """gsa_align_pair_band_info (include/gsa.h): what the last gsa_align_pair_band_dev call ran."""
    _fields_ = [("strip_rows", ctypes.c_int32), ("strips", ctypes.c_int32), ("waves", ctypes.c_int32),
                ("supersteps", ctypes.c_int32), ("proved_optimal", ctypes.c_int32), ("pad0", ctypes.c_int32),
                ("band_lo", ctypes.c_int64), ("band_hi", ctypes.c_int64), ("code_bytes", ctypes.c_int64),
                ("score_ms", ctypes.c_float), ("walk_ms", ctypes.c_float)]


class AlignBatchBandPair(ctypes.Structure):
    """gsa_align_batch_band_pair (include/gsa.h): one pair of the last gsa_align_batch_band_dev call."""
    _fields_ = [("band_lo", ctypes.c_int64), ("band_hi", ctypes.c_int64), ("code_bytes", ctypes.c_int64),
                ("strips", ctypes.c_int32), ("supersteps", ctypes.c_int32), ("proved_optimal", ctypes.c_int32),
                ("round", ctypes.c_int32)]


class AlignBatchBandInfo(ctypes.Structure):
    """gsa_align_batch_band_info (include/gsa.h): what the last gsa_align_batch_band_dev call ran."""
    _fields_ = [("batch_pairs", ctypes.c_int32), ("host_pairs", ctypes.c_int32), ("nocode_pairs", ctypes.c_int32),
                ("rounds", ctypes.c_int32), ("waves", ctypes.c_int32), ("strip_rows", ctypes.c_int32),
                ("code_bytes", ctypes.c_int64),
                ("fill_ms", ctypes.c_float), ("nocode_ms", ctypes.c_float), ("walk_ms", ctypes.c_float),
                ("pad0", ctypes.c_int32)]


class AlignPairBandExtInfo(ctypes.Structure):
    """gsa_align_pair_band_ext_info (include/gsa.h): what the last gsa_align_pair_band_ext_dev call ran."""
    _fields_ = AlignPairBandInfo._fields_ + [("rows_used", ctypes.c_int64), ("cols_used", ctypes.c_int64)]


class AlignBatchBandExtPair(ctypes.Structure):
    """gsa_align_batch_band_ext_pair (include/gsa.h): one pair of the last gsa_align_batch_band_ext_dev call."""
    _fields_ = [("band_lo", ctypes.c_int64), ("band_hi", ctypes.c_int64), ("code_bytes", ctypes.c_int64),
                ("rows_used", ctypes.c_int64), ("cols_used", ctypes.c_int64),
                ("strips", ctypes.c_int32), ("supersteps", ctypes.c_int32), ("proved_optimal", ctypes.c_int32),
                ("round", ctypes.c_int32)]


class AlignBatchBandExtInfo(ctypes.Structure):
    """gsa_align_batch_band_ext_info (include/gsa.h): what the last gsa_align_batch_band_ext_dev call ran."""
    _fields_ = AlignBatchBandInfo._fields_ + [("rows_used", ctypes.c_int64), ("cols_used", ctypes.c_int64)]


class AlignBatchInfo(ctypes.Structure):
    """gsa_align_batch_info (include/gsa.h): what the last gsa_align_batch_dev call ran."""
    _fields_ = [("batch_pairs", ctypes.c_int32), ("alone_pairs", ctypes.c_int32), ("host_pairs", ctypes.c_int32),
                ("strip_rows", ctypes.c_int32), ("strips", ctypes.c_int32), ("strips_filled", ctypes.c_int32),
                ("rounds", ctypes.c_int32), ("pad0", ctypes.c_int32), ("code_bytes", ctypes.c_int64),
                ("score_ms", ctypes.c_float), ("fill_ms", ctypes.c_float), ("walk_ms", ctypes.c_float),
                ("pad1", ctypes.c_int32)]


class AlignBatchSemiInfo(ctypes.Structure):
    """gsa_align_batch_semi_info (include/gsa.h): what the last gsa_align_batch_semi_dev call ran."""
    _fields_ = [("batch_pairs", ctypes.c_int32), ("host_pairs", ctypes.c_int32), ("strip_rows", ctypes.c_int32),
                ("strips", ctypes.c_int32), ("strips_filled", ctypes.c_int32), ("rounds", ctypes.c_int32),
                ("code_bytes", ctypes.c_int64), ("window_cols", ctypes.c_int64), ("gran_bytes", ctypes.c_int64),
                ("score_ms", ctypes.c_float), ("fill_ms", ctypes.c_float), ("walk_ms", ctypes.c_float),
                ("pad0", ctypes.c_int32)]


class AlignBatchOverlapInfo(ctypes.Structure):
    """gsa_align_batch_overlap_info (include/gsa.h): what the last gsa_align_batch_overlap_dev call ran."""
    _fields_ = [("batch_pairs", ctypes.c_int32), ("host_pairs", ctypes.c_int32), ("strip_rows", ctypes.c_int32),
                ("strips", ctypes.c_int32), ("strips_filled", ctypes.c_int32), ("rounds", ctypes.c_int32),
                ("code_bytes", ctypes.c_int64), ("gran_bytes", ctypes.c_int64),
                ("score_ms", ctypes.c_float), ("fill_ms", ctypes.c_float), ("walk_ms", ctypes.c_float),
                ("pad0", ctypes.c_int32)]


class DbHit(ctypes.Structure):
    """gsa_db_hit (include/gsa.h): one ranked subject of a query of gsa_score_db_multi_dev."""
    _fields_ = [("subject", ctypes.c_int32), ("score", ctypes.c_int32), ("i_end", ctypes.c_int32),
                ("j_end", ctypes.c_int32)]


class ScoreDbMultiInfo(ctypes.Structure):
    """gsa_score_db_multi_info (include/gsa.h): what the last gsa_score_db_multi_dev call ran."""
    _fields_ = [("lane_queries", ctypes.c_int32), ("other_queries", ctypes.c_int32), ("launches", ctypes.c_int32),
                ("workgroups", ctypes.c_int32), ("lane_pairs", ctypes.c_int64), ("units", ctypes.c_int64),
                ("profile_builds", ctypes.c_int64), ("result_bytes", ctypes.c_int64), ("lanes_ms", ctypes.c_float),
                ("select_ms", ctypes.c_float)]


class AlignDbMultiInfo(ctypes.Structure):
    """gsa_align_db_multi_info (include/gsa.h): what the last gsa_align_db_multi_dev call ran."""
    _fields_ = [("lane_hits", ctypes.c_int32), ("unsupported", ctypes.c_int32), ("chunks", ctypes.c_int32),
                ("launches", ctypes.c_int32), ("workgroups", ctypes.c_int32), ("lane_queries", ctypes.c_int32),
                ("tasks", ctypes.c_int64), ("units", ctypes.c_int64), ("profile_builds", ctypes.c_int64),
                ("code_bytes", ctypes.c_int64), ("fill_ms", ctypes.c_float), ("walk_ms", ctypes.c_float)]


# numpy view of DbHit: the records of Engine.score_db_multi_dev's "hits"
DB_HIT_DTYPE = np.dtype([("subject", np.int32), ("score", np.int32), ("i_end", np.int32), ("j_end", np.int32)])

_LAPFN = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.c_char_p)  # gsa_lap_fn
_i32p = ctypes.POINTER(ctypes.c_int32)
_vp = ctypes.c_void_p
_i32 = ctypes.c_int32
_i64 = ctypes.c_int64

# symbol -> (restype, argtypes); every function declared in include/gsa.h
SIGNATURES = {
    "gsa_ctx_create": (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(_vp)]),
    "gsa_ctx_destroy": (None, [_vp]),
    "gsa_last_hip_error": (ctypes.c_int, [_vp]),
    "gsa_device_cu_count": (ctypes.c_int, [_vp]),
    "gsa_version": (ctypes.c_char_p, []),
    "gsa_debug_stamps": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.POINTER(ctypes.c_int64)]),
    "gsa_set_lap_callback": (ctypes.c_int, [_vp, _vp, _vp]),
    "gsa_set_knob": (ctypes.c_int, [_vp, ctypes.c_char_p, ctypes.c_char_p]),
    "gsa_set_full_timing": (ctypes.c_int, [_vp, _i32]),
    "gsa_last_full_timing": (ctypes.c_int, [_vp, ctypes.POINTER(FullTiming)]),
    "gsa_last_launch": (ctypes.c_int, [_vp, ctypes.POINTER(LaunchInfo)]),
    "gsa_sparse_tile_by": (_i32, []),
    "gsa_sparse_geometry": (ctypes.c_int, [_i32, _i32, _i32, ctypes.POINTER(SparseGeom)]),
    "gsa_fill_full_dev": (ctypes.c_int, [_vp, _vp, _i32, _vp, _i32, _vp, _i32, _i32, _vp, _vp]),
    "gsa_fill_sparse_dev": (ctypes.c_int, [_vp, _vp, _i32, _vp, _i32, _vp, _i32, _i32, _i32, _vp, _vp, _vp]),
    "gsa_sync": (ctypes.c_int, [_vp, _vp]),
    "gsa_set_watchdog": (ctypes.c_int, [_vp, _i64]),
    "gsa_mem_stats_get": (ctypes.c_int, [_vp, ctypes.POINTER(MemStats)]),
    "gsa_mem_stats_reset": (ctypes.c_int, [_vp]),
    "gsa_fill_full_batch_dev": (ctypes.c_int, [_vp, _i32, ctypes.POINTER(PairDev), _vp, _i32, _i32, _vp]),
    "gsa_full_pitch": (_i32, [_i32]),
    "gsa_full_base_offset": (_i32, []),
    "gsa_fill_full_pitched_dev": (ctypes.c_int, [_vp, _vp, _i32, _vp, _i32, _vp, _i32, _i32, _vp, _i32, _vp]),
    "gsa_fill_full_batch_pitched_dev": (ctypes.c_int, [_vp, _i32, ctypes.POINTER(PairDev), _i32p, _vp, _i32, _i32,
                                                       _vp]),
    "gsa_fill_sparse_batch_dev": (ctypes.c_int, [_vp, _i32, ctypes.POINTER(PairDev), _vp, _i32, _i32, _i32, _vp]),
    "gsa_align_full": (ctypes.c_int, [_vp, _i32p, _i32, _i32p, _i32, _i32p, _i32, _i32, _i32p, _i32p,
                                      ctypes.POINTER(_Laps)]),
    "gsa_align_sparse": (ctypes.c_int, [_vp, _i32p, _i32, _i32p, _i32, _i32p, _i32, _i32, _i32, _i32p, _i32p,
                                        ctypes.POINTER(SparseGeom), _i32p, ctypes.POINTER(_Laps)]),
    "gsa_align_sparse_pt": (ctypes.c_int, [_vp, _i32p, _i32, _i32p, _i32, _i32p, _i32, _i32, _i32, _i32p, _i32p,
                                           ctypes.POINTER(SparseGeom), _i32p, ctypes.POINTER(_Laps)]),
    "gsa_hash_full": (ctypes.c_uint32, [_i32p, _i32, _i32]),
    "gsa_trace_full": (ctypes.c_int, [_i32p, _i32p, _i32, _i32p, _i32, ctypes.c_char_p, _i64,
                                      ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_uint32)]),
    "gsa_trace_sparse": (ctypes.c_int, [_i32p, _i32p, ctypes.POINTER(SparseGeom), _i32p, _i32, _i32p, _i32, _i32p,
                                        _i32, _i32, ctypes.c_char_p, _i64, ctypes.POINTER(ctypes.c_int64),
                                        ctypes.POINTER(ctypes.c_uint32), _i32p]),
    "gsa_hash_sparse": (ctypes.c_uint32, [_i32p, _i32p, ctypes.POINTER(SparseGeom), _i32p, _i32, _i32p, _i32, _i32p,
                                          _i32, _i32]),
    "gsa_sparse_align_cost": (_i32, [_i32p, _i32p, ctypes.POINTER(SparseGeom), _i32p, _i32, _i32p, _i32, _i32p,
                                     _i32, _i32]),
    "gsa_check_sparse_dev": (ctypes.c_int, [_vp, _vp, _i32, _vp, _i32, _vp, _i32, _i32, ctypes.POINTER(SparseGeom),
                                            _vp, _vp, ctypes.POINTER(CheckResult), _vp]),
    "gsa_check_full_dev": (ctypes.c_int, [_vp, _vp, _i32, _vp, _i32, _vp, _i32, _i32, _vp,
                                          ctypes.POINTER(CheckResult), _vp]),
    "gsa_check_full_pitched_dev": (ctypes.c_int, [_vp, _vp, _i32, _vp, _i32, _vp, _i32, _i32, _vp, _i32,
                                                  ctypes.POINTER(CheckResult), _vp]),
    "gsa_hash_full_dev": (ctypes.c_int, [_vp, _vp, _i32, _i32, _i32, ctypes.POINTER(ctypes.c_uint32), _vp]),
    "gsa_trace_full_dev": (ctypes.c_int, [_vp, _vp, _i32, _vp, _i32, _vp, _i32, ctypes.c_char_p, _i64,
                                          ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_uint32), _i32p,
                                          _vp]),
    "gsa_score_dev": (ctypes.c_int, [_vp, _vp, _i32, _vp, _i32, _vp, _i32, _i32, _i32, _i32,
                                     ctypes.POINTER(ScoreResult), _vp]),
    "gsa_score_semi_dev": (ctypes.c_int, [_vp, _vp, _i32, _vp, _i32, _vp, _i32, _i32, _i32,
                                          ctypes.POINTER(ScoreResult), _vp]),
    "gsa_align_pair_semi_dev": (ctypes.c_int, [_vp, _vp, _i32, _vp, _i32, _vp, _i32, _i32, _i32, _i64,
                                               ctypes.POINTER(AlignDbResult), ctypes.c_char_p, _i64, ctypes.POINTER(_i64),
                                               ctypes.POINTER(AlignPairSemiInfo), ctypes.POINTER(ctypes.c_float), _vp]),
    "gsa_score_overlap_dev": (ctypes.c_int, [_vp, _vp, _i32, _vp, _i32, _vp, _i32, _i32, _i32,
                                             ctypes.POINTER(ScoreResult), _vp]),
    "gsa_align_pair_overlap_dev": (ctypes.c_int, [_vp, _vp, _i32, _vp, _i32, _vp, _i32, _i32, _i32, _i64,
                                                  ctypes.POINTER(AlignDbResult), ctypes.c_char_p, _i64,
                                                  ctypes.POINTER(_i64), ctypes.POINTER(AlignPairOverlapInfo),
                                                  ctypes.POINTER(ctypes.c_float), _vp]),
    "gsa_band_max_width": (ctypes.c_int64, []),
    "gsa_score_band_dev": (ctypes.c_int, [_vp, _vp, _i32, _vp, _i32, _vp, _i32, _i32, _i32, _i64, _i64,
                                          ctypes.POINTER(ScoreResult), _vp]),
    "gsa_align_pair_band_dev": (ctypes.c_int, [_vp, _vp, _i32, _vp, _i32, _vp, _i32, _i32, _i32, _i64, _i64, _i64,
                                               ctypes.POINTER(AlignDbResult), ctypes.c_char_p, _i64, ctypes.POINTER(_i64),
                                               ctypes.POINTER(AlignPairBandInfo), ctypes.POINTER(ctypes.c_float), _vp]),
    "gsa_score_band_batch_dev": (ctypes.c_int, [_vp, _i32, ctypes.POINTER(PairDev), _vp, _i32, _i32, _i32,
                                                ctypes.POINTER(_i64), ctypes.POINTER(_i64), _i32, _i32,
                                                ctypes.POINTER(ScoreResult), ctypes.POINTER(ctypes.c_float), _vp]),
    "gsa_align_batch_band_dev": (ctypes.c_int, [_vp, _i32, ctypes.POINTER(PairDev), _vp, _i32, _i32, _i32,
                                                ctypes.POINTER(_i64), ctypes.POINTER(_i64), _i32, _i32, _i64,
                                                ctypes.POINTER(AlignDbResult), ctypes.c_char_p, _i64, ctypes.POINTER(_i64),
                                                ctypes.POINTER(AlignBatchBandPair), ctypes.POINTER(AlignBatchBandInfo),
                                                ctypes.POINTER(ctypes.c_float), _vp]),
    "gsa_score_band_ext_dev": (ctypes.c_int, [_vp, _vp, _i32, _vp, _i32, _vp, _i32, _i32, _i32, _i64, _i64,
                                              ctypes.POINTER(ScoreResult), _vp]),
    "gsa_align_pair_band_ext_dev": (ctypes.c_int, [_vp, _vp, _i32, _vp, _i32, _vp, _i32, _i32, _i32, _i64, _i64, _i64,
                                                   ctypes.POINTER(AlignDbResult), ctypes.c_char_p, _i64,
                                                   ctypes.POINTER(_i64), ctypes.POINTER(AlignPairBandExtInfo),
                                                   ctypes.POINTER(ctypes.c_float), _vp]),
    "gsa_score_band_ext_batch_dev": (ctypes.c_int, [_vp, _i32, ctypes.POINTER(PairDev), _vp, _i32, _i32, _i32,
                                                    ctypes.POINTER(_i64), ctypes.POINTER(_i64), _i32, _i32,
                                                    ctypes.POINTER(ScoreResult), ctypes.POINTER(ctypes.c_float), _vp]),
    "gsa_align_batch_band_ext_dev": (ctypes.c_int, [_vp, _i32, ctypes.POINTER(PairDev), _vp, _i32, _i32, _i32,
                                                    ctypes.POINTER(_i64), ctypes.POINTER(_i64), _i32, _i32, _i64,
                                                    ctypes.POINTER(AlignDbResult), ctypes.c_char_p, _i64,
                                                    ctypes.POINTER(_i64), ctypes.POINTER(AlignBatchBandExtPair),
                                                    ctypes.POINTER(AlignBatchBandExtInfo),
                                                    ctypes.POINTER(ctypes.c_float), _vp]),
    "gsa_score_batch_dev": (ctypes.c_int, [_vp, _i32, ctypes.POINTER(PairDev), _vp, _i32, _i32, _i32, _i32,
                                           ctypes.POINTER(ScoreResult), ctypes.POINTER(ctypes.c_float), _vp]),
    "gsa_score_db_dev": (ctypes.c_int, [_vp, _vp, _i32, _vp, ctypes.POINTER(_i64), _i32, _vp, _i32, _i32, _i32, _i32,
                                        ctypes.POINTER(ScoreResult), ctypes.POINTER(ctypes.c_float), _vp]),
    "gsa_align_db_dev": (ctypes.c_int, [_vp, _vp, _i32, _vp, ctypes.POINTER(_i64), _i32, _i32p, _i32, _vp, _i32, _i32,
                                        _i32, _i32, _i64, ctypes.POINTER(AlignDbResult), ctypes.c_char_p, _i64,
                                        ctypes.POINTER(_i64), ctypes.POINTER(AlignDbInfo),
                                        ctypes.POINTER(ctypes.c_float), _vp]),
    "gsa_align_pair_dev": (ctypes.c_int, [_vp, _vp, _i32, _vp, _i32, _vp, _i32, _i32, _i32, _i32, _i64,
                                          ctypes.POINTER(AlignDbResult), ctypes.c_char_p, _i64, ctypes.POINTER(_i64),
                                          ctypes.POINTER(AlignPairInfo), ctypes.POINTER(ctypes.c_float), _vp]),
    "gsa_align_batch_dev": (ctypes.c_int, [_vp, _i32, ctypes.POINTER(PairDev), _vp, _i32, _i32, _i32, _i32, _i32, _i64,
                                           ctypes.POINTER(AlignDbResult), ctypes.c_char_p, _i64, ctypes.POINTER(_i64),
                                           ctypes.POINTER(AlignBatchInfo), ctypes.POINTER(ctypes.c_float), _vp]),
    "gsa_score_semi_batch_dev": (ctypes.c_int, [_vp, _i32, ctypes.POINTER(PairDev), _vp, _i32, _i32, _i32,
                                                ctypes.POINTER(ScoreResult), ctypes.POINTER(ctypes.c_float), _vp]),
    "gsa_align_batch_semi_dev": (ctypes.c_int, [_vp, _i32, ctypes.POINTER(PairDev), _vp, _i32, _i32, _i32, _i32, _i64,
                                                ctypes.POINTER(AlignDbResult), ctypes.c_char_p, _i64, ctypes.POINTER(_i64),
                                                ctypes.POINTER(AlignBatchSemiInfo), ctypes.POINTER(ctypes.c_float), _vp]),
    "gsa_score_overlap_batch_dev": (ctypes.c_int, [_vp, _i32, ctypes.POINTER(PairDev), _vp, _i32, _i32, _i32,
                                                   ctypes.POINTER(ScoreResult), ctypes.POINTER(ctypes.c_float), _vp]),
    "gsa_align_batch_overlap_dev": (ctypes.c_int, [_vp, _i32, ctypes.POINTER(PairDev), _vp, _i32, _i32, _i32, _i32, _i64,
                                                   ctypes.POINTER(AlignDbResult), ctypes.c_char_p, _i64, ctypes.POINTER(_i64),
                                                   ctypes.POINTER(AlignBatchOverlapInfo), ctypes.POINTER(ctypes.c_float),
                                                   _vp]),
    "gsa_score_db_multi_dev": (ctypes.c_int, [_vp, _vp, ctypes.POINTER(_i64), _i32, _vp, ctypes.POINTER(_i64), _i32, _vp,
                                              _i32, _i32, _i32, _i32, _i32, _i32, _i64, _i32p,
                                              ctypes.POINTER(DbHit), ctypes.POINTER(ScoreDbMultiInfo),
                                              ctypes.POINTER(ctypes.c_float), _vp]),
    "gsa_score_db_multi_unit": (_i32, []),
    "gsa_align_db_multi_dev": (ctypes.c_int, [_vp, _vp, ctypes.POINTER(_i64), _i32, _vp, ctypes.POINTER(_i64), _i32, _i32p,
                                              _i32p, _i32, _vp, _i32, _i32, _i32, _i32, _i32, _i64,
                                              ctypes.POINTER(AlignDbResult), ctypes.c_char_p, _i64, ctypes.POINTER(_i64),
                                              ctypes.POINTER(AlignDbMultiInfo), ctypes.POINTER(ctypes.c_float), _vp]),
    "gsa_align_db_multi_unit": (_i32, []),
    "gsa_score_db_multi_semi_dev": (ctypes.c_int, [_vp, _vp, ctypes.POINTER(_i64), _i32, _vp, ctypes.POINTER(_i64), _i32,
                                                   _vp, _i32, _i32, _i32, _i32, _i32, _i64, _i32p,
                                                   ctypes.POINTER(DbHit), ctypes.POINTER(ScoreDbMultiInfo),
                                                   ctypes.POINTER(ctypes.c_float), _vp]),
    "gsa_align_db_multi_semi_dev": (ctypes.c_int, [_vp, _vp, ctypes.POINTER(_i64), _i32, _vp, ctypes.POINTER(_i64), _i32,
                                                   _i32p, _i32p, _i32, _vp, _i32, _i32, _i32, _i32, _i64,
                                                   ctypes.POINTER(AlignDbResult), ctypes.c_char_p, _i64,
                                                   ctypes.POINTER(_i64), ctypes.POINTER(AlignDbMultiInfo),
                                                   ctypes.POINTER(ctypes.c_float), _vp]),
    "gsa_score_db_multi_overlap_dev": (ctypes.c_int, [_vp, _vp, ctypes.POINTER(_i64), _i32, _vp, ctypes.POINTER(_i64),
                                                      _i32, _vp, _i32, _i32, _i32, _i32, _i32, _i64, _i32p,
                                                      ctypes.POINTER(DbHit), ctypes.POINTER(ScoreDbMultiInfo),
                                                      ctypes.POINTER(ctypes.c_float), _vp]),
    "gsa_align_db_multi_overlap_dev": (ctypes.c_int, [_vp, _vp, ctypes.POINTER(_i64), _i32, _vp, ctypes.POINTER(_i64),
                                                      _i32, _i32p, _i32p, _i32, _vp, _i32, _i32, _i32, _i32, _i64,
                                                      ctypes.POINTER(AlignDbResult), ctypes.c_char_p, _i64,
                                                      ctypes.POINTER(_i64), ctypes.POINTER(AlignDbMultiInfo),
                                                      ctypes.POINTER(ctypes.c_float), _vp]),
    "gsa_score":(ctypes.c_int, [_vp, _i32p, _i32, _i32p, _i32, _i32p, _i32, _i32, _i32, _i32,
                                 ctypes.POINTER(ScoreResult), ctypes.POINTER(_Laps)]),
    "gsa_trace_sparse_dev": (ctypes.c_int, [_vp, _vp, _i32, _vp, _i32, _vp, _i32, _i32, ctypes.POINTER(SparseGeom),
                                            _vp, _vp, ctypes.c_char_p, _i64, ctypes.POINTER(ctypes.c_int64),
                                            ctypes.POINTER(ctypes.c_uint32), _i32p, _vp]),
}

# the knobs the library knows (kKnobNames, csrc/gsa_capi.hip), in its order; gsa_set_knob refuses others
KNOB_NAMES = (
    "GSA_SPARSE_KERNEL", "GSA_KROW_K", "GSA_KROW_NS", "GSA_KROW_Q8", "GSA_LANE_NS",
    "GSA_LANE_FEED", "GSA_LANE_PAIR", "GSA_FULL_KERNEL", "GSA_FULL_FUSED", "GSA_FULL_SPLIT",
    "GSA_FUSED_STAGED",
    "GSA_EXPAND_RR", "GSA_BATCH_ORDER", "GSA_SCORE_SCAN", "GSA_SCORE_KERNEL", "GSA_SCORE_K",
    "GSA_SCORE_BIDI", "GSA_SCORE_BIDI_SW", "GSA_BIDI_GRAN", "GSA_BIDI_SKEW", "GSA_BIDI_SW_CONT",
    "GSA_BIDI_LOG", "GSA_TRACE_BAND", "GSA_TRACE_BAND_BUDGET", "GSA_STAMPS", "GSA_DB_LANES",
    "GSA_DB_MAXC")


def lib():
    """Load libgsa.so.  Raises if it has not been built: there is no fallback path."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(_SO):
            raise ImportError(f"{_SO} missing: run __graft_entry__.build() (hipcc --offload-arch=gfx950)")
        # PyTorch-ROCm may ship a HIP runtime of its own.  Loaded after libgsa.so it is a second runtime
        # in the process, and whichever of the two initialises second finds no device; loaded first, it
        # has the name libgsa.so asks for and serves both.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = ctypes.CDLL(_SO)
        for name, (res, args) in SIGNATURES.items():
            if os.environ.get("GSA_LIB") and not hasattr(L, name):
                continue  # diagnostic builds of older revisions may lack newer entry points
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _LIB = L
    return _LIB


def _p(a: np.ndarray):
    assert a.dtype == np.int32 and a.flags["C_CONTIGUOUS"], (a.dtype, a.flags)
    return a.ctypes.data_as(_i32p)


def _c32(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.int32)


def score_db_multi_unit() -> int:
    """Wave tasks (of four subjects) in a unit of gsa_score_db_multi_dev."""
    return int(lib().gsa_score_db_multi_unit())


def band_max_width() -> int:
    """Most diagonals a band of score_band / align_pair_band may hold after clamping."""
    return int(lib().gsa_band_max_width())


def align_db_multi_unit() -> int:
    """Wave tasks (of up to four hits) in a unit of gsa_align_db_multi_dev."""
    return int(lib().gsa_align_db_multi_unit())


def sparse_tile_by() -> int:
    return int(lib().gsa_sparse_tile_by())


def full_pitch(adjcols: int) -> int:
    """Row pitch (ints) of the fastest device layout of a full matrix (gsa_full_pitch: = 1 mod 32)."""
    return int(lib().gsa_full_pitch(adjcols))


def full_base_offset() -> int:
    """Ints from a 128-byte boundary to cell (0, 0) of that layout (cell (1, 0) on the boundary)."""
    return int(lib().gsa_full_base_offset())


def sparse_geometry(adjrows: int, adjcols: int, tileBx: int) -> SparseGeom:
    g = SparseGeom()
    st = lib().gsa_sparse_geometry(adjrows, adjcols, tileBx, ctypes.byref(g))
    if st != NwStat.success:
        raise NwError(st, "gsa_sparse_geometry")
    return g


@dataclasses.dataclass
class AlignResult:
    score: np.ndarray  # (adjrows, adjcols) int32
    align_cost: int
    laps: dict


@dataclasses.dataclass
class SparseResult:
    hrow: np.ndarray
    hcol: np.ndarray
    geom: SparseGeom
    align_cost: int
    laps: dict

    @property
    def trows(self):
        return self.geom.tileHdrMatRows

    @property
    def tcols(self):
        return self.geom.tileHdrMatCols


class Engine:
    """One device context (initNwInput equivalent, src/benchmark.cpp:175-223)."""

    def __init__(self, device: int = 0):
        self.device = device
        h = _vp()
        st = lib().gsa_ctx_create(device, ctypes.byref(h))
        if st != NwStat.success:
            raise NwError(st, f"gsa_ctx_create(device={device})")
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            lib().gsa_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    @property
    def cu_count(self) -> int:
        return int(lib().gsa_device_cu_count(self._h))

    def _check(self, st, where):
        if st != NwStat.success:
            raise NwError(st, where, int(lib().gsa_last_hip_error(self._h)))

    # -- NwAlignFn equivalents (host buffers) -------------------------------------------
    def align_full(self, seqY, seqX, subst, gapo: int) -> AlignResult:
        """Full int32 score matrix (the gpu3..gpu6 family's nw.score)."""
        seqY, seqX, subst = _c32(seqY), _c32(seqX), _c32(subst)
        substsz = int(round(np.sqrt(subst.size)))
        score = np.empty((len(seqY), len(seqX)), dtype=np.int32)
        cost = ctypes.c_int32(0)
        laps = _Laps()
        st = lib().gsa_align_full(self._h, _p(seqY), len(seqY), _p(seqX), len(seqX), _p(subst), substsz, gapo,
                                  _p(score), ctypes.byref(cost), ctypes.byref(laps))
        self._check(st, "gsa_align_full")
        return AlignResult(score, int(cost.value), laps.as_dict())

    def align_sparse(self, seqY, seqX, subst, gapo: int, tileBx: int = 256, overlap: bool = False) -> SparseResult:
        """Tile-header (mlsp) representation (the gpu7..gpu9 family's tileHrowMat/tileHcolMat).
        overlap=True: mlsppt, the copy-back runs tile row by tile row during the fill."""
        seqY, seqX, subst = _c32(seqY), _c32(seqX), _c32(subst)
        substsz = int(round(np.sqrt(subst.size)))
        geom = sparse_geometry(len(seqY), len(seqX), tileBx)
        hrow = np.empty(geom.hrowElems, dtype=np.int32)
        hcol = np.empty(geom.hcolElems, dtype=np.int32)
        cost = ctypes.c_int32(0)
        laps = _Laps()
        fn = lib().gsa_align_sparse_pt if overlap else lib().gsa_align_sparse
        st = fn(self._h, _p(seqY), len(seqY), _p(seqX), len(seqX), _p(subst), substsz, gapo, tileBx, _p(hrow),
                _p(hcol), ctypes.byref(geom), ctypes.byref(cost), ctypes.byref(laps))
        self._check(st, "gsa_align_sparse_pt" if overlap else "gsa_align_sparse")
        return SparseResult(hrow, hcol, geom, int(cost.value), laps.as_dict())

    # -- hot path on device-resident buffers (torch tensors or raw pointers) -------------
    def fill_full_dev(self, seqY_ptr: int, adjrows: int, seqX_ptr: int, adjcols: int, subst_ptr: int, substsz: int,
                      gapo: int, score_ptr: int, stream: Optional[int] = None, ld: Optional[int] = None):
        """Full matrix into device memory; ld = row pitch in ints (None: unpadded, adjcols)."""
        if ld is None:
            st = lib().gsa_fill_full_dev(self._h, seqY_ptr, adjrows, seqX_ptr, adjcols, subst_ptr, substsz, gapo,
                                         score_ptr, stream)
            self._check(st, "gsa_fill_full_dev")
        else:
            st = lib().gsa_fill_full_pitched_dev(self._h, seqY_ptr, adjrows, seqX_ptr, adjcols, subst_ptr, substsz,
                                                 gapo, score_ptr, int(ld), stream)
            self._check(st, "gsa_fill_full_pitched_dev")

    def fill_sparse_dev(self, seqY_ptr: int, adjrows: int, seqX_ptr: int, adjcols: int, subst_ptr: int,
                        substsz: int, gapo: int, tileBx: int, hrow_ptr: int, hcol_ptr: int,
                        stream: Optional[int] = None):
        st = lib().gsa_fill_sparse_dev(self._h, seqY_ptr, adjrows, seqX_ptr, adjcols, subst_ptr, substsz, gapo,
                                       tileBx, hrow_ptr, hcol_ptr, stream)
        self._check(st, "gsa_fill_sparse_dev")

    def fill_batch_dev(self, pairs, subst_ptr: int, substsz: int, gapo: int, mode: str = "sparse",
                       tileBx: int = 256, stream: Optional[int] = None, lds: Optional[Sequence[int]] = None):
        """One persistent launch over many pairs.  `pairs`: sequence of (seqY_ptr, adjrows,
        seqX_ptr, adjcols, out) with out = score_ptr (full) or (hrow_ptr, hcol_ptr) (sparse);
        lds: full matrices' row pitches (None: unpadded)."""
        arr = (PairDev * len(pairs))()
        for k, (yp, ar, xp, ac, out) in enumerate(pairs):
            arr[k].seqY, arr[k].adjrows, arr[k].seqX, arr[k].adjcols = yp, ar, xp, ac
            if mode == "sparse":
                arr[k].tileHrowMat, arr[k].tileHcolMat = out
            else:
                arr[k].score = out
        if mode == "sparse":
            st = lib().gsa_fill_sparse_batch_dev(self._h, len(pairs), arr, subst_ptr, substsz, gapo, tileBx, stream)
        elif lds is None:
            st = lib().gsa_fill_full_batch_dev(self._h, len(pairs), arr, subst_ptr, substsz, gapo, stream)
        else:
            la = _c32(list(lds))
            st = lib().gsa_fill_full_batch_pitched_dev(self._h, len(pairs), arr, _p(la), subst_ptr, substsz, gapo,
                                                       stream)
        self._check(st, "gsa_fill_%s_batch_dev" % mode)

    def sync(self, stream: Optional[int] = None):
        """Wait for `stream`; raises NwError if a hand-off of ANY fill enqueued since the last
        sync gave up (the error word is sticky until this call clears it)."""
        self._check(lib().gsa_sync(self._h, stream), "gsa_sync")

    def debug_stamps(self):
        """The stamps of the last launch made under GSA_STAMPS=1 (gsa_debug_stamps), uint64: a fused
        full fill's [realtime start, end, shader clock start, end] per pass-1 strip, then [claimed,
        ready, done] per expansion task; a K-rows fill's strip ledger [realtime start, end, clock
        start, end, cycles waiting, waits, 4 block spans (diagnostic builds)] per strip; empty if
        none were recorded."""
        import numpy as np
        n = ctypes.c_int64(0)
        self._check(lib().gsa_debug_stamps(self._h, None, 0, ctypes.byref(n)), "gsa_debug_stamps")
        out = np.zeros(n.value, dtype=np.uint64)
        if n.value:
            self._check(lib().gsa_debug_stamps(self._h, out.ctypes.data, n.value, ctypes.byref(n)), "gsa_debug_stamps")
        return out

    def set_full_timing(self, on: bool = True):
        """Events around the passes of every two-pass full fill and pass 2's clock stamps
        (gsa_set_full_timing; a measurement aid)."""
        self._check(lib().gsa_set_full_timing(self._h, 1 if on else 0), "gsa_set_full_timing")

    def last_full_timing(self) -> dict:
        """The last timed full fill (gsa_last_full_timing): pass1_ms, pass2_ms (HIP events; a fused
        fill: pass1_ms None, the launch in pass2_ms), pass 2's effective clock in GHz (median over
        workgroups and cycle-weighted mean of s_memtime / s_memrealtime), waits for that fill."""
        t = FullTiming()
        self._check(lib().gsa_last_full_timing(self._h, ctypes.byref(t)), "gsa_last_full_timing")
        f = lambda v: None if v < 0 else round(float(v), 4)
        return {"pass1_ms": f(t.pass1_ms), "pass2_ms": f(t.pass2_ms), "clock_ghz_median": f(t.clock_ghz_median),
                "clock_ghz_mean": f(t.clock_ghz_mean), "clock_workgroups": int(t.workgroups), "fused": bool(t.fused),
                "pipelined_groups": int(t.groups)}

    def last_launch(self) -> dict:
        """Which instance the last fill, score call or device trace on this context ran
        (gsa_last_launch; a measurement and test aid): "kind" (one of LAUNCH_KINDS) and the fields of
        gsa_launch_info.  Waits for that launch (q8_declined is written by it).  Raises NwError
        (errorInvalidValue) when nothing has been launched yet."""
        li = LaunchInfo()
        self._check(lib().gsa_last_launch(self._h, ctypes.byref(li)), "gsa_last_launch")
        d = {k: int(getattr(li, k)) for k, _ in li._fields_}
        d["kind"] = LAUNCH_KINDS[li.kind]
        return d

    def set_knob(self, name: str, value: Optional[str]):
        """Set a measurement / test switch (GSA_FULL_KERNEL, GSA_KROW_NS, ...) for this context
        (gsa_set_knob); None unsets it.  A context takes the knobs from the environment once, when
        it is created."""
        self._check(lib().gsa_set_knob(self._h, name.encode(), None if value is None else str(value).encode()),
                    "gsa_set_knob")

    def set_lap_callback(self, fn: Optional[Callable[[str], None]]):
        """fn(lap_name) at every phase boundary of the host-buffer entry points (align_full,
        align_sparse, score): gsa_set_lap_callback, the hook an adapter uses to drive the
        reference's Stopwatch::lap (src/stopwatch.hpp:19).  None removes it."""
        if fn is None:
            self._lapcb = None
            self._check(lib().gsa_set_lap_callback(self._h, None, None), "gsa_set_lap_callback")
            return
        cb = _LAPFN(lambda _user, name: fn(name.decode()))
        self._check(lib().gsa_set_lap_callback(self._h, ctypes.cast(cb, _vp), None), "gsa_set_lap_callback")
        self._lapcb = cb  # keep the thunk alive while the library holds it

    def set_watchdog(self, microseconds: int):
        """No-progress limit of every wait inside later fills (default 1 s)."""
        self._check(lib().gsa_set_watchdog(self._h, int(microseconds)), "gsa_set_watchdog")

    def mem_stats(self) -> dict:
        m = MemStats()
        self._check(lib().gsa_mem_stats_get(self._h, ctypes.byref(m)), "gsa_mem_stats_get")
        return m.as_dict()

    def reset_mem_stats(self):
        self._check(lib().gsa_mem_stats_reset(self._h), "gsa_mem_stats_reset")

    # -- score-only NW / SW, linear or affine gaps (BASELINE configs[4]) -----------------
    def score(self, seqY, seqX, subst, gapo: int, gape: Optional[int] = None, local: bool = False) -> dict:
        """Score-only alignment (host buffers): {"score", "i_end", "j_end", "laps"}; gape
        defaults to gapo (linear gaps; global + linear = the reference's NW-LG align_cost)."""
        seqY, seqX, subst = _c32(seqY), _c32(seqX), _c32(subst)
        substsz = int(round(np.sqrt(subst.size)))
        r = ScoreResult()
        laps = _Laps()
        st = lib().gsa_score(self._h, _p(seqY), len(seqY), _p(seqX), len(seqX), _p(subst), substsz, gapo,
                             gapo if gape is None else gape, int(local), ctypes.byref(r), ctypes.byref(laps))
        self._check(st, "gsa_score")
        return {"score": int(r.score), "i_end": int(r.i_end), "j_end": int(r.j_end), "laps": laps.as_dict()}

    def score_dev(self, seqY_ptr: int, adjrows: int, seqX_ptr: int, adjcols: int, subst_ptr: int, substsz: int,
                  gapo: int, gape: int, local: bool = False, stream: Optional[int] = None) -> dict:
        r = ScoreResult()
        st = lib().gsa_score_dev(self._h, seqY_ptr, adjrows, seqX_ptr, adjcols, subst_ptr, substsz, gapo, gape,
                                 int(local), ctypes.byref(r), stream)
        self._check(st, "gsa_score_dev")
        return {"score": int(r.score), "i_end": int(r.i_end), "j_end": int(r.j_end),
                "kernel_ms": float(r.calc_kernel_ms)}

    # -- long pairs, semi-global: a whole query within a long subject ---------
    def score_semi_dev(self, seqY_ptr: int, adjrows: int, seqX_ptr: int, adjcols: int, subst_ptr: int, substsz: int,
                       gapo: int, gape: Optional[int] = None, stream: Optional[int] = None) -> dict:
        """Semi-global score of one device-resident pair (gsa_score_semi_dev; synchronous): the whole
        query seqY within the subject seqX, whose head and tail are free.  The arguments of score_dev
        without `local`; gape defaults to gapo.  {"score", "i_end", "j_end", "kernel_ms"} as score_dev
        returns them: i_end is the query's length, j_end the smallest column of row i_end that attains
        the score."""
        r = ScoreResult()
        st = lib().gsa_score_semi_dev(self._h, seqY_ptr, adjrows, seqX_ptr, adjcols, subst_ptr, substsz, gapo,
                                      gapo if gape is None else gape, ctypes.byref(r), stream)
        self._check(st, "gsa_score_semi_dev")
        return {"score": int(r.score), "i_end": int(r.i_end), "j_end": int(r.j_end),
                "kernel_ms": float(r.calc_kernel_ms)}

    def score_semi(self, seqY, seqX, subst, gapo: int, gape: Optional[int] = None) -> dict:
        """score_semi_dev over host arrays: the sequences with the header element in front, as score()
        takes them; sequences and table are uploaded through torch."""
        import torch
        dev = torch.device("cuda", self.device)
        up = lambda a: torch.from_numpy(_c32(a)).to(dev)
        subst = _c32(subst)
        substsz = int(round(np.sqrt(subst.size)))
        dS, dY, dX = up(subst.ravel()), up(seqY), up(seqX)
        torch.cuda.synchronize(dev)
        return self.score_semi_dev(dY.data_ptr(), dY.numel(), dX.data_ptr(), dX.numel(), dS.data_ptr(), substsz, gapo,
                                   gape)

    def align_pair_semi_dev(self, seqY_ptr: int, adjrows: int, seqX_ptr: int, adjcols: int, subst_ptr: int,
                            substsz: int, gapo: int, gape: Optional[int] = None, scratch_limit: int = 0,
                            stream: Optional[int] = None) -> dict:
        """The semi-global alignment of one device-resident pair (gsa_align_pair_semi_dev; synchronous):
        the arguments of score_semi_dev, and `scratch_limit`, the bytes of move codes held at once (0:
        the default, 2 GiB).  {"score", "status", "i_start", "j_start", "i_end", "j_end", "cigar",
        "kernel_ms"} as align_pair_dev returns them; i_start is 0, status is 0 (never 1).
        last_align_pair_semi_info() says what ran."""
        res = AlignDbResult()
        info = AlignPairSemiInfo()
        ms = ctypes.c_float(0.0)
        need = ctypes.c_int64(0)
        # 2 (R + C) + 1 bytes always suffice
        cap = 2 * (max(adjrows - 1, 0) + max(adjcols - 1, 0)) + 1
        buf = ctypes.create_string_buffer(cap)
        st = lib().gsa_align_pair_semi_dev(self._h, seqY_ptr, adjrows, seqX_ptr, adjcols, subst_ptr, substsz, gapo,
                                           gapo if gape is None else gape, int(scratch_limit), ctypes.byref(res), buf,
                                           cap, ctypes.byref(need), ctypes.byref(info), ctypes.byref(ms), stream)
        self._check(st, "gsa_align_pair_semi_dev")
        self._align_pair_semi_info = {k: (float(getattr(info, k)) if t is ctypes.c_float else int(getattr(info, k)))
                                      for k, t in info._fields_ if k != "pad0"}
        cig = buf.raw[res.cigar_off:res.cigar_off + res.cigar_len].decode() if res.status == 0 else ""
        return {"score": int(res.score), "status": int(res.status), "i_start": int(res.i_start),
                "j_start": int(res.j_start), "i_end": int(res.i_end), "j_end": int(res.j_end), "cigar": cig,
                "kernel_ms": float(ms.value)}

    def last_align_pair_semi_info(self) -> dict:
        """gsa_align_pair_semi_info of the last align_pair_semi_dev call on this engine: "strip_rows",
        "strips" (those of the rows 1 ... R), "strips_filled", "chunks" (fill + walk launch pairs),
        "code_bytes" (peak bytes of move codes held at once), "j_window" (codes are kept for the columns
        behind it only), "score_ms", "fill_ms" and "walk_ms"."""
        info = getattr(self, "_align_pair_semi_info", None)
        if info is None:
            raise NwError(NwStat.errorInvalidValue, "last_align_pair_semi_info: no align_pair_semi_dev call yet")
        return dict(info)

    def align_pair_semi(self, seqY, seqX, subst, gapo: int, gape: Optional[int] = None, scratch_limit: int = 0) -> dict:
        """align_pair_semi_dev over host arrays: the sequences with the header element in front, as
        score() takes them; sequences and table are uploaded through torch."""
        import torch
        dev = torch.device("cuda", self.device)
        up = lambda a: torch.from_numpy(_c32(a)).to(dev)
        subst = _c32(subst)
        substsz = int(round(np.sqrt(subst.size)))
        dS, dY, dX = up(subst.ravel()), up(seqY), up(seqX)
        torch.cuda.synchronize(dev)
        return self.align_pair_semi_dev(dY.data_ptr(), dY.numel(), dX.data_ptr(), dX.numel(), dS.data_ptr(), substsz,
                                        gapo, gape, scratch_limit)

    # -- long pairs, overlap (dovetail): a suffix of either sequence on a prefix of the other --
    def score_overlap_dev(self, seqY_ptr: int, adjrows: int, seqX_ptr: int, adjcols: int, subst_ptr: int, substsz: int,
                          gapo: int, gape: Optional[int] = None, stream: Optional[int] = None) -> dict:
        """Overlap (dovetail) score of one device-resident pair (gsa_score_overlap_dev; synchronous):
        row 0 and column 0 are free, and the score is the largest value on the last row or the last
        column -- a suffix of one sequence against a prefix of the other, or either within the other.
        The arguments of score_semi_dev; gape defaults to gapo.  {"score", "i_end", "j_end",
        "kernel_ms"}: the score is never negative; the end cell is the first cell of the last row that
        attains it, or else the first such cell of the last column."""
        r = ScoreResult()
        st = lib().gsa_score_overlap_dev(self._h, seqY_ptr, adjrows, seqX_ptr, adjcols, subst_ptr, substsz, gapo,
                                         gapo if gape is None else gape, ctypes.byref(r), stream)
        self._check(st, "gsa_score_overlap_dev")
        return {"score": int(r.score), "i_end": int(r.i_end), "j_end": int(r.j_end),
                "kernel_ms": float(r.calc_kernel_ms)}

    def score_overlap(self, seqY, seqX, subst, gapo: int, gape: Optional[int] = None) -> dict:
        """score_overlap_dev over host arrays: the sequences with the header element in front, as score()
        takes them; sequences and table are uploaded through torch."""
        import torch
        dev = torch.device("cuda", self.device)
        up = lambda a: torch.from_numpy(_c32(a)).to(dev)
        subst = _c32(subst)
        substsz = int(round(np.sqrt(subst.size)))
        dS, dY, dX = up(subst.ravel()), up(seqY), up(seqX)
        torch.cuda.synchronize(dev)
        return self.score_overlap_dev(dY.data_ptr(), dY.numel(), dX.data_ptr(), dX.numel(), dS.data_ptr(), substsz, gapo,
                                      gape)

    def align_pair_overlap_dev(self, seqY_ptr: int, adjrows: int, seqX_ptr: int, adjcols: int, subst_ptr: int,
                               substsz: int, gapo: int, gape: Optional[int] = None, scratch_limit: int = 0,
                               stream: Optional[int] = None) -> dict:
        """The overlap alignment of one device-resident pair (gsa_align_pair_overlap_dev; synchronous):
        the arguments of score_overlap_dev, and `scratch_limit`, the bytes of move codes held at once
        (0: the default, 2 GiB).  {"score", "status", "i_start", "j_start", "i_end", "j_end", "cigar",
        "kernel_ms"} as align_pair_semi_dev returns them; the start cell lies on row 0 or on column 0,
        no overhang is in the CIGAR, status is 0 (never 1).  last_align_pair_overlap_info() says what ran."""
        res = AlignDbResult()
        info = AlignPairOverlapInfo()
        ms = ctypes.c_float(0.0)
        need = ctypes.c_int64(0)
        # 2 (R + C) + 1 bytes always suffice
        cap = 2 * (max(adjrows - 1, 0) + max(adjcols - 1, 0)) + 1
        buf = ctypes.create_string_buffer(cap)
        st = lib().gsa_align_pair_overlap_dev(self._h, seqY_ptr, adjrows, seqX_ptr, adjcols, subst_ptr, substsz, gapo,
                                              gapo if gape is None else gape, int(scratch_limit), ctypes.byref(res),
                                              buf, cap, ctypes.byref(need), ctypes.byref(info), ctypes.byref(ms), stream)
        self._check(st, "gsa_align_pair_overlap_dev")
        self._align_pair_overlap_info = {k: (float(getattr(info, k)) if t is ctypes.c_float else int(getattr(info, k)))
                                         for k, t in info._fields_ if k != "pad0"}
        cig = buf.raw[res.cigar_off:res.cigar_off + res.cigar_len].decode() if res.status == 0 else ""
        return {"score": int(res.score), "status": int(res.status), "i_start": int(res.i_start),
                "j_start": int(res.j_start), "i_end": int(res.i_end), "j_end": int(res.j_end), "cigar": cig,
                "kernel_ms": float(ms.value)}

    def last_align_pair_overlap_info(self) -> dict:
        """gsa_align_pair_overlap_info of the last align_pair_overlap_dev call on this engine:
        "strip_rows", "strips" (those of the rows 1 ... i_end), "strips_filled", "chunks" (fill + walk
        launch pairs), "code_bytes" (peak bytes of move codes held at once), "score_ms", "fill_ms" and
        "walk_ms"."""
        info = getattr(self, "_align_pair_overlap_info", None)
        if info is None:
            raise NwError(NwStat.errorInvalidValue, "last_align_pair_overlap_info: no align_pair_overlap_dev call yet")
        return dict(info)

    def align_pair_overlap(self, seqY, seqX, subst, gapo: int, gape: Optional[int] = None, scratch_limit: int = 0) -> dict:
        """align_pair_overlap_dev over host arrays: the sequences with the header element in front, as
        score() takes them; sequences and table are uploaded through torch."""
        import torch
        dev = torch.device("cuda", self.device)
        up = lambda a: torch.from_numpy(_c32(a)).to(dev)
        subst = _c32(subst)
        substsz = int(round(np.sqrt(subst.size)))
        dS, dY, dX = up(subst.ravel()), up(seqY), up(seqX)
        torch.cuda.synchronize(dev)
        return self.align_pair_overlap_dev(dY.data_ptr(), dY.numel(), dX.data_ptr(), dX.numel(), dS.data_ptr(), substsz,
                                           gapo, gape, scratch_limit)

    # -- long pairs, banded: global alignment inside a band of diagonals --
    def score_band_dev(self, seqY_ptr: int, adjrows: int, seqX_ptr: int, adjcols: int, subst_ptr: int, substsz: int,
                       gapo: int, gape: Optional[int], band_lo: int, band_hi: int, stream: Optional[int] = None) -> dict:
        """Banded global score of one device-resident pair (gsa_score_band_dev; synchronous): only the
        cells with band_lo <= j - i <= band_hi exist.  The arguments of score_semi_dev, with the band
        behind gape (None: gapo).  {"score", "i_end", "j_end", "kernel_ms"}; the end cell is (R, C).
        The band must hold (0, 0) and (R, C) and, clamped to the matrix, at most band_max_width()
        diagonals."""
        r = ScoreResult()
        st = lib().gsa_score_band_dev(self._h, seqY_ptr, adjrows, seqX_ptr, adjcols, subst_ptr, substsz, gapo,
                                      gapo if gape is None else gape, int(band_lo), int(band_hi), ctypes.byref(r), stream)
        self._check(st, "gsa_score_band_dev")
        return {"score": int(r.score), "i_end": int(r.i_end), "j_end": int(r.j_end),
                "kernel_ms": float(r.calc_kernel_ms)}

    @staticmethod
    def _band_of(R: int, C: int, band_lo, band_hi, band):
        """The band of the host forms: (band_lo, band_hi) as given, or `band` diagonals on either side
        of the ones that (0, 0) and (R, C) need.  Exactly one of the two forms."""
        pair = band_lo is not None or band_hi is not None
        if pair == (band is not None) or (pair and (band_lo is None or band_hi is None)):
            raise ValueError("give either band_lo and band_hi, or band")
        if pair:
            return int(band_lo), int(band_hi)
        return min(0, C - R) - int(band), max(0, C - R) + int(band)

    def score_band(self, seqY, seqX, subst, gapo: int, gape: Optional[int] = None, band_lo: Optional[int] = None,
                   band_hi: Optional[int] = None, band: Optional[int] = None) -> dict:
        """score_band_dev over host arrays: the sequences with the header element in front, as score()
        takes them.  The band as (band_lo, band_hi), or band=k for band_lo = min(0, C - R) - k and
        band_hi = max(0, C - R) + k; exactly one of the two forms, else ValueError."""
        import torch
        lo, hi = self._band_of(len(seqY) - 1, len(seqX) - 1, band_lo, band_hi, band)
        dev = torch.device("cuda", self.device)
        up = lambda a: torch.from_numpy(_c32(a)).to(dev)
        subst = _c32(subst)
        substsz = int(round(np.sqrt(subst.size)))
        dS, dY, dX = up(subst.ravel()), up(seqY), up(seqX)
        torch.cuda.synchronize(dev)
        return self.score_band_dev(dY.data_ptr(), dY.numel(), dX.data_ptr(), dX.numel(), dS.data_ptr(), substsz, gapo,
                                   gape, lo, hi)

    def align_pair_band_dev(self, seqY_ptr: int, adjrows: int, seqX_ptr: int, adjcols: int, subst_ptr: int,
                            substsz: int, gapo: int, gape: Optional[int], band_lo: int, band_hi: int,
                            scratch_limit: int = 0, stream: Optional[int] = None) -> dict:
        """The banded global alignment of one device-resident pair (gsa_align_pair_band_dev;
        synchronous): the arguments of score_band_dev, and `scratch_limit`, the bytes of move codes the
        call may hold (0: the default, 2 GiB).  {"score", "status", "i_start", "j_start", "i_end",
        "j_end", "cigar", "kernel_ms"} as align_pair_dev returns them, from (0, 0) to (R, C); status 1:
        score and end cell only (the value bound reaches 2^26, or the codes exceed scratch_limit).
        last_align_pair_band_info() says what ran, and whether the result is proved to be the unbanded
        one."""
        res = AlignDbResult()
        info = AlignPairBandInfo()
        ms = ctypes.c_float(0.0)
        need = ctypes.c_int64(0)
        # 2 (R + C) + 1 bytes always suffice
        cap = 2 * (max(adjrows - 1, 0) + max(adjcols - 1, 0)) + 1
        buf = ctypes.create_string_buffer(cap)
        st = lib().gsa_align_pair_band_dev(self._h, seqY_ptr, adjrows, seqX_ptr, adjcols, subst_ptr, substsz, gapo,
                                           gapo if gape is None else gape, int(band_lo), int(band_hi),
                                           int(scratch_limit), ctypes.byref(res), buf, cap, ctypes.byref(need),
                                           ctypes.byref(info), ctypes.byref(ms), stream)
        self._check(st, "gsa_align_pair_band_dev")
        self._align_pair_band_info = {k: (float(getattr(info, k)) if t is ctypes.c_float else int(getattr(info, k)))
                                      for k, t in info._fields_ if k != "pad0"}
        cig = buf.raw[res.cigar_off:res.cigar_off + res.cigar_len].decode() if res.status == 0 else ""
        return {"score": int(res.score), "status": int(res.status), "i_start": int(res.i_start),
                "j_start": int(res.j_start), "i_end": int(res.i_end), "j_end": int(res.j_end), "cigar": cig,
                "kernel_ms": float(ms.value)}

    def last_align_pair_band_info(self) -> dict:
        """gsa_align_pair_band_info of the last align_pair_band_dev call on this engine: "strip_rows",
        "strips", "waves", "supersteps" (the workgroup's barriers), "proved_optimal" (1: the result is
        the unbanded call's, field for field), "band_lo" and "band_hi" (clamped to the matrix),
        "code_bytes", "score_ms" (the fill) and "walk_ms"."""
        info = getattr(self, "_align_pair_band_info", None)
        if info is None:
            raise NwError(NwStat.errorInvalidValue, "last_align_pair_band_info: no align_pair_band_dev call yet")
        return dict(info)

    def align_pair_band(self, seqY, seqX, subst, gapo: int, gape: Optional[int] = None, band_lo: Optional[int] = None,
                        band_hi: Optional[int] = None, band: Optional[int] = None, scratch_limit: int = 0) -> dict:
        """align_pair_band_dev over host arrays, with the band as score_band() takes it."""
        import torch
        lo, hi = self._band_of(len(seqY) - 1, len(seqX) - 1, band_lo, band_hi, band)
        dev = torch.device("cuda", self.device)
        up = lambda a: torch.from_numpy(_c32(a)).to(dev)
        subst = _c32(subst)
        substsz = int(round(np.sqrt(subst.size)))
        dS, dY, dX = up(subst.ravel()), up(seqY), up(seqX)
        torch.cuda.synchronize(dev)
        return self.align_pair_band_dev(dY.data_ptr(), dY.numel(), dX.data_ptr(), dX.numel(), dS.data_ptr(), substsz,
                                        gapo, gape, lo, hi, scratch_limit)

    # -- long pairs, banded extension: from (0, 0) to the best cell of the band --
    def score_band_ext_dev(self, seqY_ptr: int, adjrows: int, seqX_ptr: int, adjcols: int, subst_ptr: int, substsz: int,
                           gapo: int, gape: Optional[int], band_lo: int, band_hi: int, stream: Optional[int] = None) -> dict:
        """Banded extension score of one device-resident pair (gsa_score_band_ext_dev; synchronous):
        score_band_dev's arguments; the score is the largest H of the band, never negative, and the
        end cell the first maximal one in row-major order.  The band must hold (0, 0) -- not (R, C) --
        and, clamped to the matrix, at most band_max_width() diagonals."""
        r = ScoreResult()
        st = lib().gsa_score_band_ext_dev(self._h, seqY_ptr, adjrows, seqX_ptr, adjcols, subst_ptr, substsz, gapo,
                                          gapo if gape is None else gape, int(band_lo), int(band_hi), ctypes.byref(r),
                                          stream)
        self._check(st, "gsa_score_band_ext_dev")
        return {"score": int(r.score), "i_end": int(r.i_end), "j_end": int(r.j_end),
                "kernel_ms": float(r.calc_kernel_ms)}

    @staticmethod
    def _band_ext_of(band_lo, band_hi, band):
        """The band of the extension's host forms: (band_lo, band_hi) as given, or band=w for (-w, w).
        Exactly one of the two forms."""
        pair = band_lo is not None or band_hi is not None
        if pair == (band is not None) or (pair and (band_lo is None or band_hi is None)):
            raise ValueError("give either band_lo and band_hi, or band")
        return (int(band_lo), int(band_hi)) if pair else (-int(band), int(band))

    def _upload_pair(self, seqY, seqX, subst):
        import torch
        dev = torch.device("cuda", self.device)
        up = lambda a: torch.from_numpy(_c32(a)).to(dev)
        subst = _c32(subst)
        dS, dY, dX = up(subst.ravel()), up(seqY), up(seqX)
        torch.cuda.synchronize(dev)
        return dS, dY, dX, int(round(np.sqrt(subst.size)))

    def score_band_ext(self, seqY, seqX, subst, gapo: int, gape: Optional[int] = None, band_lo: Optional[int] = None,
                       band_hi: Optional[int] = None, band: Optional[int] = None) -> dict:
        """score_band_ext_dev over host arrays, the sequences with the header element in front.  The
        band as (band_lo, band_hi), or band=w for (-w, w); exactly one of the two forms, else
        ValueError."""
        lo, hi = self._band_ext_of(band_lo, band_hi, band)
        dS, dY, dX, substsz = self._upload_pair(seqY, seqX, subst)
        return self.score_band_ext_dev(dY.data_ptr(), dY.numel(), dX.data_ptr(), dX.numel(), dS.data_ptr(), substsz,
                                       gapo, gape, lo, hi)

    def align_pair_band_ext_dev(self, seqY_ptr: int, adjrows: int, seqX_ptr: int, adjcols: int, subst_ptr: int,
                                substsz: int, gapo: int, gape: Optional[int], band_lo: int, band_hi: int,
                                scratch_limit: int = 0, stream: Optional[int] = None) -> dict:
        """The banded extension alignment of one device-resident pair (gsa_align_pair_band_ext_dev;
        synchronous): align_pair_band_dev's arguments and keys, from (0, 0) to the band's best cell;
        status 1: score and end cell only.  last_align_pair_band_ext_info() says what ran."""
        res = AlignDbResult()
        info = AlignPairBandExtInfo()
        ms = ctypes.c_float(0.0)
        need = ctypes.c_int64(0)
        # 2 (R + C) + 1 bytes always suffice
        cap = 2 * (max(adjrows - 1, 0) + max(adjcols - 1, 0)) + 1
        buf = ctypes.create_string_buffer(cap)
        st = lib().gsa_align_pair_band_ext_dev(self._h, seqY_ptr, adjrows, seqX_ptr, adjcols, subst_ptr, substsz, gapo,
                                               gapo if gape is None else gape, int(band_lo), int(band_hi),
                                               int(scratch_limit), ctypes.byref(res), buf, cap, ctypes.byref(need),
                                               ctypes.byref(info), ctypes.byref(ms), stream)
        self._check(st, "gsa_align_pair_band_ext_dev")
        self._align_pair_band_ext_info = {k: (float(getattr(info, k)) if t is ctypes.c_float else int(getattr(info, k)))
                                          for k, t in info._fields_ if k != "pad0"}
        cig = buf.raw[res.cigar_off:res.cigar_off + res.cigar_len].decode() if res.status == 0 else ""
        return {"score": int(res.score), "status": int(res.status), "i_start": int(res.i_start),
                "j_start": int(res.j_start), "i_end": int(res.i_end), "j_end": int(res.j_end), "cigar": cig,
                "kernel_ms": float(ms.value)}

    def last_align_pair_band_ext_info(self) -> dict:
        """gsa_align_pair_band_ext_info of the last align_pair_band_ext_dev call on this engine:
        last_align_pair_band_info()'s keys, of the part of the pair the band reaches, and that part's
        "rows_used" and "cols_used"; "proved_optimal" 1: the result is the unbanded extension's."""
        info = getattr(self, "_align_pair_band_ext_info", None)
        if info is None:
            raise NwError(NwStat.errorInvalidValue, "last_align_pair_band_ext_info: no align_pair_band_ext_dev call yet")
        return dict(info)

    def align_pair_band_ext(self, seqY, seqX, subst, gapo: int, gape: Optional[int] = None,
                            band_lo: Optional[int] = None, band_hi: Optional[int] = None, band: Optional[int] = None,
                            scratch_limit: int = 0) -> dict:
        """align_pair_band_ext_dev over host arrays, with the band as score_band_ext() takes it."""
        lo, hi = self._band_ext_of(band_lo, band_hi, band)
        dS, dY, dX, substsz = self._upload_pair(seqY, seqX, subst)
        return self.align_pair_band_ext_dev(dY.data_ptr(), dY.numel(), dX.data_ptr(), dX.numel(), dS.data_ptr(),
                                            substsz, gapo, gape, lo, hi, scratch_limit)

    def score_batch_dev(self, pairs, subst_ptr: int, substsz: int, gapo: int, gape: Optional[int] = None,
                        local: bool = False, stream: Optional[int] = None) -> list:
        """Score-only alignment of many device-resident pairs in one persistent launch
        (gsa_score_batch_dev; synchronous).  `pairs`: sequence of (seqY_ptr, adjrows, seqX_ptr,
        adjcols).  One dict per pair, in order, equal to score_dev's for that pair alone except
        "kernel_ms", which is the hipEvent time of the whole call's kernels in every dict."""
        n = len(pairs)
        arr = (PairDev * max(n, 1))()
        for k, (yp, ar, xp, ac) in enumerate(pairs):
            arr[k].seqY, arr[k].adjrows, arr[k].seqX, arr[k].adjcols = yp, ar, xp, ac
        res = (ScoreResult * max(n, 1))()
        ms = ctypes.c_float(0.0)
        st = lib().gsa_score_batch_dev(self._h, n, arr, subst_ptr, substsz, gapo, gapo if gape is None else gape,
                                       int(local), res, ctypes.byref(ms), stream)
        self._check(st, "gsa_score_batch_dev")
        return [{"score": int(r.score), "i_end": int(r.i_end), "j_end": int(r.j_end), "kernel_ms": float(ms.value)}
                for r in res[:n]]

    def score_batch(self, pairs, subst, gapo: int, gape: Optional[int] = None, local: bool = False) -> list:
        """score_batch_dev over host arrays: `pairs` is a sequence of (seqY, seqX) with the header
        element in front, as score() takes them; sequences and table are uploaded through torch.
        One dict per pair: {"score", "i_end", "j_end", "kernel_ms"}."""
        import torch
        dev = torch.device("cuda", self.device)
        up = lambda a: torch.from_numpy(_c32(a)).to(dev)
        subst = _c32(subst)
        substsz = int(round(np.sqrt(subst.size)))
        dS = up(subst.ravel())
        keep, ptrs = [], []
        for y, x in pairs:
            dY, dX = up(y), up(x)
            keep.append((dY, dX))
            ptrs.append((dY.data_ptr(), dY.numel(), dX.data_ptr(), dX.numel()))
        torch.cuda.synchronize(dev)
        return self.score_batch_dev(ptrs, dS.data_ptr(), substsz, gapo, gape, local)

    def score_db_dev(self, query_ptr: int, adjq: int, db_ptr: int, db_off, subst_ptr: int, substsz: int, gapo: int,
                     gape: Optional[int] = None, local: bool = False, stream: Optional[int] = None) -> list:
        """Database search (gsa_score_db_dev; synchronous): one device-resident query against the
        subjects of one device buffer `db_ptr`, each with its header element; `db_off` holds the
        len(db_off) - 1 subjects' offsets into it (ints, strictly increasing).  One dict per subject,
        equal to score_dev's for (query, subject) except "kernel_ms", the hipEvent time of the whole
        call's kernels in every dict."""
        off = np.ascontiguousarray(db_off, dtype=np.int64)
        n = len(off) - 1
        res = (ScoreResult * max(n, 1))()
        ms = ctypes.c_float(0.0)
        st = lib().gsa_score_db_dev(self._h, query_ptr, adjq, db_ptr, off.ctypes.data_as(ctypes.POINTER(_i64)), n,
                                    subst_ptr, substsz, gapo, gapo if gape is None else gape, int(local), res,
                                    ctypes.byref(ms), stream)
        self._check(st, "gsa_score_db_dev")
        return [{"score": int(r.score), "i_end": int(r.i_end), "j_end": int(r.j_end), "kernel_ms": float(ms.value)}
                for r in res[:n]]

    def score_db(self, query, subjects, subst, gapo: int, gape: Optional[int] = None, local: bool = False) -> list:
        """score_db_dev over host arrays: `query` and every entry of `subjects` with the header
        element in front, as score() takes them.  The subjects are concatenated and uploaded once
        through torch.  One dict per subject: {"score", "i_end", "j_end", "kernel_ms"}."""
        import torch
        dev = torch.device("cuda", self.device)
        up = lambda a: torch.from_numpy(_c32(a)).to(dev)
        subst = _c32(subst)
        substsz = int(round(np.sqrt(subst.size)))
        subjects = [_c32(x) for x in subjects]
        off = np.zeros(len(subjects) + 1, dtype=np.int64)
        if subjects:
            off[1:] = np.cumsum([len(x) for x in subjects])
        dS, dQ = up(subst.ravel()), up(query)
        dD = up(np.concatenate(subjects) if subjects else np.zeros(1, np.int32))
        torch.cuda.synchronize(dev)
        return self.score_db_dev(dQ.data_ptr(), dQ.numel(), dD.data_ptr(), off, dS.data_ptr(), substsz, gapo, gape,
                                 local)

    # -- alignments of database hits, traced on the device ----------------

    def align_db_dev(self, query_ptr: int, adjq: int, db_ptr: int, db_off, hits, subst_ptr: int, substsz: int,
                     gapo: int, gape: Optional[int] = None, local: bool = False, scratch_limit: int = 0,
                     stream: Optional[int] = None) -> list:
        """The alignments of chosen subjects of a database (gsa_align_db_dev; synchronous): query,
        database and table as score_db_dev takes them, `hits` the subject indices (any order, repeats
        allowed), `scratch_limit` the bytes of move codes held at once (0: the default).  One dict per
        hit, in order: {"score", "status", "i_start", "j_start", "i_end", "j_end", "cigar", "kernel_ms"};
        status 0 aligned, 1 score and end cell only (outside the trace kernel's limits; "cigar" is "").
        "kernel_ms" is the hipEvent time of the whole call's kernels in every dict.
        last_align_db_info() says what the call ran."""
        off = np.ascontiguousarray(db_off, dtype=np.int64)
        hit = np.ascontiguousarray(hits, dtype=np.int32).ravel()
        n, nh = len(off) - 1, len(hit)
        res = (AlignDbResult * max(nh, 1))()
        info = AlignDbInfo()
        ms = ctypes.c_float(0.0)
        need = ctypes.c_int64(0)
        # 2 (R + C) + 1 bytes per hit always suffice
        cap = 0
        if nh and n >= 1 and hit.min() >= 0 and hit.max() < n:
            cap = int(2 * (np.diff(off)[hit].clip(1) - 1 + max(adjq - 1, 0)).sum() + nh)
        buf = ctypes.create_string_buffer(max(cap, 1))
        st = lib().gsa_align_db_dev(self._h, query_ptr, adjq, db_ptr, off.ctypes.data_as(ctypes.POINTER(_i64)), n,
                                    hit.ctypes.data_as(_i32p), nh, subst_ptr, substsz, gapo,
                                    gapo if gape is None else gape, int(local), int(scratch_limit), res, buf, cap,
                                    ctypes.byref(need), ctypes.byref(info), ctypes.byref(ms), stream)
        self._check(st, "gsa_align_db_dev")
        self._align_db_info = {k: (float(getattr(info, k)) if t is ctypes.c_float else int(getattr(info, k)))
                               for k, t in info._fields_}
        raw = buf.raw
        out = []
        for r in res[:nh]:
            cig = raw[r.cigar_off:r.cigar_off + r.cigar_len].decode() if r.status == 0 else ""
            out.append({"score": int(r.score), "status": int(r.status), "i_start": int(r.i_start),
                        "j_start": int(r.j_start), "i_end": int(r.i_end), "j_end": int(r.j_end), "cigar": cig,
                        "kernel_ms": float(ms.value)})
        return out

    def last_align_db_info(self) -> dict:
        """gsa_align_db_info of the last align_db_dev call on this engine: "lane_hits" traced on the
        device, "unsupported" (status 1), "chunks" (fill + walk launch pairs), "tasks", "code_bytes"
        (peak bytes of move codes held at once), "fill_ms" and "walk_ms"."""
        info = getattr(self, "_align_db_info", None)
        if info is None:
            raise NwError(NwStat.errorInvalidValue, "last_align_db_info: no align_db_dev call yet")
        return dict(info)

    def align_db(self, query, subjects, hits, subst, gapo: int, gape: Optional[int] = None,
                 local: bool = False) -> list:
        """align_db_dev over host arrays: `query` and every entry of `subjects` with the header element
        in front, as score_db takes them; `hits` indexes `subjects`."""
        import torch
        dev = torch.device("cuda", self.device)
        up = lambda a: torch.from_numpy(_c32(a)).to(dev)
        subst = _c32(subst)
        substsz = int(round(np.sqrt(subst.size)))
        subjects = [_c32(x) for x in subjects]
        off = np.zeros(len(subjects) + 1, dtype=np.int64)
        if subjects:
            off[1:] = np.cumsum([len(x) for x in subjects])
        dS, dQ = up(subst.ravel()), up(query)
        dD = up(np.concatenate(subjects) if subjects else np.zeros(1, np.int32))
        torch.cuda.synchronize(dev)
        return self.align_db_dev(dQ.data_ptr(), dQ.numel(), dD.data_ptr(), off, hits, dS.data_ptr(), substsz, gapo,
                                 gape, local)

    def search_db(self, query, subjects, subst, gapo: int, gape: Optional[int] = None, local: bool = False,
                  top: int = 10) -> list:
        """Database search with alignments: score_db over all subjects, then align_db on the `top` best
        scores (equal scores: the smaller index first).  [(subject_index, result dict)] in that order."""
        scores = self.score_db(query, subjects, subst, gapo, gape, local)
        order = sorted(range(len(scores)), key=lambda s: (-scores[s]["score"], s))[:max(int(top), 0)]
        if not order:
            return []
        return list(zip(order, self.align_db(query, subjects, order, subst, gapo, gape, local)))

    # -- the alignment of one long pair, traced on the device -----------------

    def align_pair_dev(self, seqY_ptr: int, adjrows: int, seqX_ptr: int, adjcols: int, subst_ptr: int, substsz: int,
                       gapo: int, gape: Optional[int] = None, local: bool = False, scratch_limit: int = 0,
                       stream: Optional[int] = None) -> dict:
        """The alignment of one device-resident pair of any length the K-rows score kernel takes
        (gsa_align_pair_dev; synchronous): the arguments of score_dev, and `scratch_limit`, the bytes
        of move codes held at once (0: the default, 2 GiB).  {"score", "status", "i_start",
        "j_start", "i_end", "j_end", "cigar", "kernel_ms"} as align_db_dev returns per hit; status 0
        aligned, 1 score and end cell only ("cigar" is "").  last_align_pair_info() says what ran."""
        res = AlignDbResult()
        info = AlignPairInfo()
        ms = ctypes.c_float(0.0)
        need = ctypes.c_int64(0)
        # 2 (R + C) + 1 bytes always suffice
        cap = 2 * (max(adjrows - 1, 0) + max(adjcols - 1, 0)) + 1
        buf = ctypes.create_string_buffer(cap)
        st = lib().gsa_align_pair_dev(self._h, seqY_ptr, adjrows, seqX_ptr, adjcols, subst_ptr, substsz, gapo,
                                      gapo if gape is None else gape, int(local), int(scratch_limit),
                                      ctypes.byref(res), buf, cap, ctypes.byref(need), ctypes.byref(info),
                                      ctypes.byref(ms), stream)
        self._check(st, "gsa_align_pair_dev")
        self._align_pair_info = {k: (float(getattr(info, k)) if t is ctypes.c_float else int(getattr(info, k)))
                                 for k, t in info._fields_ if k != "pad0"}
        cig = buf.raw[res.cigar_off:res.cigar_off + res.cigar_len].decode() if res.status == 0 else ""
        return {"score": int(res.score), "status": int(res.status), "i_start": int(res.i_start),
                "j_start": int(res.j_start), "i_end": int(res.i_end), "j_end": int(res.j_end), "cigar": cig,
                "kernel_ms": float(ms.value)}

    def last_align_pair_info(self) -> dict:
        """gsa_align_pair_info of the last align_pair_dev call on this engine: "strip_rows" (the score
        kernel's ticket, 0 when it did not run), "strips" up to the end cell's row, "strips_filled",
        "chunks" (fill + walk launch pairs), "code_bytes" (peak bytes of move codes held at once),
        "score_ms", "fill_ms" and "walk_ms"."""
        info = getattr(self, "_align_pair_info", None)
        if info is None:
            raise NwError(NwStat.errorInvalidValue, "last_align_pair_info: no align_pair_dev call yet")
        return dict(info)

    def align_pair(self, seqY, seqX, subst, gapo: int, gape: Optional[int] = None, local: bool = False,
                   scratch_limit: int = 0) -> dict:
        """align_pair_dev over host arrays: the sequences with the header element in front, as score()
        takes them; sequences and table are uploaded through torch."""
        import torch
        dev = torch.device("cuda", self.device)
        up = lambda a: torch.from_numpy(_c32(a)).to(dev)
        subst = _c32(subst)
        substsz = int(round(np.sqrt(subst.size)))
        dS, dY, dX = up(subst.ravel()), up(seqY), up(seqX)
        torch.cuda.synchronize(dev)
        return self.align_pair_dev(dY.data_ptr(), dY.numel(), dX.data_ptr(), dX.numel(), dS.data_ptr(), substsz, gapo,
                                   gape, local, scratch_limit)

    # -- the alignments of a batch of long pairs in one call -----------------

    def align_batch_dev(self, pairs, subst_ptr: int, substsz: int, gapo: int, gape: Optional[int] = None,
                        local: bool = False, max_workgroups: int = 0, scratch_limit: int = 0,
                        stream: Optional[int] = None) -> list:
        """The alignments of many device-resident long pairs, traced on the device together
        (gsa_align_batch_dev; synchronous).  `pairs`: sequence of (seqY_ptr, adjrows, seqX_ptr,
        adjcols), as score_batch_dev takes it.  One dict per pair, in order, with align_pair_dev's keys
        and, "kernel_ms" apart (the hipEvent time of the whole call's kernels in every dict), its
        values for that pair alone.  `max_workgroups` caps the grids of the fill and of the walk (0: all
        resident), `scratch_limit` the bytes of move codes held at once (0: the default, 8 GiB).
        last_align_batch_info() says what ran."""
        n = len(pairs)
        arr = (PairDev * max(n, 1))()
        cap = 0
        for k, (yp, ar, xp, ac) in enumerate(pairs):
            arr[k].seqY, arr[k].adjrows, arr[k].seqX, arr[k].adjcols = yp, ar, xp, ac
            cap += 2 * (max(ar - 1, 0) + max(ac - 1, 0)) + 1  # 2 (R + C) + 1 bytes always suffice
        res = (AlignDbResult * max(n, 1))()
        info = AlignBatchInfo()
        ms = ctypes.c_float(0.0)
        need = ctypes.c_int64(0)
        buf = ctypes.create_string_buffer(max(cap, 1))
        st = lib().gsa_align_batch_dev(self._h, n, arr, subst_ptr, substsz, gapo, gapo if gape is None else gape,
                                       int(local), int(max_workgroups), int(scratch_limit), res, buf, cap,
                                       ctypes.byref(need), ctypes.byref(info), ctypes.byref(ms), stream)
        self._check(st, "gsa_align_batch_dev")
        self._align_batch_info = {k: (float(getattr(info, k)) if t is ctypes.c_float else int(getattr(info, k)))
                                  for k, t in info._fields_ if not k.startswith("pad")}
        raw = buf.raw
        return [{"score": int(r.score), "status": int(r.status), "i_start": int(r.i_start), "j_start": int(r.j_start),
                 "i_end": int(r.i_end), "j_end": int(r.j_end),
                 "cigar": raw[r.cigar_off:r.cigar_off + r.cigar_len].decode() if r.status == 0 else "",
                 "kernel_ms": float(ms.value)} for r in res[:n]]

    def last_align_batch_info(self) -> dict:
        """gsa_align_batch_info of the last align_batch_dev call on this engine: "batch_pairs" (traced
        by the batched route), "alone_pairs" (passed on to align_pair_dev's path), "host_pairs",
        "strip_rows", "strips" over all batch pairs up to each end cell's row, "strips_filled", "rounds"
        (fill + walk launch pairs), "code_bytes" (peak bytes of move codes held at once), "score_ms",
        "fill_ms" and "walk_ms"."""
        info = getattr(self, "_align_batch_info", None)
        if info is None:
            raise NwError(NwStat.errorInvalidValue, "last_align_batch_info: no align_batch_dev call yet")
        return dict(info)

    def align_batch(self, pairs, subst, gapo: int, gape: Optional[int] = None, local: bool = False,
                    scratch_limit: int = 0) -> list:
        """align_batch_dev over host arrays: `pairs` is a sequence of (seqY, seqX) with the header
        element in front, as score_batch() takes them; sequences and table are uploaded through torch."""
        import torch
        dev = torch.device("cuda", self.device)
        up = lambda a: torch.from_numpy(_c32(a)).to(dev)
        subst = _c32(subst)
        substsz = int(round(np.sqrt(subst.size)))
        dS = up(subst.ravel())
        keep, ptrs = [], []
        for y, x in pairs:
            dY, dX = up(y), up(x)
            keep.append((dY, dX))
            ptrs.append((dY.data_ptr(), dY.numel(), dX.data_ptr(), dX.numel()))
        torch.cuda.synchronize(dev)
        return self.align_batch_dev(ptrs, dS.data_ptr(), substsz, gapo, gape, local, 0, scratch_limit)

    # -- long pairs, semi-global: scores and alignments of a batch in one call --

    def _upload_pairs(self, pairs, subst):
        """(pointer tuples, table pointer, substsz, the tensors to keep alive) of host pairs and table."""
        import torch
        dev = torch.device("cuda", self.device)
        up = lambda a: torch.from_numpy(_c32(a)).to(dev)
        subst = _c32(subst)
        substsz = int(round(np.sqrt(subst.size)))
        dS = up(subst.ravel())
        keep, ptrs = [dS], []
        for y, x in pairs:
            dY, dX = up(y), up(x)
            keep.append((dY, dX))
            ptrs.append((dY.data_ptr(), dY.numel(), dX.data_ptr(), dX.numel()))
        torch.cuda.synchronize(dev)
        return ptrs, dS.data_ptr(), substsz, keep

    def score_semi_batch_dev(self, pairs, subst_ptr: int, substsz: int, gapo: int, gape: Optional[int] = None,
                             stream: Optional[int] = None) -> list:
        """Semi-global scores of many device-resident pairs in one launch (gsa_score_semi_batch_dev;
        synchronous).  `pairs`: sequence of (seqY_ptr, adjrows, seqX_ptr, adjcols), seqY the query, seqX
        the subject, as score_batch_dev takes it.  One dict per pair, in order, equal to score_semi_dev's
        for that pair alone except "kernel_ms", which is the hipEvent time of the whole call's kernels
        in every dict."""
        n = len(pairs)
        arr = (PairDev * max(n, 1))()
        for k, (yp, ar, xp, ac) in enumerate(pairs):
            arr[k].seqY, arr[k].adjrows, arr[k].seqX, arr[k].adjcols = yp, ar, xp, ac
        res = (ScoreResult * max(n, 1))()
        ms = ctypes.c_float(0.0)
        st = lib().gsa_score_semi_batch_dev(self._h, n, arr, subst_ptr, substsz, gapo, gapo if gape is None else gape,
                                            res, ctypes.byref(ms), stream)
        self._check(st, "gsa_score_semi_batch_dev")
        return [{"score": int(r.score), "i_end": int(r.i_end), "j_end": int(r.j_end), "kernel_ms": float(ms.value)}
                for r in res[:n]]

    def score_semi_batch(self, pairs, subst, gapo: int, gape: Optional[int] = None) -> list:
        """score_semi_batch_dev over host arrays: `pairs` is a sequence of (seqY, seqX) with the header
        element in front, as score_batch() takes them; sequences and table are uploaded through torch."""
        ptrs, dS, substsz, keep = self._upload_pairs(pairs, subst)
        return self.score_semi_batch_dev(ptrs, dS, substsz, gapo, gape)

    def align_batch_semi_dev(self, pairs, subst_ptr: int, substsz: int, gapo: int, gape: Optional[int] = None,
                             max_workgroups: int = 0, scratch_limit: int = 0, stream: Optional[int] = None) -> list:
        """The semi-global alignments of many device-resident long pairs, traced on the device together
        (gsa_align_batch_semi_dev; synchronous).  `pairs` as score_semi_batch_dev takes it.  One dict
        per pair, in order, with align_pair_semi_dev's keys and, "kernel_ms" apart (the hipEvent time of
        the whole call's kernels in every dict), its values for that pair alone; "status" 1: one strip
        of the pair's windowed codes exceeds `scratch_limit` (score and end cell only).
        `max_workgroups` caps the grids of the fill and of the walk (0: all resident), `scratch_limit`
        the bytes of move codes held at once (0: the default, 8 GiB).  last_align_batch_semi_info()
        says what ran."""
        n = len(pairs)
        arr = (PairDev * max(n, 1))()
        cap = 0
        for k, (yp, ar, xp, ac) in enumerate(pairs):
            arr[k].seqY, arr[k].adjrows, arr[k].seqX, arr[k].adjcols = yp, ar, xp, ac
            cap += 2 * (max(ar - 1, 0) + max(ac - 1, 0)) + 1  # 2 (R + C) + 1 bytes always suffice
        res = (AlignDbResult * max(n, 1))()
        info = AlignBatchSemiInfo()
        ms = ctypes.c_float(0.0)
        need = ctypes.c_int64(0)
        buf = ctypes.create_string_buffer(max(cap, 1))
        st = lib().gsa_align_batch_semi_dev(self._h, n, arr, subst_ptr, substsz, gapo, gapo if gape is None else gape,
                                            int(max_workgroups), int(scratch_limit), res, buf, cap, ctypes.byref(need),
                                            ctypes.byref(info), ctypes.byref(ms), stream)
        self._check(st, "gsa_align_batch_semi_dev")
        self._align_batch_semi_info = {k: (float(getattr(info, k)) if t is ctypes.c_float else int(getattr(info, k)))
                                       for k, t in info._fields_ if not k.startswith("pad")}
        raw = buf.raw
        return [{"score": int(r.score), "status": int(r.status), "i_start": int(r.i_start), "j_start": int(r.j_start),
                 "i_end": int(r.i_end), "j_end": int(r.j_end),
                 "cigar": raw[r.cigar_off:r.cigar_off + r.cigar_len].decode() if r.status == 0 else "",
                 "kernel_ms": float(ms.value)} for r in res[:n]]

    def last_align_batch_semi_info(self) -> dict:
        """gsa_align_batch_semi_info of the last align_batch_semi_dev call on this engine: "batch_pairs"
        (traced on the device), "host_pairs", "strip_rows", "strips" over all traced pairs, "strips_filled",
        "rounds" (fill + walk launch pairs), "code_bytes" (peak bytes of move codes held at once),
        "window_cols" (the sum over traced pairs of j_end - jW), "gran_bytes" (checkpoint rows the score
        launch kept), "score_ms", "fill_ms" and "walk_ms"."""
        info = getattr(self, "_align_batch_semi_info", None)
        if info is None:
            raise NwError(NwStat.errorInvalidValue, "last_align_batch_semi_info: no align_batch_semi_dev call yet")
        return dict(info)

    def align_batch_semi(self, pairs, subst, gapo: int, gape: Optional[int] = None, scratch_limit: int = 0) -> list:
        """align_batch_semi_dev over host arrays: `pairs` is a sequence of (seqY, seqX) with the header
        element in front, as score_batch() takes them; sequences and table are uploaded through torch."""
        ptrs, dS, substsz, keep = self._upload_pairs(pairs, subst)
        return self.align_batch_semi_dev(ptrs, dS, substsz, gapo, gape, 0, scratch_limit)

    # -- long pairs, banded: scores and alignments of a batch in one call --

    @staticmethod
    def _band_arrays(n: int, bands):
        if len(bands) != n:
            raise ValueError("one (band_lo, band_hi) per pair")
        lo, hi = (ctypes.c_int64 * max(n, 1))(), (ctypes.c_int64 * max(n, 1))()
        for k, (a, b) in enumerate(bands):
            lo[k], hi[k] = int(a), int(b)
        return lo, hi

    def score_band_batch_dev(self, pairs, subst_ptr: int, substsz: int, gapo: int, gape: Optional[int] = None,
                             stream: Optional[int] = None, *, bands, waves: int = 0, max_workgroups: int = 0) -> list:
        """Banded global scores of many device-resident pairs in one launch (gsa_score_band_batch_dev;
        synchronous).  `pairs` as score_semi_batch_dev takes it, `bands` a sequence of (band_lo,
        band_hi), one per pair.  One dict per pair, in order, equal to score_band_dev's for that pair
        alone except "kernel_ms", which is the hipEvent time of the whole call's kernel in every dict.
        `waves` is the waves per workgroup (4, 8, 16; 0: the smallest that serves every pair),
        `max_workgroups` caps the grid (0: all resident); no result depends on either."""
        n = len(pairs)
        lo, hi = self._band_arrays(n, bands)
        arr = (PairDev * max(n, 1))()
        for k, (yp, ar, xp, ac) in enumerate(pairs):
            arr[k].seqY, arr[k].adjrows, arr[k].seqX, arr[k].adjcols = yp, ar, xp, ac
        res = (ScoreResult * max(n, 1))()
        ms = ctypes.c_float(0.0)
        st = lib().gsa_score_band_batch_dev(self._h, n, arr, subst_ptr, substsz, gapo, gapo if gape is None else gape,
                                            lo, hi, int(waves), int(max_workgroups), res, ctypes.byref(ms), stream)
        self._check(st, "gsa_score_band_batch_dev")
        return [{"score": int(r.score), "i_end": int(r.i_end), "j_end": int(r.j_end), "kernel_ms": float(ms.value)}
                for r in res[:n]]

    @staticmethod
    def _bands_of(pairs, bands, band):
        """The bands of the host batch forms: `bands` as given, or `band` through _band_of per pair;
        exactly one of the two, else ValueError."""
        if (bands is None) == (band is None):
            raise ValueError("give either bands or band")
        if bands is not None:
            return [(int(a), int(b)) for a, b in bands]
        return [Engine._band_of(len(y) - 1, len(x) - 1, None, None, band) for y, x in pairs]

    def score_band_batch(self, pairs, subst, gapo: int, gape: Optional[int] = None, *, bands=None,
                         band: Optional[int] = None, waves: int = 0, max_workgroups: int = 0) -> list:
        """score_band_batch_dev over host arrays: `pairs` is a sequence of (seqY, seqX) with the header
        element in front, as score_batch() takes them.  The bands as bands=[(band_lo, band_hi), ...] or
        band=k, applied per pair as score_band() applies it; exactly one of the two forms, else
        ValueError."""
        bl = self._bands_of(pairs, bands, band)
        ptrs, dS, substsz, keep = self._upload_pairs(pairs, subst)
        return self.score_band_batch_dev(ptrs, dS, substsz, gapo, gape, bands=bl, waves=waves,
                                         max_workgroups=max_workgroups)

    def align_batch_band_dev(self, pairs, subst_ptr: int, substsz: int, gapo: int, gape: Optional[int] = None,
                             max_workgroups: int = 0, scratch_limit: int = 0, stream: Optional[int] = None, *, bands,
                             waves: int = 0) -> list:
        """The banded global alignments of many device-resident long pairs, traced on the device
        together (gsa_align_batch_band_dev; synchronous).  `pairs` and `bands` as score_band_batch_dev
        takes them.  One dict per pair, in order, with align_pair_band_dev's keys and, "kernel_ms"
        apart (the hipEvent time of the whole call's kernels in every dict), its values for that pair
        alone; "status" 1: the pair's move codes exceed `scratch_limit`, or its values the coded
        fill's range (score and end cell only).  `scratch_limit` is the bytes of move codes held at
        once (0: the default, 8 GiB).  last_align_batch_band_info() says what ran, pair by pair."""
        n = len(pairs)
        lo, hi = self._band_arrays(n, bands)
        arr = (PairDev * max(n, 1))()
        cap = 0
        for k, (yp, ar, xp, ac) in enumerate(pairs):
            arr[k].seqY, arr[k].adjrows, arr[k].seqX, arr[k].adjcols = yp, ar, xp, ac
            cap += 2 * (max(ar - 1, 0) + max(ac - 1, 0)) + 1  # 2 (R + C) + 1 bytes always suffice
        res = (AlignDbResult * max(n, 1))()
        pinfo = (AlignBatchBandPair * max(n, 1))()
        info = AlignBatchBandInfo()
        ms = ctypes.c_float(0.0)
        need = ctypes.c_int64(0)
        buf = ctypes.create_string_buffer(max(cap, 1))
        st = lib().gsa_align_batch_band_dev(self._h, n, arr, subst_ptr, substsz, gapo, gapo if gape is None else gape,
                                            lo, hi, int(waves), int(max_workgroups), int(scratch_limit), res, buf, cap,
                                            ctypes.byref(need), pinfo, ctypes.byref(info), ctypes.byref(ms), stream)
        self._check(st, "gsa_align_batch_band_dev")
        d = {k: (float(getattr(info, k)) if t is ctypes.c_float else int(getattr(info, k)))
             for k, t in info._fields_ if not k.startswith("pad")}
        d["pairs"] = [{k: int(getattr(q, k)) for k, _ in q._fields_} for q in pinfo[:n]]
        self._align_batch_band_info = d
        raw = buf.raw
        return [{"score": int(r.score), "status": int(r.status), "i_start": int(r.i_start), "j_start": int(r.j_start),
                 "i_end": int(r.i_end), "j_end": int(r.j_end),
                 "cigar": raw[r.cigar_off:r.cigar_off + r.cigar_len].decode() if r.status == 0 else "",
                 "kernel_ms": float(ms.value)} for r in res[:n]]

    def last_align_batch_band_info(self) -> dict:
        """gsa_align_batch_band_info of the last align_batch_band_dev call on this engine: "batch_pairs"
        (traced on the device), "host_pairs", "nocode_pairs" (status 1), "rounds" (fill + walk launch
        pairs), "waves" (per workgroup), "strip_rows", "code_bytes" (peak bytes of move codes held at
        once), "fill_ms", "nocode_ms" and "walk_ms"; "pairs" is the list of the pairs' own values:
        "band_lo" and "band_hi" (clamped), "code_bytes", "strips", "supersteps", "proved_optimal" and
        "round" (-1: answered on the host, -2: ran without codes)."""
        info = getattr(self, "_align_batch_band_info", None)
        if info is None:
            raise NwError(NwStat.errorInvalidValue, "last_align_batch_band_info: no align_batch_band_dev call yet")
        d = dict(info)
        d["pairs"] = [dict(q) for q in info["pairs"]]
        return d

    def align_batch_band(self, pairs, subst, gapo: int, gape: Optional[int] = None, scratch_limit: int = 0, *,
                         bands=None, band: Optional[int] = None, waves: int = 0, max_workgroups: int = 0) -> list:
        """align_batch_band_dev over host arrays, with the pairs and the bands as score_band_batch()
        takes them."""
        bl = self._bands_of(pairs, bands, band)
        ptrs, dS, substsz, keep = self._upload_pairs(pairs, subst)
        return self.align_batch_band_dev(ptrs, dS, substsz, gapo, gape, max_workgroups, scratch_limit, bands=bl,
                                         waves=waves)

    # -- long pairs, banded extension: scores and alignments of a batch in one call --

    def score_band_ext_batch_dev(self, pairs, subst_ptr: int, substsz: int, gapo: int, gape: Optional[int] = None,
                                 stream: Optional[int] = None, *, bands, waves: int = 0, max_workgroups: int = 0) -> list:
        """Banded extension scores of many device-resident pairs in one launch
        (gsa_score_band_ext_batch_dev; synchronous): score_band_batch_dev's arguments.  One dict per
        pair, in order, equal to score_band_ext_dev's for that pair alone except "kernel_ms", the
        hipEvent time of the whole call's kernel in every dict."""
        n = len(pairs)
        lo, hi = self._band_arrays(n, bands)
        arr = (PairDev * max(n, 1))()
        for k, (yp, ar, xp, ac) in enumerate(pairs):
            arr[k].seqY, arr[k].adjrows, arr[k].seqX, arr[k].adjcols = yp, ar, xp, ac
        res = (ScoreResult * max(n, 1))()
        ms = ctypes.c_float(0.0)
        st = lib().gsa_score_band_ext_batch_dev(self._h, n, arr, subst_ptr, substsz, gapo,
                                                gapo if gape is None else gape, lo, hi, int(waves), int(max_workgroups),
                                                res, ctypes.byref(ms), stream)
        self._check(st, "gsa_score_band_ext_batch_dev")
        return [{"score": int(r.score), "i_end": int(r.i_end), "j_end": int(r.j_end), "kernel_ms": float(ms.value)}
                for r in res[:n]]

    @staticmethod
    def _bands_ext_of(pairs, bands, band):
        """The bands of the extension's host batch forms: `bands` as given, or band=w for (-w, w) per
        pair; exactly one of the two, else ValueError."""
        if (bands is None) == (band is None):
            raise ValueError("give either bands or band")
        if bands is not None:
            return [(int(a), int(b)) for a, b in bands]
        return [(-int(band), int(band)) for _ in pairs]

    def score_band_ext_batch(self, pairs, subst, gapo: int, gape: Optional[int] = None, *, bands=None,
                             band: Optional[int] = None, waves: int = 0, max_workgroups: int = 0) -> list:
        """score_band_ext_batch_dev over host arrays: `pairs` is a sequence of (seqY, seqX) with the
        header element in front.  The bands as bands=[(band_lo, band_hi), ...] or band=w for (-w, w)
        on every pair; exactly one of the two forms, else ValueError."""
        bl = self._bands_ext_of(pairs, bands, band)
        ptrs, dS, substsz, keep = self._upload_pairs(pairs, subst)
        return self.score_band_ext_batch_dev(ptrs, dS, substsz, gapo, gape, bands=bl, waves=waves,
                                             max_workgroups=max_workgroups)

    def align_batch_band_ext_dev(self, pairs, subst_ptr: int, substsz: int, gapo: int, gape: Optional[int] = None,
                                 max_workgroups: int = 0, scratch_limit: int = 0, stream: Optional[int] = None, *,
                                 bands, waves: int = 0) -> list:
        """The banded extension alignments of many device-resident long pairs, traced on the device
        together (gsa_align_batch_band_ext_dev; synchronous): align_batch_band_dev's arguments.  One
        dict per pair, in order, with align_pair_band_ext_dev's keys and, "kernel_ms" apart, its values
        for that pair alone.  last_align_batch_band_ext_info() says what ran, pair by pair."""
        n = len(pairs)
        lo, hi = self._band_arrays(n, bands)
        arr = (PairDev * max(n, 1))()
        cap = 0
        for k, (yp, ar, xp, ac) in enumerate(pairs):
            arr[k].seqY, arr[k].adjrows, arr[k].seqX, arr[k].adjcols = yp, ar, xp, ac
            cap += 2 * (max(ar - 1, 0) + max(ac - 1, 0)) + 1  # 2 (R + C) + 1 bytes always suffice
        res = (AlignDbResult * max(n, 1))()
        pinfo = (AlignBatchBandExtPair * max(n, 1))()
        info = AlignBatchBandExtInfo()
        ms = ctypes.c_float(0.0)
        need = ctypes.c_int64(0)
        buf = ctypes.create_string_buffer(max(cap, 1))
        st = lib().gsa_align_batch_band_ext_dev(self._h, n, arr, subst_ptr, substsz, gapo,
                                                gapo if gape is None else gape, lo, hi, int(waves), int(max_workgroups),
                                                int(scratch_limit), res, buf, cap, ctypes.byref(need), pinfo,
                                                ctypes.byref(info), ctypes.byref(ms), stream)
        self._check(st, "gsa_align_batch_band_ext_dev")
        d = {k: (float(getattr(info, k)) if t is ctypes.c_float else int(getattr(info, k)))
             for k, t in info._fields_ if not k.startswith("pad")}
        d["pairs"] = [{k: int(getattr(q, k)) for k, _ in q._fields_} for q in pinfo[:n]]
        self._align_batch_band_ext_info = d
        raw = buf.raw
        return [{"score": int(r.score), "status": int(r.status), "i_start": int(r.i_start), "j_start": int(r.j_start),
                 "i_end": int(r.i_end), "j_end": int(r.j_end),
                 "cigar": raw[r.cigar_off:r.cigar_off + r.cigar_len].decode() if r.status == 0 else "",
                 "kernel_ms": float(ms.value)} for r in res[:n]]

    def last_align_batch_band_ext_info(self) -> dict:
        """gsa_align_batch_band_ext_info of the last align_batch_band_ext_dev call on this engine:
        last_align_batch_band_info()'s keys with "rows_used" and "cols_used" (summed over the pairs that
        ran on the device); "pairs" lists the pairs' own values, with their "rows_used" and "cols_used"."""
        info = getattr(self, "_align_batch_band_ext_info", None)
        if info is None:
            raise NwError(NwStat.errorInvalidValue, "last_align_batch_band_ext_info: no align_batch_band_ext_dev call yet")
        d = dict(info)
        d["pairs"] = [dict(q) for q in info["pairs"]]
        return d

    def align_batch_band_ext(self, pairs, subst, gapo: int, gape: Optional[int] = None, scratch_limit: int = 0, *,
                             bands=None, band: Optional[int] = None, waves: int = 0, max_workgroups: int = 0) -> list:
        """align_batch_band_ext_dev over host arrays, with the pairs and the bands as
        score_band_ext_batch() takes them."""
        bl = self._bands_ext_of(pairs, bands, band)
        ptrs, dS, substsz, keep = self._upload_pairs(pairs, subst)
        return self.align_batch_band_ext_dev(ptrs, dS, substsz, gapo, gape, max_workgroups, scratch_limit, bands=bl,
                                             waves=waves)

    # -- long pairs, overlap (dovetail): scores and alignments of a batch in one call --

    def score_overlap_batch_dev(self, pairs, subst_ptr: int, substsz: int, gapo: int, gape: Optional[int] = None,
                                stream: Optional[int] = None) -> list:
        """Overlap scores of many device-resident pairs in one launch (gsa_score_overlap_batch_dev;
        synchronous).  `pairs`: sequence of (seqY_ptr, adjrows, seqX_ptr, adjcols), as
        score_semi_batch_dev takes it.  One dict per pair, in order, equal to score_overlap_dev's for
        that pair alone except "kernel_ms", which is the hipEvent time of the whole call's kernels in
        every dict."""
        n = len(pairs)
        arr = (PairDev * max(n, 1))()
        for k, (yp, ar, xp, ac) in enumerate(pairs):
            arr[k].seqY, arr[k].adjrows, arr[k].seqX, arr[k].adjcols = yp, ar, xp, ac
        res = (ScoreResult * max(n, 1))()
        ms = ctypes.c_float(0.0)
        st = lib().gsa_score_overlap_batch_dev(self._h, n, arr, subst_ptr, substsz, gapo, gapo if gape is None else gape,
                                               res, ctypes.byref(ms), stream)
        self._check(st, "gsa_score_overlap_batch_dev")
        return [{"score": int(r.score), "i_end": int(r.i_end), "j_end": int(r.j_end), "kernel_ms": float(ms.value)}
                for r in res[:n]]

    def score_overlap_batch(self, pairs, subst, gapo: int, gape: Optional[int] = None) -> list:
        """score_overlap_batch_dev over host arrays: `pairs` is a sequence of (seqY, seqX) with the header
        element in front, as score_batch() takes them; sequences and table are uploaded through torch."""
        ptrs, dS, substsz, keep = self._upload_pairs(pairs, subst)
        return self.score_overlap_batch_dev(ptrs, dS, substsz, gapo, gape)

    def align_batch_overlap_dev(self, pairs, subst_ptr: int, substsz: int, gapo: int, gape: Optional[int] = None,
                                max_workgroups: int = 0, scratch_limit: int = 0, stream: Optional[int] = None) -> list:
        """The overlap alignments of many device-resident long pairs, traced on the device together
        (gsa_align_batch_overlap_dev; synchronous).  `pairs` as score_overlap_batch_dev takes it.  One
        dict per pair, in order, with align_pair_overlap_dev's keys and, "kernel_ms" apart (the hipEvent
        time of the whole call's kernels in every dict), its values for that pair alone; "status" 1: one
        strip of the pair's codes exceeds `scratch_limit` (score and end cell only).  `max_workgroups`
        caps the grids of the fill and of the walk (0: all resident), `scratch_limit` the bytes of move
        codes held at once (0: the default, 8 GiB).  last_align_batch_overlap_info() says what ran."""
        n = len(pairs)
        arr = (PairDev * max(n, 1))()
        cap = 0
        for k, (yp, ar, xp, ac) in enumerate(pairs):
            arr[k].seqY, arr[k].adjrows, arr[k].seqX, arr[k].adjcols = yp, ar, xp, ac
            cap += 2 * (max(ar - 1, 0) + max(ac - 1, 0)) + 1  # 2 (R + C) + 1 bytes always suffice
        res = (AlignDbResult * max(n, 1))()
        info = AlignBatchOverlapInfo()
        ms = ctypes.c_float(0.0)
        need = ctypes.c_int64(0)
        buf = ctypes.create_string_buffer(max(cap, 1))
        st = lib().gsa_align_batch_overlap_dev(self._h, n, arr, subst_ptr, substsz, gapo, gapo if gape is None else gape,
                                               int(max_workgroups), int(scratch_limit), res, buf, cap, ctypes.byref(need),
                                               ctypes.byref(info), ctypes.byref(ms), stream)
        self._check(st, "gsa_align_batch_overlap_dev")
        self._align_batch_overlap_info = {k: (float(getattr(info, k)) if t is ctypes.c_float else int(getattr(info, k)))
                                          for k, t in info._fields_ if not k.startswith("pad")}
        raw = buf.raw
        return [{"score": int(r.score), "status": int(r.status), "i_start": int(r.i_start), "j_start": int(r.j_start),
                 "i_end": int(r.i_end), "j_end": int(r.j_end),
                 "cigar": raw[r.cigar_off:r.cigar_off + r.cigar_len].decode() if r.status == 0 else "",
                 "kernel_ms": float(ms.value)} for r in res[:n]]

    def last_align_batch_overlap_info(self) -> dict:
        """gsa_align_batch_overlap_info of the last align_batch_overlap_dev call on this engine:
        "batch_pairs" (traced on the device), "host_pairs", "strip_rows", "strips" (those of the rows
        1 ... i_end, over the traced pairs), "strips_filled", "rounds" (fill + walk launch pairs),
        "code_bytes" (peak bytes of move codes held at once), "gran_bytes" (checkpoint rows the score
        launch kept), "score_ms", "fill_ms" and "walk_ms"."""
        info = getattr(self, "_align_batch_overlap_info", None)
        if info is None:
            raise NwError(NwStat.errorInvalidValue, "last_align_batch_overlap_info: no align_batch_overlap_dev call yet")
        return dict(info)

    def align_batch_overlap(self, pairs, subst, gapo: int, gape: Optional[int] = None, scratch_limit: int = 0) -> list:
        """align_batch_overlap_dev over host arrays: `pairs` is a sequence of (seqY, seqX) with the header
        element in front, as score_batch() takes them; sequences and table are uploaded through torch."""
        ptrs, dS, substsz, keep = self._upload_pairs(pairs, subst)
        return self.align_batch_overlap_dev(ptrs, dS, substsz, gapo, gape, 0, scratch_limit)

    # -- many queries against one database in one call ----------------------

    def score_db_multi_dev(self, queries_ptr: int, q_off, db_ptr: int, db_off, subst_ptr: int, substsz: int,
                           gapo: int, gape: Optional[int] = None, local: bool = False, top: int = 0,
                           want_scores: bool = True, max_workgroups: int = 0, scratch_limit: int = 0,
                           stream: Optional[int] = None) -> dict:
        """Many queries against a database (gsa_score_db_multi_dev; synchronous): the queries in one
        device buffer `queries_ptr` with host offsets `q_off`, as `db_ptr` and `db_off` hold the
        subjects.  {"scores": int32 array [nq, nsubj] (None unless want_scores), "hits": structured
        array [nq, min(top, nsubj)] of (subject, score, i_end, j_end), every query's best subjects by
        (score descending, subject ascending), ranked on the device (None when top is 0),
        "kernel_ms"}.  Every pair's result is score_db_dev's for that query and subject.
        `max_workgroups` caps the lane kernel's grid (0: all resident), `scratch_limit` the bytes of
        results held on the device at once (0: the default).  last_score_db_multi_info() says what ran."""
        res, self._score_db_multi_info = self._score_db_many(
            "gsa_score_db_multi_dev", queries_ptr, q_off, db_ptr, db_off, subst_ptr, substsz, gapo, gape, (int(local),),
            top, want_scores, max_workgroups, scratch_limit, stream)
        return res

    def _score_db_many(self, entry: str, queries_ptr, q_off, db_ptr, db_off, subst_ptr, substsz, gapo, gape, mode: tuple,
                       top, want_scores, max_workgroups, scratch_limit, stream):
        """The call behind score_db_multi_dev (mode = (local,)), score_db_semi_dev and score_db_overlap_dev (mode = ()):
        (result dict, info dict)."""
        qo = np.ascontiguousarray(q_off, dtype=np.int64)
        off = np.ascontiguousarray(db_off, dtype=np.int64)
        nq, n = len(qo) - 1, len(off) - 1
        top = int(top)
        ntop = min(top, n) if top > 0 else 0
        scores = np.empty((max(nq, 0), max(n, 0)), dtype=np.int32) if want_scores else None
        hits = np.zeros((max(nq, 0), max(ntop, 0)), dtype=DB_HIT_DTYPE) if top > 0 else None
        info = ScoreDbMultiInfo()
        ms = ctypes.c_float(0.0)
        i64p = ctypes.POINTER(_i64)
        st = getattr(lib(), entry)(
            self._h, queries_ptr, qo.ctypes.data_as(i64p), nq, db_ptr, off.ctypes.data_as(i64p), n, subst_ptr, substsz,
            gapo, gapo if gape is None else gape, *mode, top, int(max_workgroups), int(scratch_limit),
            scores.ctypes.data_as(_i32p) if scores is not None else None,
            hits.ctypes.data_as(ctypes.POINTER(DbHit)) if hits is not None else None, ctypes.byref(info),
            ctypes.byref(ms), stream)
        self._check(st, entry)
        what = {k: (float(getattr(info, k)) if t is ctypes.c_float else int(getattr(info, k))) for k, t in info._fields_}
        return {"scores": scores, "hits": hits, "kernel_ms": float(ms.value)}, what

    def last_score_db_multi_info(self) -> dict:
        """gsa_score_db_multi_info of the last score_db_multi_dev call on this engine: "lane_queries",
        "other_queries", "launches", "workgroups", "lane_pairs", "units", "profile_builds",
        "result_bytes", "lanes_ms", "select_ms"."""
        info = getattr(self, "_score_db_multi_info", None)
        if info is None:
            raise NwError(NwStat.errorInvalidValue, "last_score_db_multi_info: no score_db_multi_dev call yet")
        return dict(info)

    def score_db_multi(self, queries, subjects, subst, gapo: int, gape: Optional[int] = None, local: bool = False,
                       top: int = 0) -> dict:
        """score_db_multi_dev over host arrays: every entry of `queries` and of `subjects` with the
        header element in front, as score_db takes them."""
        dQ, qoff, dD, off, dS, substsz = self._pack_db_multi(queries, subjects, subst)
        return self.score_db_multi_dev(dQ.data_ptr(), qoff, dD.data_ptr(), off, dS.data_ptr(), substsz, gapo, gape,
                                       local, top)

    # -- the alignments of many queries' hits in one call -------------------

    def align_db_multi_dev(self, queries_ptr: int, q_off, db_ptr: int, db_off, hit_query, hit_subject, subst_ptr: int,
                           substsz: int, gapo: int, gape: Optional[int] = None, local: bool = False,
                           max_workgroups: int = 0, scratch_limit: int = 0, stream: Optional[int] = None) -> list:
        """The alignments of chosen (query, subject) pairs (gsa_align_db_multi_dev; synchronous):
        queries, database and table as score_db_multi_dev takes them, `hit_query` and `hit_subject`
        the pairs' indices (any order, repeats allowed).  One dict per pair, in order, equal to
        align_db_dev's for that query and subject: {"score", "status", "i_start", "j_start", "i_end",
        "j_end", "cigar", "kernel_ms"}.  `max_workgroups` caps the fill's grid (0: all resident),
        `scratch_limit` the bytes of move codes held at once (0: the default).
        last_align_db_multi_info() says what the call ran."""
        res, self._align_db_multi_info = self._align_db_many(
            "gsa_align_db_multi_dev", queries_ptr, q_off, db_ptr, db_off, hit_query, hit_subject, subst_ptr, substsz, gapo,
            gape, (int(local),), max_workgroups, scratch_limit, stream)
        return res

    def _align_db_many(self, entry: str, queries_ptr, q_off, db_ptr, db_off, hit_query, hit_subject, subst_ptr, substsz,
                       gapo, gape, mode: tuple, max_workgroups, scratch_limit, stream):
        """The call behind align_db_multi_dev (mode = (local,)), align_db_semi_dev and align_db_overlap_dev (mode = ()):
        (list of result dicts, info dict)."""
        qo = np.ascontiguousarray(q_off, dtype=np.int64)
        off = np.ascontiguousarray(db_off, dtype=np.int64)
        hq = np.ascontiguousarray(hit_query, dtype=np.int32).ravel()
        hs = np.ascontiguousarray(hit_subject, dtype=np.int32).ravel()
        if len(hq) != len(hs):
            raise NwError(NwStat.errorInvalidValue, entry + ": hit_query and hit_subject differ in length")
        nq, n, nh = len(qo) - 1, len(off) - 1, len(hq)
        res = (AlignDbResult * max(nh, 1))()
        info = AlignDbMultiInfo()
        ms = ctypes.c_float(0.0)
        need = ctypes.c_int64(0)
        # 2 (R + C) + 1 bytes per hit always suffice
        cap = 0
        if nh and n >= 1 and nq >= 1 and hs.min() >= 0 and hs.max() < n and hq.min() >= 0 and hq.max() < nq:
            cap = int(2 * (np.diff(off)[hs].clip(1) - 1 + np.diff(qo)[hq].clip(1) - 1).sum() + nh)
        buf = ctypes.create_string_buffer(max(cap, 1))
        i64p = ctypes.POINTER(_i64)
        st = getattr(lib(), entry)(
            self._h, queries_ptr, qo.ctypes.data_as(i64p), nq, db_ptr, off.ctypes.data_as(i64p), n,
            hq.ctypes.data_as(_i32p), hs.ctypes.data_as(_i32p), nh, subst_ptr, substsz, gapo,
            gapo if gape is None else gape, *mode, int(max_workgroups), int(scratch_limit), res, buf, cap,
            ctypes.byref(need), ctypes.byref(info), ctypes.byref(ms), stream)
        self._check(st, entry)
        what = {k: (float(getattr(info, k)) if t is ctypes.c_float else int(getattr(info, k))) for k, t in info._fields_}
        raw = buf.raw
        out = []
        for r in res[:nh]:
            cig = raw[r.cigar_off:r.cigar_off + r.cigar_len].decode() if r.status == 0 else ""
            out.append({"score": int(r.score), "status": int(r.status), "i_start": int(r.i_start),
                        "j_start": int(r.j_start), "i_end": int(r.i_end), "j_end": int(r.j_end), "cigar": cig,
                        "kernel_ms": float(ms.value)})
        return out, what

    def last_align_db_multi_info(self) -> dict:
        """gsa_align_db_multi_info of the last align_db_multi_dev call on this engine: "lane_hits",
        "unsupported", "chunks", "launches", "workgroups", "lane_queries", "tasks", "units",
        "profile_builds", "code_bytes", "fill_ms", "walk_ms"."""
        info = getattr(self, "_align_db_multi_info", None)
        if info is None:
            raise NwError(NwStat.errorInvalidValue, "last_align_db_multi_info: no align_db_multi_dev call yet")
        return dict(info)

    def _pack_db_multi(self, queries, subjects, subst):
        """Queries, subjects and table on the device, uploaded once: (dQ, qoff, dD, off, dS, substsz)."""
        import torch
        dev = torch.device("cuda", self.device)
        up = lambda a: torch.from_numpy(_c32(a)).to(dev)
        subst = _c32(subst)
        substsz = int(round(np.sqrt(subst.size)))

        def pack(seqs):
            seqs = [_c32(x) for x in seqs]
            off = np.zeros(len(seqs) + 1, dtype=np.int64)
            if seqs:
                off[1:] = np.cumsum([len(x) for x in seqs])
            return up(np.concatenate(seqs) if seqs else np.zeros(1, np.int32)), off

        dS = up(subst.ravel())
        (dQ, qoff), (dD, off) = pack(queries), pack(subjects)
        torch.cuda.synchronize(dev)
        return dQ, qoff, dD, off, dS, substsz

    def align_db_multi(self, queries, subjects, hit_query, hit_subject, subst, gapo: int, gape: Optional[int] = None,
                       local: bool = False) -> list:
        """align_db_multi_dev over host arrays: every entry of `queries` and of `subjects` with the
        header element in front; `hit_query` indexes `queries`, `hit_subject` indexes `subjects`."""
        dQ, qoff, dD, off, dS, substsz = self._pack_db_multi(queries, subjects, subst)
        return self.align_db_multi_dev(dQ.data_ptr(), qoff, dD.data_ptr(), off, hit_query, hit_subject, dS.data_ptr(),
                                       substsz, gapo, gape, local)

    def search_db_multi(self, queries, subjects, subst, gapo: int, gape: Optional[int] = None, local: bool = False,
                        top: int = 10) -> list:
        """Database search with alignments for many queries: queries, subjects and table are uploaded
        once, then one score_db_multi_dev with `top` and one align_db_multi_dev on all the hits.  Per
        query [(subject_index, result dict)], equal to [search_db(q, ...) for q in queries]."""
        if max(int(top), 0) == 0:
            return [[] for _ in queries]
        dQ, qoff, dD, off, dS, substsz = self._pack_db_multi(queries, subjects, subst)
        hits = self.score_db_multi_dev(dQ.data_ptr(), qoff, dD.data_ptr(), off, dS.data_ptr(), substsz, gapo, gape,
                                       local, top, want_scores=False)["hits"]
        hq = np.repeat(np.arange(hits.shape[0], dtype=np.int32), hits.shape[1])
        hs = np.ascontiguousarray(hits["subject"], dtype=np.int32).ravel()
        res = self.align_db_multi_dev(dQ.data_ptr(), qoff, dD.data_ptr(), off, hq, hs, dS.data_ptr(), substsz, gapo,
                                      gape, local)
        ntop = hits.shape[1]
        return [list(zip([int(x) for x in hs[q * ntop:(q + 1) * ntop]], res[q * ntop:(q + 1) * ntop]))
                for q in range(hits.shape[0])]

    # -- semi-global database search: the whole query within each subject --

    def score_db_semi_dev(self, queries_ptr: int, q_off, db_ptr: int, db_off, subst_ptr: int, substsz: int,
                          gapo: int, gape: Optional[int] = None, top: int = 0, want_scores: bool = True,
                          max_workgroups: int = 0, scratch_limit: int = 0, stream: Optional[int] = None) -> dict:
        """Many queries against a database in the semi-global shape (gsa_score_db_multi_semi_dev;
        synchronous): every query letter aligned, the subject's head and tail free.  Arguments and
        result as score_db_multi_dev's without `local`; a hit's (i_end, j_end) is (R, the smallest
        column of row R that attains the score), and scores may be negative.  The mode has no second
        path: a pair the lane kernels cannot take makes the call errorInvalidValue (include/gsa.h).
        last_score_db_semi_info() says what ran."""
        res, self._score_db_semi_info = self._score_db_many(
            "gsa_score_db_multi_semi_dev", queries_ptr, q_off, db_ptr, db_off, subst_ptr, substsz, gapo, gape, (), top,
            want_scores, max_workgroups, scratch_limit, stream)
        return res

    def last_score_db_semi_info(self) -> dict:
        """gsa_score_db_multi_info of the last score_db_semi_dev call on this engine (the keys of
        last_score_db_multi_info(); "other_queries" is 0)."""
        info = getattr(self, "_score_db_semi_info", None)
        if info is None:
            raise NwError(NwStat.errorInvalidValue, "last_score_db_semi_info: no score_db_semi_dev call yet")
        return dict(info)

    def score_db_semi(self, queries, subjects, subst, gapo: int, gape: Optional[int] = None, top: int = 0) -> dict:
        """score_db_semi_dev over host arrays: every entry of `queries` and of `subjects` with the
        header element in front, as score_db_multi takes them."""
        dQ, qoff, dD, off, dS, substsz = self._pack_db_multi(queries, subjects, subst)
        return self.score_db_semi_dev(dQ.data_ptr(), qoff, dD.data_ptr(), off, dS.data_ptr(), substsz, gapo, gape, top)

    def align_db_semi_dev(self, queries_ptr: int, q_off, db_ptr: int, db_off, hit_query, hit_subject, subst_ptr: int,
                          substsz: int, gapo: int, gape: Optional[int] = None, max_workgroups: int = 0,
                          scratch_limit: int = 0, stream: Optional[int] = None) -> list:
        """The semi-global alignments of chosen (query, subject) pairs (gsa_align_db_multi_semi_dev;
        synchronous): arguments and result dicts as align_db_multi_dev's without `local`.  Score and
        end cell are score_db_semi_dev's; the walk stops in row 0, so "i_start" is 0, "j_start" the
        column where the query begins in the subject, and the CIGAR covers the query alone.  Status
        is never 1: what the kernels cannot take makes the call errorInvalidValue.
        last_align_db_semi_info() says what the call ran."""
        res, self._align_db_semi_info = self._align_db_many(
            "gsa_align_db_multi_semi_dev", queries_ptr, q_off, db_ptr, db_off, hit_query, hit_subject, subst_ptr, substsz,
            gapo, gape, (), max_workgroups, scratch_limit, stream)
        return res

    def last_align_db_semi_info(self) -> dict:
        """gsa_align_db_multi_info of the last align_db_semi_dev call on this engine (the keys of
        last_align_db_multi_info(); "unsupported" is 0)."""
        info = getattr(self, "_align_db_semi_info", None)
        if info is None:
            raise NwError(NwStat.errorInvalidValue, "last_align_db_semi_info: no align_db_semi_dev call yet")
        return dict(info)

    def align_db_semi(self, queries, subjects, hit_query, hit_subject, subst, gapo: int,
                      gape: Optional[int] = None) -> list:
        """align_db_semi_dev over host arrays: every entry of `queries` and of `subjects` with the
        header element in front; `hit_query` indexes `queries`, `hit_subject` indexes `subjects`."""
        dQ, qoff, dD, off, dS, substsz = self._pack_db_multi(queries, subjects, subst)
        return self.align_db_semi_dev(dQ.data_ptr(), qoff, dD.data_ptr(), off, hit_query, hit_subject, dS.data_ptr(),
                                      substsz, gapo, gape)

    def search_db_semi(self, queries, subjects, subst, gapo: int, gape: Optional[int] = None, top: int = 10) -> list:
        """Semi-global database search with alignments for many queries: one upload, one
        score_db_semi_dev with `top` and one align_db_semi_dev on all the hits.  Per query
        [(subject_index, result dict)], best subject first."""
        if max(int(top), 0) == 0:
            return [[] for _ in queries]
        dQ, qoff, dD, off, dS, substsz = self._pack_db_multi(queries, subjects, subst)
        hits = self.score_db_semi_dev(dQ.data_ptr(), qoff, dD.data_ptr(), off, dS.data_ptr(), substsz, gapo, gape, top,
                                      want_scores=False)["hits"]
        hq = np.repeat(np.arange(hits.shape[0], dtype=np.int32), hits.shape[1])
        hs = np.ascontiguousarray(hits["subject"], dtype=np.int32).ravel()
        res = self.align_db_semi_dev(dQ.data_ptr(), qoff, dD.data_ptr(), off, hq, hs, dS.data_ptr(), substsz, gapo, gape)
        ntop = hits.shape[1]
        return [list(zip([int(x) for x in hs[q * ntop:(q + 1) * ntop]], res[q * ntop:(q + 1) * ntop]))
                for q in range(hits.shape[0])]

    # -- overlap (dovetail) database search: all four overhangs free ------

    def score_db_overlap_dev(self, queries_ptr: int, q_off, db_ptr: int, db_off, subst_ptr: int, substsz: int,
                             gapo: int, gape: Optional[int] = None, top: int = 0, want_scores: bool = True,
                             max_workgroups: int = 0, scratch_limit: int = 0, stream: Optional[int] = None) -> dict:
        """Many queries against a database in the overlap (dovetail) shape
        (gsa_score_db_multi_overlap_dev; synchronous): a suffix of either sequence on a prefix of the
        other, or either within the other.  Arguments and result as score_db_semi_dev's; a hit's
        (i_end, j_end) is (R, the smallest column of row R that attains the score) if row R attains
        it, else (the smallest such row, C), and scores are never negative.  The mode has no second
        path: a pair the lane kernels cannot take makes the call errorInvalidValue (include/gsa.h).
        last_score_db_overlap_info() says what ran."""
        res, self._score_db_overlap_info = self._score_db_many(
            "gsa_score_db_multi_overlap_dev", queries_ptr, q_off, db_ptr, db_off, subst_ptr, substsz, gapo, gape, (), top,
            want_scores, max_workgroups, scratch_limit, stream)
        return res

    def last_score_db_overlap_info(self) -> dict:
        """gsa_score_db_multi_info of the last score_db_overlap_dev call on this engine (the keys of
        last_score_db_multi_info(); "other_queries" is 0)."""
        info = getattr(self, "_score_db_overlap_info", None)
        if info is None:
            raise NwError(NwStat.errorInvalidValue, "last_score_db_overlap_info: no score_db_overlap_dev call yet")
        return dict(info)

    def score_db_overlap(self, queries, subjects, subst, gapo: int, gape: Optional[int] = None, top: int = 0) -> dict:
        """score_db_overlap_dev over host arrays: every entry of `queries` and of `subjects` with the
        header element in front, as score_db_multi takes them."""
        dQ, qoff, dD, off, dS, substsz = self._pack_db_multi(queries, subjects, subst)
        return self.score_db_overlap_dev(dQ.data_ptr(), qoff, dD.data_ptr(), off, dS.data_ptr(), substsz, gapo, gape, top)

    def align_db_overlap_dev(self, queries_ptr: int, q_off, db_ptr: int, db_off, hit_query, hit_subject, subst_ptr: int,
                             substsz: int, gapo: int, gape: Optional[int] = None, max_workgroups: int = 0,
                             scratch_limit: int = 0, stream: Optional[int] = None) -> list:
        """The overlap alignments of chosen (query, subject) pairs (gsa_align_db_multi_overlap_dev;
        synchronous): arguments and result dicts as align_db_semi_dev's.  Score and end cell are
        score_db_overlap_dev's; the walk stops on row 0 or column 0, so one of "i_start" and
        "j_start" is 0 and the CIGAR covers the overlap alone.  Status is never 1: what the kernels
        cannot take makes the call errorInvalidValue.  last_align_db_overlap_info() says what the
        call ran."""
        res, self._align_db_overlap_info = self._align_db_many(
            "gsa_align_db_multi_overlap_dev", queries_ptr, q_off, db_ptr, db_off, hit_query, hit_subject, subst_ptr,
            substsz, gapo, gape, (), max_workgroups, scratch_limit, stream)
        return res

    def last_align_db_overlap_info(self) -> dict:
        """gsa_align_db_multi_info of the last align_db_overlap_dev call on this engine (the keys of
        last_align_db_multi_info(); "unsupported" is 0)."""
        info = getattr(self, "_align_db_overlap_info", None)
        if info is None:
            raise NwError(NwStat.errorInvalidValue, "last_align_db_overlap_info: no align_db_overlap_dev call yet")
        return dict(info)

    def align_db_overlap(self, queries, subjects, hit_query, hit_subject, subst, gapo: int,
                         gape: Optional[int] = None) -> list:
        """align_db_overlap_dev over host arrays: every entry of `queries` and of `subjects` with the
        header element in front; `hit_query` indexes `queries`, `hit_subject` indexes `subjects`."""
        dQ, qoff, dD, off, dS, substsz = self._pack_db_multi(queries, subjects, subst)
        return self.align_db_overlap_dev(dQ.data_ptr(), qoff, dD.data_ptr(), off, hit_query, hit_subject, dS.data_ptr(),
                                         substsz, gapo, gape)

    def search_db_overlap(self, queries, subjects, subst, gapo: int, gape: Optional[int] = None, top: int = 10) -> list:
        """Overlap database search with alignments for many queries: one upload, one
        score_db_overlap_dev with `top` and one align_db_overlap_dev on all the hits.  Per query
        [(subject_index, result dict)], best subject first."""
        if max(int(top), 0) == 0:
            return [[] for _ in queries]
        dQ, qoff, dD, off, dS, substsz = self._pack_db_multi(queries, subjects, subst)
        hits = self.score_db_overlap_dev(dQ.data_ptr(), qoff, dD.data_ptr(), off, dS.data_ptr(), substsz, gapo, gape, top,
                                         want_scores=False)["hits"]
        hq = np.repeat(np.arange(hits.shape[0], dtype=np.int32), hits.shape[1])
        hs = np.ascontiguousarray(hits["subject"], dtype=np.int32).ravel()
        res = self.align_db_overlap_dev(dQ.data_ptr(), qoff, dD.data_ptr(), off, hq, hs, dS.data_ptr(), substsz, gapo,
                                        gape)
        ntop = hits.shape[1]
        return [list(zip([int(x) for x in hs[q * ntop:(q + 1) * ntop]], res[q * ntop:(q + 1) * ntop]))
                for q in range(hits.shape[0])]

    # -- device-side verification ---------------------------------------

    def check_sparse_dev(self, seqY_ptr: int, adjrows: int, seqX_ptr: int, adjcols: int, subst_ptr: int,
                         substsz: int, gapo: int, geom: SparseGeom, hrow_ptr: int, hcol_ptr: int,
                         stream: Optional[int] = None) -> dict:
        """Every header value of a sparse fill against the recurrence (tile consistency);
        synchronous.  Returns {"checked", "mismatches", "first"}."""
        r = CheckResult()
        st = lib().gsa_check_sparse_dev(self._h, seqY_ptr, adjrows, seqX_ptr, adjcols, subst_ptr, substsz, gapo,
                                        ctypes.byref(geom), hrow_ptr, hcol_ptr, ctypes.byref(r), stream)
        self._check(st, "gsa_check_sparse_dev")
        return r.as_dict()

    def trace_sparse_dev(self, seqY_ptr: int, adjrows: int, seqX_ptr: int, adjcols: int, subst_ptr: int,
                         substsz: int, gapo: int, geom: SparseGeom, hrow_ptr: int, hcol_ptr: int,
                         stream: Optional[int] = None) -> Tuple[int, str, int]:
        """NwTrace2_Sparse on the device (headers stay in HBM): (trace_hash, edit string,
        align_cost), identical to trace_sparse()."""
        cap = 8 * (adjrows + adjcols) + 64  # run-length string: <= 2 chars per move, digits reversed
        buf = ctypes.create_string_buffer(cap)
        n = ctypes.c_int64(0)
        h = ctypes.c_uint32(0)
        cost = ctypes.c_int32(0)
        st = lib().gsa_trace_sparse_dev(self._h, seqY_ptr, adjrows, seqX_ptr, adjcols, subst_ptr, substsz, gapo,
                                        ctypes.byref(geom), hrow_ptr, hcol_ptr, buf, cap, ctypes.byref(n),
                                        ctypes.byref(h), ctypes.byref(cost), stream)
        self._check(st, "gsa_trace_sparse_dev")
        return int(h.value), buf.raw[:n.value].decode(), int(cost.value)

    def check_full_dev(self, seqY_ptr: int, adjrows: int, seqX_ptr: int, adjcols: int, subst_ptr: int,
                       substsz: int, gapo: int, score_ptr: int, stream: Optional[int] = None,
                       ld: Optional[int] = None) -> dict:
        """Every cell of a full matrix against its stored neighbours; synchronous.  ld: row pitch
        (None: unpadded)."""
        r = CheckResult()
        if ld is None:
            st = lib().gsa_check_full_dev(self._h, seqY_ptr, adjrows, seqX_ptr, adjcols, subst_ptr, substsz, gapo,
                                          score_ptr, ctypes.byref(r), stream)
        else:
            st = lib().gsa_check_full_pitched_dev(self._h, seqY_ptr, adjrows, seqX_ptr, adjcols, subst_ptr, substsz,
                                                  gapo, score_ptr, int(ld), ctypes.byref(r), stream)
        self._check(st, "gsa_check_full_dev" if ld is None else "gsa_check_full_pitched_dev")
        return r.as_dict()

    def hash_full_dev(self, score_ptr: int, adjrows: int, adjcols: int, ld: Optional[int] = None,
                      stream: Optional[int] = None) -> int:
        """NwHash1_Plain of a device-resident full matrix (gsa_hash_full_dev); equals hash_full()
        of its host copy."""
        h = ctypes.c_uint32(0)
        st = lib().gsa_hash_full_dev(self._h, score_ptr, adjrows, adjcols, adjcols if ld is None else int(ld),
                                     ctypes.byref(h), stream)
        self._check(st, "gsa_hash_full_dev")
        return int(h.value)

    def trace_full_dev(self, seqY_ptr: int, adjrows: int, seqX_ptr: int, adjcols: int, score_ptr: int,
                       ld: Optional[int] = None, stream: Optional[int] = None) -> Tuple[int, str, int]:
        """NwTrace1_Plain of a device-resident full matrix (gsa_trace_full_dev): (trace_hash, edit
        string, align_cost), equal to trace_full() of its host copy."""
        cap = 8 * (adjrows + adjcols) + 64
        buf = ctypes.create_string_buffer(cap)
        n = ctypes.c_int64(0)
        h = ctypes.c_uint32(0)
        cost = ctypes.c_int32(0)
        st = lib().gsa_trace_full_dev(self._h, seqY_ptr, adjrows, seqX_ptr, adjcols, score_ptr,
                                      adjcols if ld is None else int(ld), buf, cap, ctypes.byref(n), ctypes.byref(h),
                                      ctypes.byref(cost), stream)
        self._check(st, "gsa_trace_full_dev")
        return int(h.value), buf.raw[:n.value].decode(), int(cost.value)


# ---- host consumers (the reference's L4) ----------------------------------------------

def hash_full(score: np.ndarray) -> int:
    """NwHash1_Plain (src/nwtrace1_plain.cpp:133-154)."""
    score = _c32(score)
    return int(lib().gsa_hash_full(_p(score), score.shape[0], score.shape[1]))


def trace_full(score: np.ndarray, seqY, seqX) -> Tuple[int, str]:
    """NwTrace1_Plain (src/nwtrace1_plain.cpp:6-131) -> (trace_hash, edit_trace)."""
    score, seqY, seqX = _c32(score), _c32(seqY), _c32(seqX)
    cap = 8 * (len(seqY) + len(seqX)) + 64
    buf = ctypes.create_string_buffer(cap)
    n = ctypes.c_int64(0)
    h = ctypes.c_uint32(0)
    st = lib().gsa_trace_full(_p(score), _p(seqY), len(seqY), _p(seqX), len(seqX), buf, cap, ctypes.byref(n),
                              ctypes.byref(h))
    if st != NwStat.success:
        raise NwError(st, "gsa_trace_full")
    return int(h.value), buf.raw[:n.value].decode()


def trace_sparse(res: SparseResult, seqY, seqX, subst, gapo: int) -> Tuple[int, str, int]:
    """NwTrace2_Sparse (src/nwtrace2_sparse.cpp:102-257) -> (trace_hash, edit_trace, align_cost)."""
    seqY, seqX, subst = _c32(seqY), _c32(seqX), _c32(subst)
    substsz = int(round(np.sqrt(subst.size)))
    cap = 8 * (len(seqY) + len(seqX)) + 64
    buf = ctypes.create_string_buffer(cap)
    n = ctypes.c_int64(0)
    h = ctypes.c_uint32(0)
    cost = ctypes.c_int32(0)
    st = lib().gsa_trace_sparse(_p(_c32(res.hrow)), _p(_c32(res.hcol)), ctypes.byref(res.geom), _p(seqY), len(seqY),
                                _p(seqX), len(seqX), _p(subst), substsz, gapo, buf, cap, ctypes.byref(n),
                                ctypes.byref(h), ctypes.byref(cost))
    if st != NwStat.success:
        raise NwError(st, "gsa_trace_sparse")
    return int(h.value), buf.raw[:n.value].decode(), int(cost.value)


def hash_sparse(res: SparseResult, seqY, seqX, subst, gapo: int) -> int:
    """NwHash2_Sparse (src/nwtrace2_sparse.cpp:263-340)."""
    seqY, seqX, subst = _c32(seqY), _c32(seqX), _c32(subst)
    substsz = int(round(np.sqrt(subst.size)))
    return int(lib().gsa_hash_sparse(_p(_c32(res.hrow)), _p(_c32(res.hcol)), ctypes.byref(res.geom), _p(seqY),
                                     len(seqY), _p(seqX), len(seqX), _p(subst), substsz, gapo))


def sparse_align_cost(res: SparseResult, seqY, seqX, subst, gapo: int) -> int:
    seqY, seqX, subst = _c32(seqY), _c32(seqX), _c32(subst)
    substsz = int(round(np.sqrt(subst.size)))
    return int(lib().gsa_sparse_align_cost(_p(_c32(res.hrow)), _p(_c32(res.hcol)), ctypes.byref(res.geom),
                                           _p(seqY), len(seqY), _p(seqX), len(seqX), _p(subst), substsz, gapo))


# ---- the registry (src/nw_algorithm.hpp:8-42) --------------------------------------------

@dataclasses.dataclass
class NwResult:
    """The fields of NwAlgResult the driver verifies (src/benchmark.cpp:120-147)."""
    align_cost: int = 0
    score_hash: int = 0
    trace_hash: int = 0
    edit_trace: str = ""
    laps: dict = dataclasses.field(default_factory=dict)
    payload: object = None


@dataclasses.dataclass
class NwAlgorithm:
    name: str
    align: Callable
    trace: Callable
    hash: Callable
    params: Dict[str, list] = dataclasses.field(default_factory=dict)


def _align_plain(engine: Engine, seqY, seqX, subst, gapo, **_):
    r = engine.align_full(seqY, seqX, subst, gapo)
    return NwResult(align_cost=r.align_cost, laps=r.laps, payload=r)


def _align_mlsp(engine: Engine, seqY, seqX, subst, gapo, tileBx=256, **_):
    r = engine.align_sparse(seqY, seqX, subst, gapo, tileBx=tileBx)
    return NwResult(align_cost=r.align_cost, laps=r.laps, payload=r)


def _align_mlsppt(engine: Engine, seqY, seqX, subst, gapo, tileBx=256, **_):
    r = engine.align_sparse(seqY, seqX, subst, gapo, tileBx=tileBx, overlap=True)
    return NwResult(align_cost=r.align_cost, laps=r.laps, payload=r)


def _trace1(res: NwResult, seqY, seqX, subst, gapo):
    res.trace_hash, res.edit_trace = trace_full(res.payload.score, seqY, seqX)


def _hash1(res: NwResult, seqY, seqX, subst, gapo):
    res.score_hash = hash_full(res.payload.score)


def _trace2(res: NwResult, seqY, seqX, subst, gapo):
    res.trace_hash, res.edit_trace, _ = trace_sparse(res.payload, seqY, seqX, subst, gapo)


def _hash2(res: NwResult, seqY, seqX, subst, gapo):
    res.score_hash = hash_sparse(res.payload, seqY, seqX, subst, gapo)


def get_nw_algorithm_map() -> Dict[str, NwAlgorithm]:
    """getNwAlgorithmMap (src/nw_algorithm.cpp:48-69) for this engine.

    The reference's GPU family names resolve to the MI355X wavefront kernels: the
    full-matrix names (gpu3..gpu6) to the plain fill with Trace1/Hash1, the mlsp names
    (gpu7..gpu9) to the tile-header fill with Trace2/Hash2."""
    plain = ["NwAlign_Amd_Strip_Full", "NwAlign_Gpu3_Ml_DiagDiag", "NwAlign_Gpu4_Ml_DiagDiag2Pass",
             "NwAlign_Gpu5_Coop_DiagDiag", "NwAlign_Gpu6_Coop_DiagDiag2Pass"]
    mlsp = ["NwAlign_Amd_Strip_Mlsp", "NwAlign_Gpu7_Mlsp_DiagDiag", "NwAlign_Gpu8_Mlsp_DiagDiag",
            "NwAlign_Gpu9_Mlsp_DiagDiagDiag"]
    m = {n: NwAlgorithm(n, _align_plain, _trace1, _hash1) for n in plain}
    m.update({n: NwAlgorithm(n, _align_mlsp, _trace2, _hash2, {"tileBx": [256]}) for n in mlsp})
    # mlsppt (the reference's README.md:39 names it, never implemented): copy-back overlapped
    m["NwAlign_Amd_Strip_Mlsppt"] = NwAlgorithm("NwAlign_Amd_Strip_Mlsppt", _align_mlsppt, _trace2, _hash2,
                                                {"tileBx": [256]})
    return m
