// nw_lanes_overlap.h -- database search, score-only, overlap (dovetail): a suffix of either sequence on
// a prefix of the other, or either within the other; all four overhangs free (nw_lanes_overlap.hip;
// DESIGN.md 2.2o); used by gsa_score.hip.  The launch arguments, the unit size and the LDS footprint
// are nw_lanes_multi.h's; the value bound is nw_lanes_semi.h's kDbSemiMaxValue.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nw_lanes_multi.h"
#include "nw_lanes_semi.h"

namespace gsa {

// A query the overlap kernels take has at most this many letters: the end cell's row travels in a
// key beside the value, H * 2^13 + (8191 - i), as the column does.
constexpr int kDbOverlapMaxR = kDbLanesMaxC;

// workgroups resident at once for this sweep class
hipError_t dboverlap_resident(int passes, int substsz, bool affine, int* wgs);
// One persistent launch over the queries of one sweep class; a.out[row * ld + subject] gets
// {score, i_end, j_end, 0}: (R, smallest j) if row R attains the score, else (smallest i, C).
hipError_t launch_dboverlap(const DbMultiArgs& a, int grid, hipStream_t st);

}  // namespace gsa
