// nw_lanes_semi.h -- database search, score-only, semi-global: the whole query within each subject,
// the subject's unaligned head and tail free (nw_lanes_semi.hip); used by
// gsa_score.hip.  The launch arguments, the unit size and the LDS footprint are nw_lanes_multi.h's.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nw_lanes_multi.h"

namespace gsa {

// Every |H| of a pair the semi-global kernels take stays below this: the signed result key
// score * 2^13 + (8191 - j) and the trace fill's 4 v + tag both fit int32 with room to spare.
constexpr long long kDbSemiMaxValue = 1ll << 18;

// workgroups resident at once for this sweep class
hipError_t dbsemi_resident(int passes, int substsz, bool affine, int* wgs);
// One persistent launch over the queries of one sweep class; a.out[row * ld + subject] gets
// {score, R, j_end, 0}, j_end the smallest column of row R that attains the score.
hipError_t launch_dbsemi(const DbMultiArgs& a, int grid, hipStream_t st);

}  // namespace gsa
