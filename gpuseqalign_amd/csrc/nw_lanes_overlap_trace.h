// nw_lanes_overlap_trace.h -- database search, overlap (dovetail) alignments of many queries' hits in
// one call: the fill with move codes and the walk that stops on row 0 or column 0
// (nw_lanes_overlap_trace.hip); used by gsa_score.hip.  The launch arguments, the plan
// and the unit size are nw_lanes_trace_multi.h's; DbTraceMultiWalkArgs::local is not read.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nw_lanes_overlap.h"
#include "nw_lanes_trace_multi.h"

namespace gsa {

// workgroups of the fill resident at once for this sweep class
hipError_t dboverlap_trace_resident(int passes, int substsz, bool affine, int* wgs);
// a.out[hit] gets {score, i_end, j_end, 0}: the score kernel's result for the pair
hipError_t launch_dboverlap_trace_fill(const DbTraceMultiArgs& a, int grid, hipStream_t st);
// from (i_end, j_end) in state H until row 0 or column 0: (i_start, j_start) is where the walk stopped
hipError_t launch_dboverlap_trace_walk(const DbTraceMultiWalkArgs& a, hipStream_t st);

}  // namespace gsa
