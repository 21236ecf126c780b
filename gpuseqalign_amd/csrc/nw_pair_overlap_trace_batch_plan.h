// nw_pair_overlap_trace_batch_plan.h -- the overlap (dovetail) alignments of a batch of long pairs
// (gsa_align_batch_overlap_dev).  No HIP here: tests/align_batch_overlap_plan_driver.cpp
// checks it on the CPU.
//
// The rounds are nw_pair_trace_batch_plan.h's, without a window: a pair's state starts at
// (overlap_end_strip(TR, i_end), j_end) -- the strips below its end row's are never planned -- and its
// chunks are overlap_plan_chunk's over the columns 1 ... j.  What is the mode's own is how a pair goes on
// after a round: a pair whose walk stands on row 0 or on column 0 is done, and the strips above its chunk
// are never filled; any other walk stands on its chunk's upper boundary right of column 0
// (overlap_walk_goes_on) and the pair goes on from there.
#pragma once
#include <stdint.h>

#include "nw_pair_overlap_plan.h"
#include "nw_pair_trace_batch_plan.h"

namespace gsa {

// A pair's state after the round that ran chunk c, its walk standing on (i, j), `done` as the walk
// reported it.  On a free border the pair is finished, whatever strips lie above; otherwise the walk
// must stand on the chunk's upper boundary and goes on for the columns 1 ... j.  False: neither.
inline bool overlap_batch_advance(long long TR, const PairChunk& c, long long i, long long j, bool done, BatchPairState* s)
{
    if (done)
    {
        if (i != 0 && j != 0) return false;
        s->tHi = -1;
        return true;
    }
    if (!overlap_walk_goes_on(TR, c, i, j)) return false;
    s->tHi = c.tLo - 1;
    s->J = j;
    return true;
}

}  // namespace gsa
