// nw_pair_overlap_plan.h -- the overlap (dovetail) alignment of one long pair (gsa_align_pair_overlap_dev;
// DESIGN.md 2.2m): which strips hold the path and the chunks of strips whose move codes fit the scratch
// limit.  No HIP here: tests/align_pair_overlap_plan_driver.cpp checks it on the CPU.
//
// The end cell (i_end, j_end) lies on row R or on column C.  The path runs from it up and to the left and
// ends as soon as it stands on row 0 or on column 0, so it needs the rows 1 ... i_end over the columns
// 1 ... j_end only: the strips below i_end's are left alone, and the codes begin at column 1 (no column
// window here; the semi-global bound would carry over with R replaced by i_end).  The chunks are
// nw_pair_trace_plan.h's, bottom-up from i_end's strip, each for the columns up to the one where the
// walk left the chunk below.  When the walk reaches column 0 inside a chunk it is done, and the strips
// above that chunk are never filled.
#pragma once
#include <stdint.h>

#include "nw_pair_trace_plan.h"

namespace gsa {

// the strip that holds row iEnd >= 1: the first chunk's lowest strip
inline long long overlap_end_strip(long long TR, long long iEnd) { return pair_strips(TR, iEnd) - 1; }

// The chunk whose lowest strip is tHi, for the columns 1 ... J: pair_plan_chunk's, and false as well for
// a path that has no cell left (J < 1 or tHi < 0).
inline bool overlap_plan_chunk(long long TR, long long tHi, long long J, long long limit, PairChunk* c)
{
    return J >= 1 && tHi >= 0 && pair_plan_chunk(TR, tHi, J, limit, c);
}

// Whether the walk, standing on (i, j) after a chunk whose highest strip is tLo, goes on into another
// chunk: it stopped on the chunk's upper boundary, right of column 0 and below row 0.
inline bool overlap_walk_goes_on(long long TR, const PairChunk& c, long long i, long long j)
{
    return c.tLo > 0 && i == pair_chunk_stop_row(TR, c) && j >= 1;
}

}  // namespace gsa
