// nw_pair_semi_trace_batch_plan.h -- the semi-global alignments of a batch of long pairs
// (gsa_align_batch_semi_dev).  No HIP here: tests/align_batch_semi_plan_driver.cpp checks
// it on the CPU.
//
// The rounds are nw_pair_trace_batch_plan.h's: a pair's state starts at (pair_strips(TR, R) - 1, j_end)
// with jW its own window (semi_window on its score and end column), its strips are taken bottom-up to
// strip 0 (a semi-global path always reaches row 0), and its chunks are semi_plan_chunk's over the
// columns jW + 1 ... j.  What is the mode's own is how a pair goes on after a round.
#pragma once
#include <stdint.h>

#include "nw_pair_trace_batch_plan.h"

namespace gsa {

// A pair's state after the round that ran chunk c, its walk standing on (i, j), `done` as the walk
// reported it.  A finished walk stands in row 0; any other stands on the chunk's upper boundary inside
// the window and goes on for the columns jW + 1 ... j.  False: neither.
inline bool semi_batch_advance(long long TR, const PairChunk& c, long long i, long long j, bool done, BatchPairState* s)
{
    if (done)
    {
        if (i != 0) return false;
        s->tHi = -1;
        return true;
    }
    if (c.tLo < 1 || i != pair_chunk_stop_row(TR, c) || j <= s->jW) return false;
    s->tHi = c.tLo - 1;
    s->J = j;
    return true;
}

}  // namespace gsa
