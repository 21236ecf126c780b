// nw_pair_overlap_trace_batch_plan.h -- the overlap (dovetail) alignments of a batch of long pairs
// (gsa_align_batch_overlap_dev): how the pairs' strips are spread over rounds whose move
// codes fit the scratch limit.  No HIP here: tests/align_batch_overlap_plan_driver.cpp checks it on the CPU.
//
// It is nw_pair_semi_trace_batch_plan.h's rule over overlap_plan_chunk.  Every pair is cut as
// nw_pair_overlap_plan.h cuts one pair: strips of TR rows, taken bottom-up from the strip that holds its
// end row i_end -- the strips below it are never planned -- a later chunk only for the columns 1 ... j
// where the pair's walk left the chunk below.  A round has `limit` bytes.  The pairs that still have
// strips to fill are taken in a fixed order -- remaining code bytes descending, ties by index -- and each
// gets its next chunk by overlap_plan_chunk's rule against the bytes still free in the round: its lowest
// unfilled strip and as many above it as fit.  A pair for which nothing is left waits for the next
// round.  The first pair of a round has the whole limit, so, every strip fitting the limit alone, every
// round fills at least one strip.  After a round a pair whose walk stands on row 0 or on column 0 is
// done, and the strips above its chunk are never filled; any other walk stands on its chunk's upper
// boundary right of column 0 (overlap_walk_goes_on) and the pair goes on from there.  With one pair the
// rounds are overlap_plan_chunk's chunks.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "nw_pair_overlap_plan.h"

namespace gsa {

// Where a pair of the batch stands between rounds.  It starts at (overlap_end_strip(TR, i_end), j_end).
struct OverlapBatchPairState
{
    long long tHi;  // its lowest strip not yet filled; < 0: nothing left to fill
    long long J;    // the column its walk stands on: its next chunk needs 1 ... J
};

// A pair's chunk within a round.
struct OverlapBatchChunk
{
    int pair;           // index into the states
    PairChunk c;        // its strips, columns and bytes
    long long codeOff;  // bytes: the chunk's codes within the round's buffer
};

// code bytes a pair still needs if its walk never moves left of J and reaches row 0
inline long long overlap_batch_pair_remaining(long long TR, const OverlapBatchPairState& s)
{
    return (s.tHi < 0 || s.J < 1) ? 0 : (s.tHi + 1) * pair_strip_bytes(TR, s.J);
}

// One round: the chunks, in the order the pairs were taken, and the bytes they hold in all (0: no
// pair is active, or not even the first one's strip fits the limit).
inline long long overlap_batch_plan_round(long long TR, long long limit, const std::vector<OverlapBatchPairState>& st,
                                          std::vector<OverlapBatchChunk>* out)
{
    out->clear();
    std::vector<int> order;
    for (int p = 0; p < (int)st.size(); ++p)
        if (st[(size_t)p].tHi >= 0 && st[(size_t)p].J >= 1) order.push_back(p);
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) {
        return overlap_batch_pair_remaining(TR, st[(size_t)a]) > overlap_batch_pair_remaining(TR, st[(size_t)b]);
    });
    long long used = 0;
    for (int p : order)
    {
        OverlapBatchChunk b;
        b.pair = p;
        if (!overlap_plan_chunk(TR, st[(size_t)p].tHi, st[(size_t)p].J, limit - used, &b.c)) continue;
        b.codeOff = used;
        used += b.c.codeBytes;
        out->push_back(b);
    }
    return used;
}

// A pair's state after the round that ran chunk c, its walk standing on (i, j), `done` as the walk
// reported it.  On a free border the pair is finished, whatever strips lie above; otherwise the walk
// must stand on the chunk's upper boundary and goes on for the columns 1 ... j.  False: neither.
inline bool overlap_batch_advance(long long TR, const PairChunk& c, long long i, long long j, bool done, OverlapBatchPairState* s)
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
