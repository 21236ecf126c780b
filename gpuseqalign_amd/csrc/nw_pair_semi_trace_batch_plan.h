// nw_pair_semi_trace_batch_plan.h -- the semi-global alignments of a batch of long pairs
// (gsa_align_batch_semi_dev): how the pairs' strips are spread over rounds whose move
// codes fit the scratch limit.  No HIP here: tests/align_batch_semi_plan_driver.cpp checks it on the CPU.
//
// It is nw_pair_trace_batch_plan.h's rule over window widths.  Every pair is cut as
// nw_pair_semi_plan.h cuts one pair: strips of TR rows up to row R, taken bottom-up to strip 0 (a
// semi-global path always reaches row 0), a later chunk only for the columns jW + 1 ... j where the
// pair's walk left the chunk below, jW the pair's own window (semi_window on its score and end column).
// A round has `limit` bytes.  The pairs that still have strips to fill are taken in a fixed order --
// remaining code bytes descending, ties by index -- and each gets its next chunk by semi_plan_chunk's
// rule against the bytes still free in the round: its lowest unfilled strip and as many above it as
// fit.  A pair for which nothing is left waits for the next round.  The first pair of a round has the
// whole limit, so, every strip fitting the limit alone, every round fills at least one strip.  With
// one pair the rounds are semi_plan_chunk's chunks.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "nw_pair_semi_plan.h"

namespace gsa {

// Where a pair of the batch stands between rounds.
struct SemiBatchPairState
{
    long long tHi;  // its lowest strip not yet filled; < 0: nothing left to fill
    long long J;    // the column its walk stands on: its next chunk needs jW + 1 ... J
    long long jW;   // its window
};

// A pair's chunk within a round.
struct SemiBatchChunk
{
    int pair;           // index into the states
    PairChunk c;        // its strips, width (PairChunk::J = J - jW) and bytes
    long long codeOff;  // bytes: the chunk's codes within the round's buffer
};

// code bytes a pair still needs if its walk never moves left of J
inline long long semi_batch_pair_remaining(long long TR, const SemiBatchPairState& s)
{
    return (s.tHi < 0 || s.J <= s.jW) ? 0 : (s.tHi + 1) * pair_strip_bytes(TR, s.J - s.jW);
}

// One round: the chunks, in the order the pairs were taken, and the bytes they hold in all (0: no
// pair is active, or not even the first one's strip fits the limit).
inline long long semi_batch_plan_round(long long TR, long long limit, const std::vector<SemiBatchPairState>& st,
                                       std::vector<SemiBatchChunk>* out)
{
    out->clear();
    std::vector<int> order;
    for (int p = 0; p < (int)st.size(); ++p)
        if (st[(size_t)p].tHi >= 0 && st[(size_t)p].J > st[(size_t)p].jW) order.push_back(p);
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) {
        return semi_batch_pair_remaining(TR, st[(size_t)a]) > semi_batch_pair_remaining(TR, st[(size_t)b]);
    });
    long long used = 0;
    for (int p : order)
    {
        SemiBatchChunk b;
        b.pair = p;
        if (!semi_plan_chunk(TR, st[(size_t)p].tHi, st[(size_t)p].J, st[(size_t)p].jW, limit - used, &b.c)) continue;
        b.codeOff = used;
        used += b.c.codeBytes;
        out->push_back(b);
    }
    return used;
}

}  // namespace gsa
