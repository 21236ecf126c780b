// nw_pair_trace_batch_plan.h -- the alignments of a batch of long pairs (gsa_align_batch_dev,
// gsa_align_batch_semi_dev, gsa_align_batch_overlap_dev): how the pairs' strips are
// spread over rounds whose move codes fit the scratch limit.  No HIP here:
// tests/align_batch_plan_driver.cpp checks it on the CPU, and the semi-global and overlap drivers next
// to it check the same plan under their modes' walks.
//
// Every pair is cut as the single-pair plans cut one pair (nw_pair_trace_plan.h, nw_pair_semi_plan.h,
// nw_pair_overlap_plan.h): strips of TR rows, taken bottom-up from the strip of its walk's first row, a
// later chunk only for the columns jW + 1 ... j where the pair's walk left the chunk below, jW the
// pair's column window (0 in the global and overlap modes).  A round has `limit` bytes.  The pairs that
// still have strips to fill are taken in a fixed order -- remaining code bytes descending, ties by
// index -- and each gets its next chunk by semi_plan_chunk's rule against the bytes still free in the
// round: its lowest unfilled strip and as many above it as fit.  A pair for which nothing is left waits
// for the next round.  The first pair of a round has the whole limit, so, every strip fitting the limit
// alone, every round fills at least one strip.  With one pair the rounds are the single-pair plan's
// chunks.  After a round each mode's advance rule (pair_batch_advance here, semi_batch_advance and
// overlap_batch_advance in their headers) moves a pair's state on from where its walk stands.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "nw_pair_semi_plan.h"

namespace gsa {

// Default of gsa_align_batch_dev's scratch_limit: 40 pairs of 20k in one round (about 800 strips of
// 1024 rows, roughly one wave per SIMD of 256 CUs).
constexpr long long kPairBatchScratch = 8ll << 30;

// Where a pair of the batch stands between rounds.
struct BatchPairState
{
    long long tHi;     // its lowest strip not yet filled; < 0: nothing left to fill
    long long J;       // the column its walk stands on: its next chunk needs jW + 1 ... J
    long long jW = 0;  // its window
};

// A pair's chunk within a round.
struct BatchChunk
{
    int pair;           // index into the states
    PairChunk c;        // its strips, width (PairChunk::J = J - jW) and bytes
    long long codeOff;  // bytes: the chunk's codes within the round's buffer
};

// code bytes a pair still needs if its walk never moves left of J and reaches row 0
inline long long batch_pair_remaining(long long TR, const BatchPairState& s)
{
    return (s.tHi < 0 || s.J <= s.jW) ? 0 : (s.tHi + 1) * pair_strip_bytes(TR, s.J - s.jW);
}

// One round: the chunks, in the order the pairs were taken, and the bytes they hold in all (0: no
// pair is active, or not even the first one's strip fits the limit).
inline long long batch_plan_round(long long TR, long long limit, const std::vector<BatchPairState>& st,
                                  std::vector<BatchChunk>* out)
{
    out->clear();
    std::vector<int> order;
    for (int p = 0; p < (int)st.size(); ++p)
        if (st[(size_t)p].tHi >= 0 && st[(size_t)p].J > st[(size_t)p].jW) order.push_back(p);
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) {
        return batch_pair_remaining(TR, st[(size_t)a]) > batch_pair_remaining(TR, st[(size_t)b]);
    });
    long long used = 0;
    for (int p : order)
    {
        BatchChunk b;
        b.pair = p;
        if (!semi_plan_chunk(TR, st[(size_t)p].tHi, st[(size_t)p].J, st[(size_t)p].jW, limit - used, &b.c)) continue;
        b.codeOff = used;
        used += b.c.codeBytes;
        out->push_back(b);
    }
    return used;
}

// A pair's state after the round that ran chunk c, its walk standing on (i, j), `done` as the walk
// reported it: the path's first cell is reached, wherever it lies; otherwise the walk must stand on the
// chunk's upper boundary right of column 0 and goes on for the columns 1 ... j.  False: neither.
inline bool pair_batch_advance(long long TR, const PairChunk& c, long long i, long long j, bool done, BatchPairState* s)
{
    if (done)
    {
        s->tHi = -1;
        return true;
    }
    if (c.tLo < 1 || i != pair_chunk_stop_row(TR, c) || j < 1) return false;
    s->tHi = c.tLo - 1;
    s->J = j;
    return true;
}

}  // namespace gsa
