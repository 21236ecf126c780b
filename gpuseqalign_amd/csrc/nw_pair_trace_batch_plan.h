// nw_pair_trace_batch_plan.h -- the alignments of a batch of long pairs (gsa_align_batch_dev;
// DESIGN.md 2.2j): how the pairs' strips are spread over rounds whose move codes fit the scratch
// limit.  No HIP here: tests/align_batch_plan_driver.cpp checks it on the CPU.
//
// Every pair is cut as nw_pair_trace_plan.h cuts one pair: strips of TR rows up to its i_end, taken
// bottom-up, a later chunk only for the columns 1 ... j where the pair's walk left the chunk below.  A
// round has `limit` bytes.  The pairs that still have strips to fill are taken in a fixed order --
// remaining code bytes descending, ties by index -- and each gets its next chunk by pair_plan_chunk's
// rule against the bytes still free in the round: its lowest unfilled strip and as many above it as
// fit.  A pair for which nothing is left waits for the next round.  The first pair of a round has the
// whole limit, so, every strip fitting the limit alone, every round fills at least one strip.  With
// one pair the rounds are pair_plan_chunk's chunks.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "nw_pair_trace_plan.h"

namespace gsa {

// Default of gsa_align_batch_dev's scratch_limit: 40 pairs of 20k in one round (about 800 strips of
// 1024 rows, roughly one wave per SIMD of 256 CUs).
constexpr long long kPairBatchScratch = 8ll << 30;

// Where a pair of the batch stands between rounds.
struct BatchPairState
{
    long long tHi;  // its lowest strip not yet filled; < 0: nothing left to fill
    long long J;    // the columns its next chunk needs: 1 ... J
};

// A pair's chunk within a round.
struct BatchChunk
{
    int pair;           // index into the states
    PairChunk c;        // its strips, columns and bytes
    long long codeOff;  // bytes: the chunk's codes within the round's buffer
};

// code bytes a pair still needs if its walk never moves left of J
inline long long batch_pair_remaining(long long TR, const BatchPairState& s)
{
    return s.tHi < 0 ? 0 : (s.tHi + 1) * pair_strip_bytes(TR, s.J);
}

// One round: the chunks, in the order the pairs were taken, and the bytes they hold in all (0: no
// pair is active, or not even the first one's strip fits the limit).
inline long long batch_plan_round(long long TR, long long limit, const std::vector<BatchPairState>& st,
                                  std::vector<BatchChunk>* out)
{
    out->clear();
    std::vector<int> order;
    for (int p = 0; p < (int)st.size(); ++p)
        if (st[(size_t)p].tHi >= 0 && st[(size_t)p].J >= 1) order.push_back(p);
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) {
        return batch_pair_remaining(TR, st[(size_t)a]) > batch_pair_remaining(TR, st[(size_t)b]);
    });
    long long used = 0;
    for (int p : order)
    {
        BatchChunk b;
        b.pair = p;
        if (!pair_plan_chunk(TR, st[(size_t)p].tHi, st[(size_t)p].J, limit - used, &b.c)) continue;
        b.codeOff = used;
        used += b.c.codeBytes;
        out->push_back(b);
    }
    return used;
}

}  // namespace gsa
