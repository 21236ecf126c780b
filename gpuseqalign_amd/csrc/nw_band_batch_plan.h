// nw_band_batch_plan.h -- the banded calls over a batch of long pairs (gsa_score_band_batch_dev,
// gsa_align_batch_band_dev): how many waves a launch's workgroups get, the order in
// which the persistent workgroups claim the pairs, and the rounds of the alignment call.  HIP-free, so
// that a plain C++ program can check it (tests/band_batch_plan_driver.cpp); used by nw_band_batch.hip
// and gsa_score.hip.  A pair's own geometry is nw_band_plan.h's.
//
// Waves.  nw_band_plan.h's schedule is written over NWV waves: strip s runs on wave s mod NWV from the
// super-step s lag for nq super-steps, so the wave is free for strip s + NWV iff nq <= NWV lag.  With
// strips <= NWV no wave takes a second strip and the rule does not bind.  The ring of a wave is
// indexed by the super-step and does not depend on NWV.  A launch uses one count for all its pairs.
//
// Rounds.  The move codes of a pair are held whole (the walk needs all strips).  Pairs that need codes
// are taken by code bytes descending, ties by index; a round takes every pair that still fits the bytes
// left, first fit in that order, so its first pair has the whole limit.  A pair whose own codes exceed
// the limit runs without codes (status 1), with the pairs that have no codes for another reason.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "nw_band_plan.h"

namespace gsa {

// Default of gsa_align_batch_band_dev's scratch_limit: bytes of move codes held at once.
constexpr int64_t kBandBatchScratch = 8ll << 30;
constexpr int kBandBatchWaves[3] = {4, 8, 16};

// A workgroup of nwv waves can run a pair of `strips` strips of nq super-steps.
inline bool band_waves_ok(int nwv, int64_t strips, int64_t nq)
{
    return strips <= nwv || nq <= (int64_t)nwv * kBandLag;
}

// The widest band nwv waves take with more strips than waves: nq = ceil((W + TR + 62) / 64) <= nwv lag.
inline int64_t band_waves_max_width(int nwv) { return 64ll * nwv * kBandLag - kBandTR + 1 - 63; }

// The smallest of 4, 8 and 16 waves that every one of the n pairs (strips[k], nq[k]) can run on.  16
// takes every pair band_plan() accepts.
inline int band_batch_waves(const int64_t* strips, const int64_t* nq, size_t n)
{
    for (int nwv : kBandBatchWaves)
    {
        bool ok = true;
        for (size_t k = 0; k < n && ok; ++k) ok = band_waves_ok(nwv, strips[k], nq[k]);
        if (ok) return nwv;
    }
    return kBandWaves;
}

// `forced` is 0 (the rule above) or one of 4, 8, 16.  0: the argument is refused -- no such count, or
// too few waves for one of the pairs.
inline int band_batch_pick_waves(int forced, const int64_t* strips, const int64_t* nq, size_t n)
{
    if (forced == 0) return band_batch_waves(strips, nq, n);
    if (forced != 4 && forced != 8 && forced != 16) return 0;
    for (size_t k = 0; k < n; ++k)
        if (!band_waves_ok(forced, strips[k], nq[k])) return 0;
    return forced;
}

// The order the workgroups claim a launch's pairs in: super-steps T descending, ties by index.
inline std::vector<int> band_batch_order(const std::vector<int64_t>& T)
{
    std::vector<int> o(T.size());
    for (size_t k = 0; k < o.size(); ++k) o[k] = (int)k;
    std::stable_sort(o.begin(), o.end(), [&](int a, int b) { return T[(size_t)a] > T[(size_t)b]; });
    return o;
}

struct BandBatchRounds
{
    std::vector<std::vector<int>> rounds;  // per round the pairs, in the order they were taken
    std::vector<int> nocode;               // pairs whose own codes exceed the limit, by index
    std::vector<int> roundOf;              // per pair: its round, -2 for nocode, -3 for a pair not planned
    int64_t peakBytes = 0;                 // the most a round holds
};

// codeBytes[p] < 0: the pair takes no part (answered on the host, or without codes for another reason).
inline BandBatchRounds band_batch_rounds(const std::vector<int64_t>& codeBytes, int64_t limit)
{
    BandBatchRounds r;
    r.roundOf.assign(codeBytes.size(), -3);
    std::vector<int> todo;
    for (size_t p = 0; p < codeBytes.size(); ++p)
    {
        if (codeBytes[p] < 0) continue;
        if (codeBytes[p] > limit)
        {
            r.nocode.push_back((int)p);
            r.roundOf[p] = -2;
        }
        else
            todo.push_back((int)p);
    }
    std::stable_sort(todo.begin(), todo.end(), [&](int a, int b) { return codeBytes[(size_t)a] > codeBytes[(size_t)b]; });
    while (!todo.empty())
    {
        std::vector<int> take, rest;
        int64_t left = limit;
        for (int p : todo)
        {
            if (codeBytes[(size_t)p] <= left)
            {
                left -= codeBytes[(size_t)p];
                r.roundOf[(size_t)p] = (int)r.rounds.size();
                take.push_back(p);
            }
            else
                rest.push_back(p);
        }
        r.peakBytes = std::max(r.peakBytes, limit - left);
        r.rounds.push_back(take);
        todo.swap(rest);
    }
    return r;
}

}  // namespace gsa
