// nw_pair_trace_plan.h -- the alignment of one long pair (gsa_align_pair_dev): how
// the rows 1 ... i_end are cut into strips and the strips into chunks whose move codes fit the
// scratch limit.  No HIP here: tests/align_pair_plan_driver.cpp checks it on the CPU.
//
// A strip is the score kernel's ticket: rows t TR + 1 ... (t + 1) TR.  Its codes over the columns
// 1 ... J take J TR / 2 bytes (4 bits a cell, every row of the strip whether or not i_end cuts it).
// The chunks are taken bottom-up, because the walk goes upwards: the first holds i_end's strip and as
// many strips above it as fit, the walk runs through them and stops on the chunk's upper boundary at
// some column j, and the next chunk is planned for the columns 1 ... j only -- the path never moves
// right.  So the plan is made one chunk at a time.
#pragma once
#include <stdint.h>

namespace gsa {

// Default of gsa_align_pair_dev's scratch_limit: a 64k x 64k pair in one chunk.
constexpr long long kPairTraceScratch = 2ll << 30;

// strips that hold the rows 1 ... iEnd
inline long long pair_strips(long long TR, long long iEnd) { return (iEnd + TR - 1) / TR; }

// bytes of move codes of one strip over the columns 1 ... J
inline long long pair_strip_bytes(long long TR, long long J) { return J * (TR / 2); }

struct PairChunk
{
    long long tLo, tHi;    // the chunk's strips, tLo ... tHi (tHi the lowest in the matrix)
    long long J;           // its columns: 1 ... J
    long long stripBytes;  // codes of one strip
    long long codeBytes;   // codes of the chunk
};

// The chunk whose lowest strip is tHi, for the columns 1 ... J (J >= 1): tHi and as many strips above
// it as fit `limit` bytes (greedy).  False when one strip alone does not fit.
inline bool pair_plan_chunk(long long TR, long long tHi, long long J, long long limit, PairChunk* c)
{
    const long long sb = pair_strip_bytes(TR, J);
    if (sb > limit) return false;
    const long long fit = limit / sb;
    const long long n = fit < tHi + 1 ? fit : tHi + 1;
    c->tLo = tHi + 1 - n;
    c->tHi = tHi;
    c->J = J;
    c->stripBytes = sb;
    c->codeBytes = n * sb;
    return true;
}

// byte offset of strip s's codes within its chunk's
inline long long pair_code_off(const PairChunk& c, long long s) { return (s - c.tLo) * c.stripBytes; }

// the row a walk through the chunk stops on (0: the matrix's border, where it ends anyway)
inline long long pair_chunk_stop_row(long long TR, const PairChunk& c) { return c.tLo * TR; }

}  // namespace gsa
