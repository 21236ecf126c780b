// nw_lanes_trace.h -- database search, alignments of chosen hits: the lane kernel's fill with 4-bit
// move codes and the walk over them (nw_lanes_trace.hip); used by gsa_score.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nw_lanes.h"

namespace gsa {

// A cell's code: bits 0-1 the source of H, bit 2 "E was extended", bit 3 "F was extended".  The
// sources are numbered in the order the tie rule prefers them at equal value (the fill takes the
// maximum of 4 x value + source).
constexpr unsigned kDbTraceE = 0, kDbTraceF = 1, kDbTraceDiag = 2, kDbTraceStop = 3;
constexpr unsigned kDbTraceEExt = 4, kDbTraceFExt = 8;
// The fill keeps 4 x value + source in int32: every |value| of a pair it takes, gap runs along the
// borders included, stays below this.
constexpr long long kDbTraceMaxValue = 1ll << 26;
// A lane's kDbLanesKQ = 24 codes of one column: three dwords; the 16 lanes of a hit write 192
// contiguous bytes per column.
constexpr int kDbTraceLaneBytes = kDbLanesKQ / 2;
constexpr int kDbTraceColBytes = kDbLanesG * kDbTraceLaneBytes;
static_assert(kDbLanesKQ % 8 == 0, "a lane's codes of a column are whole dwords");

struct DbTraceOut
{
    int score, i_end, j_end, i_start, j_start, moves, pad0, pad1;
};

struct DbTraceArgs
{
    DbLanesArgs fill;             // the hits of this chunk as the score kernel takes its subjects
    unsigned char* codes;         // the chunk's move codes
    const long long* codeOff;     // per hit, byte offset into codes: passes x (C + 1) x 192 bytes each
    const long long* moveOff;     // per hit, byte offset into moves: R + C bytes each
    DbTraceOut* res;              // per hit
    unsigned char* moves;         // one byte per move ('=', 'X', 'I', 'D'), last move first
    int local;
};

// bytes of move codes of one hit
inline long long dbtrace_code_bytes(long long R, long long C)
{
    const long long passes = (R + kDbLanesPassRows - 1) / kDbLanesPassRows;
    return passes * (C + 1) * kDbTraceColBytes;
}

// workgroups of the fill resident at once for this query (the size of the boundary scratch)
hipError_t dbtrace_resident(int R, int substsz, int local, bool affine, int* wgs);
// the fill with move codes on `grid` workgroups, then the walk, one lane per hit; ev (may be null):
// three events recorded before the fill, between the two and after the walk
hipError_t launch_dbtrace(const DbTraceArgs& a, int grid, hipEvent_t* ev, hipStream_t st);

}  // namespace gsa
