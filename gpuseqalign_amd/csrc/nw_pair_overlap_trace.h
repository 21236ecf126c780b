// nw_pair_overlap_trace.h -- the overlap (dovetail) alignment of one long pair: the strip fill with
// 4-bit move codes under a free row 0 and a free column 0, seeded from the score kernel's checkpoint
// rows, and the walk that stops on either border (nw_pair_overlap_trace.hip); used by
// gsa_score.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gsa {

// The fill of a chunk of strips, as PairFillArgs (nw_pair_trace.h): a task is one strip, one wave, lane
// l holds the strip's rows l KR + 1 ... (l + 1) KR (KR = TR / 64: 8 or 16).
struct OverlapFillArgs
{
    const int* seqY;  // rows, letters at 1 ... R
    const int* seqX;  // columns
    const int* subst;
    int substsz;
    int go, ge;
    int iEnd;                        // rows 1 ... iEnd are filled (the end cell's row)
    int J;                           // columns 1 ... J
    int tLo, nstrips;                // the chunk's strips: tLo ... tLo + nstrips - 1
    const unsigned long long* gran;  // the score launch's hand-off rows: Hgo', epoch << 32 | value
    const unsigned long long* gran2; // F' (affine gaps)
    long long granStride;            // words per row
    unsigned char* codes;            // strip s at (s - tLo) stripBytes, column j at (j - 1) TR / 2,
    long long stripBytes;            // lane l at l KR / 2
    unsigned* counter;               // the task counter, zero before the launch
};

// The walk's state between chunks.
struct OverlapWalkRec
{
    int i, j;        // the cell the walk stands on
    unsigned state;  // 4: H; inside a gap the gap's source code
    int n;           // moves written so far
    int done;        // row 0 or column 0 is reached
    int pad0, pad1, pad2;
};

struct OverlapWalkArgs
{
    const int* seqY;
    const int* seqX;
    const unsigned char* codes;
    long long stripBytes;
    int krShift;  // log2 KR: 3 or 4
    int tLo;      // the chunk's first strip
    int iStop;    // stop on this row (> 0) at a column > 0: the chunk's upper boundary
    OverlapWalkRec* rec;
    unsigned char* moves;  // one byte per move, last move first
};

// a grid for nstrips tasks
hipError_t overlap_fill_grid(bool affine, int KR, int nstrips, int* grid);
// the fill of a chunk on `grid` workgroups, then the walk (one lane); ev (may be null): three events
// recorded before the fill, between the two and after the walk.  KR: 8 or 16
hipError_t launch_overlap_trace(const OverlapFillArgs& f, const OverlapWalkArgs& w, int KR, int grid, hipEvent_t* ev,
                                hipStream_t st);

}  // namespace gsa
