// nw_pair_trace.h -- the alignment of one long pair: the strip fill with 4-bit move codes, seeded
// from the score kernel's checkpoint rows, and the walk over them (nw_pair_trace.hip; DESIGN.md
// 2.2i); used by gsa_score.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gsa {

// The fill of a chunk of strips.  A task is one strip, one wave: lane l holds the strip's rows
// l KR + 1 ... (l + 1) KR (KR = TR / 64: 8 or 16) and runs one column behind lane l - 1.
struct PairFillArgs
{
    const int* seqY;  // rows, letters at 1 ... R
    const int* seqX;  // columns
    const int* subst;
    int substsz;
    int go, ge;
    int local;
    int R;                           // letters of seqY (rows past iEnd in its strip clamp to it)
    int iEnd;                        // rows 1 ... iEnd are filled
    int J;                           // columns 1 ... J
    int tLo, nstrips;                // the chunk's strips: tLo ... tLo + nstrips - 1
    const unsigned long long* gran;  // the score launch's hand-off rows: Hgo', epoch << 32 | value
    const unsigned long long* gran2; // F' (affine modes)
    long long granStride;            // words per row
    unsigned char* codes;            // strip s at (s - tLo) stripBytes, column j at (j - 1) TR / 2,
    long long stripBytes;            // lane l at l KR / 2
    unsigned* counter;               // the task counter, zero before the launch
};

// The walk's state between chunks.
struct PairWalkRec
{
    int i, j;        // the cell the walk stands on
    unsigned state;  // 4: H; inside a gap the gap's source code
    int n;           // moves written so far
    int done;        // the path's first cell is reached
    int pad0, pad1, pad2;
};

struct PairWalkArgs
{
    const int* seqY;
    const int* seqX;
    const unsigned char* codes;
    long long stripBytes;
    int krShift;  // log2 KR: 3 or 4
    int tLo;      // the chunk's first strip
    int iStop;    // stop on this row (> 0) at a column > 0: the chunk's upper boundary
    int local;
    PairWalkRec* rec;
    unsigned char* moves;  // one byte per move, last move first
};

// the fill's LDS and a grid for nstrips tasks
hipError_t pair_fill_grid(int local, bool affine, int KR, int nstrips, int* grid);
// the fill of a chunk on `grid` workgroups, then the walk (one lane); ev (may be null): three events
// recorded before the fill, between the two and after the walk.  KR: 8 or 16
hipError_t launch_pair_trace(const PairFillArgs& f, const PairWalkArgs& w, int KR, int grid, hipEvent_t* ev,
                             hipStream_t st);

}  // namespace gsa
