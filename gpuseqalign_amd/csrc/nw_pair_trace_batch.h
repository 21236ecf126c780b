// nw_pair_trace_batch.h -- the alignments of a batch of long pairs: the strips of many pairs filled
// with 4-bit move codes in one launch, seeded from the batched score launch's checkpoint rows, and the
// pairs' walks side by side (nw_pair_trace_batch.hip); used by gsa_score.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nw_pair_trace.h"

namespace gsa {

// One pair of a round's fill.
struct PairBatchDesc
{
    const int* seqY;       // rows, letters at 1 ... R
    const int* seqX;       // columns
    int R;                 // letters of seqY
    int iEnd;              // rows 1 ... iEnd are filled
    int J;                 // columns 1 ... J (this round's)
    int pad0;
    long long granBase;    // words: the pair's first hand-off row within gran / gran2 (PairDesc::granOff)
    long long granStride;  // words per row
    long long stripBytes;  // codes of one strip over the columns 1 ... J
};

// One task of a round's fill: a strip of a pair.
struct PairBatchTask
{
    int pair;           // index into the descriptor table
    int strip;          // the strip within the pair: rows strip TR + 1 ... (strip + 1) TR
    long long codeOff;  // bytes: the strip's codes within the round's buffer
};

struct PairBatchFillArgs
{
    const PairBatchDesc* pairs;
    const PairBatchTask* tasks;  // by column count descending
    int ntasks;
    const int* subst;
    int substsz;
    int go, ge;
    const unsigned long long* gran;   // the score launch's hand-off rows: Hgo', epoch << 32 | value
    const unsigned long long* gran2;  // F' (affine modes)
    unsigned char* codes;
    unsigned* counter;  // the task counter, zero before the launch
};

// One pair of a round's walk.
struct PairBatchWalk
{
    const int* seqY;
    const int* seqX;
    const unsigned char* codes;  // the pair's chunk: strip s at (s - tLo) stripBytes
    long long stripBytes;
    int tLo;    // the chunk's first strip
    int iStop;  // stop on this row (> 0) at a column > 0: the chunk's upper boundary
    int rec;    // index of the pair's record
    int pad0;
    unsigned char* moves;  // one byte per move, last move first
};

struct PairBatchWalkArgs
{
    const PairBatchWalk* walks;
    int nwalks;
    int krShift;  // log2 KR: 3 or 4
    int local;
    int pad0;
    PairWalkRec* recs;
};

// a grid for ntasks fill tasks, at most maxWgs workgroups (0: all resident).  KR: 8 or 16
hipError_t pair_batch_fill_grid(int local, bool affine, int KR, int ntasks, int maxWgs, int* grid);
// the fill of a round on `grid` workgroups, then the walks, one workgroup per pair up to walkGrid;
// ev: three events recorded before the fill, between the two and after the walks
hipError_t launch_pair_batch_trace(const PairBatchFillArgs& f, int local, const PairBatchWalkArgs& w, int KR, int grid,
                                   int walkGrid, hipEvent_t* ev, hipStream_t st);

}  // namespace gsa
