// nw_pair_overlap_trace_batch.h -- the overlap (dovetail) alignments of a batch of long pairs: the strips
// of many pairs filled with 4-bit move codes under a free row 0 and a free column 0 in one launch, seeded
// from the batched score launch's checkpoint rows, and the pairs' walks side by side
// (nw_pair_overlap_trace_batch.hip); used by gsa_score.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nw_pair_overlap_trace.h"
#include "nw_pair_trace_batch.h"

namespace gsa {

// (a pair of a round's fill is a PairBatchDesc: iEnd the pair's end row, J the round's last column,
// stripBytes the codes of one strip over the columns 1 ... J; a task is a PairBatchTask: pair, strip,
// code offset)
struct OverlapBatchFillArgs
{
    const PairBatchDesc* pairs;
    const PairBatchTask* tasks;  // by column count descending
    int ntasks;
    const int* subst;
    int substsz;
    int go, ge;
    const unsigned long long* gran;   // the score launch's hand-off rows: Hgo', epoch << 32 | value
    const unsigned long long* gran2;  // F' (affine gaps)
    unsigned char* codes;
    unsigned* counter;  // the task counter, zero before the launch
};

// One pair of a round's walk.
struct OverlapBatchWalk
{
    const int* seqY;
    const int* seqX;
    const unsigned char* codes;  // the pair's chunk: strip s at (s - tLo) stripBytes, column j at (j - 1) TR / 2
    long long stripBytes;
    int tLo;    // the chunk's first strip
    int iStop;  // stop on this row (> 0) at a column > 0: the chunk's upper boundary
    int rec;    // index of the pair's record
    int pad0;
    unsigned char* moves;  // one byte per move, last move first
};

struct OverlapBatchWalkArgs
{
    const OverlapBatchWalk* walks;
    int nwalks;
    int krShift;  // log2 KR: 3 or 4
    OverlapWalkRec* recs;
};

// a grid for ntasks fill tasks, at most maxWgs workgroups (0: all resident).  KR: 8 or 16
hipError_t overlap_batch_fill_grid(bool affine, int KR, int ntasks, int maxWgs, int* grid);
// the fill of a round on `grid` workgroups, then the walks, one workgroup per pair up to walkGrid;
// ev: three events recorded before the fill, between the two and after the walks
hipError_t launch_overlap_batch_trace(const OverlapBatchFillArgs& f, const OverlapBatchWalkArgs& w, int KR, int grid,
                                      int walkGrid, hipEvent_t* ev, hipStream_t st);

}  // namespace gsa
