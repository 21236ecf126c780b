// nw_band.h -- the banded alignment of one long pair: the one-pass fill inside a diagonal band, with
// or without 4-bit move codes, and the walk over them (nw_band.hip); used by
// gsa_score.hip.  The geometry and the schedule are nw_band_plan.h's.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nw_band_plan.h"

namespace gsa {

// One pair of the fill: workgroup b takes descs[b].
struct BandDesc
{
    const int* seqY;       // rows, letters at 1 ... R
    const int* seqX;       // columns, letters at 1 ... C
    unsigned char* codes;  // strip s at s stripBytes, column j at (j - o(s)) TR / 2, lane l at l KR / 2
    int* result;           // [0] H(R, C), [1] 1 once it is written; the extension fill (nw_band_ext.h): [0] the
                           // best H of the band, [1] 1 once written, [2] i_end, [3] j_end
    long long stripBytes;
    int R, C;
    int lo, hi;            // the clamped band
    int strips, nq, T, Wc; // BandPlan's
};

struct BandWalkRec
{
    int i, j;        // the cell the walk stopped on
    unsigned state;
    int n;           // moves written
    int done;        // (0, 0) was reached
    int offband;     // the walk stepped onto a cell outside the band
    int pad0, pad1;
};

struct BandWalkArgs
{
    const int* seqY;
    const int* seqX;
    const unsigned char* codes;
    long long stripBytes;
    int R, C, lo, hi;
    BandWalkRec* rec;
    unsigned char* moves;  // one byte per move, last move first
    const int* start;      // null: the walk starts at (R, C); else at (start[2], start[3]), an extension fill's result words
};

// The fill of npairs pairs, one workgroup of `waves` waves each, with (codes) or without move codes;
// then, if w is not null, the walk of one pair.  ev (may be null): three events recorded before the
// fill, behind it and behind the walk.
hipError_t launch_band(const BandDesc* descs, int npairs, int waves, const int* subst, int substsz, int go, int ge,
                       bool codes, const BandWalkArgs* w, hipEvent_t* ev, hipStream_t st);

}  // namespace gsa
