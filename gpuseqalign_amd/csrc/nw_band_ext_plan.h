// nw_band_ext_plan.h -- the banded extension alignment of long pairs (gsa_score_band_ext_dev,
// gsa_align_pair_band_ext_dev and their batch forms): which bands the mode takes, the
// part of the pair the band reaches, the plan of that part and the optimality certificate.  HIP-free, so
// that a plain C++ program can check it (tests/band_ext_plan_driver.cpp); used by gsa_score.hip.  The
// strips, the schedule and the bytes of codes are nw_band_plan.h's, untouched.
//
// The start is (0, 0), the end is the best cell of the band, so the band must hold (0, 0) and need not
// hold (R, C).  Row i holds the columns i + lo ... i + hi: rows beyond C - lo and columns beyond R + hi
// hold no cell of the band, and the result on the prefixes of R' = min(R, C - lo) and C' = min(C, R + hi)
// letters is the result on the whole pair.  At most one of the two cuts (R' < R needs C < R, C' < C needs
// R < C), and the band holds (R', C'): nw_band_plan.h's band_valid is true of the trimmed pair.
#pragma once
#include <stdint.h>

#include "nw_band_plan.h"

namespace gsa {

// The band holds (0, 0).
inline bool band_ext_valid(int64_t lo, int64_t hi) { return lo <= 0 && 0 <= hi; }

// The rows and columns the band reaches, for a valid band.
inline void band_ext_trim(int64_t R, int64_t C, int64_t lo, int64_t hi, int64_t* Ru, int64_t* Cu)
{
    // (lo and hi are clamped first so that C - lo and R + hi cannot overflow)
    band_clamp(R, C, &lo, &hi);
    *Ru = band_min(R, C - lo);
    *Cu = band_min(C, R + hi);
}

// The plan of a pair with R, C >= 1: band_plan of the trimmed pair, whose clamped band is the clamped
// band of the whole pair.  False: the band does not hold (0, 0), or is wider than kBandMaxWidth after
// clamping.
inline bool band_ext_plan(int64_t R, int64_t C, int64_t lo, int64_t hi, int64_t* Ru, int64_t* Cu, BandPlan* p)
{
    if (R < 1 || C < 1 || !band_ext_valid(lo, hi)) return false;
    band_ext_trim(R, C, lo, hi, Ru, Cu);
    return band_plan(*Ru, *Cu, lo, hi, p);
}

// The certificate: 1 iff the banded score S exceeds what any path from (0, 0) that leaves the band
// (lo, hi: clamped to the whole pair R x C) can reach at any of its cells.  Such a path on the high side
// reaches diagonal hi + 1: it holds at least hi + 1 letters of D, in at least one run, and every
// diagonal step of it lies in a row 1 ... R and, from diagonal hi + 1 on or with hi + 1 columns still to
// cross, in one of C - hi - 1 columns; so no cell of it, on or behind the crossing, exceeds
// pmax min(R, C - hi - 1) + go + hi ge, and its cells before the crossing are cells of the band.  The low
// side is the mirror image with a = 1 - lo letters of I.  pmax: max(0, the largest table value).  A side
// on which the band reaches the matrix's corner (hi = C, lo = -R) cannot be left.  Strict, so that ties
// are safe: then every maximal cell of the unbanded problem is reached by optimal paths inside the band
// only, and the first of them and the walk's tie rule see the same values.
inline int band_ext_certificate(int64_t R, int64_t C, int64_t lo, int64_t hi, int64_t pmax, int64_t go, int64_t ge, int64_t S)
{
    if (hi < C)
    {
        const int64_t U = pmax * band_min(R, C - hi - 1) + go + hi * ge;
        if (S <= U) return 0;
    }
    if (lo > -R)
    {
        const int64_t a = 1 - lo;
        const int64_t U = pmax * band_min(C, R - a) + go + (a - 1) * ge;
        if (S <= U) return 0;
    }
    return 1;
}

}  // namespace gsa
