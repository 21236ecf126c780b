// nw_band_batch.h -- the banded calls over a batch of long pairs: the persistent fill whose workgroups
// claim pair after pair, with or without move codes, and the pairs' walks side by side
// (nw_band_batch.hip); used by gsa_score.hip.  The pair's descriptor, the walk's
// arguments and its record are nw_band.h's; the waves rule and the rounds are nw_band_batch_plan.h's.
#pragma once
#include <hip/hip_runtime.h>

#include "nw_band.h"
#include "nw_band_batch_plan.h"

namespace gsa {

// The grid of a fill launch of `waves` waves per workgroup over npairs pairs: min(pairs, resident
// workgroups, maxWgs), maxWgs = 0 for no cap.
hipError_t band_batch_fill_grid(bool affine, bool codes, int waves, int npairs, int maxWgs, int* grid);

// One round: the fill of descs[0 ... npairs - 1] in that order -- *counter, which the call zeroes in
// stream order, hands them out -- on `grid` workgroups of `waves` waves; then, if walks is not null,
// the walks of walks[0 ... npairs - 1], one wave each, on walkGrid workgroups.  ev (may be null): three
// events recorded before the fill, behind it and behind the walks.
hipError_t launch_band_batch(const BandDesc* descs, int npairs, unsigned* counter, int waves, int grid, const int* subst,
                             int substsz, int go, int ge, bool codes, const BandWalkArgs* walks, int walkGrid,
                             hipEvent_t* ev, hipStream_t st);

}  // namespace gsa
