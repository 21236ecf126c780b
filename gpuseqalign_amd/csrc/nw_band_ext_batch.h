// nw_band_ext_batch.h -- the banded extension calls over a batch of long pairs: nw_band_batch.h's
// persistent fill with the body in its extension mode, and the pairs' walks side by side, each from the
// cell its fill found (nw_band_ext_batch.hip); used by gsa_score.hip.  The descriptor,
// the walk's arguments and its record are nw_band.h's; the waves rule and the rounds are
// nw_band_batch_plan.h's.
#pragma once
#include <hip/hip_runtime.h>

#include "nw_band.h"
#include "nw_band_batch_plan.h"
#include "nw_band_ext_plan.h"

namespace gsa {

// band_batch_fill_grid's, for the extension instances.
hipError_t band_ext_batch_fill_grid(bool affine, bool codes, int waves, int npairs, int maxWgs, int* grid);

// launch_band_batch's arguments.  Every pair has four result words (BandDesc::result), and its walk's
// `start` names them.
hipError_t launch_band_ext_batch(const BandDesc* descs, int npairs, unsigned* counter, int waves, int grid, const int* subst,
                                 int substsz, int go, int ge, bool codes, const BandWalkArgs* walks, int walkGrid,
                                 hipEvent_t* ev, hipStream_t st);

}  // namespace gsa
