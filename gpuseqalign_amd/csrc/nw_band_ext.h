// nw_band_ext.h -- the banded extension alignment of one long pair: nw_band.h's one-pass fill in the
// extension mode, which keeps the best cell of the band, and the walk from that cell (nw_band_ext.hip;
// DESIGN.md 2.2r); used by gsa_score.hip.  The descriptor, the walk's arguments and its record are
// nw_band.h's, the plan is nw_band_ext_plan.h's.
#pragma once
#include <hip/hip_runtime.h>

#include "nw_band.h"
#include "nw_band_ext_plan.h"

namespace gsa {

// launch_band's arguments.  The fill writes four result words per pair (BandDesc::result); w, if not
// null, names them in w->start, and the walk, enqueued behind the fill, starts where they say.
hipError_t launch_band_ext(const BandDesc* descs, int npairs, int waves, const int* subst, int substsz, int go, int ge,
                           bool codes, const BandWalkArgs* w, hipEvent_t* ev, hipStream_t st);

}  // namespace gsa
