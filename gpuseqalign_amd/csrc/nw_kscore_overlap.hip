// nw_kscore_overlap.hip -- the overlap (dovetail) score modes (kModeScoreOV, kModeScoreOVL) of
// nw_kscore_kernel and the kernel that takes the first maximum over row R and column C, in a
// translation unit of their own so that the instances of the other score units keep their code; built
// with the default scheduler.
#define GSA_KROW_SCORE
#define GSA_KSCORE_OVERLAP
#include "nw_krow.hip"
