// nw_kscore_overlap_batch.hip -- the overlap (dovetail) score modes (kModeScoreOV, kModeScoreOVL) of
// nw_kscore_kernel over a batch of independent pairs (the BATCH instances, every pair's row and column
// buffer in its descriptor) and the kernel that takes each pair's maximum over row R and column C, in a
// translation unit of their own so that the instances of the other score units keep their code; built
// with the default scheduler.
#define GSA_KROW_SCORE
#define GSA_KSCORE_OVERLAP_BATCH
#include "nw_krow.hip"
