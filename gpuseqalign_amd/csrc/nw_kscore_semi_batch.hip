// nw_kscore_semi_batch.hip -- the semi-global score modes (kModeScoreSG, kModeScoreSGL) of
// nw_kscore_kernel over a batch of independent pairs (the BATCH instances, every pair's row buffer in
// its descriptor) and the kernel that takes each pair's row maximum, in a translation unit of their own
// so that the instances of the other score units keep their code; built with the default scheduler.
#define GSA_KROW_SCORE
#define GSA_KSCORE_SEMI_BATCH
#include "nw_krow.hip"
