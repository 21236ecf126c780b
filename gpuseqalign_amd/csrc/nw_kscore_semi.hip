// nw_kscore_semi.hip -- the semi-global score modes (kModeScoreSG, kModeScoreSGL) of nw_kscore_kernel
// and the kernel that takes row R's first maximum, in a translation unit of their own so that the
// instances of the other score units keep their code; built with the default scheduler.
#define GSA_KROW_SCORE
#define GSA_KSCORE_SEMI
#include "nw_krow.hip"
