// ring_rs_max.hip — ReduceScatter ring kernels, reduction op Max (ring_rs_tu.h).
#include "ring_rs_tu.h"

MCCS_RS_TU(Max, mccs::OpMax)
MCCS_RING_TU_ACCESSORS(rs_max)
