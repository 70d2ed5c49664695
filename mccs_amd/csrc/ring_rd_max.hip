// ring_rd_max.hip — Reduce ring kernels, reduction op Max (ring_rd_tu.h).
#include "ring_rd_tu.h"

MCCS_RD_TU(Max, mccs::OpMax)
MCCS_RING_TU_ACCESSORS(rd_max)
