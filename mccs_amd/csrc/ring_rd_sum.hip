// ring_rd_sum.hip — Reduce ring kernels, reduction op Sum (ring_rd_tu.h).
#include "ring_rd_tu.h"

MCCS_RD_TU(Sum, mccs::OpSum)
MCCS_RING_TU_ACCESSORS(rd_sum)
