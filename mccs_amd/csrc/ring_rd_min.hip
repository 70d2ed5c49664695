// ring_rd_min.hip — Reduce ring kernels, reduction op Min (ring_rd_tu.h).
#include "ring_rd_tu.h"

MCCS_RD_TU(Min, mccs::OpMin)
MCCS_RING_TU_ACCESSORS(rd_min)
