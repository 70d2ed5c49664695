// ring_rd_premulsum.hip — Reduce ring kernels, reduction op PreMulSum (ring_rd_tu.h).
#include "ring_rd_tu.h"

MCCS_RD_TU(PreMulSum, mccs::OpPreMulSum)
MCCS_RING_TU_ACCESSORS(rd_premulsum)
