// ring_rd_sumpostdiv.hip — Reduce ring kernels, reduction op SumPostDiv: the six
// integer types (ring_rd_tu.h).
#include "ring_rd_tu.h"

MCCS_RD_TU_TYPES(SumPostDiv, mccs::OpSumPostDiv, MCCS_RING_INT_TYPES)
MCCS_RING_TU_ACCESSORS(rd_sumpostdiv)
