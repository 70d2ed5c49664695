// ring_rd_prod.hip — Reduce ring kernels, reduction op Prod (ring_rd_tu.h).
#include "ring_rd_tu.h"

MCCS_RD_TU(Prod, mccs::OpProd)
MCCS_RING_TU_ACCESSORS(rd_prod)
