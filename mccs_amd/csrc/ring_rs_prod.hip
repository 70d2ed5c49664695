// ring_rs_prod.hip — ReduceScatter ring kernels, reduction op Prod (ring_rs_tu.h).
#include "ring_rs_tu.h"

MCCS_RS_TU(Prod, mccs::OpProd)
MCCS_RING_TU_ACCESSORS(rs_prod)
