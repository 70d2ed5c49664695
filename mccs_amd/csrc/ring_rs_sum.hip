// ring_rs_sum.hip — ReduceScatter ring kernels, reduction op Sum (ring_rs_tu.h).
#include "ring_rs_tu.h"

MCCS_RS_TU(Sum, mccs::OpSum)
MCCS_RING_TU_ACCESSORS(rs_sum)
