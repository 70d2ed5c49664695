// ring_rs_min.hip — ReduceScatter ring kernels, reduction op Min (ring_rs_tu.h).
#include "ring_rs_tu.h"

MCCS_RS_TU(Min, mccs::OpMin)
MCCS_RING_TU_ACCESSORS(rs_min)
