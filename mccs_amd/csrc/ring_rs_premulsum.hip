// ring_rs_premulsum.hip — ReduceScatter ring kernels, reduction op PreMulSum (ring_rs_tu.h).
#include "ring_rs_tu.h"

MCCS_RS_TU(PreMulSum, mccs::OpPreMulSum)
MCCS_RING_TU_ACCESSORS(rs_premulsum)
