// ring_rs_sumpostdiv.hip — ReduceScatter ring kernels, reduction op SumPostDiv: the six
// integer types (ring_rs_tu.h).
#include "ring_rs_tu.h"

MCCS_RS_TU_TYPES(SumPostDiv, mccs::OpSumPostDiv, MCCS_RING_INT_TYPES)
MCCS_RING_TU_ACCESSORS(rs_sumpostdiv)
