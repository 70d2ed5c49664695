// ring_ar_sumpostdiv.hip — AllReduce ring kernels, reduction op SumPostDiv: the six
// integer types (ring_ar_tu.h; the divisor rides in each work element's
// redOpArg, dtypes.h post_op).
#include "ring_ar_tu.h"

MCCS_AR_TU_TYPES(SumPostDiv, mccs::OpSumPostDiv, MCCS_RING_INT_TYPES)
MCCS_RING_TU_ACCESSORS(ar_sumpostdiv)
