// ring_ar_premulsum.hip — AllReduce ring kernels, reduction op PreMulSum (ring_ar_tu.h;
// the scalar rides in each work element's redOpArg, dtypes.h pre_op).
#include "ring_ar_tu.h"

MCCS_AR_TU(PreMulSum, mccs::OpPreMulSum)
MCCS_RING_TU_ACCESSORS(ar_premulsum)
