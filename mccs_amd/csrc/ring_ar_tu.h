// ring_ar_tu.h — the ten AllReduce kernels of ONE reduction op: the
// reference-named entry points (collectives.h:43-49, common.h:182-188) and the
// library's multi-rank launch, instantiated in their own translation unit
// (ring_ar_<op>.hip) so the four ops compile in parallel.
#pragma once
#include "ring_kernel.h"

#define MCCS_AR_KERNEL(OPN, OPV, TN, DT)                                                               \
  extern "C" __global__ void __launch_bounds__(MCCS_RING_MAX_THREADS)                                  \
      mccsKernel_AllReduce_RING_SIMPLE_##OPN##_##TN(mccsDevComm* comm, uint64_t channelMask,           \
                                                    mccsDevWork* workHead) {                           \
    mccs::ring_kernel_body<mccsFuncAllReduce, DT, OPV, mccs::kRefUnroll<DT>>(comm, channelMask, workHead,  \
                                                                             blockIdx.x, gridDim.x,       \
                                                                             mccs::kRefCfg);              \
  }

#define MCCS_AR_CASE(OPN, OPV, TN, DT)                                                                       \
  case DT:                                                                                                   \
    return multi ? (const void*)&ring_multi_kernel<mccsFuncAllReduce, DT, OPV>                             \
                 : (const void*)&mccsKernel_AllReduce_RING_SIMPLE_##OPN##_##TN;

// Defines the kernels and mccs::ring_ar_kernel_<OPN>(dtype, multi) for the
// element types TYPES lists (MCCS_RING_TYPES, or MCCS_RING_INT_TYPES for
// SumPostDiv; nullptr for a type it does not list).
#define MCCS_AR_TU_TYPES(OPN, OPV, TYPES)                        \
  TYPES(MCCS_AR_KERNEL, OPN, OPV)                                \
  namespace mccs {                                               \
  const void* ring_ar_kernel_##OPN(int dtype, bool multi) {      \
    switch (dtype) { TYPES(MCCS_AR_CASE, OPN, OPV) }             \
    return nullptr;                                              \
  }                                                              \
  }
#define MCCS_AR_TU(OPN, OPV) MCCS_AR_TU_TYPES(OPN, OPV, MCCS_RING_TYPES)
