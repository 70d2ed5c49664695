// ring_rd_tu.h — the ten Reduce kernels of ONE reduction op, in their own
// translation unit (ring_rd_<op>.hip) so the four ops compile in parallel.
// The reference declares mccsFuncReduce (devcomm.h:12) but ships no kernel
// for it, so there are no reference-named entry points here: every launch
// goes through the library's multi-rank kernel.
#pragma once
#include "ring_kernel.h"

#define MCCS_RD_CASE(OPN, OPV, TN, DT) \
  case DT:                             \
    return (const void*)&ring_multi_kernel<mccsFuncReduce, DT, OPV>;

// Defines mccs::ring_rd_kernel_<OPN>(dtype), which instantiates the kernels,
// for the element types TYPES lists (MCCS_RING_INT_TYPES for SumPostDiv;
// nullptr for a type it does not list).
#define MCCS_RD_TU_TYPES(OPN, OPV, TYPES)                        \
  namespace mccs {                                               \
  const void* ring_rd_kernel_##OPN(int dtype) {                  \
    switch (dtype) { TYPES(MCCS_RD_CASE, OPN, OPV) }             \
    return nullptr;                                              \
  }                                                              \
  }
#define MCCS_RD_TU(OPN, OPV) MCCS_RD_TU_TYPES(OPN, OPV, MCCS_RING_TYPES)
