// ring_rs_tu.h — the ten ReduceScatter kernels of ONE reduction op, in their
// own translation unit (ring_rs_<op>.hip) so the four ops compile in parallel.
// The reference declares mccsFuncReduceScatter (devcomm.h:14) but ships no
// kernel for it, so there are no reference-named entry points here: every
// launch goes through the library's multi-rank kernel.
#pragma once
#include "ring_kernel.h"

#define MCCS_RS_CASE(OPN, OPV, TN, DT) \
  case DT:                             \
    return (const void*)&ring_multi_kernel<mccsFuncReduceScatter, DT, OPV>;

#define MCCS_RS_TYPES(X, OPN, OPV)                                                                  \
  X(OPN, OPV, int8_t, mccsInt8) X(OPN, OPV, uint8_t, mccsUint8) X(OPN, OPV, int32_t, mccsInt32)    \
  X(OPN, OPV, uint32_t, mccsUint32) X(OPN, OPV, int64_t, mccsInt64) X(OPN, OPV, uint64_t, mccsUint64) \
  X(OPN, OPV, half, mccsFloat16) X(OPN, OPV, float, mccsFloat32) X(OPN, OPV, double, mccsFloat64)  \
  X(OPN, OPV, bfloat16, mccsBfloat16)

// Defines mccs::ring_rs_kernel_<OPN>(dtype), which instantiates the kernels.
#define MCCS_RS_TU(OPN, OPV)                                     \
  namespace mccs {                                               \
  const void* ring_rs_kernel_##OPN(int dtype) {                  \
    switch (dtype) { MCCS_RS_TYPES(MCCS_RS_CASE, OPN, OPV) }     \
    return nullptr;                                              \
  }                                                              \
  }
