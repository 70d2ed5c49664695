/*
 * mccs_kernels_avg.h — the reference-named PreMulSum and SumPostDiv AllReduce
 * ring kernels exported by libmccs_hip.so, beside mccs_kernels.h's.
 *
 * Mirrors DECL2(AllReduce, PreMulSum) and DECL2(AllReduce, SumPostDiv) of
 * src/collectives/include/collectives.h:101-102, with one difference: the
 * reference's FuncSumPostDiv static_asserts on the floating types
 * (reduce_kernel.h), so SumPostDiv has the six integer kernels only.  Each
 * kernel takes its scalar from the work element's redOpArg (devcomm.h), as the
 * reference's do: PreMulSum the multiplier in the element's type (low bytes),
 * SumPostDiv the divisor as an int.  Handles, arguments and the C++-linkage /
 * ___nv_bfloat16 aliases are as described in mccs_kernels.h.
 */
#ifndef MCCS_AMD_KERNELS_AVG_H_
#define MCCS_AMD_KERNELS_AVG_H_

#include <stdint.h>

#include "mccs_devcomm.h"

#ifdef __cplusplus
extern "C" {
#endif

#ifndef MCCS_KERNEL_SYMBOL
#define MCCS_KERNEL_SYMBOL(name) \
  void name(struct mccsDevComm *comm, uint64_t channelMask, struct mccsDevWork *workHead)
#endif

MCCS_KERNEL_SYMBOL(mccsKernel_AllReduce_RING_SIMPLE_PreMulSum_int8_t);
MCCS_KERNEL_SYMBOL(mccsKernel_AllReduce_RING_SIMPLE_PreMulSum_uint8_t);
MCCS_KERNEL_SYMBOL(mccsKernel_AllReduce_RING_SIMPLE_PreMulSum_int32_t);
MCCS_KERNEL_SYMBOL(mccsKernel_AllReduce_RING_SIMPLE_PreMulSum_uint32_t);
MCCS_KERNEL_SYMBOL(mccsKernel_AllReduce_RING_SIMPLE_PreMulSum_int64_t);
MCCS_KERNEL_SYMBOL(mccsKernel_AllReduce_RING_SIMPLE_PreMulSum_uint64_t);
MCCS_KERNEL_SYMBOL(mccsKernel_AllReduce_RING_SIMPLE_PreMulSum_half);
MCCS_KERNEL_SYMBOL(mccsKernel_AllReduce_RING_SIMPLE_PreMulSum_float);
MCCS_KERNEL_SYMBOL(mccsKernel_AllReduce_RING_SIMPLE_PreMulSum_double);
MCCS_KERNEL_SYMBOL(mccsKernel_AllReduce_RING_SIMPLE_PreMulSum_bfloat16);
MCCS_KERNEL_SYMBOL(mccsKernel_AllReduce_RING_SIMPLE_SumPostDiv_int8_t);
MCCS_KERNEL_SYMBOL(mccsKernel_AllReduce_RING_SIMPLE_SumPostDiv_uint8_t);
MCCS_KERNEL_SYMBOL(mccsKernel_AllReduce_RING_SIMPLE_SumPostDiv_int32_t);
MCCS_KERNEL_SYMBOL(mccsKernel_AllReduce_RING_SIMPLE_SumPostDiv_uint32_t);
MCCS_KERNEL_SYMBOL(mccsKernel_AllReduce_RING_SIMPLE_SumPostDiv_int64_t);
MCCS_KERNEL_SYMBOL(mccsKernel_AllReduce_RING_SIMPLE_SumPostDiv_uint64_t);
/* the reference's bf16 spelling (same handle as ..._PreMulSum_bfloat16) */
MCCS_KERNEL_SYMBOL(mccsKernel_AllReduce_RING_SIMPLE_PreMulSum___nv_bfloat16);

#ifdef __cplusplus
}
#endif

#endif /* MCCS_AMD_KERNELS_AVG_H_ */
