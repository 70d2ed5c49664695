// direct_quant_ag.hip — the block-scaled FP8 streamed AllGather kernels
// (direct_quant_ag.h), one per fp16 | bf16 (there is no op and no scalar), in a
// translation unit of their own, built like direct_quant_stream.hip without
// packed fp32 instructions: every other kernel stays as it is.
#include "direct_quant_ag.h"

namespace mccs {

template <int DT>
__global__ void __launch_bounds__(MCCS_DIRECT_THREADS) direct_quant_ag_kernel(mccsDirectArgs a) {
  // Launch guard, taken as direct_kernel takes it: before the body reads the
  // control block's launch count and running totals; the rank slots' fields
  // are read where the kernel arguments live.
  __shared__ GuardSlot s_guard;
  if (threadIdx.x == 0) {
    mccsLaunchGuard* g = nullptr;
    int ok = 1;
    if (!a.no_guard) {
      const uintptr_t ka = (uintptr_t)__builtin_amdgcn_kernarg_segment_ptr();
      const mccsDirectRank* ranks = (const mccsDirectRank*)(ka + offsetof(mccsDirectArgs, r));
      GuardWait w{};
      w.abortFlagRef = (uint32_t* const*)&ranks[blockIdx.y].abort_flag;
      w.timeout = a.timeout_ticks;
      w.err_line = ranks[blockIdx.y].err_line;
      g = comm_guard(ranks[blockIdx.y].comm);
      ok = guard_acquire([&](int k) { return comm_guard(ranks[k].comm); }, (int)gridDim.y, (int)blockIdx.y,
                         a.guard_order, launch_token(), blockIdx.x == 0 && blockIdx.y == 0, w);
    }
    s_guard.g = ok ? g : nullptr;
    s_guard.ok = ok;
  }
  __syncthreads();
  if (!s_guard.ok) return;
  direct_quant_ag_body<DT>(a);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0 && s_guard.g) guard_release(s_guard.g, gridDim.x);
}

// fp16 / bf16; anything else has no quantised AllGather kernel.
const void* direct_quant_ag_kernel_ptr(int dtype) {
  switch (dtype) {
    case mccsFloat16: return (const void*)&direct_quant_ag_kernel<mccsFloat16>;
    case mccsBfloat16: return (const void*)&direct_quant_ag_kernel<mccsBfloat16>;
    default: return nullptr;
  }
}

}  // namespace mccs
