// direct_a2a.hip — the LL AllToAll / AllToAllv / AllToAllvDev kernel
// (direct_a2a.h), in a translation unit of its own: the forty direct_kernel
// instantiations of direct.hip stay as they are.
#include "direct_a2a.h"

namespace mccs {

__global__ void __launch_bounds__(MCCS_DIRECT_THREADS) direct_a2a_ll_kernel(mccsA2aLLArgs a) {
  // Launch guard, taken as direct_kernel takes it: before the body reads the
  // control block's launch count; the rank slots' fields are read where the
  // kernel arguments live.
  __shared__ GuardSlot s_guard;
  const mccsA2aLLArgs* ap = (const mccsA2aLLArgs*)(uintptr_t)__builtin_amdgcn_kernarg_segment_ptr();
  if (threadIdx.x == 0) {
    mccsLaunchGuard* g = nullptr;
    int ok = 1;
    if (!a.no_guard) {
      const mccsA2aLLRank* ranks = ap->r;
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
  direct_a2a_ll_body(a, ap);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0 && s_guard.g) guard_release(s_guard.g, gridDim.x);
}

const void* a2a_ll_kernel_ptr() { return (const void*)&direct_a2a_ll_kernel; }

}  // namespace mccs
