// direct_rooted_bc.hip — the direct Broadcast kernel (direct_rooted.h): bytes,
// so one kernel, as direct_a2a is one kernel.
#include "direct_rooted.h"

namespace mccs {

__global__ void __launch_bounds__(MCCS_DIRECT_THREADS) direct_bc_kernel(mccsDirectArgs a) {
  // Launch guard, taken as direct_kernel takes it.
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
  if (a.mode == MCCS_DIRECT_BC_LL) direct_bc_ll_body(a);
  else direct_bc_body(a);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0 && s_guard.g) guard_release(s_guard.g, gridDim.x);
}

const void* direct_bc_kernel_ptr() { return (const void*)&direct_bc_kernel; }

}  // namespace mccs
