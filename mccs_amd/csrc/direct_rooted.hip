// direct_rooted.hip — the direct Reduce kernels (direct_rooted.h), one per
// (dtype, op), in a translation unit of their own: the instantiations of
// direct.hip and direct_rs.hip stay as they are.  The one direct Broadcast
// kernel is in direct_rooted_bc.hip.
#include "direct_rooted.h"

namespace mccs {

template <int DT, int OP>
__global__ void __launch_bounds__(MCCS_DIRECT_THREADS) direct_rd_kernel(mccsDirectArgs a) {
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
  if (a.mode == MCCS_DIRECT_RD_LL) direct_rd_ll_body<DT, OP>(a);
  else direct_rd_body<DT, OP>(a);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0 && s_guard.g) guard_release(s_guard.g, gridDim.x);
}

template <int OP>
static const void* direct_rd_for_op(int dtype) {
  switch (dtype) {
    case mccsInt8: return (const void*)&direct_rd_kernel<mccsInt8, OP>;
    case mccsUint8: return (const void*)&direct_rd_kernel<mccsUint8, OP>;
    case mccsInt32: return (const void*)&direct_rd_kernel<mccsInt32, OP>;
    case mccsUint32: return (const void*)&direct_rd_kernel<mccsUint32, OP>;
    case mccsInt64: return (const void*)&direct_rd_kernel<mccsInt64, OP>;
    case mccsUint64: return (const void*)&direct_rd_kernel<mccsUint64, OP>;
    case mccsFloat16: return (const void*)&direct_rd_kernel<mccsFloat16, OP>;
    case mccsFloat32: return (const void*)&direct_rd_kernel<mccsFloat32, OP>;
    case mccsFloat64: return (const void*)&direct_rd_kernel<mccsFloat64, OP>;
    case mccsBfloat16: return (const void*)&direct_rd_kernel<mccsBfloat16, OP>;
    default: return nullptr;
  }
}

const void* direct_rd_kernel_ptr(int dtype, int op) {
  switch (op) {
    case OpSum: return direct_rd_for_op<OpSum>(dtype);
    case OpProd: return direct_rd_for_op<OpProd>(dtype);
    case OpMax: return direct_rd_for_op<OpMax>(dtype);
    case OpMin: return direct_rd_for_op<OpMin>(dtype);
    default: return nullptr;
  }
}

}  // namespace mccs
