// direct_wide_rs.hip — the wide-accumulate direct ReduceScatter and Reduce
// kernels (direct_wide_rs.h), one per function x (fp16 | bf16) x (Sum |
// PreMulSum), in a translation unit of their own, built like direct_wide.hip
// without packed fp32 instructions: every other kernel stays as it is.
#include "direct_wide_rs.h"

namespace mccs {

// The launch guard around a body, taken as direct_kernel takes it: before the
// body reads the control block's launch count and running totals; the rank
// slots' fields are read where the kernel arguments live.
template <typename Body>
__device__ __forceinline__ void wide_guarded(const mccsDirectArgs& a, Body&& body) {
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
  body();
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0 && s_guard.g) guard_release(s_guard.g, gridDim.x);
}

template <int DT, int PRE>
__global__ void __launch_bounds__(MCCS_DIRECT_THREADS) direct_wide_rs_kernel(mccsDirectArgs a) {
  wide_guarded(a, [&]() {
    if (a.mode == MCCS_DIRECT_WIDE_RS_LL) direct_wide_own_ll_body<DT, PRE != 0, false>(a);
    else direct_wide_own_body<DT, PRE != 0, false>(a);
  });
}

template <int DT, int PRE>
__global__ void __launch_bounds__(MCCS_DIRECT_THREADS) direct_wide_rd_kernel(mccsDirectArgs a) {
  wide_guarded(a, [&]() {
    if (a.mode == MCCS_DIRECT_WIDE_RD_LL) direct_wide_own_ll_body<DT, PRE != 0, true>(a);
    else direct_wide_own_body<DT, PRE != 0, true>(a);
  });
}

// fp16 / bf16 x Sum / PreMulSum; anything else has no wide kernel.
const void* direct_wide_rs_kernel_ptr(int dtype, int op) {
  const bool pre = op == OpPreMulSum;
  if (op != OpSum && !pre) return nullptr;
  switch (dtype) {
    case mccsFloat16:
      return pre ? (const void*)&direct_wide_rs_kernel<mccsFloat16, 1> : (const void*)&direct_wide_rs_kernel<mccsFloat16, 0>;
    case mccsBfloat16:
      return pre ? (const void*)&direct_wide_rs_kernel<mccsBfloat16, 1>
                 : (const void*)&direct_wide_rs_kernel<mccsBfloat16, 0>;
    default: return nullptr;
  }
}

const void* direct_wide_rd_kernel_ptr(int dtype, int op) {
  const bool pre = op == OpPreMulSum;
  if (op != OpSum && !pre) return nullptr;
  switch (dtype) {
    case mccsFloat16:
      return pre ? (const void*)&direct_wide_rd_kernel<mccsFloat16, 1> : (const void*)&direct_wide_rd_kernel<mccsFloat16, 0>;
    case mccsBfloat16:
      return pre ? (const void*)&direct_wide_rd_kernel<mccsBfloat16, 1>
                 : (const void*)&direct_wide_rd_kernel<mccsBfloat16, 0>;
    default: return nullptr;
  }
}

}  // namespace mccs
