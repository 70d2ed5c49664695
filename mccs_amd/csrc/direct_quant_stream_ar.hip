// direct_quant_stream_ar.hip — the block-scaled FP8 streamed AllReduce kernels
// (direct_quant_stream_ar.h), one per (fp16 | bf16) x (Sum | PreMulSum), in a
// translation unit of their own, built like direct_wide_stream_ar.hip without
// packed fp32 instructions: every other kernel stays as it is.
#include "direct_quant_stream_ar.h"

namespace mccs {

template <int DT, int PRE>
__global__ void __launch_bounds__(MCCS_DIRECT_THREADS) direct_quant_stream_ar_kernel(mccsDirectArgs a) {
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
  direct_quant_stream_ar_body<DT, PRE != 0>(a);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0 && s_guard.g) guard_release(s_guard.g, gridDim.x);
}

// fp16 / bf16 x Sum / PreMulSum; anything else has no streamed quant kernel.
const void* direct_quant_stream_ar_kernel_ptr(int dtype, int op) {
  const bool pre = op == OpPreMulSum;
  if (op != OpSum && !pre) return nullptr;
  switch (dtype) {
    case mccsFloat16:
      return pre ? (const void*)&direct_quant_stream_ar_kernel<mccsFloat16, 1>
                 : (const void*)&direct_quant_stream_ar_kernel<mccsFloat16, 0>;
    case mccsBfloat16:
      return pre ? (const void*)&direct_quant_stream_ar_kernel<mccsBfloat16, 1>
                 : (const void*)&direct_quant_stream_ar_kernel<mccsBfloat16, 0>;
    default: return nullptr;
  }
}

}  // namespace mccs
