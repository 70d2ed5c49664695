// direct_a2a.h — LL AllToAll / AllToAllv / AllToAllvDev (ring_cfg.h, "LL
// AllToAll": the slot layout and why every pair's header goes out in every
// launch).
//
// One byte-typed kernel for the three calls: a uniform AllToAll is the v
// exchange with equal counts and packed displacements, a Dev call reads its
// four rows from the size table when it runs.  The launch has the shape of
// the LL body of direct_kernel.h (blockIdx.y = rank slot, G workgroups of
// MCCS_DIRECT_THREADS per slot, the same launch guard, launch count, parity
// and line flag), so these launches alternate freely with LL AllReduce and LL
// AllGather in the same slots.
//   1. send: every peer's block as flag-carrying lines into that peer's slot
//      for this rank, behind a header line; the rank's own block straight from
//      send to recv;
//   2. receive: poll every peer's header and the lines of recvcounts[s] bytes,
//      store the words at recv + rdispls[s].
// Both phases deal their words thread-linearly over the CONCATENATION of all
// peers' blocks (a prefix sum of at most 8 entries in LDS), so seven blocks of
// 1 KiB fill one workgroup in one pass.  Lines are polled one by one, so the
// sender's and the receiver's mappings are independent and ranks may run
// different G.
#pragma once
#include "direct_kernel.h"

namespace mccs {

constexpr int kA2aLLPoll = 8;  // lines a thread keeps in flight per poll (the LL body polls up to 7 peers' at once)

struct A2aLLShm {
  uint64_t seq;
  char* region[MCCS_DIRECT_MAX_RANKS];
  uint64_t rows[MCCS_A2A_LL_ROWS][MCCS_DIRECT_MAX_RANKS];  // the call's rows, counts clamped to the capacity
  uint32_t spre[MCCS_DIRECT_MAX_RANKS + 1];  // words before peer t's block on the send side (own block included)
  uint32_t rpre[MCCS_DIRECT_MAX_RANKS + 1];  // words before peer s's block on the receive side (own block: none)
};

// The block holding word i: pre[t] <= i < pre[t + 1] (empty blocks are skipped).
__device__ __forceinline__ uint32_t a2a_ll_block(const uint32_t* pre, uint32_t n, uint32_t i) {
  uint32_t t = 0;
  while (t + 1 < n && i >= pre[t + 1]) ++t;
  return t;
}

// Polls the lines p[u] of `pending` until each carries seq32 in both halves;
// every pending line's two loads are issued before any flag is looked at.
// Bounded by the abort flag and the watchdog like the LL body; false: given up.
template <int U>
__device__ __forceinline__ bool a2a_ll_wait(const uint64_t* const (&p)[U], uint64_t (&h0)[U], uint64_t (&h1)[U],
                                            uint32_t pending, uint32_t seq32, volatile uint32_t* abortFlag,
                                            const mccsRingKernelCfg& ecfg, uint64_t timeout_ticks, uint64_t t0) {
  uint32_t spins = 0;
  for (;;) {
#pragma unroll
    for (int u = 0; u < U; ++u)
      if ((pending >> u) & 1u) {
        h0[u] = __hip_atomic_load(p[u], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        h1[u] = __hip_atomic_load(p[u] + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      }
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (((pending >> u) & 1u) && (uint32_t)(h0[u] >> 32) == seq32 && (uint32_t)(h1[u] >> 32) == seq32)
        pending &= ~(1u << u);
    if (!pending) return true;
    if (++spins % 64 == 0) {
      const bool ab = abort_raised(abortFlag);
      const bool to = !ab && timeout_ticks && __builtin_amdgcn_s_memrealtime() - t0 > timeout_ticks;
      if (ab || to) {
        raise_error(abortFlag, ecfg, ab ? MCCS_ERR_ABORTED : MCCS_ERR_TIMEOUT);
        return false;
      }
    }
    __builtin_amdgcn_s_sleep(MCCS_POLL_SLEEP);
  }
}

// `a`: the launch's scalars; `ap`: the same arguments where they live (arrays
// are indexed there: a dynamic index into the by-value parameter would copy
// it to scratch).
__device__ __forceinline__ void direct_a2a_ll_body(const mccsA2aLLArgs& a, const mccsA2aLLArgs* ap) {
  __shared__ A2aLLShm sh;
  const mccsA2aLLRank* me = &ap->r[blockIdx.y];
  const uint32_t n = a.nranks, rank = me->rank;
  volatile uint32_t* abortFlag = me->abort_flag;
  mccsRingKernelCfg ecfg{};
  ecfg.err_line = me->err_line;
  const char* send = (const char*)me->send;
  char* recv = (char*)me->recv;
  const int64_t lslot = (int64_t)a.ll_slot_bytes;
  const uint32_t cap = (uint32_t)MCCS_A2A_LL_CAP(a.ll_slot_bytes);
  // The four rows into LDS, one lane per word and one round trip: from the
  // arguments, or (Dev) from the size table as it stands now.  Counts are
  // clamped to the slot's capacity on both sides, so a table (or a caller)
  // that breaks the contract truncates bytes and never writes past a slot.
  if (threadIdx.x < MCCS_A2A_LL_ROWS * MCCS_DIRECT_MAX_RANKS) {
    const uint32_t row = threadIdx.x / MCCS_DIRECT_MAX_RANKS, p = threadIdx.x % MCCS_DIRECT_MAX_RANKS;
    uint64_t v = 0;
    if (p < n) v = a.table_mode ? ld_flag(me->table + a2avd_index((int)row, (int)n, (int)p)) : me->rows[row][p];
    if ((row == kA2AvdSendCounts || row == kA2AvdRecvCounts) && v > cap) v = cap;
    sh.rows[row][p] = v;
    if (threadIdx.x < MCCS_DIRECT_MAX_RANKS) sh.region[threadIdx.x] = ap->region[threadIdx.x];
  }
  char* const mine = ap->region[rank];
  if (threadIdx.x == 0)
    sh.seq = __hip_atomic_load((uint64_t*)(mine + MCCS_DIRECT_STATE) + MCCS_DIRECT_ST_LAUNCHES, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT) + 1;
  __syncthreads();
  if (threadIdx.x <= MCCS_DIRECT_MAX_RANKS) {
    uint32_t s = 0, r = 0;
    for (uint32_t t = 0; t < threadIdx.x && t < n; ++t) {
      s += ((uint32_t)sh.rows[kA2AvdSendCounts][t] + 7) / 8;
      if (t != rank) r += ((uint32_t)sh.rows[kA2AvdRecvCounts][t] + 7) / 8;
    }
    sh.spre[threadIdx.x] = s;
    sh.rpre[threadIdx.x] = r;
  }
  // every workgroup has read the launch count once it arrives; the last one
  // to arrive advances it (after phase 1)
  uint32_t arrived = 0;
  if (threadIdx.x == 0)
    arrived = __hip_atomic_fetch_add((uint32_t*)(mine + MCCS_DIRECT_DONE), 1u, __ATOMIC_RELAXED,
                                     __HIP_MEMORY_SCOPE_AGENT);
  __syncthreads();
  const uint64_t seq = sh.seq;
  const uint32_t seq32 = 1u + (uint32_t)(seq % 0xffffffffull);  // never 0: a zeroed line is never valid
  const uint64_t flag = (uint64_t)seq32 << 32;
  const int64_t llbase = MCCS_DIRECT_CTRL_BYTES + (int64_t)MCCS_DIRECT_SLOTS * (int64_t)a.slot_bytes +
                         2 * (int64_t)MCCS_DIRECT_MAX_RANKS * (int64_t)a.oslot_bytes +
                         (int64_t)(seq & 1) * MCCS_DIRECT_MAX_RANKS * lslot;
  const uint32_t stride = gridDim.x * blockDim.x;
  const uint32_t gtid = blockIdx.x * blockDim.x + threadIdx.x;
  auto put_line = [&](uint32_t t, uint32_t line, uint64_t v) {
    uint64_t* p = (uint64_t*)(sh.region[t] + llbase + (int64_t)rank * lslot + (int64_t)line * 16);
    __hip_atomic_store(p, flag | (v & 0xffffffffull), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(p + 1, flag | (v >> 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  };
  // 1. the header of every peer (global thread t writes peer t's), then every
  // word of every block: to the peer's slot, or (own block) to its place
  if (gtid < n && gtid != rank) put_line(gtid, 0, sh.rows[kA2AvdSendCounts][gtid]);
  const uint32_t stot = sh.spre[n];
  for (uint32_t i = gtid; i < stot; i += stride) {
    const uint32_t t = a2a_ll_block(sh.spre, n, i), w = i - sh.spre[t];
    const uint32_t cnt = (uint32_t)sh.rows[kA2AvdSendCounts][t];
    const char* src = send + sh.rows[kA2AvdSendDispls][t];
    const uint64_t v = ll_load_word<int8_t>(src, w, cnt, ((uintptr_t)src & 7) == 0);
    if (t == rank) {
      char* dst = recv + sh.rows[kA2AvdRecvDispls][t];
      ll_store_word<int8_t>(dst, w, cnt, ((uintptr_t)dst & 7) == 0, v);
    } else {
      put_line(t, 1 + w, v);
    }
  }
  if (threadIdx.x == 0 && arrived + 1 == gridDim.x) {
    __hip_atomic_store((uint32_t*)(mine + MCCS_DIRECT_DONE), 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store((uint64_t*)(mine + MCCS_DIRECT_STATE) + MCCS_DIRECT_ST_LAUNCHES, seq, __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
  }
  // 2. every peer's header (global thread s waits for peer s's: no launch
  // ends before every pair has handed off), then the lines of every block
  const uint64_t t0 = __builtin_amdgcn_s_memrealtime();
  const char* lb = mine + llbase;
  if (gtid < n && gtid != rank) {
    const uint64_t* const p[1] = {(const uint64_t*)(lb + (int64_t)gtid * lslot)};
    uint64_t h0[1], h1[1];
    if (!a2a_ll_wait<1>(p, h0, h1, 1u, seq32, abortFlag, ecfg, a.timeout_ticks, t0)) return;
  }
  const uint32_t rtot = sh.rpre[n];
  for (uint32_t i0 = gtid; i0 < rtot; i0 += stride * kA2aLLPoll) {
    const uint64_t* p[kA2aLLPoll];
    uint64_t h0[kA2aLLPoll], h1[kA2aLLPoll];
    uint32_t blk[kA2aLLPoll], wd[kA2aLLPoll], pending = 0;
#pragma unroll
    for (int u = 0; u < kA2aLLPoll; ++u) {
      const uint32_t i = i0 + (uint32_t)u * stride;
      p[u] = nullptr;
      blk[u] = wd[u] = 0;
      if (i < rtot) {  // (rtot < 2^20 words and stride <= 2^21: the 32-bit index cannot wrap)
        blk[u] = a2a_ll_block(sh.rpre, n, i);
        wd[u] = i - sh.rpre[blk[u]];
        p[u] = (const uint64_t*)(lb + (int64_t)blk[u] * lslot + (int64_t)(1 + wd[u]) * 16);
        pending |= 1u << u;
      }
    }
    const uint32_t valid = pending;
    if (!a2a_ll_wait<kA2aLLPoll>(p, h0, h1, pending, seq32, abortFlag, ecfg, a.timeout_ticks, t0)) return;
#pragma unroll
    for (int u = 0; u < kA2aLLPoll; ++u)
      if ((valid >> u) & 1u) {
        char* dst = recv + sh.rows[kA2AvdRecvDispls][blk[u]];
        ll_store_word<int8_t>(dst, wd[u], (uint32_t)sh.rows[kA2AvdRecvCounts][blk[u]], ((uintptr_t)dst & 7) == 0,
                              (h0[u] & 0xffffffffull) | (h1[u] << 32));
      }
  }
}

}  // namespace mccs
