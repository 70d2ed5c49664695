// direct_rs.h — direct ReduceScatter (count-based one-shot and LL) for a fully
// connected node (ring_cfg.h, "Direct ReduceScatter": the slots, the hand-off
// and the reuse argument).
//
// The ring hands a block through n-1 neighbour FIFOs; here every rank writes
// each foreign block of its input once, straight into the owner's slot, and
// every owner reduces its own block: the ring's link bytes in one exchange.
// This is two-shot AllReduce's phases 1 and 2 (direct_kernel.h) on
// ReduceScatter's cut instead of AllReduce's.  What decides a result bit for
// bit is kept: the walk is ring_walk.h's for mccsFuncReduceScatter (a block
// split over the channels, block_chunk_offset), with the channels, thread
// count and rings ring_enqueue would have picked for the call, and channel
// bid's chunk of rank r's block is folded along that channel's ring from r's
// successor: acc = x[idx i+1]; acc = fn(x[idx i+j], acc) for j = 2..n, i = r's
// ring index on ring bid, rounded in T at every step.
// Sum / Prod / Max / Min only, like the other direct kernels.
//
// The launch has direct_kernel's shape (blockIdx.y = rank slot, G workgroups
// of MCCS_DIRECT_THREADS per slot, the same launch guard, prologue, arrival
// count and state words), so these launches alternate freely with every other
// direct launch in the same slots.
//   MCCS_DIRECT_RS_ONE_SHOT (count-based)
//     1. pieces of the n-1 foreign blocks of send, dealt round-robin over the
//        G workgroups -> owner t's one-shot slot [parity seq & 1][sender me],
//        at the element offset within the block; drain / fence as
//        direct_count_out does; one add per owner to its IN_CNT(me);
//     2. wait for E_IN + recvcount on every peer's line; this rank's block,
//        chunk by chunk in the ring's order, into recv (own operand from
//        send + rank * recvcount, the others from the slots).
//   MCCS_DIRECT_RS_LL
//     1. thread-linear over the concatenation of the n-1 foreign blocks:
//        word w of block t -> line w of t's LL slot for this rank;
//     2. thread-linear over the own block's words: poll every peer's line,
//        fold in the ring order of the word's chunk, store.
//     Words are numbered from the block's start; chunk offsets are granule
//     multiples (ring_walk.h: (nthr_ref - WARP_SIZE) x 8 bytes), so no word
//     straddles two chunks.
// In place (recv == send + rank * recvcount) needs no wait on this rank's own
// workgroups, unlike the one-shot AllReduce: phase 1 never reads the own
// block, and phase 2 reads and writes each of its elements through the same
// thread (direct_reduce / the LL word loop map element e to one thread for
// its loads and its store).
// Block t of send starts at t * recvcount elements, so with an odd recvcount
// source and slot disagree modulo 16 and direct_reduce takes its typed path;
// results do not depend on it.
#pragma once
#include "direct_kernel.h"

static_assert(sizeof(mccsDirectArgs) <= 4096, "direct ReduceScatter launch arguments must stay within 4 KiB");

namespace mccs {

// ReduceScatter's walk of one block of a.count elements, in the kernel's 32 bits.
template <int DT>
__device__ __forceinline__ DirectWalk direct_rs_walk(const mccsDirectArgs& a) {
  using T = typename Elem<DT>::T;
  DirectWalk w;
  w.n = a.nranks;
  w.nch = a.nch;
  ring_walk<uint32_t>(w, mccsFuncReduceScatter, (int)a.nranks, (int)a.nch, (int)sizeof(T), (int)a.nthr_ref,
                      (int)a.buff_size, (uint32_t)a.count);
  walk_guard<uint32_t>(w);
  return w;
}

// Ring index of `rank` on channel bid's ring.
__device__ __forceinline__ uint32_t rs_ring_index(const uint8_t (*idx2rank)[MCCS_DIRECT_MAX_RANKS], uint32_t bid,
                                                  uint32_t n, uint32_t rank) {
  uint32_t i = 0;
  while (i + 1 < n && idx2rank[bid][i] != rank) ++i;
  return i;
}

template <int DT, int OP>
__device__ __forceinline__ void direct_rs_body(const mccsDirectArgs& a) {
  using T = typename Elem<DT>::T;
  __shared__ DirectShm sh;
  __shared__ uint64_t need[MCCS_DIRECT_MAX_RANKS];
  const mccsDirectRank& me = a.r[blockIdx.y];
  const int n = (int)a.nranks;
  char* const mine = a.region[me.rank];
  volatile uint32_t* abortFlag = me.abort_flag;
  mccsRingKernelCfg ecfg{};
  ecfg.err_line = me.err_line;
  const DirectWalk w = direct_rs_walk<DT>(a);
  // Prologue and arrival count: direct_body's (the state words in one round
  // trip, the abort flag left to the wait).
  if (threadIdx.x < 64) {
    const uint32_t lane = threadIdx.x;
    uint64_t v = 0;
    if (lane < MCCS_DIRECT_ST_WORDS)
      v = __hip_atomic_load((uint64_t*)(mine + MCCS_DIRECT_STATE) + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (lane == MCCS_DIRECT_ST_LAUNCHES) sh.seq = v + 1;
    if (lane == MCCS_DIRECT_ST_E_IN) sh.e_in = v;
    if (lane == MCCS_DIRECT_ST_WORDS) sh.ok = v == 0;
    if (lane < MCCS_DIRECT_MAX_RANKS) {
      sh.sent[lane] = 0;
      sh.region[lane] = a.region[lane];
    }
    ((uint32_t*)sh.idx2rank)[lane] = ((const uint32_t*)a.idx2rank)[lane];
  }
  uint32_t arrived = 0;
  if (threadIdx.x == 0) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    arrived = __hip_atomic_fetch_add((uint32_t*)(mine + MCCS_DIRECT_DONE), 1u, __ATOMIC_RELAXED,
                                     __HIP_MEMORY_SCOPE_AGENT);
  }
  __syncthreads();
  const uint64_t seq = sh.seq;
  const int64_t esz = (int64_t)sizeof(T);
  const uint32_t G = gridDim.x, bx = blockIdx.x;
  const uint32_t peers = ((1u << n) - 1u) & ~(1u << me.rank);
  const uint32_t piece = a.piece > 0 ? a.piece : 1;
  const uint32_t piece2 = a.piece2 > 0 ? a.piece2 : 1;
  const int64_t oslot = (int64_t)a.oslot_bytes;
  const int64_t obase = MCCS_DIRECT_CTRL_BYTES + (int64_t)MCCS_DIRECT_SLOTS * (int64_t)a.slot_bytes +
                        (int64_t)(seq & 1) * MCCS_DIRECT_MAX_RANKS * oslot;
  // 1. every foreign block to its owner's slot for this rank; the pieces of
  // the n-1 blocks are numbered through and piece p goes to workgroup p % G
  {
    uint32_t base = 0;
    const uint32_t nps = (w.size + piece - 1) / piece;
    for (uint32_t t = 0; t < (uint32_t)n; ++t) {
      if (t == me.rank) continue;
      for (uint32_t j = bx >= base ? bx - base : bx + G - base; j < nps && sh.ok; j += G) {
        const int64_t off = (int64_t)j * piece;
        const int64_t ne = (int64_t)w.size - off < (int64_t)piece ? (int64_t)w.size - off : (int64_t)piece;
        const void* src[MCCS_DIRECT_MAX_RANKS] = {(const T*)me.send + (int64_t)t * w.size + off};
        void* dst[MCCS_DIRECT_MAX_RANKS] = {sh.region[t] + obase + (int64_t)me.rank * oslot + off * esz};
        direct_reduce<DT, OpSum>(src, 1, dst, 1, ne);
        if (threadIdx.x == 0) sh.sent[t] += (uint64_t)ne;
      }
      base += nps;
      while (base >= G) base -= G;
    }
  }
  direct_count_out(sh, a, me, MCCS_DIRECT_IN_CNT(0));
  // The last workgroup to arrive advances the launch count and E_IN (every
  // sender sends every receiver recvcount elements) for the next launch.
  if (threadIdx.x == 0 && arrived + 1 == G) {
    uint64_t* st = (uint64_t*)(mine + MCCS_DIRECT_STATE);
    __hip_atomic_store((uint32_t*)(mine + MCCS_DIRECT_DONE), 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(st + MCCS_DIRECT_ST_E_IN, sh.e_in + (uint64_t)w.size, __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(st + MCCS_DIRECT_ST_LAUNCHES, seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  // 2. this rank's block: channel bid's chunk of every loop, in pieces dealt
  // round-robin, each folded in the order of that channel's ring
  if (threadIdx.x < MCCS_DIRECT_MAX_RANKS) need[threadIdx.x] = sh.e_in + (uint64_t)w.size;
  __syncthreads();
  bool in_seen = false;  // uniform across the workgroup
  const T* const own = (const T*)me.send + (int64_t)me.rank * w.size;
  uint32_t base = 0;
  for (uint32_t g = 0; g < w.size; g += w.loopSize) {
    const uint32_t rcs = real_chunk_size<uint32_t>(w, g, w.nch);
    for (uint32_t bid = 0; bid < w.nch; ++bid) {
      const uint32_t coff = block_chunk_offset<uint32_t>(g, bid, rcs);
      if (coff >= w.size) return;  // every later chunk of the walk is empty
      const uint32_t cne = chunk_nelem(w.size, coff, rcs);
      const uint32_t np = (cne + piece2 - 1) / piece2;
      const uint32_t i = rs_ring_index(sh.idx2rank, bid, (uint32_t)n, me.rank);
      for (uint32_t j = bx >= base ? bx - base : bx + G - base; j < np; j += G) {
        if (!sh.ok) return;
        if (!in_seen) {
          if (!direct_wait(sh, mine, MCCS_DIRECT_IN_CNT(0), peers, need, abortFlag, a, ecfg)) return;
          in_seen = true;
        }
        const uint32_t s = j * piece2;
        const int64_t off = (int64_t)(coff + s);
        const int64_t ne = (int64_t)(cne - s < piece2 ? cne - s : piece2);
        const void* src[MCCS_DIRECT_MAX_RANKS];
        void* dst[MCCS_DIRECT_MAX_RANKS] = {(T*)me.recv + off};
#pragma unroll
        for (int k = 0; k < MCCS_DIRECT_MAX_RANKS; ++k) {
          src[k] = nullptr;
          if (k < n) {
            uint32_t idx = i + 1 + (uint32_t)k;
            idx = idx >= (uint32_t)n ? idx - (uint32_t)n : idx;
            const uint32_t q = sh.idx2rank[bid][idx];
            src[k] = q == me.rank ? (const void*)(own + off) : (const void*)(mine + obase + (int64_t)q * oslot + off * esz);
          }
        }
        direct_reduce<DT, OP>(src, n, dst, 1, ne);
      }
      base += np;
      while (base >= G) base -= G;
    }
  }
}

template <int DT, int OP>
__device__ __forceinline__ void direct_rs_ll_body(const mccsDirectArgs& a) {
  using T = typename Elem<DT>::T;
  constexpr uint32_t EPW = 8 / sizeof(T);
  __shared__ uint64_t s_seq;
  __shared__ char* s_region[MCCS_DIRECT_MAX_RANKS];
  __shared__ uint8_t s_idx2rank[MCCS_MAX_NCHANNELS][MCCS_DIRECT_MAX_RANKS];
  const mccsDirectRank& me = a.r[blockIdx.y];
  const uint32_t n = a.nranks, rank = me.rank;
  char* const mine = a.region[rank];
  volatile uint32_t* abortFlag = me.abort_flag;
  mccsRingKernelCfg ecfg{};
  ecfg.err_line = me.err_line;
  const DirectWalk w = direct_rs_walk<DT>(a);
  const uint32_t nwords = (uint32_t)(((uint64_t)w.size * sizeof(T) + 7) / 8);  // of one block
  const uint32_t stride = gridDim.x * blockDim.x;
  const uint32_t gtid = blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t bbytes = (int64_t)w.size * (int64_t)sizeof(T);
  const char* in = (const char*)me.send;
  char* out = (char*)me.recv;
  const char* const own_blk = in + (int64_t)rank * bbytes;
  const bool own_al = ((uintptr_t)own_blk & 7) == 0, out_al = ((uintptr_t)out & 7) == 0;
  if (threadIdx.x == 0)
    s_seq = __hip_atomic_load((uint64_t*)(mine + MCCS_DIRECT_STATE) + MCCS_DIRECT_ST_LAUNCHES, __ATOMIC_RELAXED,
                              __HIP_MEMORY_SCOPE_AGENT) + 1;
  if (threadIdx.x < MCCS_DIRECT_MAX_RANKS) s_region[threadIdx.x] = a.region[threadIdx.x];
  if (threadIdx.x < 64) ((uint32_t*)s_idx2rank)[threadIdx.x] = ((const uint32_t*)a.idx2rank)[threadIdx.x];
  __syncthreads();
  // every workgroup has read the launch count once it arrives; the last one
  // to arrive advances it (after phase 1)
  uint32_t arrived = 0;
  if (threadIdx.x == 0)
    arrived = __hip_atomic_fetch_add((uint32_t*)(mine + MCCS_DIRECT_DONE), 1u, __ATOMIC_RELAXED,
                                     __HIP_MEMORY_SCOPE_AGENT);
  const uint64_t seq = s_seq;
  const uint32_t seq32 = 1u + (uint32_t)(seq % 0xffffffffull);  // never 0: a zeroed line is never valid
  const uint64_t flag = (uint64_t)seq32 << 32;
  const int64_t lslot = (int64_t)a.ll_slot_bytes;
  const int64_t llbase = MCCS_DIRECT_CTRL_BYTES + (int64_t)MCCS_DIRECT_SLOTS * (int64_t)a.slot_bytes +
                         2 * (int64_t)MCCS_DIRECT_MAX_RANKS * (int64_t)a.oslot_bytes +
                         (int64_t)(seq & 1) * MCCS_DIRECT_MAX_RANKS * lslot;
  // 1. word wd of foreign block t -> line wd of t's slot for this rank
  // ((n - 1) x nwords <= 7 x 2^17 with ll_bytes <= 1 MiB: the 32-bit index cannot wrap)
  const uint32_t total = (n - 1) * nwords;
  for (uint32_t i = gtid; i < total; i += stride) {
    const uint32_t b = i / nwords, wd = i - b * nwords;
    const uint32_t t = b < rank ? b : b + 1;
    const char* blk = in + (int64_t)t * bbytes;
    const uint64_t v = ll_load_word<T>(blk, wd, w.size, ((uintptr_t)blk & 7) == 0);
    uint64_t* p = (uint64_t*)(s_region[t] + llbase + (int64_t)rank * lslot + (int64_t)wd * 16);
    __hip_atomic_store(p, flag | (v & 0xffffffffull), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(p + 1, flag | (v >> 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
  if (threadIdx.x == 0 && arrived + 1 == gridDim.x) {
    __hip_atomic_store((uint32_t*)(mine + MCCS_DIRECT_DONE), 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store((uint64_t*)(mine + MCCS_DIRECT_STATE) + MCCS_DIRECT_ST_LAUNCHES, seq, __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
  }
  // 2. the own block's words: poll every peer's line, fold in the ring order
  // of the word's chunk (word 0 exists with recvcount >= 1: every ordered pair
  // hands off in every launch)
  const uint32_t peers = ((1u << n) - 1u) & ~(1u << rank);
  const uint64_t t0 = __builtin_amdgcn_s_memrealtime();
  for (uint32_t wd = gtid; wd < nwords; wd += stride) {
    const uint32_t e = wd * EPW;
    const uint32_t g = e / w.loopSize * w.loopSize;
    const uint32_t bid = (e - g) / real_chunk_size<uint32_t>(w, g, w.nch);  // block_chunk_offset's part holding e
    const uint32_t i = rs_ring_index(s_idx2rank, bid, n, rank);
    const uint64_t own = ll_load_word<T>(own_blk, wd, w.size, own_al);
    const char* lb = mine + llbase + (int64_t)wd * 16;
    uint64_t h0[MCCS_DIRECT_MAX_RANKS], h1[MCCS_DIRECT_MAX_RANKS];
    uint32_t pending = peers, spins = 0;
    for (;;) {
#pragma unroll
      for (uint32_t t = 0; t < MCCS_DIRECT_MAX_RANKS; ++t)
        if ((pending >> t) & 1u) {
          const uint64_t* p = (const uint64_t*)(lb + (int64_t)t * lslot);
          h0[t] = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
          h1[t] = __hip_atomic_load(p + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
#pragma unroll
      for (uint32_t t = 0; t < MCCS_DIRECT_MAX_RANKS; ++t)
        if (((pending >> t) & 1u) && (uint32_t)(h0[t] >> 32) == seq32 && (uint32_t)(h1[t] >> 32) == seq32)
          pending &= ~(1u << t);
      if (!pending) break;
      if (++spins % 64 == 0) {
        const bool ab = abort_raised(abortFlag);
        const bool to = !ab && a.timeout_ticks && __builtin_amdgcn_s_memrealtime() - t0 > a.timeout_ticks;
        if (ab || to) {
          raise_error(abortFlag, ecfg, ab ? MCCS_ERR_ABORTED : MCCS_ERR_TIMEOUT);
          return;
        }
      }
      __builtin_amdgcn_s_sleep(MCCS_POLL_SLEEP);
    }
    // acc = x[idx i+1]; acc = fn(x[idx i+j], acc); the last operand is this rank's own word
    u32x4 acc{};
#pragma unroll
    for (uint32_t j = 0; j < MCCS_DIRECT_MAX_RANKS; ++j)
      if (j < n) {
        uint32_t idx = i + 1 + j;
        idx = idx >= n ? idx - n : idx;
        const uint32_t q = s_idx2rank[bid][idx];
        uint64_t v = own;
#pragma unroll
        for (uint32_t t = 0; t < MCCS_DIRECT_MAX_RANKS; ++t)
          if (t == q && t != rank) v = (h0[t] & 0xffffffffull) | (h1[t] << 32);
        acc = j == 0 ? ll_pack(v) : pack_op<DT, OP>(ll_pack(v), acc);
      }
    ll_store_word<T>(out, wd, w.size, out_al, (uint64_t)acc.x | ((uint64_t)acc.y << 32));
  }
}

}  // namespace mccs
