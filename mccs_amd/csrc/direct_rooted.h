// direct_rooted.h — direct Broadcast and Reduce (count-based one-shot and LL)
// for a fully connected node (ring_cfg.h, "Direct Broadcast and Reduce": the
// hand-off rule of a rooted launch and why the reuse argument survives it).
//
// The ring runs a rooted call as a chain: n-1 serial FIFO hand-offs, the two
// ends idle.  Here the root writes its bytes once into every peer's slot
// (Broadcast), or every rank writes its input once into the root's slot and
// the root folds them (Reduce): one exchange.  Reduce is direct_rs.h's
// owner-side fold with "owner" read as "root" and the whole buffer as the one
// block: the walk is ring_walk.h's for mccsFuncReduce (the buffer cut like one
// ReduceScatter block), with the channels, thread count and rings ring_enqueue
// would have picked for the call, and channel bid's chunk is folded along that
// channel's ring from the root's successor: acc = x[idx i+1];
// acc = fn(x[idx i+j], acc) for j = 2..n, i = the root's ring index on ring
// bid, rounded in T at every step.  Sum / Prod / Max / Min only.  Broadcast
// moves bytes (T = int8, like direct_a2a's one kernel) and needs no walk.
//
// The launch has direct_kernel's shape (blockIdx.y = rank slot, G workgroups
// of MCCS_DIRECT_THREADS per slot, the same launch guard, prologue, arrival
// count and state words, slot parity seq & 1, no new slot), so these launches
// alternate freely with every other direct launch in the same slots.  The
// root is a.root, one for all fused rank slots (ranks of one communicator).
//
// THE RULE (ring_cfg.h): a rooted call moves data on n-1 of the n(n-1)
// ordered pairs only, but EVERY ordered pair hands off in EVERY launch, with
// the launch's common amount (count elements / nbytes):
//   count-based: every rank adds the amount to IN_CNT(self) of every peer --
//     where it sent data, its workgroups' pieces add up to it; where it sent
//     none, workgroup 0 adds it alone; E_IN advances by it on every rank; and
//     workgroup 0 of every rank, root or not, waits for E_IN + amount on every
//     peer's line before the kernel ends;
//   LL: every rank writes line 0, flagged with this launch's seq, into every
//     peer's LL slot for itself (a dummy word where the pair carries no data),
//     and global thread 0 of every rank polls line 0 of every peer's slot.
//
//   MCCS_DIRECT_RD_ONE_SHOT  non-root: pieces of send, dealt round-robin over
//     the G workgroups -> the root's one-shot slot [parity][sender], at the
//     element offset.  Root: direct_rs_body's phase 2 over the whole buffer
//     (own operand from send, the others from the slots) into recv.
//   MCCS_DIRECT_RD_LL        non-root: word w of send -> line w of the root's
//     LL slot for the sender.  Root: polls and folds as direct_rs_ll_body.
//     Chunk offsets are granule multiples, so no word straddles two chunks.
//   MCCS_DIRECT_BC_ONE_SHOT  root: pieces of the n-1 copies of send, dealt
//     round-robin -> peer t's one-shot slot [parity][root]; out of place, send
//     -> recv locally.  Non-root: waits, then slot -> recv.
//   MCCS_DIRECT_BC_LL        root: every word of send as a flagged line into
//     every peer's LL slot for the root (out of place: and into recv).
//     Non-root: polls each line, stores the word (ll_load_word / ll_store_word
//     with T = int8: any length and alignment).
// In place on the root (recv == send) needs no extra wait in Reduce, for
// direct_rs.h's reason: element e is loaded and stored by one thread.  A
// non-root's recv (Reduce) and send (Broadcast) are never touched: NULL is fine.
#pragma once
#include "direct_rs.h"

namespace mccs {

// Reduce's walk of the whole buffer of a.count elements, in the kernel's 32 bits.
template <int DT>
__device__ __forceinline__ DirectWalk direct_rd_walk(const mccsDirectArgs& a) {
  using T = typename Elem<DT>::T;
  DirectWalk w;
  w.n = a.nranks;
  w.nch = a.nch;
  ring_walk<uint32_t>(w, mccsFuncReduce, (int)a.nranks, (int)a.nch, (int)sizeof(T), (int)a.nthr_ref,
                      (int)a.buff_size, (uint32_t)a.count);
  walk_guard<uint32_t>(w);
  return w;
}

// The count-based prologue and arrival count: direct_rs_body's.
__device__ __forceinline__ uint32_t rooted_prologue(DirectShm& sh, const mccsDirectArgs& a, char* mine) {
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
  return arrived;
}

// The last workgroup to arrive advances the launch count and E_IN by the
// launch's common amount (the rule: every sender adds it on every receiver).
__device__ __forceinline__ void rooted_advance(const DirectShm& sh, char* mine, uint32_t arrived, uint64_t amount) {
  if (threadIdx.x == 0 && arrived + 1 == gridDim.x) {
    uint64_t* st = (uint64_t*)(mine + MCCS_DIRECT_STATE);
    __hip_atomic_store((uint32_t*)(mine + MCCS_DIRECT_DONE), 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(st + MCCS_DIRECT_ST_E_IN, sh.e_in + amount, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(st + MCCS_DIRECT_ST_LAUNCHES, sh.seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

template <int DT, int OP>
__device__ __forceinline__ void direct_rd_body(const mccsDirectArgs& a) {
  using T = typename Elem<DT>::T;
  __shared__ DirectShm sh;
  __shared__ uint64_t need[MCCS_DIRECT_MAX_RANKS];
  const mccsDirectRank& me = a.r[blockIdx.y];
  const int n = (int)a.nranks;
  const uint32_t root = a.root;
  const bool is_root = me.rank == root;
  char* const mine = a.region[me.rank];
  volatile uint32_t* abortFlag = me.abort_flag;
  mccsRingKernelCfg ecfg{};
  ecfg.err_line = me.err_line;
  const DirectWalk w = direct_rd_walk<DT>(a);
  const uint32_t arrived = rooted_prologue(sh, a, mine);
  const uint64_t seq = sh.seq;
  const int64_t esz = (int64_t)sizeof(T);
  const uint32_t G = gridDim.x, bx = blockIdx.x;
  const uint32_t peers = ((1u << n) - 1u) & ~(1u << me.rank);
  const uint32_t piece = a.piece > 0 ? a.piece : 1;
  const uint32_t piece2 = a.piece2 > 0 ? a.piece2 : 1;
  const int64_t oslot = (int64_t)a.oslot_bytes;
  const int64_t obase = MCCS_DIRECT_CTRL_BYTES + (int64_t)MCCS_DIRECT_SLOTS * (int64_t)a.slot_bytes +
                        (int64_t)(seq & 1) * MCCS_DIRECT_MAX_RANKS * oslot;
  // 1. a non-root's input to the root's slot for this rank, piece p to workgroup p % G
  if (!is_root) {
    const uint32_t nps = (w.size + piece - 1) / piece;
    for (uint32_t j = bx; j < nps && sh.ok; j += G) {
      const int64_t off = (int64_t)j * piece;
      const int64_t ne = (int64_t)w.size - off < (int64_t)piece ? (int64_t)w.size - off : (int64_t)piece;
      const void* src[MCCS_DIRECT_MAX_RANKS] = {(const T*)me.send + off};
      void* dst[MCCS_DIRECT_MAX_RANKS] = {sh.region[root] + obase + (int64_t)me.rank * oslot + off * esz};
      direct_reduce<DT, OpSum>(src, 1, dst, 1, ne);
      if (threadIdx.x == 0) sh.sent[root] += (uint64_t)ne;
    }
  }
  // the pairs that carry no data hand off the count alone (the rule): from the
  // root to everyone, from a non-root to every other non-root
  if (bx == 0 && threadIdx.x == 0)
    for (uint32_t t = 0; t < (uint32_t)n; ++t)
      if (t != me.rank && (is_root || t != root)) sh.sent[t] += (uint64_t)w.size;
  direct_count_out(sh, a, me, MCCS_DIRECT_IN_CNT(0));
  rooted_advance(sh, mine, arrived, (uint64_t)w.size);
  if (threadIdx.x < MCCS_DIRECT_MAX_RANKS) need[threadIdx.x] = sh.e_in + (uint64_t)w.size;
  __syncthreads();
  // workgroup 0 of every rank waits for every peer's count (the rule); the
  // root's other workgroups wait before their first piece
  bool in_seen = false;  // uniform across the workgroup
  if (bx == 0) {
    if (!direct_wait(sh, mine, MCCS_DIRECT_IN_CNT(0), peers, need, abortFlag, a, ecfg)) return;
    in_seen = true;
  }
  if (!is_root) return;
  // 2. the root folds the buffer: channel bid's chunk of every loop, in pieces
  // dealt round-robin, each in the order of that channel's ring
  const T* const own = (const T*)me.send;
  uint32_t base = 0;
  for (uint32_t g = 0; g < w.size; g += w.loopSize) {
    const uint32_t rcs = real_chunk_size<uint32_t>(w, g, w.nch);
    for (uint32_t bid = 0; bid < w.nch; ++bid) {
      const uint32_t coff = block_chunk_offset<uint32_t>(g, bid, rcs);
      if (coff >= w.size) return;  // every later chunk of the walk is empty
      const uint32_t cne = chunk_nelem(w.size, coff, rcs);
      const uint32_t np = (cne + piece2 - 1) / piece2;
      const uint32_t i = rs_ring_index(sh.idx2rank, bid, (uint32_t)n, root);
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
            src[k] = q == root ? (const void*)(own + off) : (const void*)(mine + obase + (int64_t)q * oslot + off * esz);
          }
        }
        direct_reduce<DT, OP>(src, n, dst, 1, ne);
      }
      base += np;
      while (base >= G) base -= G;
    }
  }
}

// Broadcast through the one-shot slots: bytes, T = int8.
__device__ __forceinline__ void direct_bc_body(const mccsDirectArgs& a) {
  constexpr int DT = mccsInt8;
  __shared__ DirectShm sh;
  __shared__ uint64_t need[MCCS_DIRECT_MAX_RANKS];
  const mccsDirectRank& me = a.r[blockIdx.y];
  const int n = (int)a.nranks;
  const uint32_t root = a.root;
  const bool is_root = me.rank == root;
  char* const mine = a.region[me.rank];
  volatile uint32_t* abortFlag = me.abort_flag;
  mccsRingKernelCfg ecfg{};
  ecfg.err_line = me.err_line;
  const uint32_t size = (uint32_t)a.count;  // bytes: at most one one-shot slot
  const uint32_t arrived = rooted_prologue(sh, a, mine);
  const uint64_t seq = sh.seq;
  const uint32_t G = gridDim.x, bx = blockIdx.x;
  const uint32_t peers = ((1u << n) - 1u) & ~(1u << me.rank);
  const uint32_t piece = a.piece > 0 ? a.piece : 1;
  const uint32_t piece2 = a.piece2 > 0 ? a.piece2 : 1;
  const int64_t oslot = (int64_t)a.oslot_bytes;
  const int64_t obase = MCCS_DIRECT_CTRL_BYTES + (int64_t)MCCS_DIRECT_SLOTS * (int64_t)a.slot_bytes +
                        (int64_t)(seq & 1) * MCCS_DIRECT_MAX_RANKS * oslot;
  const uint32_t nps2 = (size + piece2 - 1) / piece2;
  if (is_root) {
    // 1. the n-1 copies of send, one per peer's slot for the root; their
    // pieces are numbered through and piece p goes to workgroup p % G
    uint32_t base = 0;
    const uint32_t nps = (size + piece - 1) / piece;
    for (uint32_t t = 0; t < (uint32_t)n; ++t) {
      if (t == root) continue;
      for (uint32_t j = bx >= base ? bx - base : bx + G - base; j < nps && sh.ok; j += G) {
        const int64_t off = (int64_t)j * piece;
        const int64_t ne = (int64_t)size - off < (int64_t)piece ? (int64_t)size - off : (int64_t)piece;
        const void* src[MCCS_DIRECT_MAX_RANKS] = {(const char*)me.send + off};
        void* dst[MCCS_DIRECT_MAX_RANKS] = {sh.region[t] + obase + (int64_t)root * oslot + off};
        direct_reduce<DT, OpSum>(src, 1, dst, 1, ne);
        if (threadIdx.x == 0) sh.sent[t] += (uint64_t)ne;
      }
      base += nps;
      while (base >= G) base -= G;
    }
    // out of place the root's own copy is local
    if (me.recv != me.send)
      for (uint32_t j = bx; j < nps2; j += G) {
        const int64_t off = (int64_t)j * piece2;
        const int64_t ne = (int64_t)size - off < (int64_t)piece2 ? (int64_t)size - off : (int64_t)piece2;
        const void* src[MCCS_DIRECT_MAX_RANKS] = {(const char*)me.send + off};
        void* dst[MCCS_DIRECT_MAX_RANKS] = {(char*)me.recv + off};
        direct_reduce<DT, OpSum>(src, 1, dst, 1, ne);
      }
  } else if (bx == 0 && threadIdx.x == 0) {
    // a non-root sends no data: the count alone, to every peer (the rule)
    for (uint32_t t = 0; t < (uint32_t)n; ++t)
      if (t != me.rank) sh.sent[t] += (uint64_t)size;
  }
  direct_count_out(sh, a, me, MCCS_DIRECT_IN_CNT(0));
  rooted_advance(sh, mine, arrived, (uint64_t)size);
  if (threadIdx.x < MCCS_DIRECT_MAX_RANKS) need[threadIdx.x] = sh.e_in + (uint64_t)size;
  __syncthreads();
  // workgroup 0 of every rank waits for every peer's count (the rule); a
  // non-root's other workgroups wait before their first piece
  bool in_seen = false;  // uniform across the workgroup
  if (bx == 0) {
    if (!direct_wait(sh, mine, MCCS_DIRECT_IN_CNT(0), peers, need, abortFlag, a, ecfg)) return;
    in_seen = true;
  }
  if (is_root) return;
  // 2. the root's bytes, from this rank's slot for the root to recv
  for (uint32_t j = bx; j < nps2 && sh.ok; j += G) {
    if (!in_seen) {
      if (!direct_wait(sh, mine, MCCS_DIRECT_IN_CNT(0), peers, need, abortFlag, a, ecfg)) return;
      in_seen = true;
    }
    const int64_t off = (int64_t)j * piece2;
    const int64_t ne = (int64_t)size - off < (int64_t)piece2 ? (int64_t)size - off : (int64_t)piece2;
    const void* src[MCCS_DIRECT_MAX_RANKS] = {mine + obase + (int64_t)root * oslot + off};
    void* dst[MCCS_DIRECT_MAX_RANKS] = {(char*)me.recv + off};
    direct_reduce<DT, OpSum>(src, 1, dst, 1, ne);
  }
}

// ---- the LL variants ------------------------------------------------------------
struct RootedLL {
  uint64_t seq;
  uint32_t seq32;  // the line flag, never 0
  uint64_t flag;
  int64_t lslot, llbase;
  uint32_t arrived;
};

// direct_rs_ll_body's prologue: the launch count, the tables to LDS, arrival.
__device__ __forceinline__ RootedLL rooted_ll_prologue(const mccsDirectArgs& a, char* mine, uint64_t& s_seq,
                                                       char** s_region,
                                                       uint8_t (*s_idx2rank)[MCCS_DIRECT_MAX_RANKS]) {
  if (threadIdx.x == 0)
    s_seq = __hip_atomic_load((uint64_t*)(mine + MCCS_DIRECT_STATE) + MCCS_DIRECT_ST_LAUNCHES, __ATOMIC_RELAXED,
                              __HIP_MEMORY_SCOPE_AGENT) + 1;
  if (threadIdx.x < MCCS_DIRECT_MAX_RANKS) s_region[threadIdx.x] = a.region[threadIdx.x];
  if (threadIdx.x < 64) ((uint32_t*)s_idx2rank)[threadIdx.x] = ((const uint32_t*)a.idx2rank)[threadIdx.x];
  __syncthreads();
  RootedLL l;
  l.arrived = 0;
  if (threadIdx.x == 0)
    l.arrived = __hip_atomic_fetch_add((uint32_t*)(mine + MCCS_DIRECT_DONE), 1u, __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_AGENT);
  l.seq = s_seq;
  l.seq32 = 1u + (uint32_t)(l.seq % 0xffffffffull);  // never 0: a zeroed line is never valid
  l.flag = (uint64_t)l.seq32 << 32;
  l.lslot = (int64_t)a.ll_slot_bytes;
  l.llbase = MCCS_DIRECT_CTRL_BYTES + (int64_t)MCCS_DIRECT_SLOTS * (int64_t)a.slot_bytes +
             2 * (int64_t)MCCS_DIRECT_MAX_RANKS * (int64_t)a.oslot_bytes +
             (int64_t)(l.seq & 1) * MCCS_DIRECT_MAX_RANKS * l.lslot;
  return l;
}

__device__ __forceinline__ void rooted_ll_advance(const RootedLL& l, char* mine) {
  if (threadIdx.x == 0 && l.arrived + 1 == gridDim.x) {
    __hip_atomic_store((uint32_t*)(mine + MCCS_DIRECT_DONE), 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store((uint64_t*)(mine + MCCS_DIRECT_STATE) + MCCS_DIRECT_ST_LAUNCHES, l.seq, __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
  }
}

// One flagged line {lo, flag, hi, flag} of word v at p.
__device__ __forceinline__ void ll_put_line(uint64_t* p, uint64_t flag, uint64_t v) {
  __hip_atomic_store(p, flag | (v & 0xffffffffull), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  __hip_atomic_store(p + 1, flag | (v >> 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// Polls the line at lb + t x lslot of every rank t in `pending` until each
// carries seq32 (direct_rs_ll_body's loop); h0 / h1 keep the lines.  False
// after an abort or the watchdog.
__device__ __forceinline__ bool ll_poll_lines(const char* lb, int64_t lslot, uint32_t pending, uint32_t seq32,
                                              uint64_t (&h0)[MCCS_DIRECT_MAX_RANKS],
                                              uint64_t (&h1)[MCCS_DIRECT_MAX_RANKS], uint64_t t0,
                                              volatile uint32_t* abortFlag, const mccsDirectArgs& a,
                                              const mccsRingKernelCfg& ecfg) {
  uint32_t spins = 0;
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
    if (!pending) return true;
    if (++spins % 64 == 0) {
      const bool ab = abort_raised(abortFlag);
      const bool to = !ab && a.timeout_ticks && __builtin_amdgcn_s_memrealtime() - t0 > a.timeout_ticks;
      if (ab || to) {
        raise_error(abortFlag, ecfg, ab ? MCCS_ERR_ABORTED : MCCS_ERR_TIMEOUT);
        return false;
      }
    }
    __builtin_amdgcn_s_sleep(MCCS_POLL_SLEEP);
  }
}

template <int DT, int OP>
__device__ __forceinline__ void direct_rd_ll_body(const mccsDirectArgs& a) {
  using T = typename Elem<DT>::T;
  constexpr uint32_t EPW = 8 / sizeof(T);
  __shared__ uint64_t s_seq;
  __shared__ char* s_region[MCCS_DIRECT_MAX_RANKS];
  __shared__ uint8_t s_idx2rank[MCCS_MAX_NCHANNELS][MCCS_DIRECT_MAX_RANKS];
  const mccsDirectRank& me = a.r[blockIdx.y];
  const uint32_t n = a.nranks, rank = me.rank, root = a.root;
  const bool is_root = rank == root;
  char* const mine = a.region[rank];
  volatile uint32_t* abortFlag = me.abort_flag;
  mccsRingKernelCfg ecfg{};
  ecfg.err_line = me.err_line;
  const DirectWalk w = direct_rd_walk<DT>(a);
  const uint32_t nwords = (uint32_t)(((uint64_t)w.size * sizeof(T) + 7) / 8);
  const uint32_t stride = gridDim.x * blockDim.x;
  const uint32_t gtid = blockIdx.x * blockDim.x + threadIdx.x;
  const char* in = (const char*)me.send;
  char* out = (char*)me.recv;
  const bool in_al = ((uintptr_t)in & 7) == 0, out_al = ((uintptr_t)out & 7) == 0;
  const RootedLL l = rooted_ll_prologue(a, mine, s_seq, s_region, s_idx2rank);
  const uint32_t peers = ((1u << n) - 1u) & ~(1u << rank);
  // 1. a non-root's word wd -> line wd of the root's slot for this rank
  if (!is_root)
    for (uint32_t wd = gtid; wd < nwords; wd += stride)
      ll_put_line((uint64_t*)(s_region[root] + l.llbase + (int64_t)rank * l.lslot + (int64_t)wd * 16), l.flag,
                  ll_load_word<T>(in, wd, w.size, in_al));
  // the pairs that carry no data hand off line 0 with a dummy word (the rule)
  if (gtid == 0)
    for (uint32_t t = 0; t < n; ++t)
      if (t != rank && (is_root || t != root))
        ll_put_line((uint64_t*)(s_region[t] + l.llbase + (int64_t)rank * l.lslot), l.flag, 0);
  rooted_ll_advance(l, mine);
  const uint64_t t0 = __builtin_amdgcn_s_memrealtime();
  uint64_t h0[MCCS_DIRECT_MAX_RANKS], h1[MCCS_DIRECT_MAX_RANKS];
  if (!is_root) {
    // global thread 0 polls line 0 of every peer's slot (the rule)
    if (gtid == 0) (void)ll_poll_lines(mine + l.llbase, l.lslot, peers, l.seq32, h0, h1, t0, abortFlag, a, ecfg);
    return;
  }
  // 2. the root: poll every peer's line of each word, fold in the ring order
  // of the word's chunk (word 0 exists with count >= 1, so the root too polls
  // every peer's line 0)
  for (uint32_t wd = gtid; wd < nwords; wd += stride) {
    const uint32_t e = wd * EPW;
    const uint32_t g = e / w.loopSize * w.loopSize;
    const uint32_t bid = (e - g) / real_chunk_size<uint32_t>(w, g, w.nch);  // block_chunk_offset's part holding e
    const uint32_t i = rs_ring_index(s_idx2rank, bid, n, root);
    const uint64_t own = ll_load_word<T>(in, wd, w.size, in_al);
    if (!ll_poll_lines(mine + l.llbase + (int64_t)wd * 16, l.lslot, peers, l.seq32, h0, h1, t0, abortFlag, a, ecfg))
      return;
    // acc = x[idx i+1]; acc = fn(x[idx i+j], acc); the last operand is the root's own word
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

// Broadcast through the LL lines: bytes, T = int8.
__device__ __forceinline__ void direct_bc_ll_body(const mccsDirectArgs& a) {
  using T = int8_t;
  __shared__ uint64_t s_seq;
  __shared__ char* s_region[MCCS_DIRECT_MAX_RANKS];
  __shared__ uint8_t s_idx2rank[MCCS_MAX_NCHANNELS][MCCS_DIRECT_MAX_RANKS];
  const mccsDirectRank& me = a.r[blockIdx.y];
  const uint32_t n = a.nranks, rank = me.rank, root = a.root;
  const bool is_root = rank == root;
  char* const mine = a.region[rank];
  volatile uint32_t* abortFlag = me.abort_flag;
  mccsRingKernelCfg ecfg{};
  ecfg.err_line = me.err_line;
  const uint32_t size = (uint32_t)a.count;  // bytes: at most half an LL slot
  const uint32_t nwords = (size + 7) / 8;
  const uint32_t stride = gridDim.x * blockDim.x;
  const uint32_t gtid = blockIdx.x * blockDim.x + threadIdx.x;
  const char* in = (const char*)me.send;
  char* out = (char*)me.recv;
  const bool out_al = ((uintptr_t)out & 7) == 0;
  const RootedLL l = rooted_ll_prologue(a, mine, s_seq, s_region, s_idx2rank);
  const uint32_t peers = ((1u << n) - 1u) & ~(1u << rank);
  if (is_root) {
    // 1. every word as a flagged line into every peer's slot for the root
    // (out of place: and into recv)
    const bool in_al = ((uintptr_t)in & 7) == 0;
    for (uint32_t wd = gtid; wd < nwords; wd += stride) {
      const uint64_t v = ll_load_word<T>(in, wd, size, in_al);
      if (out != in) ll_store_word<T>(out, wd, size, out_al, v);
#pragma unroll
      for (uint32_t t = 0; t < MCCS_DIRECT_MAX_RANKS; ++t)
        if (t < n && t != rank)
          ll_put_line((uint64_t*)(s_region[t] + l.llbase + (int64_t)rank * l.lslot + (int64_t)wd * 16), l.flag, v);
    }
  } else if (gtid == 0) {
    // a non-root carries no data: line 0 with a dummy word, to every peer (the rule)
    for (uint32_t t = 0; t < n; ++t)
      if (t != rank) ll_put_line((uint64_t*)(s_region[t] + l.llbase + (int64_t)rank * l.lslot), l.flag, 0);
  }
  rooted_ll_advance(l, mine);
  const uint64_t t0 = __builtin_amdgcn_s_memrealtime();
  uint64_t h0[MCCS_DIRECT_MAX_RANKS], h1[MCCS_DIRECT_MAX_RANKS];
  if (is_root) {
    // global thread 0 polls line 0 of every peer's slot (the rule)
    if (gtid == 0) (void)ll_poll_lines(mine + l.llbase, l.lslot, peers, l.seq32, h0, h1, t0, abortFlag, a, ecfg);
    return;
  }
  // 2. a non-root polls the root's line of each word and stores it; with word
  // 0 (global thread 0's first) it polls every peer's line 0 (the rule)
  for (uint32_t wd = gtid; wd < nwords; wd += stride) {
    const uint32_t pending = wd == 0 ? peers : 1u << root;
    if (!ll_poll_lines(mine + l.llbase + (int64_t)wd * 16, l.lslot, pending, l.seq32, h0, h1, t0, abortFlag, a, ecfg))
      return;
    uint64_t v = 0;
#pragma unroll
    for (uint32_t t = 0; t < MCCS_DIRECT_MAX_RANKS; ++t)
      if (t == root) v = (h0[t] & 0xffffffffull) | (h1[t] << 32);
    ll_store_word<T>(out, wd, size, out_al, v);
  }
}

}  // namespace mccs
