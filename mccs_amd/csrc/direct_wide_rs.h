// direct_wide_rs.h — wide-accumulate direct ReduceScatter and Reduce for fp16 /
// bf16 (opt-in: mccsCommSetReduceScatterWide / mccsCommSetReduceWide;
// ring_cfg.h, "Wide direct ReduceScatter and Reduce").
//
// direct_wide.h's contract on ReduceScatter's and Reduce's cut: per output
// element, ranks in RANK order 0 .. n-1 whatever the rings are,
//   t_r = f32(x_r)  or  fl32(f32(x_r) * f32(s))   (PreMulSum, s in op_arg's low 16 bits)
//   acc = t_0; acc = fl32(acc + t_r); out = T(acc), one rounding to nearest even
// with the product and the sum two roundings.  Rank t receives this for block t
// (a.count = recvcount elements) of every rank's send buffer (ReduceScatter);
// the root receives it for the whole buffer of a.count elements (Reduce; a
// non-root's recv is never touched).  The bits are the corresponding slice of
// the wide AllReduce's and depend on neither rings, channels, workgroup count
// nor body.  The arithmetic is direct_wide.h's (wide_up*, wide_fold,
// wide_reduce, wide_down*), included and not copied.
//
// One owner-side fold serves both functions: a rank "owns" a contiguous range
// of `count` elements -- block `rank` of send (ReduceScatter: every rank is an
// owner) or the whole buffer (Reduce: the root alone).  There is no chunk
// walk: no direct_walk, no idx2rank in LDS, no division per word or piece.
// The launch has direct_kernel's shape (blockIdx.y = rank slot, G workgroups of
// MCCS_DIRECT_THREADS, the launch guard, prologue, arrival count and state
// words), and each mode leaves LAUNCHES, E_IN and the parity exactly as its
// ring-order counterpart (direct_rs.h / direct_rooted.h) with the same
// per-sender amounts would.
//   MCCS_DIRECT_WIDE_RS_ONE_SHOT / MCCS_DIRECT_WIDE_RD_ONE_SHOT (count-based)
//     1. the pieces of the ranges this rank sends (the n-1 foreign blocks,
//        numbered through; a non-root's buffer; a root: none) dealt round-robin
//        over the G workgroups -> the owner's one-shot slot [parity seq & 1]
//        [sender me] at the element offset within the range; direct_count_out
//        on IN_CNT;
//     2. an owner waits for E_IN + count on every peer's line, then deals the
//        pieces of its own range round-robin: wide_reduce with the sources in
//        rank order (the own operand at position `rank`, the slots elsewhere)
//        into recv.
//     E_IN advances by count.
//   MCCS_DIRECT_WIDE_RS_LL / MCCS_DIRECT_WIDE_RD_LL
//     1. thread-linear over the concatenation of the sent ranges' 8-byte words:
//        word w of a range -> line w of its owner's LL slot for this rank (the
//        range index advances by subtraction, never by division);
//     2. an owner goes thread-linear over its own range's words: polls every
//        peer's line, folds the 4 binary32 accumulators in rank order with the
//        own word at r == rank, stores with ll_store_word.
//     Only LAUNCHES moves.  The first own word's load is in flight across the
//     launch-count read.
// Reduce obeys ring_cfg.h's rule for rooted launches word for word: every
// ordered pair hands off in every launch with the common amount `count` (one
// add by workgroup 0 / a dummy line 0 where the pair carries no data), E_IN
// advances by count on every rank, and workgroup 0 (global thread 0 in LL) of
// every rank waits for every peer before the kernel ends.
// In place (ReduceScatter: recv == send + rank * recvcount; Reduce: the root's
// recv == send) needs no self wait: phase 1 never reads the own range, and
// phase 2 loads and stores each element through one thread.
// With an odd recvcount block t of send starts 2 bytes off a pack, so the
// copies and the own operand take direct_reduce's / wide_reduce's typed path
// (ll_load_word's element path in LL); results do not depend on it.
#pragma once
#include "direct_rooted.h"  // ll_put_line, ll_poll_lines
#include "direct_wide.h"

namespace mccs {

// RD = false: ReduceScatter; RD = true: Reduce to a.root.
template <int DT, bool PRE, bool RD>
__device__ __forceinline__ void direct_wide_own_body(const mccsDirectArgs& a) {
  using T = typename Elem<DT>::T;
  __shared__ DirectShm sh;  // (its idx2rank stays unwritten: there is no walk)
  __shared__ uint64_t need[MCCS_DIRECT_MAX_RANKS];
  const mccsDirectRank& me = a.r[blockIdx.y];
  const int n = (int)a.nranks;
  const uint32_t rank = me.rank, root = a.root;
  const bool owner = !RD || rank == root;
  char* const mine = a.region[rank];
  volatile uint32_t* abortFlag = me.abort_flag;
  mccsRingKernelCfg ecfg{};
  ecfg.err_line = me.err_line;
  const uint32_t size = (uint32_t)a.count;  // of one range: at most one one-shot slot
  const float s = wide_scalar<DT>(a.op_arg);
  // Prologue and arrival count: direct_rs_body's without the walk's table.
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
  const uint32_t peers = ((1u << n) - 1u) & ~(1u << rank);
  const uint32_t piece = a.piece > 0 ? a.piece : 1;
  const uint32_t piece2 = a.piece2 > 0 ? a.piece2 : 1;
  const int64_t oslot = (int64_t)a.oslot_bytes;
  const int64_t obase = MCCS_DIRECT_CTRL_BYTES + (int64_t)MCCS_DIRECT_SLOTS * (int64_t)a.slot_bytes +
                        (int64_t)(seq & 1) * MCCS_DIRECT_MAX_RANKS * oslot;
  // 1. every range this rank sends, to its owner's slot for this rank.  The
  // pieces of the ranges are numbered through and piece p goes to workgroup
  // p % G; `base` keeps the numbering mod G by subtraction.
  {
    uint32_t base = 0;
    const uint32_t nps = (size + piece - 1) / piece;  // one division per launch
    for (uint32_t t = 0; t < (uint32_t)n; ++t) {
      if (t == rank || (RD && t != root)) continue;
      const T* const blk = (const T*)me.send + (RD ? 0 : (int64_t)t * size);
      char* const slot = sh.region[t] + obase + (int64_t)rank * oslot;
      for (uint32_t j = bx >= base ? bx - base : bx + G - base; j < nps && sh.ok; j += G) {
        const int64_t off = (int64_t)j * piece;
        const int64_t ne = (int64_t)size - off < (int64_t)piece ? (int64_t)size - off : (int64_t)piece;
        const void* src[MCCS_DIRECT_MAX_RANKS] = {blk + off};
        void* dst[MCCS_DIRECT_MAX_RANKS] = {slot + off * esz};
        direct_reduce<DT, OpSum>(src, 1, dst, 1, ne);  // one source: a copy
        if (threadIdx.x == 0) sh.sent[t] += (uint64_t)ne;
      }
      base += nps;
      while (base >= G) base -= G;
    }
  }
  // Reduce: the pairs that carry no data hand off the count alone (the rule):
  // from the root to everyone, from a non-root to every other non-root
  if (RD && bx == 0 && threadIdx.x == 0)
    for (uint32_t t = 0; t < (uint32_t)n; ++t)
      if (t != rank && (owner || t != root)) sh.sent[t] += (uint64_t)size;
  direct_count_out(sh, a, me, MCCS_DIRECT_IN_CNT(0));
  // The last workgroup to arrive advances the launch count and E_IN by the
  // common amount (every sender adds `count` on every receiver).
  if (threadIdx.x == 0 && arrived + 1 == G) {
    uint64_t* st = (uint64_t*)(mine + MCCS_DIRECT_STATE);
    __hip_atomic_store((uint32_t*)(mine + MCCS_DIRECT_DONE), 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(st + MCCS_DIRECT_ST_E_IN, sh.e_in + (uint64_t)size, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(st + MCCS_DIRECT_ST_LAUNCHES, seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  if (threadIdx.x < MCCS_DIRECT_MAX_RANKS) need[threadIdx.x] = sh.e_in + (uint64_t)size;
  __syncthreads();
  bool in_seen = false;  // uniform across the workgroup
  // Reduce: workgroup 0 of every rank waits for every peer's count (the rule)
  if (RD && bx == 0) {
    if (!direct_wait(sh, mine, MCCS_DIRECT_IN_CNT(0), peers, need, abortFlag, a, ecfg)) return;
    in_seen = true;
  }
  if (!owner) return;
  // 2. the own range: pieces dealt round-robin, every source in rank order
  const T* const own = (const T*)me.send + (RD ? 0 : (int64_t)rank * size);
  const uint32_t np2 = (size + piece2 - 1) / piece2;
  for (uint32_t j = bx; j < np2 && sh.ok; j += G) {
    if (!in_seen) {
      if (!direct_wait(sh, mine, MCCS_DIRECT_IN_CNT(0), peers, need, abortFlag, a, ecfg)) return;
      in_seen = true;
    }
    const int64_t off = (int64_t)j * piece2;
    const int64_t ne = (int64_t)size - off < (int64_t)piece2 ? (int64_t)size - off : (int64_t)piece2;
    const void* src[MCCS_DIRECT_MAX_RANKS];
    void* dst[MCCS_DIRECT_MAX_RANKS] = {(T*)me.recv + off};
#pragma unroll
    for (int r = 0; r < MCCS_DIRECT_MAX_RANKS; ++r)
      src[r] = r >= n            ? nullptr
               : r == (int)rank  ? (const void*)(own + off)
                                 : (const void*)(mine + obase + (int64_t)r * oslot + off * esz);
    wide_reduce<DT, PRE>(src, n, dst, 1, ne, s);
  }
}

// The LL bodies: direct_rs_ll_body's / direct_rd_ll_body's lines, flags, parity
// and polling, with the fold of direct_wide_ll_body.
template <int DT, bool PRE, bool RD>
__device__ __forceinline__ void direct_wide_own_ll_body(const mccsDirectArgs& a) {
  using T = typename Elem<DT>::T;
  __shared__ uint64_t s_seq;
  __shared__ char* s_region[MCCS_DIRECT_MAX_RANKS];  // phase 1 picks a region per word
  const mccsDirectRank& me = a.r[blockIdx.y];
  const uint32_t n = a.nranks, rank = me.rank, root = a.root;
  const bool owner = !RD || rank == root;
  char* const mine = a.region[rank];
  volatile uint32_t* abortFlag = me.abort_flag;
  mccsRingKernelCfg ecfg{};
  ecfg.err_line = me.err_line;
  const uint32_t size = (uint32_t)a.count;
  const float s = wide_scalar<DT>(a.op_arg);
  const uint32_t nwords = (uint32_t)(((uint64_t)size * sizeof(T) + 7) / 8);  // of one range
  const uint32_t stride = gridDim.x * blockDim.x;
  const uint32_t gtid = blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t bbytes = (int64_t)size * (int64_t)sizeof(T);
  const char* in = (const char*)me.send;
  char* out = (char*)me.recv;
  const char* const own_blk = in + (RD ? 0 : (int64_t)rank * bbytes);
  const bool own_al = ((uintptr_t)own_blk & 7) == 0, out_al = ((uintptr_t)out & 7) == 0;
  // an owner's first own word is in flight while thread 0 reads the launch count
  uint64_t own0 = 0;
  if (owner && gtid < nwords) own0 = ll_load_word<T>(own_blk, gtid, size, own_al);
  if (threadIdx.x == 0)
    s_seq = __hip_atomic_load((uint64_t*)(mine + MCCS_DIRECT_STATE) + MCCS_DIRECT_ST_LAUNCHES, __ATOMIC_RELAXED,
                              __HIP_MEMORY_SCOPE_AGENT) + 1;
  if (threadIdx.x < MCCS_DIRECT_MAX_RANKS) s_region[threadIdx.x] = a.region[threadIdx.x];
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
  const int64_t my_lines = llbase + (int64_t)rank * lslot;  // this rank's slot in a peer's region
  // 1. word wd of sent range b -> line wd of its owner's slot for this rank.
  // A thread's position (b, wd) in the concatenation starts at gtid and moves
  // on by `stride`, carried into the next range by subtraction.
  if (RD) {
    if (!owner)
      for (uint32_t wd = gtid; wd < nwords; wd += stride)
        ll_put_line((uint64_t*)(s_region[root] + my_lines + (int64_t)wd * 16), flag, ll_load_word<T>(in, wd, size, own_al));
    // the pairs that carry no data hand off line 0 with a dummy word (the rule)
    if (gtid == 0)
      for (uint32_t t = 0; t < n; ++t)
        if (t != rank && (owner || t != root)) ll_put_line((uint64_t*)(s_region[t] + my_lines), flag, 0);
  } else {
    uint32_t b = 0, wd = gtid;
    for (;;) {
      while (wd >= nwords && b < n - 1) {
        wd -= nwords;
        ++b;
      }
      if (b >= n - 1) break;
      const uint32_t t = b < rank ? b : b + 1;
      const char* blk = in + (int64_t)t * bbytes;
      ll_put_line((uint64_t*)(s_region[t] + my_lines + (int64_t)wd * 16), flag,
                  ll_load_word<T>(blk, wd, size, ((uintptr_t)blk & 7) == 0));
      wd += stride;
    }
  }
  if (threadIdx.x == 0 && arrived + 1 == gridDim.x) {
    __hip_atomic_store((uint32_t*)(mine + MCCS_DIRECT_DONE), 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store((uint64_t*)(mine + MCCS_DIRECT_STATE) + MCCS_DIRECT_ST_LAUNCHES, seq, __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
  }
  const uint32_t peers = ((1u << n) - 1u) & ~(1u << rank);
  const uint64_t t0 = __builtin_amdgcn_s_memrealtime();
  uint64_t h0[MCCS_DIRECT_MAX_RANKS], h1[MCCS_DIRECT_MAX_RANKS];
  if (!owner) {
    // a Reduce non-root: global thread 0 polls line 0 of every peer's slot (the rule)
    if (gtid == 0) (void)ll_poll_lines(mine + llbase, lslot, peers, seq32, h0, h1, t0, abortFlag, a, ecfg);
    return;
  }
  // 2. the own range's words: poll every peer's line, fold in rank order (word
  // 0 exists with count >= 1, so every owner polls every peer's line 0)
  for (uint32_t wd = gtid; wd < nwords; wd += stride) {
    const uint64_t own = wd == gtid ? own0 : ll_load_word<T>(own_blk, wd, size, own_al);
    if (!ll_poll_lines(mine + llbase + (int64_t)wd * 16, lslot, peers, seq32, h0, h1, t0, abortFlag, a, ecfg)) return;
    f32x4 acc{};
#pragma unroll
    for (uint32_t r = 0; r < MCCS_DIRECT_MAX_RANKS; ++r)
      if (r < n) {
        const uint64_t v = r == rank ? own : (h0[r] & 0xffffffffull) | (h1[r] << 32);
        acc = wide_fold<PRE>(acc, wide_up4<DT>(v), s, r == 0);
      }
    ll_store_word<T>(out, wd, size, out_al, wide_down4<DT>(acc));
  }
}

}  // namespace mccs
