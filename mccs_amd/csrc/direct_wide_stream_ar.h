// direct_wide_stream_ar.h — wide streamed AllReduce for fp16 / bf16 (opt-in:
// mccsCommSetAllReduceWideStream; ring_cfg.h, "Wide streamed AllReduce").
//
// direct_wide.h's contract for a buffer of ANY size: per element, ranks in RANK
// order 0 .. n-1 whatever the rings are,
//   t_r = f32(x_r)  or  fl32(f32(x_r) * f32(s))   (PreMulSum, s in op_arg's low 16 bits)
//   acc = t_0; acc = fl32(acc + t_r); out = T(acc), one rounding to nearest even
// with the product and the sum two roundings; the same bits on every rank, the
// wide LL / one-shot / two-shot bodies' for a size that fits both, independent
// of rings, channels, workgroup count, round size and round count.  The
// arithmetic is direct_wide.h's (wide_reduce and what it calls), included and
// not copied.
//
// The split is the wide two-shot's: rank t owns [t q, t q + a.owned[t]), q =
// MCCS_WIDE_SHARE(count, n), and the planner streams only when every rank owns
// an element.  A share moves in K = a.rounds = ceil(q / B) rounds of B =
// a.round_elems elements; round k covers [k B, k B + len_k(t)) of share t,
// len_k(t) = min(B, owned[t] - k B) or 0 once a (short, last) share is
// exhausted.  Round k has seq0 + k for its sequence number (seq0 = LAUNCHES +
// 1) and three legs:
//   send(k)  round k of the n-1 foreign shares -> the owner's one-shot slot
//            [parity (seq0 + k) & 1][sender me] at the offset within the round;
//            every workgroup arrives on SEND_DONE and the last adds len_k(t) to
//            IN_CNT(me) of every owner t: counted whole or not at all;
//   fold(k)  wait for E_IN + min(owned[me], (k+1) B) on every peer's line;
//            wide_reduce of round k of the own share (the own input at position
//            `rank`, the n-1 slots elsewhere) into recv AND into every peer t's
//            gather buffer: t's two-shot in slot [me], the half of the round's
//            parity, at the offset within the round; every workgroup arrives
//            on FOLD_DONE and the last adds len_k(me) to OUT_CNT(me) of every
//            peer;
//   copy(k)  wait for E_OUT[o] + min(owned[o], (k+1) B) on every owner o's
//            line; round k of the n-1 foreign shares, gather buffer -> recv.
// Per workgroup, step i = 0 .. K+1 is
//   wait ACK >= seq0 + i-2 (2 <= i <= K); send(i) (i < K); fold(i-1)
//   (1 <= i <= K); copy(i-2) (2 <= i); arrive on ROUND_DONE (1 <= i), whose
//   last arriver stores seq0 + i-1 into ACK(me) of every peer
// so round i is on the links while round i-1 is folded and round i-2 copied
// out.  Before send(1) every workgroup has waited for round 0's in-counts
// (fold(0)'s wait, taken first), and the kernel ends after every peer's ACK >=
// seq0 + K.  The pieces of each leg are numbered through ALL rounds and piece p
// goes to workgroup p % G, kept mod G by subtraction; send(k) and copy(k) deal
// identical pieces (one function, two counters), so a workgroup rewrites in
// copy(k) exactly the ranges it read in send(k): in place is safe.  Divisions:
// one per leg for a full round at launch, one per partial range (at most 2n a
// launch), none per piece.  Share bases and round offsets are 64-bit.
// The launch leaves LAUNCHES += K + 1, E_IN += owned[me], E_OUT[t] += owned[t],
// E_SELF untouched.  Every wait is direct_wait; none is for the own rank.  Why
// this is free of races and cycles: ring_cfg.h.
//
// The round loop, its counts and its waits are written once, in
// direct_stream_ar_body, templated on the data path: a Path supplies share()
// (q), piece() (a planner's piece made usable), send() (one piece of a foreign
// share into a scatter slot), at() (where a round offset lies in a buffer; the
// body builds fold's tables with it: per rank in rank order the own input or
// the scatter slot, and the output or the peer's gather buffer), fold() (one
// piece of the own share through those tables) and copy() (one piece of a
// foreign share's results out of a gather buffer).
// WideStreamArPath below is this file's 16-bit path; direct_quant_stream_ar.h's
// QuantStreamArPath puts FP8 codes and scale bytes into the same buffers.
#pragma once
#include "direct_wide_stream.h"

static_assert(MCCS_DIRECT_FOLD_DONE(4) <= MCCS_DIRECT_CTRL_BYTES && MCCS_DIRECT_SEND_DONE(4) <= MCCS_DIRECT_FOLD_DONE(0),
              "the streamed AllReduce's arrival words lie in the control block's unused part");

namespace mccs {

// The 16-bit data path: element e of a round at byte 2 e of a scatter slot and
// of a gather buffer; piece() and send() are the streamed ReduceScatter's.
template <int DT, bool PRE>
struct WideStreamArPath : WideStreamPath<DT, PRE> {
  using T = typename Elem<DT>::T;
  static __device__ __forceinline__ uint64_t share(uint64_t count, uint64_t n) { return MCCS_WIDE_SHARE(count, n); }
  // where round element off lies in a scatter slot and in a gather buffer (bytes)
  static __device__ __forceinline__ int64_t at(int64_t off) { return off * (int64_t)sizeof(T); }
  // ne elements in rank order: src[r] the own input (r == rank) or scatter slot r at at(off), dst[r] the output or
  // peer r's gather buffer for this rank at at(off)
  static __device__ __forceinline__ void fold(int64_t, int64_t, int n, uint32_t, const void** src, void** dst, int64_t,
                                              int64_t ne, float s) {
    wide_reduce<DT, PRE>(src, n, dst, n, ne, s);
  }
  // ne elements of a foreign share's results at round offset off of this rank's gather buffer for their owner
  static __device__ __forceinline__ void copy(int64_t, const char* gath, int64_t off, T* out, int64_t ne) {
    const void* src[MCCS_DIRECT_MAX_RANKS] = {gath + off * (int64_t)sizeof(T)};
    void* dst[MCCS_DIRECT_MAX_RANKS] = {out};
    direct_reduce<DT, OpSum>(src, 1, dst, 1, ne);  // one source: a copy
  }
};

template <int DT, bool PRE, class Path>
__device__ __forceinline__ void direct_stream_ar_body(const mccsDirectArgs& a) {
  using T = typename Elem<DT>::T;
  __shared__ DirectShm sh;  // (its idx2rank stays unwritten: there is no walk)
  __shared__ uint64_t need[MCCS_DIRECT_MAX_RANKS];
  const mccsDirectRank& me = a.r[blockIdx.y];
  const int n = (int)a.nranks;
  const uint32_t rank = me.rank;
  char* const mine = a.region[rank];
  volatile uint32_t* abortFlag = me.abort_flag;
  mccsRingKernelCfg ecfg{};
  ecfg.err_line = me.err_line;
  const uint64_t K = a.rounds;
  const uint32_t B = a.round_elems;
  const float s = wide_scalar<DT>(a.op_arg);
  // Prologue and arrival count: direct_wide_body's.
  if (threadIdx.x < 64) {
    const uint32_t lane = threadIdx.x;
    uint64_t v = 0;
    if (lane < MCCS_DIRECT_ST_WORDS)
      v = __hip_atomic_load((uint64_t*)(mine + MCCS_DIRECT_STATE) + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (lane == MCCS_DIRECT_ST_LAUNCHES) sh.seq = v + 1;
    if (lane == MCCS_DIRECT_ST_E_IN) sh.e_in = v;
    if (lane >= 2 && lane < 2 + MCCS_DIRECT_MAX_RANKS) sh.e_out[lane - 2] = v;
    if (lane == MCCS_DIRECT_ST_WORDS) sh.ok = v == 0;
    if (lane < MCCS_DIRECT_MAX_RANKS) {
      sh.owned[lane] = lane < (uint32_t)n ? a.owned[lane] : 0;
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
  const uint64_t seq0 = sh.seq;
  const uint32_t G = gridDim.x, bx = blockIdx.x;
  const uint32_t peers = ((1u << n) - 1u) & ~(1u << rank);
  const uint32_t piece = Path::piece(a.piece), piece2 = Path::piece(a.piece2);
  const uint64_t q = Path::share(a.count, (uint64_t)n);  // one 64-bit division per launch
  const int64_t oslot = (int64_t)a.oslot_bytes, slot = (int64_t)a.slot_bytes;
  const int64_t obase = MCCS_DIRECT_CTRL_BYTES + (int64_t)MCCS_DIRECT_SLOTS * slot;
  const int64_t half = (slot / 2) & ~(int64_t)15;  // of a two-shot in slot: one parity's gather buffer
  const uint32_t nps_full = (B + piece - 1) / piece, np2_full = (B + piece2 - 1) / piece2;
  uint32_t sbase = 0, fbase = 0, cbase = 0;  // (pieces sent / folded / copied before this range) mod G, through all rounds

  // Elements of share t in round k, and of rounds 0 .. k together.
  auto len_of = [&](uint32_t t, uint64_t k) {
    const uint64_t o = sh.owned[t], lo = k * (uint64_t)B;
    return lo >= o ? 0u : o - lo < (uint64_t)B ? (uint32_t)(o - lo) : B;
  };
  auto upto = [&](uint32_t t, uint64_t k) {
    const uint64_t o = sh.owned[t], hi = (k + 1) * (uint64_t)B;
    return hi < o ? hi : o;
  };
  // Wave 0 polls every peer's line at `cnt_base` for need[]; false: abort or watchdog.
  auto wait = [&](int cnt_base, auto&& v) {
    if (threadIdx.x < MCCS_DIRECT_MAX_RANKS) need[threadIdx.x] = v(threadIdx.x);
    __syncthreads();
    return direct_wait(sh, mine, cnt_base, peers, need, abortFlag, a, ecfg);
  };
  auto wait_ack = [&](uint64_t v) { return wait(MCCS_DIRECT_ACK(0), [&](uint32_t) { return v; }); };
  auto wait_in = [&](uint64_t k) {
    return wait(MCCS_DIRECT_IN_CNT(0), [&](uint32_t) { return sh.e_in + upto(rank, k); });
  };
  auto wait_out = [&](uint64_t k) {
    return wait(MCCS_DIRECT_OUT_CNT(0), [&](uint32_t o) { return sh.e_out[o] + upto(o, k); });
  };
  // This workgroup's pieces of round k of the n-1 foreign shares, numbered
  // through all rounds from `base`: f(owner, element offset within the round,
  // elements).  send(k) and copy(k) both deal through here.
  auto foreign = [&](uint64_t k, uint32_t& base, auto&& f) {
    for (uint32_t t = 0; t < (uint32_t)n; ++t) {
      if (t == rank) continue;
      const uint32_t len = len_of(t, k);
      const uint32_t nps = len == B ? nps_full : len == 0 ? 0 : (len + piece - 1) / piece;
      for (uint32_t j = bx >= base ? bx - base : bx + G - base; j < nps && sh.ok; j += G) {
        const uint32_t so = j * piece;
        f(t, (int64_t)so, (int64_t)(len - so < piece ? len - so : piece));
      }
      base += nps;
      while (base >= G) base -= G;
    }
  };
  // A leg's count is indivisible: this workgroup's writes are complete (and,
  // for cached arenas, written back: direct_count_out's fence) when it arrives
  // on `word`, with or without pieces, and the LAST of the rank's workgroups
  // to arrive puts the word back to 0 and adds amount(t) to its line at
  // `cnt_base` on every peer t.  So a peer that sees a round's total has all of
  // that round and of every earlier one from this rank.
  auto count_whole = [&](int word, int cnt_base, auto&& amount) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0 && sh.ok) {
      if (a.fence_mode != MCCS_FENCE_UNCACHED) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
      uint32_t* const cnt = (uint32_t*)(mine + word);
      if (__hip_atomic_fetch_add(cnt, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1 == G) {
        __hip_atomic_store(cnt, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        for (uint32_t t = 0; t < (uint32_t)n; ++t)
          if (t != rank && amount(t))
            __hip_atomic_fetch_add((uint64_t*)(sh.region[t] + cnt_base + (int)rank * MCCS_FLAG_LINE_BYTES),
                                   (uint64_t)amount(t), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        // the word is back at 0 before this workgroup can arrive anywhere again
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
    }
  };
  // Round k of the foreign shares, to their owners' one-shot slots for this rank.
  auto send = [&](uint64_t k) {
    const int64_t roff = (int64_t)(k * (uint64_t)B);
    const int64_t pbase = obase + (int64_t)((seq0 + k) & 1) * MCCS_DIRECT_MAX_RANKS * oslot + (int64_t)rank * oslot;
    foreign(k, sbase, [&](uint32_t t, int64_t off, int64_t ne) {
      Path::send(oslot, (const T*)me.send + (int64_t)(t * q) + roff + off, sh.region[t] + pbase, off, ne);
    });
    count_whole(MCCS_DIRECT_SEND_DONE((seq0 + k) & 3), MCCS_DIRECT_IN_CNT(0), [&](uint32_t t) { return len_of(t, k); });
  };
  // Round k of the own share: every source in rank order, into the output and
  // every peer's gather buffer for this rank.
  auto fold = [&](uint64_t k) {
    const uint32_t len = len_of(rank, k);
    const uint32_t np2 = len == B ? np2_full : len == 0 ? 0 : (len + piece2 - 1) / piece2;
    const int64_t roff = (int64_t)(rank * q + k * (uint64_t)B);
    const int64_t par = (int64_t)((seq0 + k) & 1);
    const char* const slots = mine + obase + par * MCCS_DIRECT_MAX_RANKS * oslot;
    const int64_t gbase = MCCS_DIRECT_CTRL_BYTES + (int64_t)rank * slot + par * half;
    for (uint32_t j = bx >= fbase ? bx - fbase : bx + G - fbase; j < np2 && sh.ok; j += G) {
      const int64_t off = (int64_t)j * piece2;
      const int64_t ne = (int64_t)len - off < (int64_t)piece2 ? (int64_t)len - off : (int64_t)piece2;
      const int64_t boff = Path::at(off);
      const void* src[MCCS_DIRECT_MAX_RANKS];
      void* dst[MCCS_DIRECT_MAX_RANKS];
#pragma unroll
      for (int r = 0; r < MCCS_DIRECT_MAX_RANKS; ++r) {
        src[r] = nullptr;
        dst[r] = nullptr;
        if (r < n) {
          src[r] = r == (int)rank ? (const void*)((const T*)me.send + roff + off)
                                  : (const void*)(slots + (int64_t)r * oslot + boff);
          dst[r] = r == (int)rank ? (void*)((T*)me.recv + roff + off) : (void*)(sh.region[r] + gbase + boff);
        }
      }
      Path::fold(oslot, half, n, rank, src, dst, off, ne, s);
    }
    fbase += np2;
    while (fbase >= G) fbase -= G;
    count_whole(MCCS_DIRECT_FOLD_DONE((seq0 + k) & 3), MCCS_DIRECT_OUT_CNT(0), [&](uint32_t) { return len; });
  };
  // Round k of the foreign shares' results, from this rank's gather buffers to the output.
  auto copy = [&](uint64_t k) {
    const int64_t roff = (int64_t)(k * (uint64_t)B);
    const char* const gath = mine + MCCS_DIRECT_CTRL_BYTES + (int64_t)((seq0 + k) & 1) * half;
    foreign(k, cbase, [&](uint32_t t, int64_t off, int64_t ne) {
      Path::copy(half, gath + (int64_t)t * slot, off, (T*)me.recv + (int64_t)(t * q) + roff + off, ne);
    });
  };
  // This workgroup has read all it reads of step i's buffers (the scatter slots
  // of round i-1, the gather buffers of round i-2); the last of the rank's
  // workgroups to say so tells every peer.
  auto arrive = [&](uint64_t i) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0 && sh.ok) {
      uint32_t* const cnt = (uint32_t*)(mine + MCCS_DIRECT_ROUND_DONE((seq0 + i - 1) & 3));
      if (__hip_atomic_fetch_add(cnt, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1 == G) {
        __hip_atomic_store(cnt, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        for (int t = 0; t < n; ++t)
          if (t != (int)rank)
            __hip_atomic_store((uint64_t*)(sh.region[t] + MCCS_DIRECT_ACK(rank)), seq0 + i - 1, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_SYSTEM);
        // drained before this workgroup can arrive anywhere again: ACK only grows
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
    }
  };

  for (uint64_t i = 0; i <= K + 1; ++i) {
    // one wait covers both rewrites of a parity: the scatter slots send(i)
    // fills were folded in step i-1, the gather buffers fold(i-1) fills were
    // copied out in step i-1 (as round i-3)
    if (i >= 2 && i <= K && !wait_ack(seq0 + i - 2)) return;
    // round 0's in-counts: every peer is inside this launch (the hand-off
    // against the previous one), before send(1) and fold(0) write anything
    if (i == 1 && !wait_in(0)) return;
    if (i < K) send(i);
    if (i == 0) {
      // The last workgroup to arrive in the launch advances the launch count
      // by the rounds and the drain step, and the totals by the wide
      // two-shot's amounts.
      if (threadIdx.x == 0 && arrived + 1 == G) {
        uint64_t* st = (uint64_t*)(mine + MCCS_DIRECT_STATE);
        __hip_atomic_store((uint32_t*)(mine + MCCS_DIRECT_DONE), 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(st + MCCS_DIRECT_ST_E_IN, sh.e_in + sh.owned[rank], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        for (int t = 0; t < n; ++t)
          __hip_atomic_store(st + MCCS_DIRECT_ST_E_OUT(t), sh.e_out[t] + sh.owned[t], __ATOMIC_RELAXED,
                             __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(st + MCCS_DIRECT_ST_LAUNCHES, seq0 + K, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      continue;
    }
    if (i <= K) {
      if (i >= 2 && !wait_in(i - 1)) return;
      fold(i - 1);
    }
    if (i >= 2) {
      if (!wait_out(i - 2)) return;
      copy(i - 2);
    }
    arrive(i);
  }
  // Every peer has read every scatter slot and gather buffer of this launch:
  // the next launch of any kind may refill either at once.
  (void)wait_ack(seq0 + K);
}

template <int DT, bool PRE>
__device__ __forceinline__ void direct_wide_stream_ar_body(const mccsDirectArgs& a) {
  direct_stream_ar_body<DT, PRE, WideStreamArPath<DT, PRE>>(a);
}

}  // namespace mccs
