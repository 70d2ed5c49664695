// direct_wide_stream.h — wide streamed ReduceScatter for fp16 / bf16 (opt-in:
// mccsCommSetReduceScatterWideStream; ring_cfg.h, "Wide streamed
// ReduceScatter").
//
// direct_wide_rs.h's contract for a block of ANY size: per output element,
// ranks in RANK order 0 .. n-1 whatever the rings are,
//   t_r = f32(x_r)  or  fl32(f32(x_r) * f32(s))   (PreMulSum, s in op_arg's low 16 bits)
//   acc = t_0; acc = fl32(acc + t_r); out = T(acc), one rounding to nearest even
// with the product and the sum two roundings.  Rank t receives this for block t
// (a.count = recvcount elements) of every rank's send buffer: the wide
// AllReduce's bits, sliced, and so the wide one-shot ReduceScatter's for a
// block that fits both.  They depend on neither rings, channels, workgroup
// count, round size nor round count.  The arithmetic is direct_wide.h's
// (wide_up*, wide_fold, wide_reduce, wide_down*), included and not copied.
//
// direct_wide_rs_kernel serves a block up to one one-shot slot.  Here a block
// moves through the slot in K = a.rounds rounds of B = a.round_elems elements
// (a multiple of 8, at most one slot; the last round may be shorter).  Round k
// has seq0 + k for its sequence number (seq0 = LAUNCHES + 1):
//   send(k)  the elements [k B, k B + len_k) of the n-1 foreign blocks -> the
//            owner's one-shot slot [parity (seq0 + k) & 1][sender me] at the
//            offset within the round; every workgroup then arrives on
//            SEND_DONE, and the last of the rank's workgroups to arrive adds
//            len_k to every owner's IN_CNT: a round is counted whole or not
//            at all (workgroups of one rank may be a round apart);
//   fold(k)  wait for E_IN + k B + len_k on every peer's line; wide_reduce of
//            the same range of the own block: the own input at position `rank`,
//            the n-1 slots elsewhere, in rank order, into recv + k B.
// Per workgroup the order is
//   send(0); for k = 1 .. K: { send(k) if k < K; fold(k-1) }
// so round k's bytes are on the links while round k-1 is folded.  The pieces of
// the sends (n-1 ranges per round) and of the folds are each numbered through
// ALL rounds and piece p goes to workgroup p % G; the numbering is kept mod G
// by subtraction (direct_wide_own_body's `base`), so with rounds of fewer
// pieces than workgroups the work still goes round, and no piece costs a
// division.  Block bases and round offsets are 64-bit, a round's counts 32-bit.
// Flow control (why a count proves a whole round, the three hazards, the four
// SEND_DONE and ROUND_DONE words and why the waits form no cycle: ring_cfg.h): before send(1) every workgroup waits for round
// 0's in-counts; before send(k), k >= 2, for every peer's ACK >= seq0 + k-2;
// after fold(k), k <= K-2, it arrives on ROUND_DONE, and the last arriver
// stores seq0 + k into ACK(me) of every peer; before the kernel ends, K >= 2,
// every workgroup waits for every peer's ACK >= seq0 + K-2.  Every wait is
// direct_wait (abort flag and watchdog polled, return on either); none is for
// a workgroup of the own rank.
// The launch leaves LAUNCHES += K, E_IN += count, E_OUT and E_SELF untouched;
// with K = 1 no ack is sent or awaited and the state is the wide RS
// one-shot's.  In place (recv == send + rank * recvcount) needs no self wait:
// no send reads the own block, and a fold loads and stores each element through
// one thread.  With an odd recvcount block t starts 2 bytes off a pack, so the
// copies and the own operand take direct_reduce's / wide_reduce's typed path.
//
// The round loop, its counts and its waits are written once, in
// direct_stream_body, templated on the data path: a Path supplies piece() (a
// planner's piece made usable), send() (one piece of a foreign block into a
// slot) and fold() (one piece of the own block out of the n-1 slots).
// WideStreamPath below is this file's 16-bit path; direct_quant_stream.h's
// QuantStreamPath puts FP8 codes and scale bytes into the same slots.
#pragma once
#include "direct_wide.h"

static_assert(MCCS_DIRECT_SEND_DONE(4) <= MCCS_DIRECT_CTRL_BYTES && MCCS_DIRECT_ROUND_DONE(4) <= MCCS_DIRECT_SEND_DONE(0) &&
                  MCCS_DIRECT_ACK(MCCS_DIRECT_MAX_RANKS) <= MCCS_DIRECT_ROUND_DONE(0) &&
                  MCCS_DIRECT_DONE + 4 <= MCCS_DIRECT_ACK(0),
              "the streamed ReduceScatter's lines lie in the control block's unused part");

namespace mccs {

// The 16-bit data path: element e of a round at byte 2 e of the slot.
template <int DT, bool PRE>
struct WideStreamPath {
  using T = typename Elem<DT>::T;
  static __device__ __forceinline__ uint32_t piece(uint32_t p) { return p > 0 ? p : 1; }
  // ne elements at src (a foreign block's, at round offset off) into the owner's slot for this rank
  static __device__ __forceinline__ void send(int64_t, const T* src1, char* slot, int64_t off, int64_t ne) {
    const void* src[MCCS_DIRECT_MAX_RANKS] = {src1};
    void* dst[MCCS_DIRECT_MAX_RANKS] = {slot + off * (int64_t)sizeof(T)};
    direct_reduce<DT, OpSum>(src, 1, dst, 1, ne);  // one source: a copy
  }
  // ne elements of the own block at `own` and of the n-1 slots of this parity at round offset off, into out
  static __device__ __forceinline__ void fold(int64_t oslot, int n, uint32_t rank, const T* own, const char* slots,
                                              int64_t off, T* out, int64_t ne, float s) {
    const void* src[MCCS_DIRECT_MAX_RANKS];
    void* dst[MCCS_DIRECT_MAX_RANKS] = {out};
#pragma unroll
    for (int r = 0; r < MCCS_DIRECT_MAX_RANKS; ++r)
      src[r] = r >= n           ? nullptr
               : r == (int)rank ? (const void*)own
                                : (const void*)(slots + (int64_t)r * oslot + off * (int64_t)sizeof(T));
    wide_reduce<DT, PRE>(src, n, dst, 1, ne, s);
  }
};

template <int DT, bool PRE, class Path>
__device__ __forceinline__ void direct_stream_body(const mccsDirectArgs& a) {
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
  const uint64_t size = a.count;  // of one block: any size
  const uint64_t K = a.rounds;
  const uint32_t B = a.round_elems;
  const float s = wide_scalar<DT>(a.op_arg);
  // Prologue and arrival count: direct_wide_own_body's.
  if (threadIdx.x < 64) {
    const uint32_t lane = threadIdx.x;
    uint64_t v = 0;
    if (lane < MCCS_DIRECT_ST_WORDS)
      v = __hip_atomic_load((uint64_t*)(mine + MCCS_DIRECT_STATE) + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (lane == MCCS_DIRECT_ST_LAUNCHES) sh.seq = v + 1;
    if (lane == MCCS_DIRECT_ST_E_IN) sh.e_in = v;
    if (lane == MCCS_DIRECT_ST_WORDS) sh.ok = v == 0;
    if (lane < MCCS_DIRECT_MAX_RANKS) sh.region[lane] = a.region[lane];
  }
  uint32_t arrived = 0;
  if (threadIdx.x == 0) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    arrived = __hip_atomic_fetch_add((uint32_t*)(mine + MCCS_DIRECT_DONE), 1u, __ATOMIC_RELAXED,
                                     __HIP_MEMORY_SCOPE_AGENT);
  }
  __syncthreads();
  const uint64_t seq0 = sh.seq, e_in = sh.e_in;
  const uint32_t G = gridDim.x, bx = blockIdx.x;
  const uint32_t peers = ((1u << n) - 1u) & ~(1u << rank);
  const uint32_t piece = Path::piece(a.piece), piece2 = Path::piece(a.piece2);
  const int64_t oslot = (int64_t)a.oslot_bytes;
  const int64_t obase = MCCS_DIRECT_CTRL_BYTES + (int64_t)MCCS_DIRECT_SLOTS * (int64_t)a.slot_bytes;
  // a full round's and the last round's lengths and piece counts: four divisions per launch
  const uint32_t tail = (uint32_t)(size - (K - 1) * (uint64_t)B);
  const uint32_t nps_full = (B + piece - 1) / piece, nps_tail = (tail + piece - 1) / piece;
  const uint32_t np2_full = (B + piece2 - 1) / piece2, np2_tail = (tail + piece2 - 1) / piece2;
  uint32_t sbase = 0, fbase = 0;  // (pieces sent / folded before this range) mod G, through all rounds

  // Wave 0 polls every peer's line at `cnt_base` for `v`; false: abort or watchdog.
  auto wait = [&](int cnt_base, uint64_t v) {
    if (threadIdx.x < MCCS_DIRECT_MAX_RANKS) need[threadIdx.x] = v;
    __syncthreads();
    return direct_wait(sh, mine, cnt_base, peers, need, abortFlag, a, ecfg);
  };
  // Round k of the n-1 foreign blocks, to their owners' slots for this rank.
  auto send = [&](uint64_t k) {
    const bool last = k + 1 == K;
    const uint32_t len = last ? tail : B, nps = last ? nps_tail : nps_full;
    const int64_t roff = (int64_t)(k * (uint64_t)B);
    const int64_t pbase = obase + (int64_t)((seq0 + k) & 1) * MCCS_DIRECT_MAX_RANKS * oslot + (int64_t)rank * oslot;
    for (uint32_t t = 0; t < (uint32_t)n; ++t) {
      if (t == rank) continue;
      const T* const blk = (const T*)me.send + (int64_t)t * (int64_t)size + roff;
      char* const slot = sh.region[t] + pbase;
      for (uint32_t j = bx >= sbase ? bx - sbase : bx + G - sbase; j < nps && sh.ok; j += G) {
        const int64_t off = (int64_t)j * piece;
        const int64_t ne = (int64_t)len - off < (int64_t)piece ? (int64_t)len - off : (int64_t)piece;
        Path::send(oslot, blk + off, slot, off, ne);
      }
      sbase += nps;
      while (sbase >= G) sbase -= G;
    }
    // The round's count is indivisible: this workgroup's writes are complete
    // (and, for cached arenas, written back: direct_count_out's fence) when it
    // arrives on SEND_DONE, with or without pieces, and the LAST of the rank's
    // workgroups to arrive adds the round's whole length to every owner's line.
    // So an owner that sees E_IN + k B + len has all of rounds 0 .. k from this
    // rank, whatever round this rank's other workgroups are in.
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0 && sh.ok) {
      if (a.fence_mode != MCCS_FENCE_UNCACHED) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
      uint32_t* const cnt = (uint32_t*)(mine + MCCS_DIRECT_SEND_DONE((seq0 + k) & 3));
      if (__hip_atomic_fetch_add(cnt, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1 == G) {
        __hip_atomic_store(cnt, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        for (int t = 0; t < n; ++t)
          if (t != (int)rank)
            __hip_atomic_fetch_add((uint64_t*)(sh.region[t] + MCCS_DIRECT_IN_CNT(rank)), (uint64_t)len,
                                   __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        // the word is back at 0 before this workgroup can arrive anywhere again
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
    }
  };
  // Round k of the own block: every source in rank order, into the output.
  auto fold = [&](uint64_t k) {
    const bool last = k + 1 == K;
    const uint32_t len = last ? tail : B, np2 = last ? np2_tail : np2_full;
    const int64_t roff = (int64_t)(k * (uint64_t)B);
    const char* const slots = mine + obase + (int64_t)((seq0 + k) & 1) * MCCS_DIRECT_MAX_RANKS * oslot;
    const T* const own = (const T*)me.send + (int64_t)rank * (int64_t)size + roff;
    for (uint32_t j = bx >= fbase ? bx - fbase : bx + G - fbase; j < np2 && sh.ok; j += G) {
      const int64_t off = (int64_t)j * piece2;
      const int64_t ne = (int64_t)len - off < (int64_t)piece2 ? (int64_t)len - off : (int64_t)piece2;
      Path::fold(oslot, n, rank, own + off, slots, off, (T*)me.recv + roff + off, ne, s);
    }
    fbase += np2;
    while (fbase >= G) fbase -= G;
  };
  // This workgroup has read all it reads of round k's slots; the last of the
  // rank's workgroups to say so tells every peer (hazard 1's acknowledgement).
  auto arrive = [&](uint64_t k) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0 && sh.ok) {
      uint32_t* const cnt = (uint32_t*)(mine + MCCS_DIRECT_ROUND_DONE((seq0 + k) & 3));
      if (__hip_atomic_fetch_add(cnt, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1 == G) {
        __hip_atomic_store(cnt, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        for (int t = 0; t < n; ++t)
          if (t != (int)rank)
            __hip_atomic_store((uint64_t*)(sh.region[t] + MCCS_DIRECT_ACK(rank)), seq0 + k, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_SYSTEM);
        // drained before this workgroup can arrive anywhere again: ACK only grows
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
    }
  };

  for (uint64_t k = 0; k <= K; ++k) {
    // elements every sender has counted once round k-1 is complete
    const uint64_t cum = k == K ? size : k * (uint64_t)B;
    bool counted = k == 0;  // (no fold before round 0)
    if (k < K) {
      if (k == 1) {  // hazard 2: every peer is inside this launch
        if (!wait(MCCS_DIRECT_IN_CNT(0), e_in + cum)) return;
        counted = true;
      } else if (k >= 2 && !wait(MCCS_DIRECT_ACK(0), seq0 + k - 2)) {  // hazard 1: round k-2's parity is read out
        return;
      }
      send(k);
      // The last workgroup to arrive in the launch advances the launch count
      // by the rounds and E_IN by the block (every sender adds every round's
      // count on every owner).
      if (k == 0 && threadIdx.x == 0 && arrived + 1 == G) {
        uint64_t* st = (uint64_t*)(mine + MCCS_DIRECT_STATE);
        __hip_atomic_store((uint32_t*)(mine + MCCS_DIRECT_DONE), 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(st + MCCS_DIRECT_ST_E_IN, e_in + size, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(st + MCCS_DIRECT_ST_LAUNCHES, seq0 + K - 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
    if (k == 0) continue;
    if (!counted && !wait(MCCS_DIRECT_IN_CNT(0), e_in + cum)) return;
    fold(k - 1);
    if (k < K) arrive(k - 1);  // rounds 0 .. K-2 are acknowledged
  }
  if (K >= 2) (void)wait(MCCS_DIRECT_ACK(0), seq0 + K - 2);  // hazard 3: the next launch's first parity is read out
}

template <int DT, bool PRE>
__device__ __forceinline__ void direct_wide_stream_body(const mccsDirectArgs& a) {
  direct_stream_body<DT, PRE, WideStreamPath<DT, PRE>>(a);
}

}  // namespace mccs
