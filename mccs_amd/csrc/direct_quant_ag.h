// direct_quant_ag.h — block-scaled FP8 streamed AllGather for fp16 / bf16
// (mccsAllGatherQuant, an explicit call; ring_cfg.h, "Wide streamed
// ReduceScatter", last paragraph).
//
// The byte-typed AllGather above the one-shot / LL limits has only the ring:
// n-1 serial hops at 16 bits per element.  This one sends every rank's block
// to every peer at once as direct_quant.h's wire format, an OCP E4M3FN code per
// element plus one E8M0 scale byte per block of 32: 8.25 bits per element.  It
// is lossy on purpose, which is why it is a call of its own and mccsAllGather
// never takes it; the definition below is the contract.
//
// a.count = sendcount = c elements per rank, any c >= 1.  A quantisation block
// is the 32 elements [32k, 32k + 32) counted from the start of EACH RANK'S
// block (not of the receive buffer); elements past c read as +0 and are never
// stored.  QDQ is direct_quant.h's, unchanged.  On every rank, for every source
// r (the rank's OWN block included, so every rank ends with the same bits):
//   recv[r c + i] = T(QDQ(f32(x_r))[i]), one rounding to nearest even
// The bits depend on the inputs alone: not on rings, channels, workgroup
// count, round size or round count, because a round is a whole number of
// quantisation blocks.  One Inf / NaN makes its block of 32 NaN on every rank;
// a value whose code rounds up past the largest finite T (an amax of 65504 in
// fp16, of (2 - 2^-7) 2^127 in bf16) arrives as Inf, as QDQ and T() define.
// QDQ alone, on N(0,1) bf16 inputs, has a relative L2 error of 2.7e-2 (computed
// on the CPU from tests/quant_ref.py, 2^20 elements).
//
// A block moves in K = a.rounds rounds of B = a.round_elems elements (a multiple
// of 512 of at most PAY_O = MCCS_QUANT_PAY(oslot_bytes); the last round may be
// shorter).  Round k has the sequence number seq0 + k (seq0 = LAUNCHES + 1) and
// uses the one-shot slot [parity (seq0 + k) & 1][sender] of every peer, split as
// QuantStreamPath splits it: the code of round element e at byte e, the scale
// byte of the round's block j at PAY_O + j.  Per workgroup the order is
//   send(0); for k = 1 .. K: { send(k) if k < K; copy(k-1) }
//   send(k)  ONE pass over the own block's round.  A wave takes units of 512
//            elements, lane l holding 8, a quad of lanes one block, kDirectUnroll
//            units in flight: one 16-byte non-temporal load per lane
//            (quant_load8, bounded on the tail and off a pack), wide_up8, quant8
//            ONCE; then the 8 code bytes and the wave's scale row
//            (quant_scale_word) go from registers into the slots for this rank
//            of ALL n-1 peers (bases wave-uniform, QuantStreamArPath::uni), and
//            T(dequant8(codes)) goes to recv + rank c through the thread that
//            did the load.  The source is read from memory once, not n-1 times,
//            and each own element is loaded and stored by one thread, so in
//            place (send == recv + rank c) needs no self wait.  Every workgroup
//            then arrives on SEND_DONE; the last arriver adds len_k to every
//            peer's IN_CNT(rank).
//   copy(k)  wait for E_IN + k B + len_k on every peer's line; for each of the
//            n-1 sources r the round is dequantised out of the own slot for r
//            into recv + r c + k B (QuantStreamArPath::copy, kDirectUnroll units
//            in flight).  With c odd, block r starts 2 bytes off a pack for odd
//            r: vec is decided per piece.
// The pieces of the sends (one range per round) and the (source, piece) pairs
// of the copies are each numbered through ALL rounds and dealt p % G, the
// running base kept mod G by subtraction: no division per piece.
// Counts and flow control are the streamed ReduceScatter's, unchanged in
// meaning (direct_wide_stream.h; ring_cfg.h has the argument and why it carries
// over): ROUND_DONE / ACK after copy(k), k <= K-2; the round-0 counts before
// send(1), every peer's ACK >= seq0 + k-2 before send(k), and a closing ACK
// wait when K >= 2.  The launch leaves LAUNCHES += K, E_IN += c, E_OUT and
// E_SELF untouched, so any other direct launch may follow, and K = 1 sends and
// awaits no acknowledgement.  The loop is written here and not as a third path
// of direct_stream_body: that body deals n-1 foreign blocks per send and folds
// into one output, and changing it would change the eight kernels built on it.
#pragma once
#include "direct_quant_stream_ar.h"

namespace mccs {

template <int DT>
__device__ __forceinline__ void direct_quant_ag_body(const mccsDirectArgs& a) {
  using T = typename Elem<DT>::T;
  using P = QuantStreamArPath<DT, false>;  // piece, valid_of, uni and copy are its own
  __shared__ DirectShm sh;                 // (its idx2rank stays unwritten: there is no walk)
  __shared__ uint64_t need[MCCS_DIRECT_MAX_RANKS];
  const mccsDirectRank& me = a.r[blockIdx.y];
  const int n = (int)a.nranks;
  const uint32_t rank = me.rank;
  char* const mine = a.region[rank];
  volatile uint32_t* abortFlag = me.abort_flag;
  mccsRingKernelCfg ecfg{};
  ecfg.err_line = me.err_line;
  const uint64_t size = a.count;  // of one rank's block: any size
  const uint64_t K = a.rounds;
  const uint32_t B = a.round_elems;
  // Prologue and arrival count: direct_stream_body's.
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
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const uint32_t peers = ((1u << n) - 1u) & ~(1u << rank);
  const uint32_t piece = P::piece(a.piece), piece2 = P::piece(a.piece2);  // whole units
  const int64_t oslot = (int64_t)a.oslot_bytes;
  const int64_t pay = (int64_t)MCCS_QUANT_PAY(oslot);
  const int64_t obase = MCCS_DIRECT_CTRL_BYTES + (int64_t)MCCS_DIRECT_SLOTS * (int64_t)a.slot_bytes;
  // a full round's and the last round's lengths and piece counts: four divisions per launch
  const uint32_t tail = (uint32_t)(size - (K - 1) * (uint64_t)B);
  const uint32_t nps_full = (B + piece - 1) / piece, nps_tail = (tail + piece - 1) / piece;
  const uint32_t np2_full = (B + piece2 - 1) / piece2, np2_tail = (tail + piece2 - 1) / piece2;
  uint32_t sbase = 0, cbase = 0;  // (pieces sent / copied before this range) mod G, through all rounds

  // Wave 0 polls every peer's line at `cnt_base` for `v`; false: abort or watchdog.
  auto wait = [&](int cnt_base, uint64_t v) {
    if (threadIdx.x < MCCS_DIRECT_MAX_RANKS) need[threadIdx.x] = v;
    __syncthreads();
    return direct_wait(sh, mine, cnt_base, peers, need, abortFlag, a, ecfg);
  };
  // ne elements of the own block at src, at round offset off (a multiple of
  // 512): quantised once, the codes and scale bytes to every peer's slot for
  // this rank (sbase: this rank's slot of the round's parity, from a region's
  // start), the dequantised values to dst.
  auto fan_out = [&](const uint16_t* src, uint16_t* dst, int64_t sbase_off, int64_t off, int64_t ne) {
    constexpr uint32_t U = kDirectUnroll;
    const bool svec = ((uintptr_t)src & 15) == 0, dvec = ((uintptr_t)dst & 15) == 0;
    const uint32_t nu = (uint32_t)((ne + kQuantUnit - 1) / kQuantUnit);
    for (uint32_t u0 = wave; u0 < nu; u0 += nw * U) {
      u32x4 v[U];
#pragma unroll
      for (uint32_t k = 0; k < U; ++k) {
        const uint32_t u = u0 + k * nw;
        if (u < nu) v[k] = quant_load8(src + (int64_t)u * kQuantUnit + lane * 8, P::valid_of(ne, u, lane), svec);
      }
#pragma unroll
      for (uint32_t k = 0; k < U; ++k) {
        const uint32_t u = u0 + k * nw;
        if (u >= nu) continue;  // wave-uniform: every lane is active in quant8 / quant_scale_word
        const QuantCodes c = quant8(wide_up8<DT>(v[k]));
        const uint32_t sw = quant_scale_word(c.b);
        const int64_t eoff = off + (int64_t)u * kQuantUnit;  // a multiple of 512, < B <= PAY_O
#pragma unroll
        for (int r = 0; r < MCCS_DIRECT_MAX_RANKS; ++r)
          if (r < n && r != (int)rank) {
            char* const g = P::uni(a.region[r]) + sbase_off;
            *(u32x2*)(g + eoff + lane * 8) = u32x2{c.lo, c.hi};
            if (lane < 4) ((uint32_t*)(g + pay + eoff / 32))[lane] = sw;
          }
        quant_store8(dst + (int64_t)u * kQuantUnit + lane * 8, P::valid_of(ne, u, lane), dvec,
                     wide_down8<DT>(dequant8(c.lo, c.hi, c.b)));
      }
    }
  };
  // Round k of the own block: to every peer's slot for this rank and, through QDQ, to the own output block.
  auto send = [&](uint64_t k) {
    const bool last = k + 1 == K;
    const uint32_t len = last ? tail : B, nps = last ? nps_tail : nps_full;
    const int64_t roff = (int64_t)(k * (uint64_t)B);
    const int64_t pbase = obase + (int64_t)((seq0 + k) & 1) * MCCS_DIRECT_MAX_RANKS * oslot + (int64_t)rank * oslot;
    const uint16_t* const src = (const uint16_t*)me.send + roff;
    uint16_t* const dst = (uint16_t*)me.recv + (int64_t)rank * (int64_t)size + roff;
    for (uint32_t j = bx >= sbase ? bx - sbase : bx + G - sbase; j < nps && sh.ok; j += G) {
      const int64_t off = (int64_t)j * piece;
      const int64_t ne = (int64_t)len - off < (int64_t)piece ? (int64_t)len - off : (int64_t)piece;
      fan_out(src + off, dst + off, pbase, off, ne);
    }
    sbase += nps;
    while (sbase >= G) sbase -= G;
    // The round's count is indivisible, as in direct_stream_body: this
    // workgroup's writes are complete (cached arenas: written back) when it
    // arrives on SEND_DONE, with or without pieces, and the LAST of the rank's
    // workgroups to arrive adds the round's whole length to every peer's line.
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
  // Round k of the n-1 foreign blocks: out of the own slots of the round's parity, into the output.
  auto copy = [&](uint64_t k) {
    const bool last = k + 1 == K;
    const uint32_t len = last ? tail : B, np2 = last ? np2_tail : np2_full;
    const int64_t roff = (int64_t)(k * (uint64_t)B);
    const char* const slots = mine + obase + (int64_t)((seq0 + k) & 1) * MCCS_DIRECT_MAX_RANKS * oslot;
    for (uint32_t r = 0; r < (uint32_t)n; ++r) {
      if (r == rank) continue;
      const char* const slot = slots + (int64_t)r * oslot;
      T* const out = (T*)me.recv + (int64_t)r * (int64_t)size + roff;
      for (uint32_t j = bx >= cbase ? bx - cbase : bx + G - cbase; j < np2 && sh.ok; j += G) {
        const int64_t off = (int64_t)j * piece2;
        const int64_t ne = (int64_t)len - off < (int64_t)piece2 ? (int64_t)len - off : (int64_t)piece2;
        P::copy(oslot, slot, off, out + off, ne);  // (its payload is MCCS_QUANT_PAY of what it is given: a whole slot)
      }
      cbase += np2;
      while (cbase >= G) cbase -= G;
    }
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
    bool counted = k == 0;  // (no copy before round 0)
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
      // count on every peer).
      if (k == 0 && threadIdx.x == 0 && arrived + 1 == G) {
        uint64_t* st = (uint64_t*)(mine + MCCS_DIRECT_STATE);
        __hip_atomic_store((uint32_t*)(mine + MCCS_DIRECT_DONE), 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(st + MCCS_DIRECT_ST_E_IN, e_in + size, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(st + MCCS_DIRECT_ST_LAUNCHES, seq0 + K - 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
    if (k == 0) continue;
    if (!counted && !wait(MCCS_DIRECT_IN_CNT(0), e_in + cum)) return;
    copy(k - 1);
    if (k < K) arrive(k - 1);  // rounds 0 .. K-2 are acknowledged
  }
  if (K >= 2) (void)wait(MCCS_DIRECT_ACK(0), seq0 + K - 2);  // hazard 3: the next launch's first parity is read out
}

}  // namespace mccs
