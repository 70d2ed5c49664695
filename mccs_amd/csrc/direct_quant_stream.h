// direct_quant_stream.h — block-scaled FP8 streamed ReduceScatter for fp16 /
// bf16 (opt-in: mccsCommSetReduceScatterQuant; ring_cfg.h, "Wide streamed
// ReduceScatter", last paragraph).
//
// The streamed ReduceScatter (direct_wide_stream.h) moves the n-1 foreign
// blocks at 16 bits per element.  This one moves them as direct_quant.h's wire
// format, an OCP E4M3FN code per element plus one E8M0 scale byte per block of
// 32: 8.25 bits per element, once (a ReduceScatter has no gather leg, and the
// owner's own input never crosses the wire).  It is lossy on purpose; the
// definition below is the contract (tests/quant_rs_ref.py restates it in numpy).
//
// a.count = recvcount = c elements per ReduceScatter block, any c >= 1.  A
// quantisation block is the 32 elements [32k, 32k + 32) counted from the start
// of a ReduceScatter block (not of the buffer); elements past c read as +0 and
// are never stored.  QDQ is direct_quant.h's, unchanged.  For output block t on
// rank t, ranks in RANK order 0 .. n-1 whatever the rings are:
//   y_r = f32(x_r[t])           if r == t  (the owner's own input: exact)
//       = QDQ(f32(x_r[t]))      otherwise
//   t_r = y_r (Sum) or fl32(y_r x f32(s)) (PreMulSum, never an fma: wide_fold)
//   acc = t_0; acc = fl32(acc + t_r);  out = T(acc), one RNE
// The bits depend on the inputs, n and t alone: not on rings, channels,
// workgroup count, round size or round count, because a round is a whole number
// of quantisation blocks.  One Inf / NaN in a foreign input makes that block of
// 32 NaN on the owner; one in the owner's own input touches only its element.
//
// The launch IS the streamed ReduceScatter's: direct_stream_body's round loop,
// counts in elements, SEND_DONE / ROUND_DONE / ACK lines and three hazard
// waits, instantiated with the data path below (the four 16-bit kernels keep
// their registers, LDS and scratch: tools/kernel_resources.py --diff).
// Wire layout: the one-shot slot [parity][sender] is split as the FP8 AllReduce
// splits a two-shot slot: PAY_O = MCCS_QUANT_PAY(oslot_bytes) code bytes, the
// code of round element e at byte e, then the scale bytes, block k's at PAY_O +
// k.  A round holds B = a.round_elems elements, a multiple of 512 of at most
// PAY_O (1.94 times a 16-bit round of the same slot), so round offsets and
// pieces (whole units too) keep quantisation blocks whole, and the slot side is
// always whole units: only send and recv are bounded (quant_load8 /
// quant_store8: the tail unit, and blocks 2 bytes off a pack when c is odd;
// vec is decided per piece).
//   send  per foreign block a wave moves units of 512 elements, lane l holding
//         8, a quad of lanes one block: a 16-byte non-temporal load, wide_up8,
//         quant8 (amax by two DPP quad-permute steps, packed FP8 converts), 8
//         code bytes per lane and the wave's 16 scale bytes as one row
//         (quant_scale_word); kDirectUnroll units per wave in flight.
//   fold  per unit of the own block every load is issued before any arithmetic:
//         the own pack and, from each of the n-1 slots, one u32x2 of codes and
//         one scale byte; dequant8, wide_fold in rank order with the own input
//         through wide_up8 unquantised, wide_down8, quant_store8.
// In place needs no self wait, as in direct_wide_stream.h.
#pragma once
#include "direct_quant.h"
#include "direct_wide_stream.h"

namespace mccs {

template <int DT, bool PRE>
struct QuantStreamPath {
  using T = typename Elem<DT>::T;
  static_assert(sizeof(T) == 2, "8 elements are one 16-byte pack");
  // pieces are whole units (the planner's are multiples of 2048 elements)
  static __device__ __forceinline__ uint32_t piece(uint32_t p) {
    return p >= (uint32_t)kQuantUnit ? p & ~(uint32_t)(kQuantUnit - 1) : (uint32_t)kQuantUnit;
  }
  // lane's elements of unit u of a piece of ne elements: how many exist (<= 0: none)
  static __device__ __forceinline__ int valid_of(int64_t ne, uint32_t u, uint32_t lane) {
    const int64_t rem = ne - (int64_t)u * kQuantUnit - (int64_t)lane * 8;
    return rem > 8 ? 8 : (int)rem;
  }

  static __device__ __forceinline__ void send(int64_t oslot, const T* src1, char* slot, int64_t off, int64_t ne) {
    constexpr uint32_t U = kDirectUnroll;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const int64_t pay = (int64_t)MCCS_QUANT_PAY(oslot);
    const uint16_t* src = (const uint16_t*)src1;
    const bool vec = ((uintptr_t)src & 15) == 0;
    const uint32_t nu = (uint32_t)((ne + kQuantUnit - 1) / kQuantUnit);
    for (uint32_t u0 = wave; u0 < nu; u0 += nw * U) {
      u32x4 v[U];
#pragma unroll
      for (uint32_t k = 0; k < U; ++k) {
        const uint32_t u = u0 + k * nw;
        if (u < nu) v[k] = quant_load8(src + (int64_t)u * kQuantUnit + lane * 8, valid_of(ne, u, lane), vec);
      }
#pragma unroll
      for (uint32_t k = 0; k < U; ++k) {
        const uint32_t u = u0 + k * nw;
        if (u >= nu) continue;  // wave-uniform
        const QuantCodes c = quant8(wide_up8<DT>(v[k]));
        const uint32_t sw = quant_scale_word(c.b);
        const int64_t eoff = off + (int64_t)u * kQuantUnit;  // a multiple of 512, < B <= PAY_O
        *(u32x2*)(slot + eoff + lane * 8) = u32x2{c.lo, c.hi};
        if (lane < 4) ((uint32_t*)(slot + pay + eoff / 32))[lane] = sw;
      }
    }
  }

  static __device__ __forceinline__ void fold(int64_t oslot, int n, uint32_t rank, const T* own1, const char* slots,
                                              int64_t off, T* out, int64_t ne, float s) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const int64_t pay = (int64_t)MCCS_QUANT_PAY(oslot);
    const uint16_t* src = (const uint16_t*)own1;
    uint16_t* dst = (uint16_t*)out;
    const bool svec = ((uintptr_t)src & 15) == 0, dvec = ((uintptr_t)dst & 15) == 0;
    const uint32_t nu = (uint32_t)((ne + kQuantUnit - 1) / kQuantUnit);
    for (uint32_t u = wave; u < nu; u += nw) {
      const int64_t eoff = off + (int64_t)u * kQuantUnit;
      const int valid = valid_of(ne, u, lane);
      // every load of the unit is issued before any arithmetic
      const u32x4 own = quant_load8(src + (int64_t)u * kQuantUnit + lane * 8, valid, svec);
      u32x2 cw[MCCS_DIRECT_MAX_RANKS];
      uint32_t cb[MCCS_DIRECT_MAX_RANKS];
#pragma unroll
      for (int r = 0; r < MCCS_DIRECT_MAX_RANKS; ++r) {
        cw[r] = u32x2{0u, 0u};
        cb[r] = 1u;
        if (r < n && r != (int)rank) {
          const char* sl = slots + (int64_t)r * oslot;
          cw[r] = __builtin_nontemporal_load((const u32x2*)(sl + eoff + lane * 8));
          cb[r] = __builtin_nontemporal_load((const uint8_t*)(sl + pay + eoff / 32 + lane / 4));
        }
      }
      const f32x8 mine = wide_up8<DT>(own);  // exact: never quantised
      f32x8 acc{};
#pragma unroll
      for (int r = 0; r < MCCS_DIRECT_MAX_RANKS; ++r)
        if (r < n) acc = wide_fold<PRE>(acc, r == (int)rank ? mine : dequant8(cw[r][0], cw[r][1], cb[r]), s, r == 0);
      quant_store8(dst + (int64_t)u * kQuantUnit + lane * 8, valid, dvec, wide_down8<DT>(acc));
    }
  }
};

template <int DT, bool PRE>
__device__ __forceinline__ void direct_quant_stream_body(const mccsDirectArgs& a) {
  direct_stream_body<DT, PRE, QuantStreamPath<DT, PRE>>(a);
}

}  // namespace mccs
