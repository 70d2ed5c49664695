// direct_quant_stream_ar.h — block-scaled FP8 streamed AllReduce for fp16 /
// bf16 (opt-in: mccsCommSetAllReduceQuantStream; ring_cfg.h, "Wide streamed
// AllReduce", last paragraph).
//
// direct_quant.h's contract, unchanged, for a buffer of ANY size: a
// quantisation block is the 32 elements [32k, 32k + 32) counted from the start
// of the buffer, every rank's input goes through QDQ (the owner's own
// included), the fold runs in binary32 in RANK order (wide_fold, PreMulSum
// never fused), the sum goes through QDQ again and is rounded once to T; the
// same bits on every rank.  The split is MCCS_QUANT_SHARE (shares start on
// multiples of 512 elements) and a round is a whole number of 512-element
// units, so share bases and round offsets keep quantisation blocks whole: the
// bits depend on the inputs and n alone, not on rings, workgroup count, round
// size or round count, and are direct_quant_kernel's for a size that fits
// both.  One Inf / NaN makes its block of 32 NaN on every rank.
//
// The launch IS the streamed AllReduce's: direct_stream_ar_body's round loop,
// counts in elements, IN_CNT / SEND_DONE, OUT_CNT / FOLD_DONE, ACK / ROUND_DONE,
// the one ACK wait per step, the round-0 hand-off and the closing wait,
// instantiated with the data path below (tools/kernel_resources.py --diff
// against the parent: 4 kernels added, none changed).
// Wire layout, both legs split as the FP8 AllReduce splits a two-shot slot:
//   scatter  the one-shot slot [parity][sender], PAY_O = MCCS_QUANT_PAY(
//            oslot_bytes) code bytes, the code of round element e at byte e,
//            the scale byte of the round's block k at PAY_O + k
//            (QuantStreamPath's layout and its send, reused);
//   gather   the half [parity] (floor16(slot_bytes / 2) bytes) of peer t's
//            two-shot in slot [owner], PAY_H = MCCS_QUANT_PAY(half) code bytes,
//            codes and scale bytes placed the same way.
// A round holds B = a.round_elems elements, a multiple of 512 of at most
// min(PAY_O, PAY_H); pieces are whole units, so the slot side is always whole
// units (a tail unit's padding travels as zero codes, never stored to recv) and only send and recv are
// bounded (quant_load8 / quant_store8: the tail unit, and operands off a
// 16-byte boundary; vec is decided per piece).  A wave moves units of 512
// elements, lane l holding 8, a quad of lanes one block:
//   send  QuantStreamPath::send: a 16-byte non-temporal load, quant8, 8 code
//         bytes per lane and one 16-byte scale row per wave into the owner's
//         scatter slot; kDirectUnroll units per wave in flight.
//   fold  per unit of the own share every load is issued before any
//         arithmetic: the own pack, n-1 u32x2 of codes and n-1 scale bytes;
//         QDQ of the own input in registers, dequant8 of the others, wide_fold
//         in rank order, quant8(acc); the codes and the scale row go to EVERY
//         peer's gather half, T(dequant8(codes)) to recv.
//   copy  codes and scales from the own gather halves, dequant8, wide_down8,
//         into recv; kDirectUnroll units per wave in flight.
// send(k) and copy(k) deal their pieces through direct_stream_ar_body's one
// function with equal counters and split a piece into units alike (unit u to
// wave u mod waves), so in place is safe by ring_cfg.h's argument.
#pragma once
#include "direct_quant_stream.h"
#include "direct_wide_stream_ar.h"

namespace mccs {

template <int DT, bool PRE>
struct QuantStreamArPath : QuantStreamPath<DT, PRE> {
  using P = QuantStreamPath<DT, PRE>;
  using T = typename P::T;
  static __device__ __forceinline__ uint64_t share(uint64_t count, uint64_t n) { return MCCS_QUANT_SHARE(count, n); }

  // a table entry is the same on every lane: keep it in scalar registers
  static __device__ __forceinline__ char* uni(const void* p) {
    const uint64_t v = (uint64_t)(uintptr_t)p;
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32));
    return (char*)(uintptr_t)(((uint64_t)hi << 32) | lo);
  }
  // codes and scale bytes are addressed from the start of a slot or half: the tables hold the bases
  static __device__ __forceinline__ int64_t at(int64_t) { return 0; }
  // ne elements of the own share at round offset off, in rank order: from[r]
  // the own input (r == rank) or scatter slot r, to[r] the output or peer r's
  // gather half for this rank
  static __device__ __forceinline__ void fold(int64_t oslot, int64_t half, int n, uint32_t rank, const void** from,
                                              void** to, int64_t off, int64_t ne, float s) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const int64_t pay_o = (int64_t)MCCS_QUANT_PAY(oslot), pay_h = (int64_t)MCCS_QUANT_PAY(half);
    const uint16_t* src = nullptr;
    uint16_t* dst = nullptr;
#pragma unroll
    for (int r = 0; r < MCCS_DIRECT_MAX_RANKS; ++r)
      if (r == (int)rank) {
        src = (const uint16_t*)from[r];
        dst = (uint16_t*)to[r];
      }
    const bool svec = ((uintptr_t)src & 15) == 0, dvec = ((uintptr_t)dst & 15) == 0;
    const uint32_t nu = (uint32_t)((ne + kQuantUnit - 1) / kQuantUnit);
    for (uint32_t u = wave; u < nu; u += nw) {
      const int64_t eoff = off + (int64_t)u * kQuantUnit;  // a multiple of 512, < B <= min(PAY_O, PAY_H)
      const int valid = P::valid_of(ne, u, lane);
      // every load of the unit is issued before any arithmetic
      const u32x4 own = quant_load8(src + (int64_t)u * kQuantUnit + lane * 8, valid, svec);
      u32x2 cw[MCCS_DIRECT_MAX_RANKS];
      uint32_t cb[MCCS_DIRECT_MAX_RANKS];
#pragma unroll
      for (int r = 0; r < MCCS_DIRECT_MAX_RANKS; ++r) {
        cw[r] = u32x2{0u, 0u};
        cb[r] = 1u;
        if (r < n && r != (int)rank) {
          const char* sl = uni(from[r]);
          cw[r] = __builtin_nontemporal_load((const u32x2*)(sl + eoff + lane * 8));
          cb[r] = __builtin_nontemporal_load((const uint8_t*)(sl + pay_o + eoff / 32 + lane / 4));
        }
      }
      const QuantCodes oc = quant8(wide_up8<DT>(own));  // the own input is quantised too
      f32x8 acc{};
#pragma unroll
      for (int r = 0; r < MCCS_DIRECT_MAX_RANKS; ++r)
        if (r < n) {
          const bool self = r == (int)rank;
          const f32x8 y = dequant8(self ? oc.lo : cw[r][0], self ? oc.hi : cw[r][1], self ? oc.b : cb[r]);
          acc = wide_fold<PRE>(acc, y, s, r == 0);
        }
      const QuantCodes zc = quant8(acc);
      const uint32_t sw = quant_scale_word(zc.b);
#pragma unroll
      for (int r = 0; r < MCCS_DIRECT_MAX_RANKS; ++r)
        if (r < n && r != (int)rank) {
          char* const g = uni(to[r]);
          *(u32x2*)(g + eoff + lane * 8) = u32x2{zc.lo, zc.hi};
          if (lane < 4) ((uint32_t*)(g + pay_h + eoff / 32))[lane] = sw;
        }
      quant_store8(dst + (int64_t)u * kQuantUnit + lane * 8, valid, dvec, wide_down8<DT>(dequant8(zc.lo, zc.hi, zc.b)));
    }
  }

  // ne elements of a foreign share's results, from this rank's gather half for their owner at round offset off
  static __device__ __forceinline__ void copy(int64_t half, const char* gath, int64_t off, T* out, int64_t ne) {
    constexpr uint32_t U = kDirectUnroll;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const int64_t pay_h = (int64_t)MCCS_QUANT_PAY(half);
    uint16_t* dst = (uint16_t*)out;
    const bool vec = ((uintptr_t)dst & 15) == 0;
    const uint32_t nu = (uint32_t)((ne + kQuantUnit - 1) / kQuantUnit);
    for (uint32_t u0 = wave; u0 < nu; u0 += nw * U) {
      u32x2 cw[U];
      uint32_t cb[U];
#pragma unroll
      for (uint32_t k = 0; k < U; ++k) {
        const uint32_t u = u0 + k * nw;
        if (u >= nu) continue;  // wave-uniform
        const int64_t eoff = off + (int64_t)u * kQuantUnit;
        cw[k] = __builtin_nontemporal_load((const u32x2*)(gath + eoff + lane * 8));
        cb[k] = __builtin_nontemporal_load((const uint8_t*)(gath + pay_h + eoff / 32 + lane / 4));
      }
#pragma unroll
      for (uint32_t k = 0; k < U; ++k) {
        const uint32_t u = u0 + k * nw;
        if (u >= nu) continue;
        quant_store8(dst + (int64_t)u * kQuantUnit + lane * 8, P::valid_of(ne, u, lane), vec,
                     wide_down8<DT>(dequant8(cw[k][0], cw[k][1], cb[k])));
      }
    }
  }
};

template <int DT, bool PRE>
__device__ __forceinline__ void direct_quant_stream_ar_body(const mccsDirectArgs& a) {
  direct_stream_ar_body<DT, PRE, QuantStreamArPath<DT, PRE>>(a);
}

}  // namespace mccs
