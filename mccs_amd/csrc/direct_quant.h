// direct_quant.h — block-scaled FP8 direct AllReduce for fp16 / bf16 (opt-in:
// mccsCommSetAllReduceQuant; ring_cfg.h, "Block-scaled FP8 AllReduce").
//
// Every other AllReduce moves a 16-bit element as 16 bits.  This one moves it
// as an OCP E4M3FN code plus one E8M0 scale byte per block of 32 elements
// (the MX layout): 8.25 bits per element on the wire, twice.  It is lossy on
// purpose; the definition below is the contract (tests/quant_ref.py restates
// it in numpy), and the result is a function of the inputs and n alone.
//
// A block is the 32 elements at absolute indices [32k, 32k + 32) of the buffer;
// elements past count are +0 and never stored.  QDQ(y), y one block in binary32:
//   amax = max |y_i|, f = its biased exponent field.  Any Inf / NaN (f = 255):
//   scale byte b = 255, every element dequantises to NaN.  Else b = max(f - 7,
//   1), scale 2^(b - 127) (b is never 0: the scale is never a denormal);
//   v_i = y_i x 2^(127 - b), |v_i| < 256 (nothing saturates); code c_i = v_i
//   rounded to nearest even onto E4M3FN, subnormals and the sign (of zeros
//   too) kept; d_i = e4m3(c_i) x 2^(b - 127), exact in binary32.
// Per block, ranks in RANK order 0 .. n-1 whatever the rings are:
//   y_r = QDQ(f32(x_r))      every rank's input, the owner's own included
//   t_r = y_r (Sum) or fl32(y_r x f32(s)) (PreMulSum, never an fma: wide_fold)
//   acc = t_0; acc = fl32(acc + t_r);  z = QDQ(acc);  out_i = T(z_i), one RNE
// One Inf / NaN, or a sum that leaves binary32, makes its block of 32 NaN on
// every rank: documented, not fixed.
//
// The launch is the wide two-shot's (direct_wide.h: blockIdx.y = rank slot, G
// workgroups of MCCS_DIRECT_THREADS, launch guard, prologue, arrival count,
// state words left as a two-shot with owned[] leaves them), with a data path
// of its own.  A wave moves UNITS of 512 elements: lane l holds elements 8l ..
// 8l + 7, so a quad of lanes is one block.
//   load     one 16-byte non-temporal load per lane, widened by wide_up8; the
//            tail and a misaligned send / recv take 2-byte loads / stores into
//            the same pack, so the arithmetic below is the only one
//   amax     on the magnitudes' bit patterns as integers (orders finite
//            values, puts Inf / NaN on top): 7 v_max_u32, then two DPP
//            quad-permute steps; no LDS
//   codes    y x 2^(127 - b) (exact), then v_cvt_pk_fp8_f32 four times: 8 bytes
//            per lane, 512 contiguous bytes per wave
//   scales   the 16 bytes of a wave are gathered by ds_bpermute into lanes
//            0 .. 3, one word each: one 16-byte row per store instruction
//   decode   v_cvt_pk_f32_fp8, times 2^(b - 127) as a binary32 bit pattern
//            (b = 255: a NaN)
// The packed converts are used for every input class: gfx950's are OCP E4M3FN
// with round-to-nearest-even, subnormal results and signed zeros, which is the
// definition; no class falls back to integer arithmetic.
// The slot side is always whole units (PAY is a multiple of 512 and count <=
// PAY), so slot loads and stores are never bounded; send and recv are.
//   1. scatter: the foreign shares, quantised from send into the owner's in
//      slot for this rank (kDirectUnroll units per wave in flight); count.
//   2. fold: wait; per unit of the own share the n-1 in slots are decoded, the
//      own input goes through QDQ in registers, the fold runs in rank order,
//      QDQ(acc) goes as codes + scales to every peer's out slot and as T(z)
//      to recv; count.
//   3. gather: wait; the foreign shares, decoded from the own out slot to recv.
// Phases 1 and 3 deal identical pieces and units (in place is safe: ring_cfg.h).
#pragma once
#include "direct_wide.h"

static_assert(sizeof(mccsDirectArgs) <= 4096, "quant direct launch arguments must stay within 4 KiB");

namespace mccs {

using u32x2 = uint32_t __attribute__((ext_vector_type(2)));
using f32x2 = float __attribute__((ext_vector_type(2)));

constexpr int kQuantUnit = MCCS_QUANT_UNIT;  // elements per wave iteration: 64 lanes x 8
static_assert(kQuantUnit == 64 * 8, "one lane holds 8 elements, one quad of lanes one block of 32");

// 8 codes of one lane (element i in byte i of lo | hi << 32) and its block's
// scale byte (the same on the 4 lanes of the quad).
struct QuantCodes {
  uint32_t lo, hi, b;
};

// max over the 4 lanes of a quad: quad_perm [1,0,3,2], then [2,3,0,1].  Every
// lane of the wave is active wherever this is called.
__device__ __forceinline__ uint32_t quant_quad_umax(uint32_t m) {
  const uint32_t a = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)m, 0xB1, 0xf, 0xf, true);
  m = a > m ? a : m;
  const uint32_t c = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)m, 0x4E, 0xf, 0xf, true);
  return c > m ? c : m;
}

__device__ __forceinline__ QuantCodes quant8(const f32x8& y) {
  uint32_t m = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const float e = y[i];  // (a bit_cast of the vector element itself reads element 0 for every i)
    const uint32_t a = __builtin_bit_cast(uint32_t, e) & 0x7fffffffu;
    m = a > m ? a : m;
  }
  m = quant_quad_umax(m);
  const uint32_t f = m >> 23;
  QuantCodes q;
  q.b = f == 255u ? 255u : f > 8u ? f - 7u : 1u;
  // 2^(127 - b) for b in 1 .. 248 (a normal number); b = 255: the codes are
  // never decoded, any multiplier does
  const float mul = __builtin_bit_cast(float, q.b == 255u ? 0u : (254u - q.b) << 23);
  int lo = 0, hi = 0;
  lo = __builtin_amdgcn_cvt_pk_fp8_f32(y[0] * mul, y[1] * mul, lo, false);
  lo = __builtin_amdgcn_cvt_pk_fp8_f32(y[2] * mul, y[3] * mul, lo, true);
  hi = __builtin_amdgcn_cvt_pk_fp8_f32(y[4] * mul, y[5] * mul, hi, false);
  hi = __builtin_amdgcn_cvt_pk_fp8_f32(y[6] * mul, y[7] * mul, hi, true);
  q.lo = (uint32_t)lo;
  q.hi = (uint32_t)hi;
  return q;
}

__device__ __forceinline__ f32x8 dequant8(uint32_t lo, uint32_t hi, uint32_t b) {
  const float s = __builtin_bit_cast(float, b == 255u ? 0x7fc00000u : b << 23);
  const f32x2 p0 = __builtin_amdgcn_cvt_pk_f32_fp8((int)lo, false), p1 = __builtin_amdgcn_cvt_pk_f32_fp8((int)lo, true);
  const f32x2 p2 = __builtin_amdgcn_cvt_pk_f32_fp8((int)hi, false), p3 = __builtin_amdgcn_cvt_pk_f32_fp8((int)hi, true);
  return f32x8{p0[0] * s, p0[1] * s, p1[0] * s, p1[1] * s, p2[0] * s, p2[1] * s, p3[0] * s, p3[1] * s};
}

// Elements p[0 .. 8) of a send / recv buffer as one pack; only the first
// `valid` (any int; <= 0: none) exist, the rest read as +0 and are not stored.
// vec: p is 16-byte aligned.
__device__ __forceinline__ u32x4 quant_load8(const uint16_t* p, int valid, bool vec) {
  if (vec && valid >= 8) return __builtin_nontemporal_load((const u32x4*)p);
  uint32_t h[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) h[i] = i < valid ? (uint32_t)__builtin_nontemporal_load(p + i) : 0u;
  return u32x4{h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16), h[6] | (h[7] << 16)};
}
__device__ __forceinline__ void quant_store8(uint16_t* p, int valid, bool vec, u32x4 v) {
  if (vec && valid >= 8) {
    *(u32x4*)p = v;
    return;
  }
#pragma unroll
  for (int i = 0; i < 8; ++i)
    if (i < valid) p[i] = (uint16_t)(v[i / 2] >> (16 * (i & 1)));
}

// The wave's 16 scale bytes as 4 words: lane L < 4 gets the bytes of quads
// 4L .. 4L + 3, i.e. of lanes 16L + 4k (every lane active).
__device__ __forceinline__ uint32_t quant_scale_word(uint32_t b) {
  const uint32_t lane = threadIdx.x & 63u;
  uint32_t w = 0;
#pragma unroll
  for (uint32_t k = 0; k < 4; ++k)
    w |= (uint32_t)__builtin_amdgcn_ds_bpermute((int)(((lane & 3u) * 16u + k * 4u) * 4u), (int)b) << (8 * k);
  return w;
}

template <int DT, bool PRE>
__device__ __forceinline__ void direct_quant_body(const mccsDirectArgs& a) {
  __shared__ DirectShm sh;
  __shared__ uint64_t need[MCCS_DIRECT_MAX_RANKS];
  const mccsDirectRank& me = a.r[blockIdx.y];
  const int n = (int)a.nranks;
  char* const mine = a.region[me.rank];
  volatile uint32_t* abortFlag = me.abort_flag;
  mccsRingKernelCfg ecfg{};
  ecfg.err_line = me.err_line;
  const uint32_t size = (uint32_t)a.count;  // <= PAY < 2^30
  const float s = wide_scalar<DT>(a.op_arg);
  // Prologue and arrival count: direct_body's.
  if (threadIdx.x < 64) {
    const uint32_t lane = threadIdx.x;
    uint64_t v = 0;
    if (lane < MCCS_DIRECT_ST_WORDS)
      v = __hip_atomic_load((uint64_t*)(mine + MCCS_DIRECT_STATE) + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (lane == MCCS_DIRECT_ST_LAUNCHES) sh.seq = v + 1;
    if (lane == MCCS_DIRECT_ST_E_IN) sh.e_in = v;
    if (lane >= 2 && lane < 2 + MCCS_DIRECT_MAX_RANKS) sh.e_out[lane - 2] = v;
    if (lane == MCCS_DIRECT_ST_E_SELF) sh.e_self = v;
    if (lane == MCCS_DIRECT_ST_WORDS) sh.ok = v == 0;
    if (lane < MCCS_DIRECT_MAX_RANKS) {
      sh.owned[lane] = a.owned[lane];
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
  const uint32_t G = gridDim.x, bx = blockIdx.x;
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const uint32_t peers = ((1u << n) - 1u) & ~(1u << me.rank);
  // pieces are whole units (the planner's are multiples of 2048 elements)
  const uint32_t piece = a.piece >= (uint32_t)kQuantUnit ? a.piece & ~(uint32_t)(kQuantUnit - 1) : kQuantUnit;
  const uint32_t piece2 = a.piece2 >= (uint32_t)kQuantUnit ? a.piece2 & ~(uint32_t)(kQuantUnit - 1) : kQuantUnit;
  // The last workgroup to arrive advances the totals and the launch count by
  // the two-shot's amounts for owned[].
  auto advance = [&]() {
    if (threadIdx.x == 0 && arrived + 1 == G) {
      uint64_t* st = (uint64_t*)(mine + MCCS_DIRECT_STATE);
      __hip_atomic_store((uint32_t*)(mine + MCCS_DIRECT_DONE), 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(st + MCCS_DIRECT_ST_E_IN, sh.e_in + sh.owned[me.rank], __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_AGENT);
      for (int t = 0; t < n; ++t)
        __hip_atomic_store(st + MCCS_DIRECT_ST_E_OUT(t), sh.e_out[t] + sh.owned[t], __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(st + MCCS_DIRECT_ST_LAUNCHES, seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  };
  const int64_t slot = (int64_t)a.slot_bytes;
  const int64_t pay = (int64_t)MCCS_QUANT_PAY(a.slot_bytes);
  auto in_slot = [&](char* region, uint32_t sender) { return region + MCCS_DIRECT_CTRL_BYTES + (int64_t)sender * slot; };
  auto out_slot = [&](char* region) { return region + MCCS_DIRECT_CTRL_BYTES + (int64_t)MCCS_DIRECT_MAX_RANKS * slot; };
  // codes and scales of the unit at element eoff, to / from a slot
  auto put = [&](char* sl, int64_t eoff, const QuantCodes& q, uint32_t sw) {
    *(u32x2*)(sl + eoff + lane * 8) = u32x2{q.lo, q.hi};
    if (lane < 4) ((uint32_t*)(sl + pay + eoff / 32))[lane] = sw;
  };
  const uint32_t q = (uint32_t)MCCS_QUANT_SHARE(size, (uint32_t)n);  // one 32-bit division per launch
  // lane's elements of unit u of the piece at off with ne elements: how many exist (<= 0: none)
  auto valid_of = [&](int64_t ne, uint32_t u) {
    const int64_t rem = ne - (int64_t)u * kQuantUnit - (int64_t)lane * 8;
    return rem > 8 ? 8 : (int)rem;
  };
  // The pieces of the n-1 foreign shares, numbered through; piece p belongs to
  // workgroup p % G in phase 1 and in phase 3.  f(owner, off, ne); false: stop.
  auto foreign = [&](auto&& f) {
    uint32_t base = 0;
    for (uint32_t t = 0; t < (uint32_t)n; ++t) {
      const uint32_t lo = t * q;  // (n - 1) q < count + 512 n: no wrap
      if (t == me.rank || lo >= size) continue;
      const uint32_t len = size - lo < q ? size - lo : q;
      const uint32_t nps = (len + piece - 1) / piece;
      for (uint32_t j = bx >= base ? bx - base : bx + G - base; j < nps && sh.ok; j += G) {
        const uint32_t so = j * piece;
        if (!f(t, (int64_t)(lo + so), (int64_t)(len - so < piece ? len - so : piece))) return;
      }
      base += nps;
      while (base >= G) base -= G;
    }
  };
  // 1. every foreign share, quantised, to its owner's in slot for this rank
  foreign([&](uint32_t t, int64_t off, int64_t ne) {
    constexpr uint32_t U = kDirectUnroll;
    const uint16_t* src = (const uint16_t*)me.send + off;
    const bool vec = ((uintptr_t)src & 15) == 0;
    char* const sl = in_slot(sh.region[t], me.rank);
    const uint32_t nu = (uint32_t)((ne + kQuantUnit - 1) / kQuantUnit);
    for (uint32_t u0 = wave; u0 < nu; u0 += nw * U) {
      u32x4 v[U];
#pragma unroll
      for (uint32_t k = 0; k < U; ++k) {
        const uint32_t u = u0 + k * nw;
        if (u < nu) v[k] = quant_load8(src + (int64_t)u * kQuantUnit + lane * 8, valid_of(ne, u), vec);
      }
#pragma unroll
      for (uint32_t k = 0; k < U; ++k) {
        const uint32_t u = u0 + k * nw;
        if (u >= nu) continue;  // wave-uniform
        const QuantCodes c = quant8(wide_up8<DT>(v[k]));
        put(sl, off + (int64_t)u * kQuantUnit, c, quant_scale_word(c.b));
      }
    }
    if (threadIdx.x == 0) sh.sent[t] += (uint64_t)ne;
    return true;
  });
  direct_count_out(sh, a, me, MCCS_DIRECT_IN_CNT(0));
  advance();
  // 2. the own share: QDQ of every source in rank order, folded, QDQ again ->
  // the output and every peer's out slot
  if (threadIdx.x < MCCS_DIRECT_MAX_RANKS) need[threadIdx.x] = sh.e_in + sh.owned[me.rank];
  __syncthreads();
  {
    const uint32_t lo = me.rank * q;
    const uint32_t len = lo >= size ? 0 : size - lo < q ? size - lo : q;
    const uint32_t np2 = (len + piece2 - 1) / piece2;
    bool in_seen = false;  // uniform across the workgroup, like out_seen below
    for (uint32_t j = bx; j < np2 && sh.ok; j += G) {
      if (!in_seen) {
        if (!direct_wait(sh, mine, MCCS_DIRECT_IN_CNT(0), peers, need, abortFlag, a, ecfg)) break;
        in_seen = true;
      }
      const uint32_t so = j * piece2;
      const int64_t off = (int64_t)(lo + so);
      const int64_t ne = (int64_t)(len - so < piece2 ? len - so : piece2);
      const uint16_t* src = (const uint16_t*)me.send + off;
      uint16_t* dst = (uint16_t*)me.recv + off;
      const bool svec = ((uintptr_t)src & 15) == 0, dvec = ((uintptr_t)dst & 15) == 0;
      const uint32_t nu = (uint32_t)((ne + kQuantUnit - 1) / kQuantUnit);
      for (uint32_t u = wave; u < nu; u += nw) {
        const int64_t eoff = off + (int64_t)u * kQuantUnit;
        const int valid = valid_of(ne, u);
        // every load of the unit is issued before any arithmetic
        const u32x4 own = quant_load8(src + (int64_t)u * kQuantUnit + lane * 8, valid, svec);
        u32x2 cw[MCCS_DIRECT_MAX_RANKS];
        uint32_t cb[MCCS_DIRECT_MAX_RANKS];
#pragma unroll
        for (int r = 0; r < MCCS_DIRECT_MAX_RANKS; ++r) {
          cw[r] = u32x2{0u, 0u};
          cb[r] = 1u;
          if (r < n && r != (int)me.rank) {
            const char* sl = in_slot(mine, (uint32_t)r);
            cw[r] = __builtin_nontemporal_load((const u32x2*)(sl + eoff + lane * 8));
            cb[r] = __builtin_nontemporal_load((const uint8_t*)(sl + pay + eoff / 32 + lane / 4));
          }
        }
        const QuantCodes oc = quant8(wide_up8<DT>(own));
        f32x8 acc{};
#pragma unroll
        for (int r = 0; r < MCCS_DIRECT_MAX_RANKS; ++r)
          if (r < n) {
            const bool self = r == (int)me.rank;
            const f32x8 y = dequant8(self ? oc.lo : cw[r][0], self ? oc.hi : cw[r][1], self ? oc.b : cb[r]);
            acc = wide_fold<PRE>(acc, y, s, r == 0);
          }
        const QuantCodes zc = quant8(acc);
        const uint32_t sw = quant_scale_word(zc.b);
#pragma unroll
        for (int r = 0; r < MCCS_DIRECT_MAX_RANKS; ++r)
          if (r < n && r != (int)me.rank) put(out_slot(sh.region[r]), eoff, zc, sw);
        quant_store8(dst + (int64_t)u * kQuantUnit + lane * 8, valid, dvec,
                     wide_down8<DT>(dequant8(zc.lo, zc.hi, zc.b)));
      }
      if (threadIdx.x == 0)
        for (int t = 0; t < n; ++t) sh.sent[t] += (uint64_t)ne;
    }
  }
  direct_count_out(sh, a, me, MCCS_DIRECT_OUT_CNT(0));
  // 3. the foreign shares' results, decoded from this rank's out slot to the output
  if (threadIdx.x < MCCS_DIRECT_MAX_RANKS) need[threadIdx.x] = sh.e_out[threadIdx.x] + sh.owned[threadIdx.x];
  __syncthreads();
  bool out_seen = false;
  foreign([&](uint32_t, int64_t off, int64_t ne) {
    if (!out_seen) {
      if (!direct_wait(sh, mine, MCCS_DIRECT_OUT_CNT(0), peers, need, abortFlag, a, ecfg)) return false;
      out_seen = true;
    }
    constexpr uint32_t U = kDirectUnroll;
    uint16_t* dst = (uint16_t*)me.recv + off;
    const bool vec = ((uintptr_t)dst & 15) == 0;
    const char* const sl = out_slot(mine);
    const uint32_t nu = (uint32_t)((ne + kQuantUnit - 1) / kQuantUnit);
    for (uint32_t u0 = wave; u0 < nu; u0 += nw * U) {
      u32x2 cw[U];
      uint32_t cb[U];
#pragma unroll
      for (uint32_t k = 0; k < U; ++k) {
        const uint32_t u = u0 + k * nw;
        if (u >= nu) continue;
        const int64_t eoff = off + (int64_t)u * kQuantUnit;
        cw[k] = __builtin_nontemporal_load((const u32x2*)(sl + eoff + lane * 8));
        cb[k] = __builtin_nontemporal_load((const uint8_t*)(sl + pay + eoff / 32 + lane / 4));
      }
#pragma unroll
      for (uint32_t k = 0; k < U; ++k) {
        const uint32_t u = u0 + k * nw;
        if (u >= nu) continue;
        quant_store8(dst + (int64_t)u * kQuantUnit + lane * 8, valid_of(ne, u), vec,
                     wide_down8<DT>(dequant8(cw[k][0], cw[k][1], cb[k])));
      }
    }
    return true;
  });
}

}  // namespace mccs
