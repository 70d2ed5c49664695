// direct_wide.h — wide-accumulate direct AllReduce for fp16 / bf16 (opt-in:
// mccsCommSetAllReduceWide; ring_cfg.h, "Wide direct AllReduce").
//
// Every other reducing path reproduces the ring bit for bit, so a 16-bit sum
// is rounded to 16 bits after each of its n-1 additions (dtypes.h pack_op).
// These kernels read all n inputs, accumulate in binary32 and round once.
// Per element i, ranks in RANK order 0, 1, ..., n-1 whatever the rings are:
//   t_r = f32(x_r[i])                  Sum
//   t_r = fl32(f32(x_r[i]) * f32(s))   PreMulSum, s = the T scalar in op_arg's low 16 bits
//   acc = t_0; acc = fl32(acc + t_r), r = 1 .. n-1   (RNE, denormals kept)
//   out[i] = T(acc)                    one rounding, nearest even
// The product and the sum stay two roundings (fp contraction off below: a
// bf16 product can leave binary32's range, so an fma is not equivalent).
// The result depends on neither rings, channels, workgroup count nor body, is
// the same on every rank, and differs from the ring's: the price of opting in.
//
// There is no chunk walk: no direct_walk, no idx2rank, no division per word
// or piece.  The launch has direct_kernel's shape (blockIdx.y = rank slot, G
// workgroups of MCCS_DIRECT_THREADS, the launch guard, prologue, arrival count
// and state words), and each body leaves LAUNCHES, E_IN, E_OUT, E_SELF and the
// parity as its ring-order counterpart with the same per-sender amounts would.
//   MCCS_DIRECT_WIDE_LL        thread-linear over 8-byte words (4 elements);
//     lines, flags, parity and polling as direct_ll_body; the 4 accumulators
//     are folded in rank order with the own word at r = rank.
//   MCCS_DIRECT_WIDE_ONE_SHOT  1. pieces of [0, count) -> every peer's
//     one-shot slot of this parity; count.  2. wait; pieces of [0, count) dealt
//     round-robin: the own input and the n-1 slots, in rank order, into recv.
//     In place waits on E_SELF as the one-shot does.
//   MCCS_DIRECT_WIDE_TWO_SHOT  rank t owns the contiguous share [t q,
//     min((t+1) q, count)), q = MCCS_WIDE_SHARE(count, n): shares start on
//     16-byte packs, trailing ranks may own nothing (a.owned[] holds the
//     split).  1. foreign shares -> the owner's in slot at the element offset;
//     count.  2. wait; the own share, reduced wide -> recv and every peer's out
//     slot; count.  3. wait; foreign shares, out slot -> recv.  Phases 1 and 3
//     deal identical pieces, so a workgroup rewrites in phase 3 exactly what
//     it read in phase 1 (in place is safe: direct_body's argument).
#pragma once
#include "direct_kernel.h"

static_assert(sizeof(mccsDirectArgs) <= 4096, "wide direct launch arguments must stay within 4 KiB");

namespace mccs {

using f32x8 = float __attribute__((ext_vector_type(8)));

// The scalar of a PreMulSum, widened (Sum: unused).
template <int DT>
__device__ __forceinline__ float wide_scalar(uint64_t arg) {
  if constexpr (DT == mccsFloat16) return (float)__builtin_bit_cast(_Float16, (uint16_t)arg);
  else return bf16_lo((uint32_t)(uint16_t)arg);
}

// One element / one 8-byte word / one 16-byte pack widened to binary32 lanes
// (bf16: shift and mask; fp16: the packed v_cvt_f32_f16 forms), and narrowed
// back with one rounding to nearest even.
template <int DT>
__device__ __forceinline__ float wide_up(typename Elem<DT>::T x) {
  if constexpr (DT == mccsFloat16) return (float)x;
  else return bf16_lo(x);
}
template <int DT>
__device__ __forceinline__ typename Elem<DT>::T wide_down(float x) {
  if constexpr (DT == mccsFloat16) return (_Float16)x;
  else return (uint16_t)(pack_bf16x2(x, 0.f) & 0xffffu);
}
template <int DT>
__device__ __forceinline__ f32x4 wide_up4(uint64_t v) {
  if constexpr (DT == mccsFloat16) {
    using h16x4 = _Float16 __attribute__((ext_vector_type(4)));
    return __builtin_convertvector(__builtin_bit_cast(h16x4, v), f32x4);
  } else {
    const uint32_t lo = (uint32_t)v, hi = (uint32_t)(v >> 32);
    return f32x4{bf16_lo(lo), bf16_hi(lo), bf16_lo(hi), bf16_hi(hi)};
  }
}
template <int DT>
__device__ __forceinline__ uint64_t wide_down4(f32x4 x) {
  if constexpr (DT == mccsFloat16) {
    using h16x4 = _Float16 __attribute__((ext_vector_type(4)));
    return __builtin_bit_cast(uint64_t, __builtin_convertvector(x, h16x4));
  } else {
    return (uint64_t)pack_bf16x2(x[0], x[1]) | ((uint64_t)pack_bf16x2(x[2], x[3]) << 32);
  }
}
template <int DT>
__device__ __forceinline__ f32x8 wide_up8(u32x4 v) {
  if constexpr (DT == mccsFloat16) {
    return __builtin_convertvector(__builtin_bit_cast(h16x8, v), f32x8);
  } else {
    return f32x8{bf16_lo(v[0]), bf16_hi(v[0]), bf16_lo(v[1]), bf16_hi(v[1]),
                 bf16_lo(v[2]), bf16_hi(v[2]), bf16_lo(v[3]), bf16_hi(v[3])};
  }
}
template <int DT>
__device__ __forceinline__ u32x4 wide_down8(f32x8 x) {
  if constexpr (DT == mccsFloat16) {
    return __builtin_bit_cast(u32x4, __builtin_convertvector(x, h16x8));
  } else {
    return u32x4{pack_bf16x2(x[0], x[1]), pack_bf16x2(x[2], x[3]), pack_bf16x2(x[4], x[5]), pack_bf16x2(x[6], x[7])};
  }
}

// acc = first ? t : acc + t with t = x (Sum) or fl32(x * s) (PreMulSum): two
// roundings, never an fma (V: float, f32x4 or f32x8).
template <bool PRE, typename V>
__device__ __forceinline__ V wide_fold(V acc, V x, float s, bool first) {
#pragma clang fp contract(off)
  V t = x;
  if constexpr (PRE) t = x * s;
  return first ? t : acc + t;
}

// The sources in rank order (the own input at its rank's position), folded in
// binary32 and stored once to every non-null destination among dst[0 .. ndst).
// Per thread U packs x n sources are issued as non-temporal 16-byte loads
// before any arithmetic.  Misaligned operands and the sub-pack tail take the
// typed path with the same arithmetic.
template <int DT, bool PRE>
__device__ __forceinline__ void wide_reduce(const void* const* src, int n, void* const* dst, int ndst, int64_t ne,
                                            float s) {
  using T = typename Elem<DT>::T;
  constexpr int PACK = kPackElems<DT>;
  constexpr int U = kDirectUnroll;
  const int tid = threadIdx.x, nthr = blockDim.x;
  uintptr_t mis = 0;
#pragma unroll
  for (int j = 0; j < MCCS_DIRECT_MAX_RANKS; ++j) {
    if (j < n) mis |= (uintptr_t)src[j];
    if (j < ndst) mis |= (uintptr_t)dst[j];
  }
  int64_t done = 0;
  if ((mis & 15) == 0) {
    const int64_t npack = ne / PACK;
    for (int64_t base = tid; base < npack; base += (int64_t)nthr * U) {
      u32x4 v[MCCS_DIRECT_MAX_RANKS][U];
#pragma unroll
      for (int j = 0; j < MCCS_DIRECT_MAX_RANKS; ++j)
        if (j < n) {
#pragma unroll
          for (int u = 0; u < U; ++u)
            if (base + (int64_t)u * nthr < npack)
              v[j][u] = __builtin_nontemporal_load((const u32x4*)src[j] + base + (int64_t)u * nthr);
        }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (base + (int64_t)u * nthr >= npack) continue;
        f32x8 acc{};
#pragma unroll
        for (int j = 0; j < MCCS_DIRECT_MAX_RANKS; ++j)
          if (j < n) acc = wide_fold<PRE>(acc, wide_up8<DT>(v[j][u]), s, j == 0);
        const u32x4 out = wide_down8<DT>(acc);
#pragma unroll
        for (int d = 0; d < MCCS_DIRECT_MAX_RANKS; ++d)
          if (d < ndst && dst[d]) ((u32x4*)dst[d])[base + (int64_t)u * nthr] = out;
      }
    }
    done = npack * PACK;
  }
  for (int64_t e = done + tid; e < ne; e += nthr) {
    float acc = 0.f;
#pragma unroll
    for (int j = 0; j < MCCS_DIRECT_MAX_RANKS; ++j)
      if (j < n) acc = wide_fold<PRE>(acc, wide_up<DT>(__builtin_nontemporal_load((const T*)src[j] + e)), s, j == 0);
    const T out = wide_down<DT>(acc);
#pragma unroll
    for (int d = 0; d < MCCS_DIRECT_MAX_RANKS; ++d)
      if (d < ndst && dst[d]) ((T*)dst[d])[e] = out;
  }
}

// The count-based bodies (one-shot and two-shot).
template <int DT, bool PRE>
__device__ __forceinline__ void direct_wide_body(const mccsDirectArgs& a) {
  using T = typename Elem<DT>::T;
  __shared__ DirectShm sh;
  __shared__ uint64_t need[MCCS_DIRECT_MAX_RANKS];
  const mccsDirectRank& me = a.r[blockIdx.y];
  const int n = (int)a.nranks;
  char* const mine = a.region[me.rank];
  volatile uint32_t* abortFlag = me.abort_flag;
  mccsRingKernelCfg ecfg{};
  ecfg.err_line = me.err_line;
  const uint32_t size = (uint32_t)a.count;  // < 2^31: a direct bucket is at most 1 GiB
  const float s = wide_scalar<DT>(a.op_arg);
  const bool one_shot = a.mode == MCCS_DIRECT_WIDE_ONE_SHOT;
  // in place, phase 2 overwrites input other workgroups of this rank may still
  // be sending: wait for their counts too (direct_body's self_wait)
  const bool self_wait = one_shot && me.send == me.recv;
  // Prologue and arrival count: direct_body's (the state words in one round
  // trip, the abort flag left to the waits).
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
  const int64_t esz = (int64_t)sizeof(T);
  const uint32_t G = gridDim.x, bx = blockIdx.x;
  const uint32_t peers = ((1u << n) - 1u) & ~(1u << me.rank);
  const uint32_t piece = a.piece > 0 ? a.piece : 1;
  const uint32_t piece2 = a.piece2 > 0 ? a.piece2 : 1;
  // The last workgroup to arrive advances the totals and the launch count,
  // by the amounts of the ring-order one-shot (the whole count) / two-shot
  // (owned[]) with the same per-sender amounts.
  auto advance = [&]() {
    if (threadIdx.x == 0 && arrived + 1 == G) {
      uint64_t* st = (uint64_t*)(mine + MCCS_DIRECT_STATE);
      __hip_atomic_store((uint32_t*)(mine + MCCS_DIRECT_DONE), 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(st + MCCS_DIRECT_ST_E_IN, sh.e_in + (one_shot ? (uint64_t)size : sh.owned[me.rank]),
                         __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (!one_shot)
        for (int t = 0; t < n; ++t)
          __hip_atomic_store(st + MCCS_DIRECT_ST_E_OUT(t), sh.e_out[t] + sh.owned[t], __ATOMIC_RELAXED,
                             __HIP_MEMORY_SCOPE_AGENT);
      if (self_wait)
        __hip_atomic_store(st + MCCS_DIRECT_ST_E_SELF, sh.e_self + (uint64_t)size, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(st + MCCS_DIRECT_ST_LAUNCHES, seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  };

  if (one_shot) {
    const int64_t oslot = (int64_t)a.oslot_bytes;
    const int64_t obase = MCCS_DIRECT_CTRL_BYTES + (int64_t)MCCS_DIRECT_SLOTS * (int64_t)a.slot_bytes +
                          (int64_t)(seq & 1) * MCCS_DIRECT_MAX_RANKS * oslot;
    // 1. pieces of [0, count) to every peer's slot for this rank
    const uint32_t np = (size + piece - 1) / piece;
    for (uint32_t j = bx; j < np && sh.ok; j += G) {
      const int64_t off = (int64_t)j * piece;
      const int64_t ne = (int64_t)size - off < (int64_t)piece ? (int64_t)size - off : (int64_t)piece;
      const void* src[MCCS_DIRECT_MAX_RANKS] = {(const T*)me.send + off};
      void* dst[MCCS_DIRECT_MAX_RANKS];
#pragma unroll
      for (int t = 0; t < MCCS_DIRECT_MAX_RANKS; ++t)
        dst[t] = t < n && t != (int)me.rank ? (void*)(sh.region[t] + obase + (int64_t)me.rank * oslot + off * esz)
                                            : nullptr;
      direct_reduce<DT, OpSum>(src, 1, dst, n, ne);  // one source: a copy to several places
      if (threadIdx.x == 0)
        for (int t = 0; t < n; ++t) sh.sent[t] += (uint64_t)ne;
    }
    direct_count_out(sh, a, me, MCCS_DIRECT_IN_CNT(0), self_wait);
    advance();
    if (threadIdx.x < MCCS_DIRECT_MAX_RANKS)
      need[threadIdx.x] = (threadIdx.x == me.rank ? sh.e_self : sh.e_in) + (uint64_t)size;
    __syncthreads();
    const uint32_t waitmask = self_wait ? peers | (1u << me.rank) : peers;
    // 2. pieces of [0, count), every source in rank order, into the output
    bool in_seen = false;  // uniform across the workgroup
    const uint32_t np2 = (size + piece2 - 1) / piece2;
    for (uint32_t j = bx; j < np2 && sh.ok; j += G) {
      if (!in_seen) {
        if (!direct_wait(sh, mine, MCCS_DIRECT_IN_CNT(0), waitmask, need, abortFlag, a, ecfg)) return;
        in_seen = true;
      }
      const int64_t off = (int64_t)j * piece2;
      const int64_t ne = (int64_t)size - off < (int64_t)piece2 ? (int64_t)size - off : (int64_t)piece2;
      const void* src[MCCS_DIRECT_MAX_RANKS];
      void* dst[MCCS_DIRECT_MAX_RANKS] = {(T*)me.recv + off};
#pragma unroll
      for (int r = 0; r < MCCS_DIRECT_MAX_RANKS; ++r)
        src[r] = r >= n                ? nullptr
                 : r == (int)me.rank   ? (const void*)((const T*)me.send + off)
                                       : (const void*)(mine + obase + (int64_t)r * oslot + off * esz);
      wide_reduce<DT, PRE>(src, n, dst, 1, ne, s);
    }
    return;
  }

  const int64_t slot = (int64_t)a.slot_bytes;
  auto in_slot = [&](char* region, uint32_t sender) { return region + MCCS_DIRECT_CTRL_BYTES + (int64_t)sender * slot; };
  auto out_slot = [&](char* region) { return region + MCCS_DIRECT_CTRL_BYTES + (int64_t)MCCS_DIRECT_MAX_RANKS * slot; };
  const uint32_t q = (uint32_t)MCCS_WIDE_SHARE(size, (uint32_t)n);  // one 32-bit division per launch
  // The pieces of the n-1 foreign shares, numbered through; piece p belongs to
  // workgroup p % G in phase 1 and in phase 3.  f(owner, off, ne); false: stop.
  auto foreign = [&](auto&& f) {
    uint32_t base = 0;
    for (uint32_t t = 0; t < (uint32_t)n; ++t) {
      const uint32_t lo = t * q;  // (n - 1) q < count + 8 n: no wrap
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
  // 1. every foreign share to its owner's in slot for this rank
  foreign([&](uint32_t t, int64_t off, int64_t ne) {
    const void* src[MCCS_DIRECT_MAX_RANKS] = {(const T*)me.send + off};
    void* dst[MCCS_DIRECT_MAX_RANKS] = {in_slot(sh.region[t], me.rank) + off * esz};
    direct_reduce<DT, OpSum>(src, 1, dst, 1, ne);
    if (threadIdx.x == 0) sh.sent[t] += (uint64_t)ne;
    return true;
  });
  direct_count_out(sh, a, me, MCCS_DIRECT_IN_CNT(0));
  advance();
  // 2. the own share, every source in rank order -> the output and every peer's out slot
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
      const void* src[MCCS_DIRECT_MAX_RANKS];
      void* dst[MCCS_DIRECT_MAX_RANKS];
#pragma unroll
      for (int r = 0; r < MCCS_DIRECT_MAX_RANKS; ++r) {
        src[r] = nullptr;
        dst[r] = nullptr;
        if (r < n) {
          src[r] = r == (int)me.rank ? (const void*)((const T*)me.send + off) : (const void*)(in_slot(mine, r) + off * esz);
          dst[r] = r == (int)me.rank ? (void*)((T*)me.recv + off) : (void*)(out_slot(sh.region[r]) + off * esz);
        }
      }
      wide_reduce<DT, PRE>(src, n, dst, n, ne, s);
      if (threadIdx.x == 0)
        for (int t = 0; t < n; ++t) sh.sent[t] += (uint64_t)ne;
    }
  }
  direct_count_out(sh, a, me, MCCS_DIRECT_OUT_CNT(0));
  // 3. the foreign shares' results, from this rank's out slot to the output
  if (threadIdx.x < MCCS_DIRECT_MAX_RANKS) need[threadIdx.x] = sh.e_out[threadIdx.x] + sh.owned[threadIdx.x];
  __syncthreads();
  bool out_seen = false;
  foreign([&](uint32_t, int64_t off, int64_t ne) {
    if (!out_seen) {
      if (!direct_wait(sh, mine, MCCS_DIRECT_OUT_CNT(0), peers, need, abortFlag, a, ecfg)) return false;
      out_seen = true;
    }
    const void* src[MCCS_DIRECT_MAX_RANKS] = {out_slot(mine) + off * esz};
    void* dst[MCCS_DIRECT_MAX_RANKS] = {(T*)me.recv + off};
    direct_reduce<DT, OpSum>(src, 1, dst, 1, ne);
    return true;
  });
}

// The LL body: direct_ll_body's lines, flags, parity and polling; word wd
// belongs to global thread wd mod (G x threads) in both phases, so an in-place
// call overwrites a word only after the same thread has read and sent it.
template <int DT, bool PRE>
__device__ __forceinline__ void direct_wide_ll_body(const mccsDirectArgs& a) {
  using T = typename Elem<DT>::T;
  __shared__ uint64_t s_seq;
  const mccsDirectRank& me = a.r[blockIdx.y];
  const uint32_t n = a.nranks, rank = me.rank;
  char* const mine = a.region[rank];
  volatile uint32_t* abortFlag = me.abort_flag;
  mccsRingKernelCfg ecfg{};
  ecfg.err_line = me.err_line;
  const uint32_t size = (uint32_t)a.count;
  const float s = wide_scalar<DT>(a.op_arg);
  const uint32_t nwords = (uint32_t)(((uint64_t)size * sizeof(T) + 7) / 8);
  const uint32_t stride = gridDim.x * blockDim.x;
  const uint32_t gtid = blockIdx.x * blockDim.x + threadIdx.x;
  const char* in = (const char*)me.send;
  char* out = (char*)me.recv;
  const bool in_al = ((uintptr_t)in & 7) == 0, out_al = ((uintptr_t)out & 7) == 0;
  // the first word's input load is in flight while thread 0 reads the launch count
  uint64_t own0 = 0;
  if (gtid < nwords) own0 = ll_load_word<T>(in, gtid, size, in_al);
  if (threadIdx.x == 0)
    s_seq = __hip_atomic_load((uint64_t*)(mine + MCCS_DIRECT_STATE) + MCCS_DIRECT_ST_LAUNCHES, __ATOMIC_RELAXED,
                              __HIP_MEMORY_SCOPE_AGENT) + 1;
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
  // 1. every word to every peer's LL slot for this rank, as a flag-carrying line
  for (uint32_t wd = gtid; wd < nwords; wd += stride) {
    const uint64_t v = wd == gtid ? own0 : ll_load_word<T>(in, wd, size, in_al);
    const uint64_t lo = flag | (v & 0xffffffffull), hi = flag | (v >> 32);
#pragma unroll
    for (uint32_t t = 0; t < MCCS_DIRECT_MAX_RANKS; ++t)
      if (t < n && t != rank) {
        uint64_t* p = (uint64_t*)(a.region[t] + llbase + (int64_t)rank * lslot + (int64_t)wd * 16);
        __hip_atomic_store(p, lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(p + 1, hi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      }
  }
  if (threadIdx.x == 0 && arrived + 1 == gridDim.x) {
    __hip_atomic_store((uint32_t*)(mine + MCCS_DIRECT_DONE), 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store((uint64_t*)(mine + MCCS_DIRECT_STATE) + MCCS_DIRECT_ST_LAUNCHES, seq, __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
  }
  // 2. poll every peer's line of each word, fold in rank order
  const uint32_t peers = ((1u << n) - 1u) & ~(1u << rank);
  const uint64_t t0 = __builtin_amdgcn_s_memrealtime();
  for (uint32_t wd = gtid; wd < nwords; wd += stride) {
    const uint64_t own = wd == gtid ? own0 : ll_load_word<T>(in, wd, size, in_al);
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
