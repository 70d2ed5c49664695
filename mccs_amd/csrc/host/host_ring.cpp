// host_ring.cpp — the ring AllReduce protocol run by host threads over host
// memory: BASELINE configs[0] ("2-rank loopback allreduce, 1 KiB fp32,
// host-side elementwise sum; plumbing, no GPU").
//
// Same protocol as the gfx950 kernels (ring.hip) and the reference
// (all_reduce.h:10-87 schedule; prims_simple.h:68-237 FIFO: 8 slots, slices of
// 2 steps, sender waits head + 8 >= step + 2, receiver waits tail >= step + 2,
// operand order fn(own input, received)), with one host thread per
// (rank, channel) and std::atomic head/tail counters.  The threads and the
// FIFOs persist across calls (HostRingPool): a call hands each task to its
// own parked worker, so a 1 KiB AllReduce costs no thread creation.  It exists so the FIFO
// protocol and schedule can be exercised end to end without a GPU; it is not
// a fallback for the device path (nothing on the device path calls it).
// mccs_host_ring_reduce_scatter runs the ring ReduceScatter schedule
// (ring_kernel.h; not in the reference) through the same primitive, so the
// device walk has a second implementation that runs without a GPU;
// mccs_host_ring_broadcast / mccs_host_ring_reduce do the same for the rooted
// chains.
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <mutex>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <memory>
#include <thread>
#include <vector>

#include "comm.h"  // SrOp, SrElem, sendrecv_elements: the planner's pairing rule
#include "dtypes.h"
#include "half_bits.h"
#include "mccs_devcomm.h"
#include "mccs_hip.h"
#include "ring_cfg.h"
#include "ring_walk.h"

namespace mccs {
void alltoall_route(int nranks, int nch, const int* rings, bool force_relay, int* hops, int* m, int* send_bid,
                    int* recv_bid);  // plan.cpp: the one route, shared with the planner
}

namespace {

using mccs::RingWalk;
using mccs::b2f;
using mccs::f2b;
using mccs::f2h;
using mccs::h2f;

template <typename T>
T iop(int op, T x, T y) {
  using U = typename std::make_unsigned<T>::type;
  switch (op) {
    case mccsDevSum: return (T)((U)x + (U)y);
    case mccsDevProd: return (T)((U)x * (U)y);
    case mccsDevMax: return x < y ? y : x;
    default: return x < y ? x : y;
  }
}

// fmaxf/fminf/fmax/fmin as the reference's device computes them
// (reduce_kernel.h:338-463): one NaN operand yields the other, and +0 > -0 in
// either operand order (libm's fmax leaves the order of the zeros open).
template <typename T>
T fmax_ref(T x, T y) {
  if (x != x) return y;
  if (y != y) return x;
  if (x == y) return std::signbit(x) ? y : x;
  return x < y ? y : x;
}

template <typename T>
T fmin_ref(T x, T y) {
  if (x != x) return y;
  if (y != y) return x;
  if (x == y) return std::signbit(x) ? x : y;
  return x < y ? x : y;
}

template <typename T>
T fop(int op, T x, T y) {
  switch (op) {
    case mccsDevSum: return x + y;
    case mccsDevProd: return x * y;
    case mccsDevMax: return fmax_ref(x, y);
    default: return fmin_ref(x, y);
  }
}

float hop(int op, float x, float y) { return fop<float>(op, x, y); }

// out[i] = fn(x[i], y[i]); out may alias either input
void apply(int dt, int op, void* out, const void* x, const void* y, size_t n) {
#define INT_CASE(D, T)                                                                       \
  case D:                                                                                    \
    for (size_t i = 0; i < n; ++i) ((T*)out)[i] = iop<T>(op, ((const T*)x)[i], ((const T*)y)[i]); \
    break;
  switch (dt) {
    INT_CASE(mccsInt8, int8_t)
    INT_CASE(mccsUint8, uint8_t)
    INT_CASE(mccsInt32, int32_t)
    INT_CASE(mccsUint32, uint32_t)
    INT_CASE(mccsInt64, int64_t)
    INT_CASE(mccsUint64, uint64_t)
    case mccsFloat32:
      for (size_t i = 0; i < n; ++i) ((float*)out)[i] = fop<float>(op, ((const float*)x)[i], ((const float*)y)[i]);
      break;
    case mccsFloat64:
      for (size_t i = 0; i < n; ++i)
        ((double*)out)[i] = fop<double>(op, ((const double*)x)[i], ((const double*)y)[i]);
      break;
    case mccsFloat16:
      for (size_t i = 0; i < n; ++i)
        ((uint16_t*)out)[i] = f2h(hop(op, h2f(((const uint16_t*)x)[i]), h2f(((const uint16_t*)y)[i])));
      break;
    case mccsBfloat16:
      for (size_t i = 0; i < n; ++i)
        ((uint16_t*)out)[i] = f2b(hop(op, b2f(((const uint16_t*)x)[i]), b2f(((const uint16_t*)y)[i])));
      break;
  }
#undef INT_CASE
}

// PreMulSum's pre step (dtypes.h pre_op): out[i] = x[i] * s rounded once in
// the type, s the low bytes of arg; integers modulo 2^w.  The product is a
// statement of its own, compiled with contraction off, so no host compiler
// fuses it with the add that follows (the kernels keep the two roundings too).
// out may alias x.
void pre_apply(int dt, uint64_t arg, void* out, const void* x, size_t n) {
#pragma clang fp contract(off)
#define INT_CASE(D, T)                                                                                       \
  case D:                                                                                                    \
    for (size_t i = 0; i < n; ++i)                                                                           \
      ((T*)out)[i] = (T)((std::make_unsigned<T>::type)((const T*)x)[i] * (std::make_unsigned<T>::type)arg);  \
    break;
  switch (dt) {
    INT_CASE(mccsInt8, int8_t)
    INT_CASE(mccsUint8, uint8_t)
    INT_CASE(mccsInt32, int32_t)
    INT_CASE(mccsUint32, uint32_t)
    INT_CASE(mccsInt64, int64_t)
    INT_CASE(mccsUint64, uint64_t)
    case mccsFloat32: {
      float s;
      const uint32_t b = (uint32_t)arg;
      std::memcpy(&s, &b, 4);
      for (size_t i = 0; i < n; ++i) {
        volatile float p = ((const float*)x)[i] * s;
        ((float*)out)[i] = p;
      }
      break;
    }
    case mccsFloat64: {
      double s;
      std::memcpy(&s, &arg, 8);
      for (size_t i = 0; i < n; ++i) {
        volatile double p = ((const double*)x)[i] * s;
        ((double*)out)[i] = p;
      }
      break;
    }
    case mccsFloat16:  // the exact product fits binary32: one rounding, to binary16
      for (size_t i = 0; i < n; ++i) ((uint16_t*)out)[i] = f2h(h2f(((const uint16_t*)x)[i]) * h2f((uint16_t)arg));
      break;
    case mccsBfloat16:
      for (size_t i = 0; i < n; ++i) ((uint16_t*)out)[i] = f2b(b2f(((const uint16_t*)x)[i]) * b2f((uint16_t)arg));
      break;
  }
#undef INT_CASE
}

// SumPostDiv's post step (dtypes.h post_op): v[i] = T(v[i] / n), n = (int)arg,
// C division after the usual promotions (n unsigned for uint32 / uint64).
void post_apply(int dt, uint64_t arg, void* v, size_t cnt) {
  const int n = (int)arg;
  switch (dt) {
    case mccsInt8: for (size_t i = 0; i < cnt; ++i) ((int8_t*)v)[i] = (int8_t)(((int8_t*)v)[i] / n); break;
    case mccsUint8: for (size_t i = 0; i < cnt; ++i) ((uint8_t*)v)[i] = (uint8_t)(((uint8_t*)v)[i] / n); break;
    case mccsInt32: for (size_t i = 0; i < cnt; ++i) ((int32_t*)v)[i] /= n; break;
    case mccsUint32: for (size_t i = 0; i < cnt; ++i) ((uint32_t*)v)[i] /= (uint32_t)n; break;
    case mccsInt64: for (size_t i = 0; i < cnt; ++i) ((int64_t*)v)[i] /= (int64_t)n; break;
    case mccsUint64: for (size_t i = 0; i < cnt; ++i) ((uint64_t*)v)[i] /= (uint64_t)n; break;
  }
}

struct HostConn {  // one directed FIFO (rank -> next) of one channel
  // uninitialised: only the slots a call touches are ever faulted in (a
  // zero-filled 4 MiB FIFO per connector cost ms per 1 KiB call)
  std::unique_ptr<char[]> data;
  // written by different threads (head: receiver, tail: sender): one cache
  // line each, so a post does not invalidate the line the other side polls
  alignas(64) std::atomic<uint64_t> head{0};
  alignas(64) std::atomic<uint64_t> tail{0};
};

struct Ctx {
  int func, n, nch, dt, op, nthreads_ref, buff_size, root;
  uint64_t op_arg;  // PreMulSum / SumPostDiv (0 otherwise)
  // AllToAll: the route (plan.cpp alltoall_route); walk_nch = the channels a block is cut over
  int a2a_hops = 0, walk_nch = 0;
  const int* a2a_send_bid = nullptr;  // n x nch
  const int* a2a_recv_bid = nullptr;
  // AllToAllv: the n x n byte counts ([s * n + t]: s sends to t) and per-rank displacement rows
  const size_t* v_counts = nullptr;
  const size_t* v_sdispls = nullptr;  // [r * n + t]
  const size_t* v_rdispls = nullptr;  // [r * n + s]
  const uint64_t* const* v_tables = nullptr;  // or: each rank's size table (ring_cfg.h MCCS_FUNC_ALLTOALLV_DEV)
  // Send/Recv: each (rank, channel)'s elements, [r * nch + ch] (plan.cpp sendrecv_elements)
  const std::vector<std::vector<mccs::SrElem>>* sr_elems = nullptr;
  size_t es, count;
  const void* const* send;
  void* const* recv;
  const int* rings;  // nch x n, nullptr = identity
  std::vector<HostConn>* conns;  // [ch * n + rank]: FIFO rank -> next on channel ch
  std::atomic<int> failed{0};
  double timeout_s;
};

// One (rank, channel) task: its place on the channel's ring, its two
// connectors and the FIFO primitive every schedule is written in.
struct RankChannel {
  Ctx* c;
  int n, rank, ch;
  int ring[64];  // n <= 64 (checked by the entry points)
  int pos, ringIx;
  HostConn* out;
  HostConn* in;
  RingWalk<int64_t> w;  // the element's geometry (ring_walk.h)
  int64_t parts;        // chunks per loop
  int64_t stepSize;
  const char* input;
  char* output;
  uint64_t rstep = 0, sstep = 0;
  char* tmp;
  std::chrono::steady_clock::time_point t0;

  RankChannel(Ctx* ctx, int rank_, int ch_) : c(ctx), n(ctx->n), rank(rank_), ch(ch_) {
    for (int i = 0; i < n; ++i) ring[i] = c->rings ? c->rings[ch * n + i] : i;
    int pos0 = 0;
    pos = 0;
    for (int i = 0; i < n; ++i) {
      if (ring[i] == rank) pos = i;
      if (ring[i] == 0) pos0 = i;
    }
    const int prev = ring[(pos + n - 1) % n];
    ringIx = (pos - pos0 + n) % n;
    out = &(*c->conns)[ch * n + rank];
    in = &(*c->conns)[ch * n + prev];
    const int walk_nch = c->walk_nch > 0 ? c->walk_nch : c->nch;
    mccs::ring_walk<int64_t>(w, c->func, n, walk_nch, (int)c->es, c->nthreads_ref, c->buff_size, (int64_t)c->count);
    mccs::walk_guard(w);
    parts = mccs::walk_parts<int64_t>(c->func, walk_nch, n);
    stepSize = w.stepSize;
    input = (const char*)c->send[rank];
    output = (char*)c->recv[rank];
    thread_local std::vector<char> tmp_store;  // this worker's staging slice, kept across calls
    if (tmp_store.size() < (size_t)(2 * stepSize * c->es)) tmp_store.resize((size_t)(2 * stepSize * c->es));
    tmp = tmp_store.data();
    t0 = std::chrono::steady_clock::now();
  }

  // ring.userRanks: the ring order starting at this rank
  int user_rank(int i) const { return ring[(pos + i) % n]; }

  bool wait_geq(std::atomic<uint64_t>& f, uint64_t target) {
    // the peer is a running thread: spin (pause) before giving up the core
    for (int spin = 0; spin < 4096; ++spin) {
      if (f.load(std::memory_order_acquire) >= target) return true;
      __builtin_ia32_pause();
    }
    while (f.load(std::memory_order_acquire) < target) {
      if (c->failed.load(std::memory_order_relaxed)) return false;
      if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > c->timeout_s) {
        c->failed.store(1);
        return false;
      }
      std::this_thread::yield();
    }
    return true;
  }

  // genericOp: RECV/SEND/SRC(input)/DST(output) flags, two slices per call
  bool op(bool RECV, bool SEND, bool SRC, bool DST, int64_t srcIx, int64_t dstIx, int64_t nelem) {
    if (nelem < 0) nelem = 0;
    const int64_t sliceSize =
        mccs::slice_size(nelem, stepSize, ALLREDUCE_SLICESTEPS, ALLREDUCE_CHUNKSTEPS / ALLREDUCE_SLICESTEPS);
    int64_t offset = 0;
    for (int slice = 0; slice < 2; ++slice) {
      int64_t real = nelem - offset;
      real = real < sliceSize ? real : sliceSize;
      if (real < 0) real = 0;
      if (RECV && !wait_geq(in->tail, rstep + 2)) return false;
      if (SEND && !wait_geq(out->head, sstep + 2 > 8 ? sstep + 2 - 8 : 0)) return false;
      const size_t bytes = (size_t)real * c->es;
      const char* rslot = in->data.get() + (rstep % 8) * stepSize * c->es;
      char* sslot = out->data.get() + (sstep % 8) * stepSize * c->es;
      if (bytes) {
        // vals = srcs[0]; vals = fn(vals, srcs[1]) with srcs = [input?, recv?];
        // PreMulSum: the input operand goes through pre first; SumPostDiv: the
        // final reducing call (input and FIFO in, output out) posts the value
        // that goes to every destination (ring_kernel.h stream_slice)
        const bool pre = c->op == mccsDevPreMulSum && SRC;
        const int fn = c->op > mccsDevMin ? mccsDevSum : c->op;
        const char* in0 = input + (srcIx + offset) * c->es;
        if (pre) pre_apply(c->dt, c->op_arg, tmp, in0, (size_t)real);
        if (SRC && RECV) apply(c->dt, fn, tmp, pre ? tmp : in0, rslot, (size_t)real);
        else if (SRC && !pre) std::memcpy(tmp, in0, bytes);
        else if (!SRC) std::memcpy(tmp, rslot, bytes);
        if (c->op == mccsDevSumPostDiv && SRC && RECV && DST) post_apply(c->dt, c->op_arg, tmp, (size_t)real);
        if (DST) std::memcpy(output + (dstIx + offset) * c->es, tmp, bytes);
        if (SEND) std::memcpy(sslot, tmp, bytes);
      }
      // a call whose elements all fit in this slice posts the steps of its
      // remaining (empty) slices with this one: the same step counts as a
      // post per slice, one cross-thread hand-off instead of two
      const int64_t adv = offset + sliceSize >= nelem ? 2 * (2 - slice) : 2;
      if (SEND) out->tail.store(sstep + adv, std::memory_order_release);
      if (RECV) in->head.store(rstep + adv, std::memory_order_release);
      if (RECV) rstep += adv;
      if (SEND) sstep += adv;
      if (adv > 2) break;
      offset += sliceSize;
    }
    return true;
  }
};

// runRing of AllReduce (all_reduce.h:10-87)
void walk_allreduce(RankChannel& k) {
  const RingWalk<int64_t>& w = k.w;
  const int n = k.n;
  for (int64_t g = 0; g < w.size; g += w.loopSize) {
    const int64_t rcs = mccs::real_chunk_size(w, g, k.parts);
    // call j: send, n-2 x recvReduceSend, recvReduceCopySend, n-2 x recvCopySend, recv
    for (int j = 0; j < 2 * n - 1; ++j) {
      const int64_t c = (int64_t)k.ch * n + mccs::allreduce_call_chunk(k.ringIx, n, j);
      const int64_t off = mccs::allreduce_chunk_offset(g, c, rcs);
      if (!k.op(j > 0, j < 2 * n - 2, j <= n - 1, j >= n - 1, off, off, mccs::chunk_nelem(w.size, off, rcs))) return;
    }
  }
}

// Ring ReduceScatter (ring_kernel.h): count = elements per
// block; call j of a loop works on block userRanks[n-1-j], the last one
// (recvReduceCopy) on the rank's own block, written at the chunk's offset.
void walk_reduce_scatter(RankChannel& k) {
  const RingWalk<int64_t>& w = k.w;
  const int n = k.n;
  const int64_t size = w.size;
  for (int64_t g = 0; g < size; g += w.loopSize) {
    const int64_t rcs = mccs::real_chunk_size(w, g, k.parts);
    const int64_t chunkOffset = mccs::block_chunk_offset(g, (int64_t)k.ch, rcs);
    const int64_t nelem = mccs::chunk_nelem(size, chunkOffset, rcs);  // <= 0: empty calls
    auto src = [&](int j) { return chunkOffset + (int64_t)k.user_rank(n - 1 - j) * size; };
    if (!k.op(false, true, true, false, src(0), 0, nelem)) return;
    for (int j = 1; j < n - 1; ++j)
      if (!k.op(true, true, true, false, src(j), 0, nelem)) return;
    if (!k.op(true, false, true, true, src(n - 1), chunkOffset, nelem)) return;
  }
}

// Ring Broadcast and Reduce (ring_kernel.h): the whole buffer
// cut like a block, one call per loop whose kind is the rank's role on the
// chain: d is the root's distance ahead of the rank along the ring.
void walk_rooted(RankChannel& k) {
  const RingWalk<int64_t>& w = k.w;
  const int n = k.n;
  int d = 0;
  while (d < n - 1 && k.user_rank(d) != k.c->root) ++d;
  bool RECV, SEND, SRC, DST;
  if (k.c->func == mccsFuncBoadcast) {
    RECV = d != 0;               // root: send / copySend
    SEND = d != 1;               // the rank whose next is the root: recv
    SRC = d == 0;
    DST = d != 0 || k.input != k.output;
  } else {
    RECV = d != n - 1;           // first after the root: send
    SEND = d != 0;               // root: recvReduceCopy
    SRC = true;
    DST = d == 0;
  }
  for (int64_t g = 0; g < w.size; g += w.loopSize) {
    const int64_t rcs = mccs::real_chunk_size(w, g, k.parts);
    const int64_t off = mccs::block_chunk_offset(g, (int64_t)k.ch, rcs);
    if (!k.op(RECV, SEND, SRC, DST, off, off, mccs::chunk_nelem(w.size, off, rcs))) return;
  }
}

// AllToAll (ring_walk.h a2a_call): count = bytes per peer; the
// rank's own block is a local copy (channel 0 makes it), every other block
// travels `d` hops: one send, d-1 recvSend relays, one recv.
void walk_alltoall(RankChannel& k) {
  const RingWalk<int64_t>& w = k.w;
  const int n = k.n, hops = k.c->a2a_hops;
  const int64_t size = w.size;
  if (k.ch == 0) std::memcpy(k.output + (int64_t)k.rank * size, k.input + (int64_t)k.rank * size, (size_t)size);
  const int64_t sbid = k.c->a2a_send_bid[k.rank * k.c->nch + k.ch], rbid = k.c->a2a_recv_bid[k.rank * k.c->nch + k.ch];
  const int ncalls = mccs::a2a_calls_per_loop(hops);
  for (int64_t g = 0; g < size; g += w.loopSize) {
    const int64_t rcs = mccs::real_chunk_size(w, g, k.parts);
    for (int j = 0; j < ncalls; ++j) {
      int d;
      const int role = mccs::a2a_call(j, &d);
      const int64_t off = mccs::block_chunk_offset(g, role == mccs::kA2ARecv ? rbid : sbid, rcs);
      const int64_t nelem = mccs::chunk_nelem(size, off, rcs);  // <= 0: empty calls
      const int64_t src = off + (int64_t)k.user_rank(mccs::a2a_send_block(d)) * size;
      const int64_t dst = off + (int64_t)k.user_rank(mccs::a2a_recv_block(n, d)) * size;
      const bool S = role == mccs::kA2ASend, R = role == mccs::kA2ARecv;
      if (!k.op(!S, !R, S, R, src, dst, nelem)) return;
    }
  }
}

// One v element (ring_walk.h a2av_next): a send walk of S bytes from k.input
// and a receive walk of R bytes into k.output.  false: the ring failed.
bool walk_v_elem(RankChannel& k, int64_t S, int64_t R, int64_t sbid, int64_t rbid) {
  const RingWalk<int64_t>& w = k.w;
  const int64_t ncalls = mccs::a2av_loops(S, w.loopSize) + mccs::a2av_loops(R, w.loopSize);
  int64_t g = 0;
  int side = mccs::a2av_first(S);
  for (int64_t call = 0; call < ncalls; ++call) {
    const bool recv = side == mccs::kA2AvRecv;
    const int64_t size = recv ? R : S;
    const int64_t rcs = mccs::a2av_chunk_size(w, size, g, k.parts);
    const int64_t off = mccs::block_chunk_offset(g, recv ? rbid : sbid, rcs);
    if (!k.op(recv, !recv, !recv, recv, off, off, mccs::chunk_nelem(size, off, rcs))) return false;  // <= 0: an empty call
    side = mccs::a2av_next(S, R, w.loopSize, &g, side);
  }
  return true;
}

// AllToAllv (ring_walk.h a2av_next): the channel's send walk
// over the bytes for its successor and its receive walk over the bytes of its
// predecessor, each of its own length; the self block is a local copy
// (channel 0 makes it).  With size tables (mccs_host_ring_all_to_all_v_tables)
// the channel's element and the self element are resolved from the rank's table
// as the AllToAllvDev kernel resolves them (ring_walk.h a2avd_resolve), from the
// route words the planner gives them; the walk is the same.
void walk_alltoallv(RankChannel& k) {
  const RingWalk<int64_t>& w = k.w;
  const int n = k.n, r = k.rank;
  const int t = k.user_rank(1), p = k.user_rank(n - 1);
  const int64_t sbid = k.c->a2a_send_bid[r * k.c->nch + k.ch], rbid = k.c->a2a_recv_bid[r * k.c->nch + k.ch];
  mccs::A2AvdElem e, self;
  if (k.c->v_tables) {
    auto ld = [](const uint64_t* q) { return *q; };
    e = mccs::a2avd_resolve(k.c->v_tables[r], n, r, MCCS_A2AVD_ROUTE(rbid, t, p), ld);
    self = mccs::a2avd_resolve(k.c->v_tables[r], n, r, MCCS_A2A_ROUTE(0, 0, k.ch, k.c->nch), ld);
  } else {
    const size_t* cnt = k.c->v_counts;
    const size_t* sd = k.c->v_sdispls + (size_t)r * n;
    const size_t* rd = k.c->v_rdispls + (size_t)r * n;
    e = {cnt[(size_t)r * n + t], sd[t], cnt[(size_t)p * n + r], rd[p]};
    self = {cnt[(size_t)r * n + r], sd[r], 0, rd[r]};
  }
  if (k.ch == 0 && self.S) std::memcpy(k.output + self.recvOff, k.input + self.sendOff, self.S);
  k.input += e.sendOff;
  k.output += e.recvOff;
  walk_v_elem(k, (int64_t)e.S, (int64_t)e.R, sbid, rbid);
}

// Send/Recv (plan.cpp sendrecv_elements): the channel's
// elements in order, each an AllToAllv element on the calls' own buffers; the
// connection's steps carry over from one element to the next.
void walk_sendrecv(RankChannel& k) {
  const int r = k.rank;
  const int64_t sbid = k.c->a2a_send_bid[r * k.c->nch + k.ch], rbid = k.c->a2a_recv_bid[r * k.c->nch + k.ch];
  for (const mccs::SrElem& e : (*k.c->sr_elems)[(size_t)r * k.c->nch + k.ch]) {
    k.input = (const char*)e.send;
    k.output = (char*)e.recv;
    if (!walk_v_elem(k, (int64_t)e.S, (int64_t)e.R, sbid, rbid)) return;
  }
}

// one (rank, channel) thread
void run_rank_channel(Ctx* c, int rank, int ch) {
  RankChannel k(c, rank, ch);
  if (c->func == MCCS_FUNC_SENDRECV) walk_sendrecv(k);
  else if (c->func == MCCS_FUNC_ALLTOALLV) walk_alltoallv(k);
  else if (c->func == MCCS_FUNC_ALLTOALL) walk_alltoall(k);
  else if (c->func == mccsFuncReduceScatter) walk_reduce_scatter(k);
  else if (c->func == mccsFuncBoadcast || c->func == mccsFuncReduce) walk_rooted(k);
  else walk_allreduce(k);
}

// Parked worker threads, one per concurrent (rank, channel) task: every task
// of a call must run at the same time (they spin on each other's FIFO flags),
// so task i >= 1 always goes to worker i and task 0 runs on the caller.  Workers spin briefly after a call (back
// to back calls wake them in ~1 us) and then sleep on a condition variable.
class HostRingPool {
 public:
  static HostRingPool& get() {
    static HostRingPool* p = new HostRingPool();  // never destroyed: workers stay parked at exit
    return *p;
  }
  std::mutex call_mu;

  // FIFOs of `nconn` connectors of `bytes` each, counters reset
  std::vector<HostConn>& fifos(size_t nconn, size_t bytes) {
    if (conns_.size() != nconn || conn_bytes_ != bytes) {
      conns_ = std::vector<HostConn>(nconn);
      for (auto& hc : conns_) hc.data.reset(new char[bytes]);
      conn_bytes_ = bytes;
    }
    for (auto& hc : conns_) {
      hc.head.store(0, std::memory_order_relaxed);
      hc.tail.store(0, std::memory_order_relaxed);
    }
    return conns_;
  }

  // Task 0 runs on the calling thread; tasks 1.. go to parked workers 1..
  // (a 2-rank call wakes one worker).  The job, its task count and the
  // generation change together under mu_, and a worker reads them together
  // under mu_, so a worker that lagged behind a call it had no task in
  // cannot pair an old generation with a newer job.
  void run(Ctx* c, int ntasks) {
    while ((int)workers_.size() < ntasks - 1) {
      const int id = (int)workers_.size() + 1;
      workers_.emplace_back([this, id] { loop(id); });
    }
    remaining_.store(ntasks - 1, std::memory_order_relaxed);
    {
      std::lock_guard<std::mutex> lk(mu_);  // also pairs with a sleeper's predicate check
      job_.store(c, std::memory_order_relaxed);
      ntasks_.store(ntasks, std::memory_order_relaxed);
      gen_.fetch_add(1, std::memory_order_release);
    }
    if (sleepers_.load(std::memory_order_acquire)) cv_.notify_all();
    run_rank_channel(c, 0, 0);
    for (int spin = 0; remaining_.load(std::memory_order_acquire) != 0; ++spin) {
      if (spin < 4096) __builtin_ia32_pause();
      else std::this_thread::yield();
    }
  }

 private:
  void loop(int id) {
    uint64_t seen = 0;
    for (;;) {
      // spin ~200 us for the next call, then sleep
      const auto t0 = std::chrono::steady_clock::now();
      for (int i = 0; gen_.load(std::memory_order_acquire) == seen; ++i) {
        __builtin_ia32_pause();
        if ((i & 255) == 255 && std::chrono::steady_clock::now() - t0 > std::chrono::microseconds(200)) break;
      }
      if (gen_.load(std::memory_order_acquire) == seen) {
        std::unique_lock<std::mutex> lk(mu_);
        sleepers_.fetch_add(1, std::memory_order_acq_rel);
        cv_.wait(lk, [&] { return gen_.load(std::memory_order_acquire) != seen; });
        sleepers_.fetch_sub(1, std::memory_order_acq_rel);
      }
      Ctx* c;
      int ntasks;
      {
        std::lock_guard<std::mutex> lk(mu_);
        seen = gen_.load(std::memory_order_acquire);
        c = job_.load(std::memory_order_relaxed);
        ntasks = ntasks_.load(std::memory_order_relaxed);
      }
      if (id < ntasks) {
        run_rank_channel(c, id / c->nch, id % c->nch);
        remaining_.fetch_sub(1, std::memory_order_acq_rel);
      }
    }
  }

  std::vector<std::thread> workers_;
  std::vector<HostConn> conns_;
  size_t conn_bytes_ = 0;
  std::mutex mu_;
  std::condition_variable cv_;
  std::atomic<uint64_t> gen_{0};
  std::atomic<int> remaining_{0};
  std::atomic<int> sleepers_{0};
  std::atomic<Ctx*> job_{nullptr};
  std::atomic<int> ntasks_{0};
};

}  // namespace

static mccsResult_t host_ring_run(int func, int nranks, const void* const* sendbufs, void* const* recvbufs,
                                  size_t count, int dtype, int op, int nchannels, int nthreads_ref, int buff_size,
                                  const int* rings, int root = 0, const uint64_t* op_arg = nullptr,
                                  bool a2a_force_relay = false) {
  if (root < 0 || root >= nranks) return mccsInvalidArgument;
  // the plain entry points (op_arg == nullptr) know Sum / Prod / Max / Min
  if (nranks < 1 || nranks > 64 || !sendbufs || !recvbufs || dtype < 0 || dtype >= mccsNumTypes || op < 0 ||
      op > (op_arg ? mccsDevSumPostDiv : mccsDevMin) || nchannels < 1 || nchannels > MCCS_MAX_NCHANNELS ||
      nthreads_ref <= WARP_SIZE || buff_size < 8192 || buff_size % 8192)
    return mccsInvalidArgument;
  const size_t es = (size_t)mccs::elem_bytes(dtype);
  const uint64_t arg = op_arg ? *op_arg : 0;
  // the argument rules of the mccs*OpArg entry points (mccs_hip.h)
  if (op <= mccsDevMin && arg != 0) return mccsInvalidArgument;
  if (op == mccsDevPreMulSum && es < 8 && (arg >> (8 * es)) != 0) return mccsInvalidArgument;
  if (op == mccsDevSumPostDiv && (!mccs::is_integer_dtype(dtype) || arg < 1 || arg > (uint64_t)INT32_MAX))
    return mccsInvalidArgument;
  if (nranks == 1) {
    if (recvbufs[0] != sendbufs[0]) std::memmove(recvbufs[0], sendbufs[0], count * es);
    // one rank: post(pre(x))
    if (op == mccsDevPreMulSum) pre_apply(dtype, arg, recvbufs[0], recvbufs[0], count);
    if (op == mccsDevSumPostDiv) post_apply(dtype, arg, recvbufs[0], count);
    return mccsSuccess;
  }
  HostRingPool& pool = HostRingPool::get();
  std::lock_guard<std::mutex> call(pool.call_mu);  // one host-ring collective at a time
  std::vector<HostConn>& conns = pool.fifos((size_t)nchannels * nranks, (size_t)buff_size);
  Ctx c;
  c.func = func;
  c.n = nranks;
  c.nch = nchannels;
  c.dt = dtype;
  c.op = op;
  c.op_arg = arg;
  c.nthreads_ref = nthreads_ref;
  c.buff_size = buff_size;
  c.es = es;
  c.count = count;
  c.send = sendbufs;
  c.recv = recvbufs;
  c.rings = rings;
  c.root = root;
  c.conns = &conns;
  c.timeout_s = 60.0;
  std::vector<int> ident, a2a_sb, a2a_rb;
  if (func == MCCS_FUNC_ALLTOALL) {
    if (!rings) {
      for (int ch = 0; ch < nchannels; ++ch)
        for (int i = 0; i < nranks; ++i) ident.push_back(i);
    }
    a2a_sb.resize((size_t)nranks * nchannels);
    a2a_rb.resize((size_t)nranks * nchannels);
    int m = 0;
    mccs::alltoall_route(nranks, nchannels, rings ? rings : ident.data(), a2a_force_relay, &c.a2a_hops, &m,
                         a2a_sb.data(), a2a_rb.data());
    c.walk_nch = m > 0 ? m : nchannels;  // relay: every channel given, as the other host rings
    c.a2a_send_bid = a2a_sb.data();
    c.a2a_recv_bid = a2a_rb.data();
  }
  pool.run(&c, nranks * nchannels);
  return c.failed.load() ? mccsTimeout : mccsSuccess;
}

extern "C" mccsResult_t mccs_host_ring_allreduce(int nranks, const void* const* sendbufs, void* const* recvbufs,
                                                 size_t count, int dtype, int op, int nchannels, int nthreads_ref,
                                                 int buff_size, const int* rings) {
  return host_ring_run(mccsFuncAllReduce, nranks, sendbufs, recvbufs, count, dtype, op, nchannels, nthreads_ref,
                       buff_size, rings);
}

extern "C" mccsResult_t mccs_host_ring_reduce_scatter(int nranks, const void* const* sendbufs, void* const* recvbufs,
                                                      size_t recvcount, int dtype, int op, int nchannels,
                                                      int nthreads_ref, int buff_size, const int* rings) {
  return host_ring_run(mccsFuncReduceScatter, nranks, sendbufs, recvbufs, recvcount, dtype, op, nchannels,
                       nthreads_ref, buff_size, rings);
}

extern "C" mccsResult_t mccs_host_ring_broadcast(int nranks, const void* const* sendbufs, void* const* recvbufs,
                                                 size_t nbytes, int root, int nchannels, int nthreads_ref,
                                                 int buff_size, const int* rings) {
  return host_ring_run(mccsFuncBoadcast, nranks, sendbufs, recvbufs, nbytes, mccsInt8, mccsDevSum, nchannels,
                       nthreads_ref, buff_size, rings, root);
}

extern "C" mccsResult_t mccs_host_ring_reduce(int nranks, const void* const* sendbufs, void* const* recvbufs,
                                              size_t count, int dtype, int op, int root, int nchannels,
                                              int nthreads_ref, int buff_size, const int* rings) {
  return host_ring_run(mccsFuncReduce, nranks, sendbufs, recvbufs, count, dtype, op, nchannels, nthreads_ref,
                       buff_size, rings, root);
}

extern "C" mccsResult_t mccs_host_ring_all_to_all(int nranks, const void* const* sendbufs, void* const* recvbufs,
                                                  size_t bytes_per_peer, int nchannels, int nthreads_ref,
                                                  int buff_size, const int* rings, int force_relay) {
  if (rings && nranks >= 1 && nranks <= 64 && nchannels >= 1 && nchannels <= MCCS_MAX_NCHANNELS)
    for (int ch = 0; ch < nchannels; ++ch) {
      uint64_t seen = 0;
      for (int i = 0; i < nranks; ++i)
        if (rings[ch * nranks + i] >= 0 && rings[ch * nranks + i] < nranks) seen |= 1ull << rings[ch * nranks + i];
      if (seen != (nranks == 64 ? ~0ull : (1ull << nranks) - 1)) return mccsInvalidArgument;  // not a permutation
    }
  return host_ring_run(MCCS_FUNC_ALLTOALL, nranks, sendbufs, recvbufs, bytes_per_peer, mccsInt8, mccsDevSum,
                       nchannels, nthreads_ref, buff_size, rings, 0, nullptr, force_relay != 0);
}

// AllToAllv on host threads: counts is the n x n byte matrix (counts[s * n + t]:
// what s sends to t), sdispls / rdispls hold each rank's displacement row
// (sdispls[r * n + t], rdispls[r * n + s]).  One hop only, as mccsAllToAllv.
// With `tables` (each rank's size table, mccs_host_ring_all_to_all_v_tables) the
// three arrays are unused and every size is read from the tables.
static mccsResult_t host_ring_a2av(int nranks, const void* const* sendbufs, void* const* recvbufs,
                                   const size_t* counts, const size_t* sdispls, const size_t* rdispls,
                                   const uint64_t* const* tables, int nchannels, int nthreads_ref, int buff_size,
                                   const int* rings, int force_relay) {
  if (nranks < 1 || nranks > 64 || !sendbufs || !recvbufs || (!tables && (!counts || !sdispls || !rdispls)) ||
      nchannels < 1 || nchannels > MCCS_MAX_NCHANNELS || nthreads_ref <= WARP_SIZE || buff_size < 8192 || buff_size % 8192)
    return mccsInvalidArgument;
  if (rings)
    for (int ch = 0; ch < nchannels; ++ch) {
      uint64_t seen = 0;
      for (int i = 0; i < nranks; ++i)
        if (rings[ch * nranks + i] >= 0 && rings[ch * nranks + i] < nranks) seen |= 1ull << rings[ch * nranks + i];
      if (seen != (nranks == 64 ? ~0ull : (1ull << nranks) - 1)) return mccsInvalidArgument;  // not a permutation
    }
  if (tables)
    for (int r = 0; r < nranks; ++r)
      if (!tables[r]) return mccsInvalidArgument;
  if (nranks == 1) {
    mccs::A2AvdElem self = {counts ? counts[0] : 0, sdispls ? sdispls[0] : 0, 0, rdispls ? rdispls[0] : 0};
    if (tables)
      self = mccs::a2avd_resolve(tables[0], 1, 0, MCCS_A2A_ROUTE(0, 0, 0, 1), [](const uint64_t* q) { return *q; });
    if (self.S) std::memmove((char*)recvbufs[0] + self.recvOff, (const char*)sendbufs[0] + self.sendOff, self.S);
    return mccsSuccess;
  }
  std::vector<int> ident;
  if (!rings)
    for (int ch = 0; ch < nchannels; ++ch)
      for (int i = 0; i < nranks; ++i) ident.push_back(i);
  std::vector<int> sb((size_t)nranks * nchannels), rb((size_t)nranks * nchannels);
  int hops = 0, m = 0;
  mccs::alltoall_route(nranks, nchannels, rings ? rings : ident.data(), force_relay != 0, &hops, &m, sb.data(),
                       rb.data());
  if (hops != 1 || m < 1) return mccsInvalidUsage;  // a relay would need sizes that are neither its row nor its column
  HostRingPool& pool = HostRingPool::get();
  std::lock_guard<std::mutex> call(pool.call_mu);
  std::vector<HostConn>& conns = pool.fifos((size_t)nchannels * nranks, (size_t)buff_size);
  Ctx c;
  c.func = MCCS_FUNC_ALLTOALLV;
  c.n = nranks;
  c.nch = nchannels;
  c.dt = mccsInt8;
  c.op = mccsDevSum;
  c.op_arg = 0;
  c.nthreads_ref = nthreads_ref;
  c.buff_size = buff_size;
  c.es = 1;
  c.count = 0;  // each walk has its own size
  c.send = sendbufs;
  c.recv = recvbufs;
  c.rings = rings;
  c.root = 0;
  c.conns = &conns;
  c.timeout_s = 60.0;
  c.a2a_hops = 1;
  c.walk_nch = m;
  c.a2a_send_bid = sb.data();
  c.a2a_recv_bid = rb.data();
  c.v_counts = counts;
  c.v_sdispls = sdispls;
  c.v_rdispls = rdispls;
  c.v_tables = tables;
  pool.run(&c, nranks * nchannels);
  return c.failed.load() ? mccsTimeout : mccsSuccess;
}

extern "C" mccsResult_t mccs_host_ring_all_to_all_v(int nranks, const void* const* sendbufs, void* const* recvbufs,
                                                    const size_t* counts, const size_t* sdispls,
                                                    const size_t* rdispls, int nchannels, int nthreads_ref,
                                                    int buff_size, const int* rings, int force_relay) {
  if (!counts || !sdispls || !rdispls) return mccsInvalidArgument;
  return host_ring_a2av(nranks, sendbufs, recvbufs, counts, sdispls, rdispls, nullptr, nchannels, nthreads_ref,
                        buff_size, rings, force_relay);
}

// The AllToAllvDev schedule on host threads: tables[r] is rank r's size table
// in host memory (4 * nranks words, ring_walk.h a2avd_index).  Each channel's
// element is resolved through a2avd_resolve, then walked as above.
extern "C" mccsResult_t mccs_host_ring_all_to_all_v_tables(int nranks, const void* const* sendbufs,
                                                           void* const* recvbufs, const uint64_t* const* tables,
                                                           int nchannels, int nthreads_ref, int buff_size,
                                                           const int* rings, int force_relay) {
  if (!tables) return mccsInvalidArgument;
  return host_ring_a2av(nranks, sendbufs, recvbufs, nullptr, nullptr, nullptr, tables, nchannels, nthreads_ref,
                        buff_size, rings, force_relay);
}

// Send/Recv on host threads (mccsSend / mccsRecv): op i is a send or a receive
// of op_bytes[i] bytes at op_buf[i] that rank op_rank[i] issues with
// op_peer[i]; each rank's ops, in list order, form one group.  The elements
// come from the planner's pairing rule (plan.cpp sendrecv_elements) and are
// walked as AllToAllv's.  One hop only.  This entry point sees every rank, so
// unlike the device path it refuses a send without its receive, or of another
// size (mccsInvalidArgument), instead of stalling.
extern "C" mccsResult_t mccs_host_ring_send_recv(int nranks, int nops, const int* op_rank, const int* op_is_send,
                                                 const int* op_peer, void* const* op_buf, const size_t* op_bytes,
                                                 int nchannels, int nthreads_ref, int buff_size, const int* rings) {
  if (nranks < 2 || nranks > 64 || nops < 0 || (nops && (!op_rank || !op_is_send || !op_peer || !op_buf || !op_bytes)) ||
      nchannels < 1 || nchannels > MCCS_MAX_NCHANNELS || nthreads_ref <= WARP_SIZE || buff_size < 8192 || buff_size % 8192)
    return mccsInvalidArgument;
  if (rings)
    for (int ch = 0; ch < nchannels; ++ch) {
      uint64_t seen = 0;
      for (int i = 0; i < nranks; ++i)
        if (rings[ch * nranks + i] >= 0 && rings[ch * nranks + i] < nranks) seen |= 1ull << rings[ch * nranks + i];
      if (seen != (nranks == 64 ? ~0ull : (1ull << nranks) - 1)) return mccsInvalidArgument;  // not a permutation
    }
  std::vector<std::vector<mccs::SrOp>> ops((size_t)nranks);
  // per ordered pair (s, t) the sizes of its sends and of its receives, in order: they must agree
  std::vector<std::vector<size_t>> sent((size_t)nranks * nranks), rcvd((size_t)nranks * nranks);
  for (int i = 0; i < nops; ++i) {
    const int r = op_rank[i], p = op_peer[i];
    if (r < 0 || r >= nranks || p < 0 || p >= nranks || p == r || (!op_buf[i] && op_bytes[i])) return mccsInvalidArgument;
    ops[r].push_back(mccs::SrOp{op_is_send[i] != 0, p, op_buf[i], op_bytes[i]});
    (op_is_send[i] ? sent[(size_t)r * nranks + p] : rcvd[(size_t)p * nranks + r]).push_back(op_bytes[i]);
  }
  if (sent != rcvd) return mccsInvalidArgument;
  std::vector<int> ident;
  if (!rings) {
    for (int ch = 0; ch < nchannels; ++ch)
      for (int i = 0; i < nranks; ++i) ident.push_back(i);
    rings = ident.data();
  }
  std::vector<int> sb((size_t)nranks * nchannels), rb((size_t)nranks * nchannels);
  int hops = 0, m = 0;
  mccs::alltoall_route(nranks, nchannels, rings, false, &hops, &m, sb.data(), rb.data());
  if (hops != 1 || m < 1) return mccsInvalidUsage;  // a relay: a message would need ranks that are not its two ends
  std::vector<std::vector<mccs::SrElem>> elems((size_t)nranks * nchannels), one;
  for (int r = 0; r < nranks; ++r) {
    int next[MCCS_MAX_NCHANNELS], prev[MCCS_MAX_NCHANNELS];
    for (int ch = 0; ch < nchannels; ++ch)
      for (int i = 0; i < nranks; ++i)
        if (rings[ch * nranks + i] == r) {
          next[ch] = rings[ch * nranks + (i + 1) % nranks];
          prev[ch] = rings[ch * nranks + (i + nranks - 1) % nranks];
        }
    mccs::sendrecv_elements(nchannels, next, prev, ops[r].data(), (int)ops[r].size(), &one);
    for (int ch = 0; ch < nchannels; ++ch) elems[(size_t)r * nchannels + ch] = one[ch];
  }
  const std::vector<const void*> no_send((size_t)nranks, nullptr);
  const std::vector<void*> no_recv((size_t)nranks, nullptr);
  HostRingPool& pool = HostRingPool::get();
  std::lock_guard<std::mutex> call(pool.call_mu);
  std::vector<HostConn>& conns = pool.fifos((size_t)nchannels * nranks, (size_t)buff_size);
  Ctx c;
  c.func = MCCS_FUNC_SENDRECV;
  c.n = nranks;
  c.nch = nchannels;
  c.dt = mccsInt8;
  c.op = mccsDevSum;
  c.op_arg = 0;
  c.nthreads_ref = nthreads_ref;
  c.buff_size = buff_size;
  c.es = 1;
  c.count = 0;  // each walk has its own size
  c.send = no_send.data();  // every element names its own buffers
  c.recv = no_recv.data();
  c.rings = rings;
  c.root = 0;
  c.conns = &conns;
  c.timeout_s = 60.0;
  c.a2a_hops = 1;
  c.walk_nch = m;
  c.a2a_send_bid = sb.data();
  c.a2a_recv_bid = rb.data();
  c.sr_elems = &elems;
  pool.run(&c, nranks * nchannels);
  return c.failed.load() ? mccsTimeout : mccsSuccess;
}

// The three reducing collectives with an op argument: all six ops, PreMulSum's
// scalar / SumPostDiv's divisor in op_arg under the rules of the mccs*OpArg
// entry points; same schedule, pre and post applied where the kernels do.
extern "C" mccsResult_t mccs_host_ring_allreduce_oparg(int nranks, const void* const* sendbufs, void* const* recvbufs,
                                                       size_t count, int dtype, int op, int nchannels,
                                                       int nthreads_ref, int buff_size, const int* rings,
                                                       uint64_t op_arg) {
  return host_ring_run(mccsFuncAllReduce, nranks, sendbufs, recvbufs, count, dtype, op, nchannels, nthreads_ref,
                       buff_size, rings, 0, &op_arg);
}

extern "C" mccsResult_t mccs_host_ring_reduce_scatter_oparg(int nranks, const void* const* sendbufs,
                                                            void* const* recvbufs, size_t recvcount, int dtype, int op,
                                                            int nchannels, int nthreads_ref, int buff_size,
                                                            const int* rings, uint64_t op_arg) {
  return host_ring_run(mccsFuncReduceScatter, nranks, sendbufs, recvbufs, recvcount, dtype, op, nchannels,
                       nthreads_ref, buff_size, rings, 0, &op_arg);
}

extern "C" mccsResult_t mccs_host_ring_reduce_oparg(int nranks, const void* const* sendbufs, void* const* recvbufs,
                                                    size_t count, int dtype, int op, int root, int nchannels,
                                                    int nthreads_ref, int buff_size, const int* rings,
                                                    uint64_t op_arg) {
  return host_ring_run(mccsFuncReduce, nranks, sendbufs, recvbufs, count, dtype, op, nchannels, nthreads_ref,
                       buff_size, rings, root, &op_arg);
}
