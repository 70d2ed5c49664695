// ring_walk.h — the ring chunk walk, stated once.
//
// Every path that produces an AllReduce, AllGather or ReduceScatter result
// cuts the buffer into the same chunks: the ring kernels (ring_kernel.h), the
// direct and LL kernels (direct_kernel.h), the planner's owned[] counts
// (host/plan.cpp build_direct) and the host-thread ring (host/host_ring.cpp).
// They all take the arithmetic from here, so "the ring's result, bit for bit"
// cannot drift between them.  mccs_ring_walk (host/api.cpp) prints the walk
// for tests/test_ring_walk.py, which holds it to the Python models.
// AllToAll cuts a pair's block as AllGather cuts a block; which call of a loop
// moves which block (a2a_call) is stated here too, for the kernel and the
// host-thread ring alike.
//
// I is the integer type of the walk: int64_t for the ring and the host
// paths, uint32_t for the direct kernels (direct_kernel.h says why).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mccs_devcomm.h"
#include "ring_cfg.h"  // the AllToAll route word (a2avd_resolve)

namespace mccs {

template <typename I>
__host__ __device__ __forceinline__ I div_up(I a, I b) {
  return (a + b - 1) / b;
}
template <typename I>
__host__ __device__ __forceinline__ I round_up(I a, I b) {
  return div_up(a, b) * b;
}

// Geometry of one work element, in elements of `esize` bytes.  The number of
// parts (chunks) per loop is not kept: walk_parts gives it.
template <typename I>
struct RingWalk {
  I size;       // AllReduce, Broadcast, Reduce: the buffer; AllGather / ReduceScatter: one rank's block
  I stepSize;   // one FIFO step
  I chunkSize;  // the largest chunk
  I loopSize;   // what one loop of all channels covers
  I gran;       // realChunkSize is a multiple of this
};

// Chunks per loop: AllReduce cuts a loop into a chunk per channel and rank,
// the block collectives into one per channel.
template <typename I>
__host__ __device__ __forceinline__ I walk_parts(int func, I nChannels, int nranks) {
  return func == mccsFuncAllReduce ? nChannels * nranks : nChannels;
}

// all_reduce.h:17-21,30 / all_gather.h:16-20,30.  func is mccsFuncAllReduce,
// mccsFuncAllGather (esize = 1: the int8 kernel counts bytes) or
// mccsFuncReduceScatter (a block split over the channels like AllGather's, in
// AllReduce's element granule).  mccsFuncBoadcast and
// mccsFuncReduce cut the whole buffer (size) as a block is cut: Broadcast as
// AllGather does (esize = 1), Reduce as ReduceScatter does.  nthreads_ref is the
// reference's thread count (nWarps * WARP_SIZE), buff_size the FIFO's bytes.
// The reference holds chunkSize in an int: the (int) here and the ones in
// real_chunk_size / block_chunk_offset are its truncations.
// Fills w in place (the ring kernel's lives in LDS); walk_guard completes it.
template <typename I>
__host__ __device__ __forceinline__ void ring_walk(RingWalk<I>& w, int func, int nranks, int nChannels, int esize,
                                                   int nthreads_ref, int buff_size, I size) {
  static_assert(ALLGATHER_CHUNKSTEPS == ALLREDUCE_CHUNKSTEPS, "one chunkSize for the three functions");
  w.stepSize = (I)(buff_size / MCCS_BUFFER_SLOTS / esize);
  w.size = size;
  w.chunkSize = (I)(int)(w.stepSize * ALLREDUCE_CHUNKSTEPS);
  if constexpr (sizeof(I) == 4) {
    // 32 bits hold a bucket of < 2^31 elements, not every loopSize: one at or
    // above the bucket's size means a single loop whatever its value
    const uint64_t loop = walk_parts(func, (uint64_t)nChannels, nranks) * w.chunkSize;
    w.loopSize = loop > 0x7fffffffu ? 0x7fffffffu : (I)loop;
  } else {
    w.loopSize = walk_parts(func, (I)nChannels, nranks) * w.chunkSize;
  }
  w.gran = (I)(nthreads_ref - WARP_SIZE) * 8 / (I)esize;
}

// A work element of fewer than two reference warps, which no host path sends,
// has no granule: 1 keeps the walk's divisions defined.  Apart from ring_walk
// because the ring kernel applies it after the rest of its schedule: next to
// the store of gran the compiler folds the two into a select, which moved
// registers and spills in most ring kernels (tools/kernel_resources.py --diff).
template <typename I>
__host__ __device__ __forceinline__ void walk_guard(RingWalk<I>& w) {
  if (w.gran < 1) w.gran = 1;
}

// realChunkSize of the loop at gridOffset (all_reduce.h:31-36, all_gather.h:
// 31-35): what is left over the loop's parts, at most chunkSize, rounded up
// to the granule.
template <typename I>
__host__ __device__ __forceinline__ I real_chunk_size(const RingWalk<I>& w, I gridOffset, I parts) {
  I rcs = div_up(w.size - gridOffset, parts);
  rcs = w.chunkSize < rcs ? w.chunkSize : rcs;
  return (I)(int)round_up(rcs, w.gran);
}

// AllReduce: chunk `chunk` (a ring index) of channel bid is part bid * nranks
// + chunk of the loop (all_reduce.h:38-42); the second form takes the part.
template <typename I>
__host__ __device__ __forceinline__ I allreduce_chunk_offset(I gridOffset, I bid, int nranks, int chunk, I rcs) {
  return gridOffset + bid * nranks * rcs + (I)chunk * rcs;
}
template <typename I>
__host__ __device__ __forceinline__ I allreduce_chunk_offset(I gridOffset, I part, I rcs) {
  return gridOffset + part * rcs;
}
// AllGather / ReduceScatter: channel bid's chunk of the block (all_gather.h:36).
template <typename I>
__host__ __device__ __forceinline__ I block_chunk_offset(I gridOffset, I bid, I rcs) {
  return gridOffset + (I)(int)(bid * rcs);
}
// Elements of the chunk at `off` (all_reduce.h:42, all_gather.h:37).  Signed
// I: <= 0 past the end, an empty call that still takes and posts its steps.
template <typename I>
__host__ __device__ __forceinline__ I chunk_nelem(I size, I off, I rcs) {
  return rcs < size - off ? rcs : size - off;
}

// AllReduce: the chunk primitive call j = 0 .. 2n-2 of a loop works on, for
// the rank at ring index ringIx (all_reduce.h:46-84: send ringIx+n-1, the
// reduce calls down to ringIx, the copy calls from ringIx+n-1 down to ringIx+1).
__host__ __device__ __forceinline__ int allreduce_call_chunk(int ringIx, int n, int j) {
  const int chunk = j <= n - 1 ? ringIx + n - 1 - j : ringIx + 2 * n - 1 - j;
  return chunk >= n ? chunk - n : chunk;
}

// AllToAll: the primitive calls of one loop (ring_cfg.h has the route a work
// element carries).  For each distance d = 1 .. hops a rank
//   sends its block for userRanks[d]                          (send),
//   hands on the d-1 blocks that arrive for ranks beyond it   (recvSend: FIFO
//     slot to FIFO slot, no user buffer),
//   receives the block of userRanks[n-d] into its place       (recv).
// The k-th block to arrive in phase d left the rank k hops back, so the d-th
// is this rank's.  hops = 1 is the one-hop route (send to the successor,
// receive from the predecessor); hops = n-1 the relay.
enum : int { kA2ASend = 0, kA2ARelay = 1, kA2ARecv = 2 };
__host__ __device__ __forceinline__ int a2a_calls_per_loop(int hops) { return hops * (hops + 3) / 2; }
// Call j of a loop: its distance d and role.  Phase d holds d + 1 calls.
__host__ __device__ __forceinline__ int a2a_call(int j, int* d_out) {
  int d = 1;
  while (j > d) {
    j -= d + 1;
    ++d;
  }
  *d_out = d;
  return j == 0 ? kA2ASend : j == d ? kA2ARecv : kA2ARelay;
}
// Index into ring.userRanks of the block a call of distance d reads from the
// send buffer (send) or writes in the receive buffer (recv).
__host__ __device__ __forceinline__ int a2a_send_block(int d) { return d; }
__host__ __device__ __forceinline__ int a2a_recv_block(int n, int d) { return n - d; }

// AllToAllv: per-peer byte counts on the one-hop route (ring_cfg.h
// MCCS_FUNC_ALLTOALLV).  Channel c of rank r, with successor t
// and predecessor p, walks two blocks cut over the pair's m channels as
// AllToAll cuts one (esize 1, nChannels = m): the send walk over S =
// sendcounts[t] with part send_bid, the receive walk over R = recvcounts[p]
// with part recv_bid.  stepSize, chunkSize, loopSize and the granule are
// common (one thread count, one buffer size); only `size` differs.  With Ls =
// a2av_loops(S) and Lr = a2av_loops(R), the element's calls are, for loop
// i = 0 .. max(Ls, Lr) - 1:  send(i) if i < Ls,  recv(i) if i < Lr.
// An exhausted side makes no call and takes no step, so a connection advances
// by its own pair's count alone, on both of its ends.  Inside a live side a
// channel past the end of a short block still makes its empty, stepping call.
// The list has Ls + Lr calls; a2av_first / a2av_next step through it (the
// caller counts the calls: a2av_next after the last one is meaningless).
enum : int { kA2AvSend = 0, kA2AvRecv = 1 };
template <typename I>
__host__ __device__ __forceinline__ I a2av_loops(I size, I loopSize) {
  return size > 0 ? div_up(size, loopSize) : 0;
}
template <typename I>
__host__ __device__ __forceinline__ int a2av_first(I S) {
  return S > 0 ? kA2AvSend : kA2AvRecv;
}
// The call after `side` of the loop at *g: its side; *g moves to its loop.
template <typename I>
__host__ __device__ __forceinline__ int a2av_next(I S, I R, I loopSize, I* g, int side) {
  if (side == kA2AvSend && *g < R) return kA2AvRecv;
  *g += loopSize;
  return *g < S ? kA2AvSend : kA2AvRecv;
}
// realChunkSize of one side's loop: real_chunk_size with that side's size.
template <typename I>
__host__ __device__ __forceinline__ I a2av_chunk_size(const RingWalk<I>& w, I size, I gridOffset, I parts) {
  I rcs = div_up(size - gridOffset, parts);
  rcs = w.chunkSize < rcs ? w.chunkSize : rcs;
  return (I)(int)round_up(rcs, w.gran);
}

// AllToAllvDev: the size table a call's elements are resolved from (ring_cfg.h
// MCCS_FUNC_ALLTOALLV_DEV).  4 * nranks 64-bit words in bytes; the word of
// `row` for `peer` is at a2avd_index.  The kernel, the host-thread ring and
// the tests' expectations index the table through this one definition.
enum : int { kA2AvdSendCounts = 0, kA2AvdSendDispls = 1, kA2AvdRecvCounts = 2, kA2AvdRecvDispls = 3, kA2AvdRows = 4 };
__host__ __device__ __forceinline__ int64_t a2avd_index(int row, int nranks, int peer) {
  return (int64_t)row * nranks + peer;
}
// What an AllToAllv element holds, read from the table: the send walk's bytes
// S and offset into sendbuff, the receive walk's bytes R and offset into
// recvbuff.
struct A2AvdElem {
  uint64_t S, sendOff, R, recvOff;
};
// Element of the route word `route` on rank `rank`.  hops = 1: S and its
// displacement are the successor's words of rows 0 and 1, R and its
// displacement the predecessor's words of rows 2 and 3.  hops = 0 (the self
// element, and the one element of a one-rank call): the rank's own words of
// rows 0, 1 and 3; R = 0, as in the AllToAllv self element (the contract makes
// recvcounts[rank] == sendcounts[rank]).  ld(p) loads the word at p.
template <typename Load>
__host__ __device__ __forceinline__ A2AvdElem a2avd_resolve(const uint64_t* table, int nranks, int rank,
                                                            uint32_t route, Load ld) {
  const bool self = MCCS_A2A_HOPS(route) == 0;
  const int t = self ? rank : MCCS_A2AVD_NEXT(route), p = self ? rank : MCCS_A2AVD_PREV(route);
  A2AvdElem e;
  e.S = ld(table + a2avd_index(kA2AvdSendCounts, nranks, t));
  e.sendOff = ld(table + a2avd_index(kA2AvdSendDispls, nranks, t));
  e.R = self ? 0 : ld(table + a2avd_index(kA2AvdRecvCounts, nranks, p));
  e.recvOff = ld(table + a2avd_index(kA2AvdRecvDispls, nranks, p));
  return e;
}

// Slice size of a primitive call of nelem elements (prims_simple.h:156-157):
// sps steps per slice, spc slices per call.
template <typename I>
__host__ __device__ __forceinline__ I slice_size(I nelem, I stepSize, int sps, int spc) {
  const I sliceSize = (nelem + 16 * (I)spc - 1) / (16 * (I)spc) * 16;
  const I span = stepSize * sps;
  return sliceSize > span / 32 ? sliceSize : span / 32;
}

}  // namespace mccs
