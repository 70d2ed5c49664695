// ring_cfg.h — conventions shared by the ring kernels and the C++ host.
//
// FIFO flag lines.  A connector's `tail` / `head` pointers (mccsDevConnInfo,
// devcomm.h:36-46) point at an array of 128-byte lines, one per lane (a lane
// is one workgroup of a channel; the reference has exactly one, lane 0):
//   word 0  the step counter the peer polls / we poll
//   word 1  this side's saved step for the lane (local lines only)
// With one lane this is binary-compatible with the reference SHM metadata
// (SendBufMeta.head / RecvBufMeta.tail at offset 0 followed by 120 pad bytes,
// src/mccs/src/transport/meta.rs:7-67), so word 1 is free padding there.
#pragma once
#include <stdint.h>

#include "mccs_devcomm.h"

#define MCCS_FLAG_LINE_BYTES 128
#define MCCS_FLAG_LINE_WORDS (MCCS_FLAG_LINE_BYTES / 8)
#define MCCS_MAX_LANES 64
// Largest ring workgroup.  576 = 9 waves covers the reference's 17-warp (544
// thread) blocks (get_task_schema, plan.rs:602-635) and keeps ~168 VGPRs per
// lane (3 waves per SIMD): the fully inlined ring loop with 8 packs in flight
// per source fits without spilling, which a 1024-thread bound (128 VGPRs) did not.
#define MCCS_RING_MAX_THREADS 576

// Fence policy for FIFO hand-offs.  Communicator launches carry it in their
// launch arguments (mccsMultiLaunchArgs.cfg); the reference-named kernels,
// launched by an external planner that cannot say what memory its FIFOs are,
// always run with the reference defaults (system-scope fences, 2-step slices).
#define MCCS_FENCE_SYSTEM 0   // FIFO memory may be cached: system-scope release/acquire
#define MCCS_FENCE_UNCACHED 1 // FIFO memory is uncached (hipDeviceMallocUncached): drains only
// Uncached FIFO memory, but a system-scope release fence before every post
// (the analogue of __threadfence_system before postPeer, prims_simple.h:
// 120-125,211); polls stay relaxed.  The step between relaxed hand-offs and
// the cached-memory mode for links where a drained store might not yet be
// visible to the peer when the flag lands.
#define MCCS_FENCE_UNCACHED_RELEASE 2

// Error bits a ring kernel reports for ONE communicator: word 1 of the
// communicator's own abort line (abortFlag[1]; the library allocates that line,
// 64 bytes, zeroed at init), read back by mccsCommSync.  A process-wide word
// would let one communicator's abort fail another's sync.
#define MCCS_ERR_TIMEOUT 1u
#define MCCS_ERR_ABORTED 2u

struct mccsRingKernelCfg {
  uint32_t fence_mode;    // MCCS_FENCE_*
  uint32_t slice_steps;   // FIFO steps per slice: 2 (reference SliceSteps) or 4 (one slice per chunk)
  uint64_t timeout_ticks; // s_memrealtime ticks (100 MHz); 0 = never
  uint32_t profile;       // 1: accumulate per-slice wait / work ticks (mccs_ring_profile)
  uint32_t err_line;      // 1: error bits go to abortFlag[1] (library launches: the abort line is
                          // ours); 0: reference-named kernels, whose abortFlag is the caller's
                          // 4-byte allocation: only abortFlag itself is raised (the reference's
                          // one error channel, devcomm.h abortFlag)
  uint32_t fifo_slots;    // physical FIFO slots (power of two >= MCCS_BUFFER_SLOTS): slot = step % fifo_slots,
                          // a sender may run fifo_slots steps ahead; the reference has 8
  uint32_t no_guard;      // 1: skip the launch guard (test hook MCCS_LAUNCH_GUARD=0 only)
};

// ---- Launch guard (launch_guard.h): one launch of a communicator at a time.
// A communicator's kernels share its FIFO flag lines, the lanes' saved steps
// (word 1 above) and the direct control block, so two of its launches running
// at once return wrong sums.  The host orders eager launches across streams
// (plan.cpp), but a graph replay makes no library call; so every library
// launch first takes its communicator's guard line on the device and gives it
// back when its last workgroup is done.  The line lives in the communicator's
// device allocation, after mccsDevCommAndChannels and the per-channel views.
// One word holds the whole state, so each step is one atomic: the holder's
// token in bits 17..63 (0 = free), bit 16 "every slot held" (fused launches),
// bits 0..15 the holder's workgroups of this slot that have finished.
#define MCCS_GUARD_FIN_MASK 0xffffull
#define MCCS_GUARD_CONFIRMED (1ull << 16)
#define MCCS_GUARD_TOK_SHIFT 17
struct mccsLaunchGuard {
  uint64_t word;   // token << MCCS_GUARD_TOK_SHIFT | confirmed | finished workgroups; 0 = free
  uint64_t waits;  // workgroups that found the guard held by another launch (diagnostic, only grows)
  uint64_t pad[14];
};
#define MCCS_GUARD_OFF                                                                                      \
  ((sizeof(struct mccsDevCommAndChannels) + MCCS_MAX_NCHANNELS * sizeof(struct mccsRingConnView) + 127) / \
   128 * 128)

// ---- AllToAll (ring_a2a.hip, ring_walk.h a2a_call, host/plan.cpp) ----------
// The function id is the library's own: the device ABI (mccsDevFunc_t) names
// no all-to-all, and the id never leaves the library (it selects the kernel on
// the host and the walk at compile time; work headers carry funcIndex 0).
#define MCCS_FUNC_ALLTOALL 8  // == mccsNumFuncs: past every mccsDevFunc_t value
// An AllToAll work element: count = bytes per peer, nChannels = m (the
// channels a pair's block is cut over), bid = the part of the block this
// channel SENDS, and mccsDevWorkElem.root, free for this function, holds the
// rest of the route:
//   bits  0..7   hops: the largest distance a loop walks.  1: the channel
//                carries only the block for its ring successor (one hop);
//                nranks - 1: every block, relayed along the ring
//   bits  8..15  recv_bid: the part of the block this channel RECEIVES (one
//                hop: counted from the receiver's side, it may differ from
//                bid; relay: == bid)
//   bits 16..23  part, bits 24..31 parts: the rank's own block, copied send ->
//                recv without a FIFO step, is cut into `parts` pieces over the
//                element's channels and this channel copies piece `part`
// Captured graphs and batched groups carry the route with the element.
#define MCCS_A2A_ROUTE(hops, recv_bid, part, parts) \
  ((uint32_t)(hops) | (uint32_t)(recv_bid) << 8 | (uint32_t)(part) << 16 | (uint32_t)(parts) << 24)
#define MCCS_A2A_HOPS(route) ((int)((route) & 0xffu))
#define MCCS_A2A_RECV_BID(route) ((int)((route) >> 8 & 0xffu))
#define MCCS_A2A_PART(route) ((int)((route) >> 16 & 0xffu))
#define MCCS_A2A_PARTS(route) ((int)((route) >> 24 & 0xffu))

// ---- AllToAllv (ring_a2av.hip, ring_walk.h a2av_next, host/plan.cpp) -------
// Per-peer byte counts on the one-hop route only.  Library-internal like 8.
#define MCCS_FUNC_ALLTOALLV 9
// An AllToAllv work element of channel c (successor t, predecessor p) holds two
// walks over the pair's m channels: sendbuff = send + sdispls[t] and count =
// sendcounts[t] (part bid), recvbuff = recv + rdispls[p] and redOpArg =
// recvcounts[p] (part recv_bid of the route word, hops = 1).  The rank's own
// block is a second element: hops = 0, both buffers offset to the self
// segments, count its bytes, part / parts over the comm's channels; it makes no
// FIFO call.  nWarps is the same in every element of every rank: the granule
// it sets cuts the pair's block on both ends of a connection.

// ---- AllToAllvDev (ring_a2avd.hip, ring_walk.h a2avd_resolve, host/plan.cpp) -
// AllToAllv whose sizes the kernel reads from device memory when it runs, so a
// replayed graph takes the sizes of the moment.  Library-internal like 8 and 9.
#define MCCS_FUNC_ALLTOALLV_DEV 10
// The size table of a call: 4 * nranks 64-bit words in bytes, row * nranks +
// peer (ring_walk.h a2avd_index): row 0 sendcounts, 1 sdispls, 2 recvcounts,
// 3 rdispls.  An AllToAllvDev work element holds the call's BASE pointers in
// sendbuff / recvbuff, the table's address in count, and redOpArg = 0; bid,
// nChannels, nWarps and the route word are those of the AllToAllv element.
// The part / parts bytes of a hops = 1 route word are unused, so there they
// name the pair's peers: bits 16..23 the successor t, bits 24..31 the
// predecessor p (a rank is < 64).  The self element (hops = 0) keeps part /
// parts; the kernel takes the rank from the communicator.  The kernel rewrites
// its LDS copy of the element into the AllToAllv form (count = S, redOpArg =
// R, both buffers offset) before anything else reads it.
#define MCCS_A2AVD_ROUTE(recv_bid, next, prev) MCCS_A2A_ROUTE(1, recv_bid, next, prev)
#define MCCS_A2AVD_NEXT(route) MCCS_A2A_PART(route)
#define MCCS_A2AVD_PREV(route) MCCS_A2A_PARTS(route)

// ---- Send/Recv (ring_sr.hip, host/plan.cpp sendrecv_elements) ---------------
// Grouped point-to-point on the one-hop route.  The reference reserves
// mccsFuncSendRecv = 5, mccsFuncSend = 6 and mccsFuncRecv = 7 with a P2p work
// element (mccsDevWorkElemP2p) that presumes peer-indexed connectors; this
// library builds ring connectors only, so Send/Recv runs on them under an id
// of its own, with mccsDevWorkTypeColl works of the usual element layout.
#define MCCS_FUNC_SENDRECV 11
// A Send/Recv work element is an AllToAllv element with hops = 1 and no
// displacement: sendbuff = a send's buffer and count = its bytes S, for the
// channel's successor (part bid of the pair's m channels); recvbuff = a
// receive's buffer and redOpArg = its bytes R, from the channel's predecessor
// (part recv_bid of the route word).  S = 0 or R = 0: that side makes no call
// and takes no step.  Which call of a group lands in which element of which
// channel is the pairing rule of host/plan.cpp sendrecv_elements.

// Per-device ring profile counters (s_memrealtime ticks, 100 MHz), summed
// over every slice of every workgroup while mccsRingKernelCfg.profile is set.
#define MCCS_PROF_SLICES 0  // slices executed
#define MCCS_PROF_WAIT 1    // slice start -> peer flags satisfied (thread 0)
#define MCCS_PROF_WORK 2    // flags satisfied -> stores drained, both barriers included
#define MCCS_PROF_DRAIN 3   // part of WORK: thread 0's wave done issuing -> every wave drained (barrier)
#define MCCS_PROF_N 4

// Communicator launch: one or several communicators of one device in ONE
// launch (several when ranks share a GPU: tests' virtual node).
// blockIdx.y = rank slot.
#define MCCS_MULTI_MAX_RANKS 16
// A launch whose ranks' channels each run one work of one element may carry
// those works in its arguments (kernarg memory is device memory on MI355X)
// instead of the host-mapped work FIFO, whose read over PCIe is the long pole
// of the kernel prologue; inFifo = 0, so nothing is acknowledged.  Rank slot
// k's works are inline_work[k * channels used ...], each only its header and
// its one element (mccsInlineWork, 56 B instead of mccsDevWork's 512): HIP
// copies every argument byte at every launch, and 4 KiB of them cost 1-3 us
// of host time per launch (profiles/r05_host_overhead.json).  8 works: the
// n = 8 rings (7 channels), or two fused rank slots of 4 channels.
#define MCCS_INLINE_WORKS 8
struct mccsInlineWork {
  struct mccsDevWorkHeader header;
  struct mccsDevWorkElem elem;
};
// The connector addresses one channel's lanes need (the prev recv and next
// send mccsDevConnInfo fields), kept by this library beside its device
// communicator (comm.cpp comm_build_device): a launch loads them together with
// the communicator instead of one dependent round trip later through
// mccsDevChannel.peers.  Reference-built communicators have none (view = 0).
struct mccsRingConnView {
  char* rbuf;        // receive FIFO data
  char* sbuf;        // send FIFO data
  uint64_t* r_tail;  // recv: polled (ours)
  uint64_t* r_head;  // recv: posted (prev's)
  uint64_t* s_head;  // send: polled (ours)
  uint64_t* s_tail;  // send: posted (next's)
};
struct mccsMultiLaunchArgs {
  struct mccsDevComm* comm[MCCS_MULTI_MAX_RANKS];
  struct mccsDevWork* work[MCCS_MULTI_MAX_RANKS];
  const struct mccsRingConnView* view[MCCS_MULTI_MAX_RANKS];  // per channel id; 0: use comm's peers
  uint64_t channelMask;
  struct mccsRingKernelCfg cfg;  // this launch's hand-off policy
  uint32_t inline_works;         // > 0: the works are inline_work[0 .. inline_works)
  uint32_t pad3;
  uint64_t guard_order;          // rank slots by guard address, 4 bits each (launch_guard.h)
  struct mccsInlineWork inline_work[MCCS_INLINE_WORKS];
};
#ifdef __cplusplus
static_assert(sizeof(mccsInlineWork) == 56 && offsetof(mccsInlineWork, elem) == offsetof(mccsDevWork, elems),
              "an inline work is the head of a mccsDevWork: header + one element");
static_assert(sizeof(mccsMultiLaunchArgs) <= 1024, "ring launch arguments must stay within 1 KiB");
#endif

// ---- Direct AllReduce on a fully connected node (direct_kernel.h)
// Every rank reaches every peer's arena over its own xGMI link, so instead of
// 2(n-1) ring hops a bucket takes two (two-shot: each rank writes every chunk
// it does not own into the owner's "in" slot, each owner reduces its chunks
// in exactly the ring's order and writes the result into every peer's "out"
// slot, every rank copies the results it does not own to its output) or one
// (one-shot, small buckets: every rank writes its whole input into every
// peer's one-shot slot and every rank reduces every chunk itself, in the
// ring's order).  Chunk ownership and summation order are the ring's
// (all_reduce.h), so results are bit-identical to the ring and the oracle.
//
// A rank's direct region (in its FIFO arena, after the ring's data):
//   [control, MCCS_DIRECT_CTRL_BYTES]
//   [two-shot in : MCCS_DIRECT_MAX_RANKS senders x slot_bytes]  (by element offset)
//   [two-shot out: slot_bytes]
//   [one-shot in : 2 parities x MCCS_DIRECT_MAX_RANKS senders x oslot_bytes]
//   [LL one-shot : 2 parities x MCCS_DIRECT_MAX_RANKS senders x ll_slot_bytes]
// LL one-shot (the smallest buckets): every 8 data bytes travel as one
// 16-byte line {data lo, flag, data hi, flag} written with two 8-byte
// system-scope stores, flag = 1 + seq mod (2^32 - 1) (never 0, so a zeroed
// line is never valid); a receiver polls the lines
// themselves, so the hand-off needs no drain, no count atomic and no
// separate flag round trip.  Its region is written only with such lines
// (zero at init), so a line left from an earlier launch carries a smaller
// seq; its slots alternate by parity like the one-shot's (same argument).
// Hand-offs are element counts: a sender adds the elements it wrote into a
// rank's slot to that rank's IN_CNT line (one remote atomic per workgroup and
// target, after its stores drained), an owner adds the elements it broadcast
// to every peer's OUT_CNT line.  Counts only grow; the receiver keeps running
// totals of what it has been sent so far (E_IN, E_OUT) and waits for
// total + this launch's share.  Launch seq s (1, 2, ...) and the totals are
// advanced in the control block by the last workgroup of a launch to arrive
// (after every workgroup read them), so graph replays keep counting.
// Reuse across back-to-back launches:
//   two-shot slots: a rank's in slots are refilled (phase 1 of launch s+1,
//     which waits for nothing) only by a peer that finished launch s, which
//     needed this rank's broadcast of s (or this rank owned nothing and read
//     no in slot); its out slot is refilled only by an owner that counted this
//     rank's scatter of s+1, made after this rank finished launch s;
//   one-shot slots alternate by parity s & 1: a peer writes parity p in
//     launch s+2 only after finishing s+1, which needed this rank's writes of
//     s+1, made after this rank finished reading parity p in launch s.
// Both hold across any mix of variants (and AllGather): a peer cannot finish
// a launch without a hand-off this rank makes in that same launch (with
// count >= 1 some rank owns elements, and whoever it is waits, directly or
// through its broadcast, for this rank's phase-1 count).
//
// Direct ReduceScatter (direct_rs.h, opt-in: mccsCommSetReduceScatterDirect)
// uses the same region and state and adds no slot: sender s writes block t of
// its input only into t's region, at the element offset within the block --
//   count-based: the one-shot slot [parity seq & 1][sender s] (a block of at
//     most oslot_bytes), then one add of recvcount to t's IN_CNT(s);
//   LL: line w of the LL slot [parity][sender s] for the block's 8-byte word
//     w (a block of at most ll_slot_bytes / 2), flagged like every LL line.
// E_IN advances by recvcount per count-based launch: every sender sends every
// receiver exactly one block, so the single word stays the running total of
// every sender's line across any mix with one-shot / two-shot AllReduce and
// AllGather launches (each of which also adds one common amount per sender).
// Parity reuse is the one-shot's argument, and here it needs no case split:
// with recvcount >= 1 EVERY ordered pair (s, t) hands off in EVERY launch (t
// waits for s's count, or polls line 0 of s's slot), so s cannot finish
// launch L+1 -- and start writing parity p again in L+2 -- before t made its
// own writes of L+1; and a rank's launch L+1 starts only after its launch L
// ended (stream order between eager launches, the launch guard between graph
// replays), i.e. after it finished reading parity p.
//
// Direct Broadcast and Reduce (direct_rooted.h, opt-in:
// mccsCommSetRootedDirect) use the same region and state and add no slot:
//   Reduce: sender s != root writes its input into the root's one-shot slot
//     [parity][sender s] at the element offset, or word w into line w of the
//     root's LL slot [parity][sender s]; the root folds as a direct
//     ReduceScatter owner folds its block (the whole buffer is the block);
//   Broadcast: the root writes its bytes into every peer t's one-shot slot
//     [parity][root], or word w into line w of t's LL slot [parity][root].
// Data moves on n-1 of the n(n-1) ordered pairs only, and that alone would
// break both facts the argument above rests on: the pairs without data would
// not hand off (after a Reduce to root 0 and a Reduce to root 1 nothing would
// stop rank 2 from overwriting a slot rank 0 is still reading), and senders
// would have sent a receiver different amounts (the single E_IN word would no
// longer be every line's running total).  So a rooted launch keeps both facts
// by rule.  With the launch's common amount A (count elements for Reduce,
// nbytes for Broadcast):
//   count-based: EVERY rank adds A to IN_CNT(self) of EVERY peer -- summed
//     over its workgroups' pieces where the pair carries data, by one add of
//     workgroup 0 where it carries none; E_IN advances by A on EVERY rank; and
//     on EVERY rank, root or not, workgroup 0 waits for E_IN + A on every
//     peer's line before the kernel ends;
//   LL: EVERY rank writes line 0, flagged with this launch's seq, into EVERY
//     peer's LL slot for itself (a dummy word where the pair carries no
//     data), and on EVERY rank global thread 0 polls line 0 of every peer's
//     slot before the kernel ends.
// Then every ordered pair (s, t) hands off in every launch and every sender
// sends every receiver the same amount, and the ReduceScatter paragraph holds
// word for word: s cannot finish launch L+1 -- and start writing parity p
// again in L+2 -- before t made its hand-off of L+1, which t makes only after
// its launch L ended, i.e. after it finished reading parity p; and E_IN stays
// the running total of every line.  This holds across any mix of rooted,
// ReduceScatter, AllReduce, AllGather and all-to-all direct launches, and
// under every change of root between launches: the rule does not mention the
// root.
//
// Wide direct AllReduce (direct_wide.h, opt-in: mccsCommSetAllReduceWide; fp16
// and bf16, Sum and PreMulSum) uses the same region and state and adds no
// slot.  Only its arithmetic (binary32 accumulation in rank order, one
// rounding) and its cut differ from the AllReduce variants above; every
// hand-off is one of theirs with the same per-sender amounts:
//   wide LL: the LL one-shot's lines word for word (every rank writes every
//     word into every peer's LL slot [parity][sender]; LAUNCHES alone moves);
//   wide one-shot: the one-shot's -- every sender adds the whole count to
//     every peer's IN_CNT, E_IN += count, E_SELF += count in place;
//   wide two-shot: the two-shot's with owned[t] = rank t's contiguous share
//     (MCCS_WIDE_SHARE; 0 for trailing ranks of a small count) instead of the
//     walk's chunks -- sender s adds owned[t] to t's IN_CNT(s), owner o adds
//     owned[o] to every peer's OUT_CNT(o), E_IN += owned[self],
//     E_OUT[t] += owned[t].
// So the reuse paragraphs above hold word for word across any mix of wide and
// other direct launches: nothing in them depends on how owned[] cuts the
// buffer, only on "a peer cannot finish a launch without a hand-off this rank
// makes in that same launch", which count >= 1 gives (rank 0 always owns
// elements, and it waits, directly or through its broadcast, for every rank's
// phase-1 count; a rank that owns nothing reads no in slot).
//
// Wide direct ReduceScatter and Reduce (direct_wide_rs.h, opt-in:
// mccsCommSetReduceScatterWide / mccsCommSetReduceWide; fp16 and bf16, Sum and
// PreMulSum) use the same region and state and add no slot.  Only the
// arithmetic (binary32 in rank order, one rounding) and the absence of a walk
// differ from the ring-order kernels; every hand-off is one of theirs with the
// same per-sender amounts:
//   wide RS one-shot: the direct ReduceScatter's count-based hand-off --
//     sender s writes block t into t's one-shot slot [parity][s] and adds
//     recvcount to t's IN_CNT(s); E_IN += recvcount on every rank;
//   wide RS LL: the direct ReduceScatter's lines -- word w of block t into
//     line w of t's LL slot [parity][s]; LAUNCHES alone moves;
//   wide RD one-shot: the direct Reduce's under THE RULE above, word for word
//     -- every rank adds count to IN_CNT(self) of every peer (over its pieces
//     towards the root, by one add of workgroup 0 elsewhere), E_IN += count on
//     every rank, and workgroup 0 of every rank waits for every peer's line;
//   wide RD LL: the direct Reduce's lines under the rule -- every rank writes a
//     flagged line 0 into every peer's slot (a dummy word where the pair
//     carries no data) and global thread 0 of every rank polls line 0 of every
//     peer's slot.
// So with count >= 1 every ordered pair hands off in every such launch with
// one common amount per sender, which is all the ReduceScatter and rooted
// paragraphs above rest on: parity reuse and the single E_IN word hold across
// any mix of these with every other direct launch and under every change of
// root.
//
// Wide streamed ReduceScatter (direct_wide_stream.h, opt-in:
// mccsCommSetReduceScatterWideStream; fp16 and bf16, Sum and PreMulSum) moves a
// block of ANY size through the same one-shot slots and adds none.  A launch
// runs K = ceil(recvcount / B) rounds, B = round_elems (a multiple of 8 that
// fits one slot).  Round k has the sequence number seq0 + k (seq0 = LAUNCHES +
// 1) and is, on the wire, one wide one-shot ReduceScatter of the elements
// [k B, min((k+1) B, recvcount)) of every block: sender s writes them into t's
// slot [parity (seq0 + k) & 1][s] at the offset within the round, and t's
// IN_CNT(s) grows by the round's count.  The launch ends with LAUNCHES += K and E_IN
// += recvcount (every sender added every round's count on every owner, so the
// single word stays every line's running total); E_OUT and E_SELF stay.  With
// K = 1 that is the wide RS one-shot's state word for word.  A workgroup runs
// send(0); for k = 1 .. K: { send(k) if k < K; fold(k-1) }, so round k's bytes
// are in flight while round k-1 is folded -- and a launch now crosses its own
// parities, which the launch-boundary argument above does not cover.  Three new
// kinds of line in the control block (zero at init with it) close the gap:
//   SEND_DONE(q), q = round seq & 3: u32, this rank's workgroups that finished
//     sending that round.  IN_CNT is one running total per sender, and the
//     workgroups of one rank may be a round apart; if each added its own pieces
//     (as direct_count_out does in the one-launch kernels, whose count is one
//     total per launch), elements one workgroup counted for round k would stand
//     in for elements a slower one has not yet written for round k-1.  So a
//     round's count is INDIVISIBLE: EVERY workgroup, with or without pieces in
//     the round, drains its stores (cached arenas: and writes them back, as
//     direct_count_out) and arrives; the last to arrive puts the word back to
//     0, adds the round's WHOLE length to IN_CNT(s) of every owner, and drains.
//     Its add follows every workgroup's drained stores of round k, and the
//     same holds for the adds of rounds < k, each made before some workgroup
//     could arrive at round k.  Hence IN_CNT(s) >= E_IN + k B + len_k at t
//     means ALL of rounds 0 .. k from s are in t's slots.
//   ROUND_DONE(q), q = round seq & 3: u32, this rank's workgroups that finished
//     folding that round.  EVERY workgroup, with or without pieces in the
//     round, waits for the round's in-count, folds its pieces, drains its loads
//     and arrives; the last to arrive puts the word back to 0 and
//   ACK(t): u64 in every peer's block, written only by rank t -- stores the
//     round's seq there and drains.  Rounds 0 .. K-2 are acknowledged; nobody
//     waits for an ack of round K-1.  The value only grows (LAUNCHES only
//     grows; the last arriver of round k+1 arrives after the last arriver of
//     round k drained its stores), so a value left by an earlier streamed
//     launch never satisfies a later wait.
// The three hazards:
//   1. within a launch: s writes round k+2 into the parity of round k only
//      after it polled ACK(t) >= seq0 + k on its own block for every peer t,
//      i.e. after EVERY workgroup of t finished reading round k.  (t's
//      in-count of round k+1 would not show that: workgroups send ahead of
//      folding.)  Every workgroup polls before every round k >= 2, whether or
//      not it holds a piece of it.
//   2. against the previous launch L-1 of any kind, which used round 1's
//      parity: before round 1 every workgroup of s waits for the in-count of
//      round 0 from every peer t, which t adds only inside its launch L, i.e.
//      after its launch L-1 ended.  Round 0's parity is launch L-2's and the
//      one-shot argument covers it (s finished L-1, which needed t's hand-off
//      of L-1, made after t finished L-2).
//   3. against the next launch of any kind, whose first write goes to the
//      parity of round K-2: with K >= 2 every workgroup polls ACK(t) >= seq0 +
//      K-2 for every peer before the kernel ends, so every peer finished
//      reading that parity.  The parity of round K-1 is written next in the
//      launch after, and the one-shot argument holds for it: every ordered pair
//      hands off in the next launch, which t enters only after this one ended.
// Four ROUND_DONE words suffice: a workgroup arrives at round k only after the
// in-count of round k, which the peers add only after this rank's ack of round
// k-2, i.e. after every workgroup of this rank arrived at round k-2; so at most
// rounds k-1, k, k+1 are counted at once, and round k+4 finds the word its
// last arriver of round k put back to 0 and drained.  Four SEND_DONE words
// suffice likewise: a workgroup sends round k >= 2 only after every peer's ack
// of round k-2, which a peer gives after folding it, i.e. after this rank's
// count of round k-2, i.e. after every workgroup of this rank arrived there.
// No workgroup waits for a workgroup of its own rank (arriving on SEND_DONE or
// ROUND_DONE is an add, not a wait), and the waits form no cycle: round j
// completes (every workgroup of every rank folded it and arrived) given the
// counts of round j, i.e. every workgroup of every rank reaching the end of
// send(j), which needs its fold of round j-2 and the acks of round j-2 (and,
// j = 1, the in-counts of round 0), and given that every workgroup passed
// send(j+1), which needs the acks of round j-1; both are completions of earlier
// rounds, so induction on j from rounds 0 and 1 (which wait for no ack) ends.
// Every wait is direct_wait: it polls the abort flag and the watchdog and
// returns on either.
// The block-scaled FP8 streamed ReduceScatter (direct_quant_stream.h, opt-in:
// mccsCommSetReduceScatterQuant; mode MCCS_DIRECT_QUANT_RS_STREAM) is this
// launch with other bytes inside the slots, and runs the same round loop
// (direct_stream_body): the counts stay in ELEMENTS, the lines, the three
// hazard waits and the state words are the ones above, so the argument holds
// word for word.  Only the slot layout differs: slot [parity][sender] is split
// as the FP8 AllReduce splits a two-shot slot (MCCS_QUANT_PAY below, of
// oslot_bytes): the code of round element e at byte e, the scale byte of the
// round's block k at PAY_O + k.  B is a multiple of 512 of at most PAY_O, so a
// round is a whole number of units on the slot side, a sender writes only
// bytes of its own slot and only below PAY_O + B / 32 <= oslot_bytes, and a
// reader that saw the round's count reads only bytes that round's senders
// wrote (the padding of a tail unit included: it is written as +0 codes).
// The block-scaled FP8 streamed AllGather (direct_quant_ag.h, the explicit call
// mccsAllGatherQuant; mode MCCS_DIRECT_QUANT_AG_STREAM) uses these slots, lines,
// counts, waits and state words with the data moving the other way: sender s
// writes round k of its OWN block, once quantised, into slot [parity][s] of
// every peer, and a reader dequantises the n-1 slots of one parity into n-1
// output blocks.  The no-cycle argument carries over because it never looked at
// what the bytes are, only at who counts and who reads: every sender still adds
// the same length len_k to IN_CNT(s) of EVERY peer, after every one of its
// workgroups drained its stores of the round, so IN_CNT(s) >= E_IN + k B + len_k
// at t still means all of rounds 0 .. k from s are in t's slots; and a reader
// still reads exactly the n-1 slots of ONE parity per round and acknowledges
// rounds 0 .. K-2 once every one of its workgroups has read them, so hazards 1
// to 3 and the bound of four SEND_DONE / ROUND_DONE words read as above with
// "copy" for "fold".  The own block never enters a slot: a thread loads its 8
// elements, and the same thread stores their QDQ to the output, so in place
// needs no self wait.  The launch leaves LAUNCHES += K, E_IN += count, E_OUT
// and E_SELF untouched, as the streamed ReduceScatter does.
//
// Wide streamed AllReduce (direct_wide_stream_ar.h, opt-in:
// mccsCommSetAllReduceWideStream; fp16 and bf16, Sum and PreMulSum) runs
// scatter -> wide fold -> gather in rounds inside one launch, for a buffer of
// ANY size, and adds no slot.  The split is the wide two-shot's (rank t owns
// owned[t] elements from t q, q = MCCS_WIDE_SHARE), the planner streams only a
// count > 8 n (n-1), which gives every rank an element, and a launch runs K =
// ceil(q / B) rounds, B = round_elems; round k has the sequence number seq0 + k
// (seq0 = LAUNCHES + 1), parity (seq0 + k) & 1, and covers len_k(t) = min(B,
// owned[t] - k B) elements of share t, 0 once the short last share is exhausted.
// Two kinds of buffer, each with two parities:
//   scatter slots: the one-shot in slots, as the streamed ReduceScatter uses
//     them -- sender s writes round k of share t into t's slot [parity][s];
//   gather buffers: the two halves (floor16(slot_bytes / 2) each) of the
//     two-shot IN slots, which a streamed launch otherwise leaves idle -- owner
//     o writes round k's results into t's in slot [o], half [parity].
// A workgroup runs, for step i = 0 .. K+1: send(i) if i < K; fold(i-1) if 1 <=
// i <= K; copy(i-2) if i >= 2.  Counts and acknowledgements:
//   IN_CNT / SEND_DONE(q): as in the streamed ReduceScatter, a round's count is
//     indivisible; the last workgroup to arrive after send(k) adds len_k(t) to
//     IN_CNT(s) of every owner t.  Owner t starts fold(k) at E_IN + min(owned[t],
//     (k+1) B) on every peer's line.  Over the launch every sender adds owned[t]
//     on t: the wide two-shot's amount, E_IN += owned[self].
//   OUT_CNT / FOLD_DONE(q), q = round seq & 3: the same for the gather leg, the
//     new word: EVERY workgroup drains its stores of fold(k) (cached arenas: and
//     writes them back) and arrives, with or without pieces; the last puts the
//     word back to 0 and adds len_k(o) to OUT_CNT(o) of every peer.  copy(k)
//     starts at E_OUT[o] + min(owned[o], (k+1) B) on every owner o's line, which
//     therefore proves ALL of rounds 0 .. k from o.  E_OUT[t] += owned[t].
//   ACK / ROUND_DONE(q): ONE acknowledgement per step.  At the end of step i >=
//     1 every workgroup drains its loads and arrives on ROUND_DONE((seq0 + i-1)
//     & 3); the last stores seq0 + i-1 into ACK(me) of every peer and drains.
//     The value says: every workgroup of this rank finished step i, i.e.
//     finished reading the scatter slots of round i-1 (fold) AND the gather
//     buffers of round i-2 (copy).  Every workgroup polls every peer's ACK >=
//     seq0 + i-2 at the top of step 2 <= i <= K, and ACK >= seq0 + K before the
//     kernel ends.  The launch leaves LAUNCHES += K + 1: the drain step K+1 has
//     a number of its own, so every ACK value of a launch is below every value
//     the next streamed launch of either kind waits for.
// Hazards within a launch.  send(i) rewrites the scatter parity of round i-2;
// fold(i-1) rewrites the gather parity of round i-3.  Both run in step i after
// the wait for ACK >= seq0 + i-2 from every peer t, i.e. after every workgroup
// of t finished step i-1: fold(i-2) and copy(i-3).  The one wait covers both
// rewrites, and it stands before fold(K-1) in step K too, which has no send.
// Steps 0 and 1 rewrite nothing of this launch.
// Against the previous launch L-1 of any kind.  send(0) writes the scatter
// parity launch L-1 did NOT use (that of seq0 - 2): the one-shot argument above
// covers it (s finished L-1, which needed t's hand-off of L-1, made after t
// finished reading in L-2; where seq0 - 2 was a round of a streamed launch,
// that launch's closing ACK wait covers it).  send(1) writes the parity of seq0
// - 1, which a peer may still be reading in L-1, and fold(0) writes gather
// buffers, i.e. two-shot in slots a peer may still be folding from in a
// two-shot L-1: both come after the wait for round 0's in-count from EVERY peer
// t (taken once, at the top of step 1), which t adds only inside its launch L,
// after its L-1 ended.  That is a hand-off only if t adds something: len_0(me)
// >= 1 on every rank, which is the planner's owned[n-1] >= 1.
// Against the next launch of any kind.  The kernel ends on s only after ACK >=
// seq0 + K from every peer t: every workgroup of t finished step K+1, so t has
// read every scatter slot and every gather buffer of the launch.  The next
// launch may refill one-shot slots of either parity and two-shot in slots (which
// have no parity of their own in the two-shot kernels) at once; the two-shot out
// slot is not touched here.  Conversely t's counts of the next launch cannot
// reach s early: t is in the next launch only after s's last workgroup finished
// step K+1.
// Four words per arrival kind suffice.  Passing the top of step j (3 <= j <= K)
// needs every peer's ACK of step j-1, hence a peer's copy(j-3), hence this
// rank's out-count of round j-3, hence EVERY workgroup of this rank past
// fold(j-3), which lies in step j-2: all of them finished step j-3, and the
// last arriver there put its word back and drained before it went on.  A
// workgroup that arrives for step i+4 (ROUND_DONE), round k+4 (SEND_DONE, in
// step k+4; FOLD_DONE, in step k+5) has passed the top of step min(i+4, K) >=
// i+3, resp. k+4, resp. k+5 <= K, so every workgroup finished step i, resp.
// k+1, resp. k+2: the earlier use of the word is over and the word is 0.
// No workgroup waits on its own rank (arrivals are adds, never waits), and the
// waits form no cycle: every wait of step i is for something the peers do in a
// step below i -- ACK >= seq0 + i-2 is their step i-1; round 0's and round
// i-1's in-counts are their send in steps 0 and i-1; round i-2's out-count is
// their fold in step i-1 -- so by induction on i every workgroup of every rank
// finishes every step, and the closing wait needs only step K+1.  A rank whose
// share is exhausted (len_k = 0) still waits, arrives and acknowledges.
// In place (recv == send).  fold(k) loads and stores each element of the own
// share through one thread, and no send reads the own share.  copy(k) stores
// into foreign shares' round k, which only send(k) reads: send and copy deal
// their pieces through ONE function with equal counters (numbered through all
// rounds, piece p to workgroup p % G), so the workgroup that stores a range in
// copy(k), step k+2, is the one that read it in send(k), step k, and has long
// drained those loads (its arrival on SEND_DONE).  A slower workgroup of the
// same rank sends other ranges.
// Every wait is direct_wait: it polls the abort flag and the watchdog and
// returns on either.
// The block-scaled FP8 streamed AllReduce (direct_quant_stream_ar.h, opt-in:
// mccsCommSetAllReduceQuantStream; mode MCCS_DIRECT_QUANT_AR_STREAM) is this
// launch with other bytes inside the buffers, and runs the same round loop
// (direct_stream_ar_body): the counts stay in ELEMENTS, the lines, the one ACK
// wait per step, the round-0 hand-off, the closing wait and the state words are
// the ones above, so the argument holds word for word, with q and owned[] from
// MCCS_QUANT_SHARE (multiples of 512 elements).  Only the layout differs, and
// it is one layout for both kinds of buffer, the FP8 AllReduce's split of a
// two-shot slot (MCCS_QUANT_PAY below): a scatter slot [parity][sender] has
// PAY_O = MCCS_QUANT_PAY(oslot_bytes) code bytes, a gather buffer (the half
// [parity] of the in slot [owner], floor16(slot_bytes / 2) bytes) has PAY_H =
// MCCS_QUANT_PAY(half); the code of round element e lies at byte e, the scale
// byte of the round's block k at PAY + k.  B is a multiple of 512 of at most
// min(PAY_O, PAY_H) and pieces are whole units, so a round is a whole number of
// units on the slot side: a sender writes only bytes of its own scatter slot
// and only below PAY_O + B / 32 <= oslot_bytes, an owner only bytes of its own
// half of each peer's in slot [owner] and only below PAY_H + B / 32 <= half (so
// never into the other parity's half or the next slot), and a reader that saw
// a round's in-count or out-count reads only the units of len_k, all of which
// that round's writers wrote, codes and scale row alike (the padding of a tail
// unit included: it is written as zero codes of either sign, which neither
// move a block's scale nor are stored to recv).  The round-0 hand-off needs every
// rank to add something to every owner's line, i.e. owned[n-1] >= 1 under
// MCCS_QUANT_SHARE: (n-1) q < count, which is 512 times coarser than the 16-bit
// split's condition; the planner tests it and streams nothing else.  In place:
// send(k) and copy(k) deal pieces through the one function and split a piece
// into units alike (unit u to wave u mod waves, lane l its 8 elements), so the
// lane that stores an element in copy(k) is the one that loaded it in send(k).
//
// Block-scaled FP8 AllReduce (direct_quant.h, opt-in: mccsCommSetAllReduceQuant;
// fp16 and bf16, Sum and PreMulSum) uses the two-shot slots, counts and state
// and adds no slot; only the bytes inside a slot differ (MCCS_QUANT_PAY below).
// Its hand-offs are the wide two-shot's with owned[t] = rank t's share by
// MCCS_QUANT_SHARE (multiples of 512 elements; trailing ranks may own nothing):
// sender s adds owned[t] ELEMENTS to t's IN_CNT(s), owner o adds owned[o] to
// every peer's OUT_CNT(o), E_IN += owned[self], E_OUT[t] += owned[t], LAUNCHES
// += 1.  So the reuse paragraphs and the parity of the one-shot and LL slots
// hold across any mix with the other direct launches, by the wide two-shot's
// argument: count >= 1 makes rank 0 an owner, every rank hands rank 0 its part
// of that share inside the launch, and a rank that owns nothing reads no in
// slot and writes no out slot.
// In place (recv == send).  Phase 2 loads and stores each element of the own
// share through one lane, and phase 1 never reads the own share.  Phase 3
// stores into foreign shares, which only phase 1 reads: both phases deal their
// pieces through one function with the same numbering (piece p to workgroup p
// mod G, unit u of a piece to wave u mod waves), so the wave that stores a unit
// in phase 3 is the one that loaded it in phase 1, two count-outs (each a drain
// and a barrier) earlier.  That is direct_body's argument, with units for packs.
#define MCCS_DIRECT_MAX_RANKS 8
#define MCCS_DIRECT_CTRL_BYTES 65536
// u64, added to by sender s; a rank's own line IN_CNT(rank) counts its own
// workgroups' reads of an in-place one-shot input (nobody else writes it)
#define MCCS_DIRECT_IN_CNT(s) ((s) * MCCS_FLAG_LINE_BYTES)
#define MCCS_DIRECT_OUT_CNT(o) (1024 + (o) * MCCS_FLAG_LINE_BYTES)     // u64, added to by owner o
// u64 state words (one line, read by one wave load): launches completed,
// E_IN (elements each sender has sent so far), E_OUT[o] (elements owner o
// has broadcast so far)
#define MCCS_DIRECT_STATE 2048
#define MCCS_DIRECT_ST_LAUNCHES 0
#define MCCS_DIRECT_ST_E_IN 1
#define MCCS_DIRECT_ST_E_OUT(o) (2 + (o))
#define MCCS_DIRECT_ST_E_SELF (2 + MCCS_DIRECT_MAX_RANKS)  // elements this rank counted to itself (in-place one-shot)
#define MCCS_DIRECT_ST_WORDS (3 + MCCS_DIRECT_MAX_RANKS)
#define MCCS_DIRECT_DONE 4096                                          // u32: workgroups arrived in the launch
// wide streamed ReduceScatter (above): u64, the latest round seq rank t acknowledged to this rank; u32, this
// rank's workgroups that finished folding the round of seq & 3
#define MCCS_DIRECT_ACK(t) (8192 + (t) * MCCS_FLAG_LINE_BYTES)
#define MCCS_DIRECT_ROUND_DONE(q) (12288 + (q) * MCCS_FLAG_LINE_BYTES)
// u32, this rank's workgroups that finished sending the round of seq & 3 (the last one adds the round's count)
#define MCCS_DIRECT_SEND_DONE(q) (16384 + (q) * MCCS_FLAG_LINE_BYTES)
// wide streamed AllReduce (above): u32, this rank's workgroups that finished folding the round of seq & 3 (the last
// one adds the round's count to OUT_CNT); its ACK / ROUND_DONE / SEND_DONE are the lines above, one step per value
#define MCCS_DIRECT_FOLD_DONE(q) (20480 + (q) * MCCS_FLAG_LINE_BYTES)
#define MCCS_DIRECT_SLOTS (MCCS_DIRECT_MAX_RANKS + 1)                  // two-shot slots
#define MCCS_DIRECT_THREADS 512
#define MCCS_DIRECT_TWO_SHOT 0
#define MCCS_DIRECT_ONE_SHOT 1
#define MCCS_DIRECT_AG_ONE_SHOT 2  // AllGather: count = bytes per rank (dtype int8)
#define MCCS_DIRECT_LL_ONE_SHOT 3  // one-shot through flag-carrying 16-byte lines (uncached arenas)
#define MCCS_DIRECT_LL_AG 4        // AllGather through the same lines (count = bytes per rank)
// direct ReduceScatter (direct_rs.h; count = recvcount, the elements of one block)
#define MCCS_DIRECT_RS_ONE_SHOT 5  // through the one-shot slots, counted on IN_CNT
#define MCCS_DIRECT_RS_LL 6        // through the LL lines
// direct Reduce and Broadcast (direct_rooted.h; count = the buffer's elements / bytes, root = the root)
#define MCCS_DIRECT_RD_ONE_SHOT 7  // Reduce through the root's one-shot slots, counted on IN_CNT
#define MCCS_DIRECT_RD_LL 8        // Reduce through the root's LL lines
#define MCCS_DIRECT_BC_ONE_SHOT 9  // Broadcast through every peer's one-shot slot for the root
#define MCCS_DIRECT_BC_LL 10       // Broadcast through every peer's LL lines for the root
// wide-accumulate AllReduce (direct_wide.h; fp16 / bf16, op_arg = the PreMulSum scalar)
#define MCCS_DIRECT_WIDE_LL 11        // through the LL lines
#define MCCS_DIRECT_WIDE_ONE_SHOT 12  // through the one-shot slots, counted on IN_CNT
#define MCCS_DIRECT_WIDE_TWO_SHOT 13  // through the two-shot slots, contiguous shares
// elements of one rank's share of a wide two-shot: ceil(count / n) rounded up
// to 8, so every share starts on a 16-byte pack of 2-byte elements
#define MCCS_WIDE_SHARE(count, n) ((((count) + (n) - 1) / (n) + 7) & ~(uint64_t)7)
// wide-accumulate ReduceScatter and Reduce (direct_wide_rs.h; count / root as RS / RD above, op_arg as WIDE)
#define MCCS_DIRECT_WIDE_RS_LL 14        // ReduceScatter through the LL lines
#define MCCS_DIRECT_WIDE_RS_ONE_SHOT 15  // ReduceScatter through the one-shot slots, counted on IN_CNT
#define MCCS_DIRECT_WIDE_RD_LL 16        // Reduce through the root's LL lines
#define MCCS_DIRECT_WIDE_RD_ONE_SHOT 17  // Reduce through the root's one-shot slots, counted on IN_CNT
// wide streamed ReduceScatter (direct_wide_stream.h; count = recvcount of any size, rounds x round_elems)
#define MCCS_DIRECT_WIDE_RS_STREAM 18    // rounds through the one-shot slots, counted on IN_CNT, acknowledged on ACK
// wide streamed AllReduce (direct_wide_stream_ar.h; count of any size, owned[] the two-shot's split, rounds x round_elems)
#define MCCS_DIRECT_WIDE_AR_STREAM 19    // scatter through the one-shot slots, gather through the halves of the two-shot in slots
// block-scaled FP8 AllReduce (direct_quant.h; fp16 / bf16, op_arg as WIDE, owned[] = the split by MCCS_QUANT_SHARE)
#define MCCS_DIRECT_QUANT_TWO_SHOT 20  // through the two-shot slots: E4M3 codes and one E8M0 byte per 32 elements
// Its wire layout.  Every two-shot slot it uses (the in slot per sender, the out
// slot) is split in two: a payload of PAY bytes, the code of element e at byte
// e, and behind it the scale region, the byte of block k (elements [32k, 32k +
// 32) of the buffer) at PAY + k.  PAY = slot_bytes x 32 / 33 cut down to a
// multiple of 512, so PAY + PAY / 32 <= slot_bytes; count <= PAY.  A wave moves
// units of 512 elements (512 payload bytes + 16 scale bytes, always whole on
// the slot side), so shares start on multiples of 512 elements.
// block-scaled FP8 streamed ReduceScatter (direct_quant_stream.h; count = recvcount of any size, rounds x round_elems)
#define MCCS_DIRECT_QUANT_RS_STREAM 21  // WIDE_RS_STREAM's rounds and lines; the one-shot slots split as above, PAY of oslot_bytes
// block-scaled FP8 streamed AllReduce (direct_quant_stream_ar.h; count of any size, owned[] the split by MCCS_QUANT_SHARE, rounds x round_elems)
#define MCCS_DIRECT_QUANT_AR_STREAM 22  // WIDE_AR_STREAM's rounds and lines; scatter slots and gather halves split as above
// block-scaled FP8 streamed AllGather (direct_quant_ag.h; count = sendcount of any size, rounds x round_elems; no op)
#define MCCS_DIRECT_QUANT_AG_STREAM 23  // QUANT_RS_STREAM's rounds, lines and slot split; every sender's own block to every peer
#define MCCS_QUANT_UNIT 512
#define MCCS_QUANT_PAY(slot_bytes) (((uint64_t)(slot_bytes) * 32 / 33) & ~(uint64_t)(MCCS_QUANT_UNIT - 1))
#define MCCS_QUANT_SHARE(count, n) \
  ((((count) + (n) - 1) / (n) + (MCCS_QUANT_UNIT - 1)) & ~(uint64_t)(MCCS_QUANT_UNIT - 1))

struct mccsDirectRank {  // one rank slot of a direct launch (blockIdx.y)
  const void* send;
  void* recv;
  struct mccsDevComm* comm;  // the rank's device communicator
  uint32_t* abort_flag;      // comm->abortFlag (one load less in the prologue)
  uint32_t rank;
  uint32_t err_line;
};
struct mccsDirectArgs {
  struct mccsDirectRank r[MCCS_MULTI_MAX_RANKS];
  // every rank's direct region as the launching process maps it: one table
  // for all rank slots (fused slots are ranks of one communicator in one
  // process, plan.cpp direct_group), so HIP copies 64 B per launch, not 1 KiB
  char* region[MCCS_DIRECT_MAX_RANKS];
  uint64_t count;          // elements
  uint64_t slot_bytes;     // bytes of one two-shot slot (>= count * element size for two-shot)
  uint64_t oslot_bytes;    // bytes of one one-shot slot (>= count * element size for one-shot)
  uint64_t ll_slot_bytes;  // bytes of one LL slot (>= 2 x count * element size, rounded to 8 bytes, for LL)
  uint64_t timeout_ticks;  // s_memrealtime ticks; 0 = never
  uint32_t nranks, nch, nthr_ref, buff_size;  // the ring walk this launch reproduces
  uint32_t fence_mode;                        // MCCS_FENCE_*
  uint32_t mode;                              // MCCS_DIRECT_* above (RS: direct_rs_kernel only; RD / BC: direct_rooted.h's kernels only; WIDE: direct_wide_kernel only; WIDE_RS / WIDE_RD: direct_wide_rs.h's kernels only; WIDE_RS_STREAM: direct_wide_stream_kernel only; WIDE_AR_STREAM: direct_wide_stream_ar_kernel only; QUANT: direct_quant_kernel only; QUANT_RS_STREAM: direct_quant_stream_kernel only; QUANT_AR_STREAM: direct_quant_stream_ar_kernel only; QUANT_AG_STREAM: direct_quant_ag_kernel only)
  uint32_t piece;                             // elements per piece of the scatter / gather phases
  uint32_t piece2;                            // elements per piece of the reduction phase
  uint32_t no_guard;                          // 1: skip the launch guard (test hook only)
  uint32_t root;                              // the RD / BC / WIDE_RD modes: the root (one for all rank slots); else 0
  uint64_t guard_order;                       // rank slots by guard address, 4 bits each (launch_guard.h)
  uint64_t owned[MCCS_DIRECT_MAX_RANKS];      // elements of the walk's chunks each rank owns (wide two-shot, WIDE_AR_STREAM, QUANT and QUANT_AR_STREAM: of its share)
  uint8_t idx2rank[MCCS_MAX_NCHANNELS][MCCS_DIRECT_MAX_RANKS];  // rank at ring index k of channel bid
  uint64_t op_arg;  // the wide modes: the PreMulSum scalar (T in the low bits); else 0 (the fields above keep their place)
  uint64_t rounds;       // WIDE_RS_STREAM, QUANT_RS_STREAM, QUANT_AG_STREAM: K = ceil(count / round_elems) >= 1; WIDE_AR_STREAM, QUANT_AR_STREAM: ceil(share / round_elems); else 0
  uint32_t round_elems;  // the STREAM modes: elements of one round (a multiple of 8, at most one one-shot slot; AR: and half a two-shot slot; QUANT_RS_STREAM, QUANT_AG_STREAM: a multiple of 512, at most MCCS_QUANT_PAY(oslot_bytes); QUANT_AR_STREAM: and at most MCCS_QUANT_PAY of half a two-shot slot); else 0
  uint32_t pad4;
};
#ifdef __cplusplus
static_assert(sizeof(mccsDirectArgs) <= 4096, "direct launch arguments must stay within 4 KiB");
#endif

// ---- LL AllToAll / AllToAllv / AllToAllvDev (direct_a2a.h) -------------------
// The three all-to-all calls at small sizes, through the LL slots above and
// under the same launch count and parity as the LL AllReduce / AllGather.
// Nothing fans out: sender s writes the block for receiver t only into t's
// region, at llbase(parity) + s x ll_slot_bytes:
//   line 0      header {count lo32, flag, count hi32, flag}: the bytes s sends
//               t in this launch
//   line 1 + w  data word w of the block
// so a block of c bytes takes 16 x (1 + ceil(c / 8)) bytes and a pair moves at
// most MCCS_A2A_LL_CAP(ll_slot_bytes) bytes per launch.  The header goes out
// for EVERY ordered pair in EVERY launch, zero counts included, and every
// receiver waits for every peer's: the parity-reuse argument above needs every
// pair to hand off in every launch (without it a pair with a zero count would
// let the sender run two launches ahead and overwrite lines a slow receiver
// still polls for the older flag).  A receiver takes its length from its own
// count; the header's value is there for a later size check.
#define MCCS_A2A_LL_CAP(ll_slot_bytes) ((ll_slot_bytes) >= 32 ? (ll_slot_bytes) / 2 - 8 : 0)
#define MCCS_A2A_LL_ROWS 4  // ring_walk.h kA2AvdRows: sendcounts, sdispls, recvcounts, rdispls
struct mccsA2aLLRank {      // one rank slot of an LL all-to-all launch (blockIdx.y)
  const void* send;
  void* recv;
  struct mccsDevComm* comm;
  uint32_t* abort_flag;
  uint32_t rank;
  uint32_t err_line;
  const uint64_t* table;  // table mode: the AllToAllvDev size table, re-read at every launch
  uint64_t rows[MCCS_A2A_LL_ROWS][MCCS_DIRECT_MAX_RANKS];  // host mode: the call's four rows, in bytes
};
struct mccsA2aLLArgs {
  // fused rank slots are ranks of one communicator (n <= 8) in one process
  struct mccsA2aLLRank r[MCCS_DIRECT_MAX_RANKS];
  char* region[MCCS_DIRECT_MAX_RANKS];  // as mccsDirectArgs.region
  uint64_t slot_bytes, oslot_bytes;     // the two-shot / one-shot slots the LL slots lie behind
  uint64_t ll_slot_bytes;
  uint64_t timeout_ticks;
  uint64_t guard_order;
  uint32_t nranks;
  uint32_t fence_mode;
  uint32_t table_mode;  // 1: sizes from r[k].table (clamped to the capacity on both sides), 0: r[k].rows
  uint32_t no_guard;
};
#ifdef __cplusplus
static_assert(sizeof(mccsA2aLLArgs) <= 4096, "LL all-to-all launch arguments must stay within 4 KiB");
#endif
