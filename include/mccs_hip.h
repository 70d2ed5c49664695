/*
 * mccs_hip.h — C-ABI of libmccs_hip.so, the MI355X-native mCCS allreduce path.
 *
 * Plain C: pointers, sizes, ints and opaque handles only (no torch, no HIP C++
 * types beyond the hipStream_t / hipEvent_t handles, which are pointers).
 * Each entry point names the reference interface it replaces.
 */
#ifndef MCCS_AMD_HIP_H_
#define MCCS_AMD_HIP_H_

#include <stddef.h>
#include <stdint.h>

#include "mccs_devcomm.h"

#ifdef __cplusplus
extern "C" {
#endif

/* hipStream_t is an opaque pointer in the HIP C API; the identical typedef in
 * hip_runtime_api.h is a compatible redeclaration (C11 / C++). */
typedef struct ihipStream_t *hipStream_t;

/* Result codes (NCCL/mCCS convention; the reference surfaces errors as
 * Result<(), Error> in libmccs and logs CUDA errors via cuda_warning!). */
typedef enum {
  mccsSuccess = 0,
  mccsUnhandledCudaError = 1, /* a HIP runtime call failed */
  mccsSystemError = 2,
  mccsInternalError = 3,
  mccsInvalidArgument = 4,
  mccsInvalidUsage = 5,
  mccsRemoteError = 6,
  mccsInProgress = 7,
  mccsTimeout = 8, /* a FIFO spin exceeded the watchdog; abortFlag raised */
  mccsNumResults = 9
} mccsResult_t;

/* ======================================================================
 * Device-resident chunk reduce (north-star kernel; BASELINE config 2).
 * Replaces the reduce/reduce-copy loop of the reference ring kernel,
 * ReduceOrCopyMulti (src/collectives/src/common_kernel.h:624-685), as a
 * standalone full-chip launch: y = src[0] (op) src[1] (op) ... in the element
 * type, written to every dst.  dst may alias src[0] (in-place a += b).
 * Tested (tests/test_gpu_footprint.py): any dst may be src[0] itself, also
 * among several dsts; no other overlap of buffers is supported; nothing
 * outside [dst, dst + count) is written, whatever the operands' alignment.
 * dtype: mccsDevDataType_t; op: mccsDevSum/Prod/Max/Min.
 * ====================================================================== */
#define MCCS_REDUCE_MAX_SRCS 8
#define MCCS_REDUCE_MAX_DSTS 4
#define MCCS_REDUCE_VARIANT_REG 1 /* register streaming main loop */
#define MCCS_REDUCE_VARIANT_LDS 2 /* LDS-DMA multi-stage staging main loop */
#define MCCS_REDUCE_VARIANT_REG_BLOCKED 3 /* REG with a contiguous run of tiles per block */
#define MCCS_REDUCE_VARIANT_REG_ROWS 4    /* REG with wave-contiguous 1 KiB rows */

mccsResult_t mccs_hip_reduce(void *dst, const void *const *srcs, int nsrcs, size_t count, int dtype,
                             int op, hipStream_t stream);
mccsResult_t mccs_hip_reduce_copy(void *const *dsts, int ndsts, const void *const *srcs, int nsrcs,
                                  size_t count, int dtype, int op, hipStream_t stream);
/* Select the main loop (0 = default), unroll = KiB per source per wave tile
 * for LDS / 16-byte packs per lane for REG (1/2/4/8, 0 = default), cache
 * policy (0 plain, 1 non-temporal, -1 default; REG: 2 nt loads + plain
 * stores, 3 plain loads + nt stores; LDS: 2 plain LDS-DMA + nt stores,
 * 3 nt + sc1 stores, 4 write-through sc1 stores (default), 5 sc0 sc1 nt),
 * persistent blocks per CU,
 * LDS ring stages (2..4) and waves per block (4/8); 0 = default for each.
 * Process-wide; for benchmarking and tests. */
mccsResult_t mccs_hip_reduce_tune(int variant, int unroll, int policy, int blocks_per_cu, int stages,
                                  int waves);
void mccs_hip_reduce_get_tune(int *variant, int *unroll, int *policy, int *blocks_per_cu, int *stages,
                              int *waves);
/* Caps the LDS main loop's grid at `blocks` workgroups (0 = blocks_per_cu x
 * CUs, the default).  Process-wide; for benchmarking. */
mccsResult_t mccs_hip_reduce_tune_grid(int blocks);

/* ======================================================================
 * Ring collectives: device kernels (reference src/collectives) and the
 * host runtime that plans and launches them (reference src/mccs/src/proxy,
 * comm, transport; src/libmccs).
 * ====================================================================== */

/* Host stub of the reference-named kernel mccsKernel_<Func>_RING_SIMPLE_<Op>_<T>
 * (collectives.h:43-49) for hipLaunchKernel: the value plan.rs:142-166 stores
 * in KernelPlan.kernel_fn.  func: mccsFuncAllReduce | mccsFuncAllGather.
 * op: for AllReduce any mccsDevRedOp_t; the mccsDevPreMulSum / mccsDevSumPostDiv
 * kernels (mccs_kernels_avg.h) take their scalar from each work element's
 * redOpArg, as the reference's do.  NULL for SumPostDiv on a floating dtype
 * (no such kernel), which mccs_hip_launch_coll refuses likewise. */
const void *mccs_hip_coll_kernel(int func, int dtype, int op);
/* plan.rs:638-669 launch_plan: hipLaunchKernel(fn, grid, block, {comm,
 * channelMask, workHead}, 0, stream).  grid = #channels * lanes; block =
 * 96..576 threads (one wave of it is the control wave).
 * One launch per rank, one rank per GPU (the reference deployment): ranks
 * that share a GPU spin on each other's FIFO flags, so their kernels must be
 * co-resident, which separate launches do not guarantee (two co-located ranks
 * launched one after the other deadlock until the watchdog fires).  While an
 * earlier launch of ANOTHER communicator on the current device, issued through
 * this function by this process, is still running, the call is refused with
 * mccsInvalidUsage and nothing is launched.  Co-located ranks go through the
 * communicator API (mccsCommInitAll + mccsGroupStart/End), which fuses them
 * into one launch.  The reference-named kernels run the reference FIFO depth
 * (MCCS_BUFFER_SLOTS = 8 slots per connection): a communicator of this library
 * built with another fifo_slots is refused with mccsInvalidUsage (its peers
 * would index a different slot ring). */
mccsResult_t mccs_hip_launch_coll(int func, int dtype, int op, struct mccsDevComm *comm, uint64_t channelMask,
                                  struct mccsDevWork *workHead, unsigned grid, unsigned block,
                                  hipStream_t stream);
/* Watchdog of the reference-named kernels on the current device: ms without
 * FIFO progress before a kernel raises abortFlag and returns; 0 = the default
 * (10 min), < 0 = none.  The reference kernels have none and the reference host
 * never reads abortFlag, so the default outlasts any late peer a deployment
 * sees (a watchdog that fired on one would silently end every later collective
 * of the communicator); tests lower it so a hang ends quickly.  Call it once
 * per device before the launches it should govern. */
mccsResult_t mccs_hip_set_ref_watchdog(int timeout_ms);

typedef struct mccsComm *mccsComm_t;

#define MCCS_LOCALITY_SENDER 0   /* FIFO data in the sender's HBM; receiver reads over xGMI */
#define MCCS_LOCALITY_RECEIVER 1 /* FIFO data in the receiver's HBM; sender writes over xGMI */
#define MCCS_FIFO_UNCACHED 0     /* hipDeviceMallocUncached arena: no L2 maintenance needed */
#define MCCS_FIFO_DEVICE 1       /* hipMalloc arena + system-scope release/acquire */
#define MCCS_FIFO_UNCACHED_RELEASE 2 /* uncached arena + a system-scope release fence before every
                                        post (the reference's __threadfence_system before postPeer,
                                        prims_simple.h:120-125,211); polls stay relaxed */

/* Communicator profile: comm_default_config (mccs.toml:18-20, config.rs:15-97)
 * plus the MI355X execution knobs.  Zero fields take defaults.
 * ABI note: `fifo_slots`, `direct_bytes` and `oneshot_bytes` were appended in
 * library version 0.3 and `ll_bytes` in 0.3.1, which grew the struct;
 * mccsCommConfigDefault() writes sizeof(mccsCommConfig) bytes, so a caller
 * compiled against an older header must be rebuilt.  From 0.4 the struct ends
 * in reserved words that later fields will take, so its size stays fixed;
 * callers binding the struct by hand (ctypes, bindgen) check
 * mccsCommConfigSize() or call mccsCommConfigDefaultSized(). */
typedef struct {
  int channel_count;    /* rings; 0 = auto: 2 x edge-disjoint Hamiltonian cycles of the node */
  int buffer_size;      /* FIFO bytes per connection (buffer_sizes[0]); 0 = 4 MiB */
  int lanes;            /* workgroups per channel; 0 = auto (64 / channels, <= 64, fitted to residency) */
  int block_threads;    /* threads per workgroup (96..576, multiple of 32); 0 = MCCS_RING_MAX_THREADS (576) */
  int locality;         /* MCCS_LOCALITY_*; default RECEIVER (remote writes; SENDER = reference shm layout) */
  int fifo_memory;      /* MCCS_FIFO_*; default UNCACHED (MCCS_FIFO_MEMORY=uncached|release|device) */
  int timeout_ms;       /* FIFO-wait watchdog: ms without progress before the kernel gives up (mccsTimeout);
                           0 = 600000 (10 min, torch's default collective timeout: a peer may arrive
                           minutes late, e.g. while rank 0 writes a checkpoint), < 0 = never;
                           MCCS_TIMEOUT_MS overrides the default */
  int work_fifo_depth;  /* mccsDevWork slots (power of two); 0 = 4096 */
  int bridge_streams;   /* -1 (default): launch on the caller's stream; 1: user stream -> comm stream -> user stream events (libmccs two-stream bridge) */
  const int *rings;     /* channel_count x nranks send orders (comm_patterns_override); NULL = auto */
  int fifo_slots;       /* FIFO slots per connection of buffer_size / 8 bytes each: 8 (the reference's
                           MCCS_BUFFER_SLOTS), 16 or 32; 0 = default (16).  More slots = more slices in
                           flight per lane; the chunk schedule (and so every result) still follows
                           buffer_size, as in the reference */
  int direct_bytes;     /* AllReduce buckets of at most this many bytes per rank run the direct
                           (two-shot) kernel on a fully connected node of <= 8 ranks: every chunk to
                           its ring owner, reduced in the ring's order, results broadcast, so the
                           output equals the ring's bit for bit; larger buckets take the ring.
                           0 = default (MCCS_DIRECT_BYTES; else 8 MiB at >= 4 ranks, 4 MiB at 3,
                           off at 2),
                           < 0 = never.  Every rank must agree
                           (it sizes the arena: Connect refuses a mismatch) */
  int oneshot_bytes;    /* buckets of at most this many bytes per rank take the one-shot variant
                           instead: every rank sends its whole input to every peer and reduces
                           every chunk itself (same order, same bits; one exchange instead of
                           two).  0 = default (MCCS_ONESHOT_BYTES; else 2 MiB at 2 ranks, 1 MiB at
                           3-4, 256 KiB above), < 0 = never; ranks must agree */
  int ll_bytes;         /* AllReduce / AllGather buckets of at most this many bytes per rank take the LL one-shot
                           (flag-carrying 16-byte lines: no drain, no count atomic) when the arena is
                           uncached; same order, same bits.  0 = default (MCCS_LL_BYTES; else 128 KiB),
                           < 0 = never, at most 1 MiB; ranks must agree (appended in 0.3.1) */
  int reserved[16];     /* zero; room for later fields, so the struct keeps this size from 0.4 on
                           (init and setup refuse a config whose reserved words are not zero) */
} mccsCommConfig;

void mccsCommConfigDefault(mccsCommConfig *cfg);
/* sizeof(mccsCommConfig) as this library was built (see the ABI note above). */
size_t mccsCommConfigSize(void);
/* mccsCommConfigDefault for a caller that states its struct size: writes
 * nothing and returns mccsInvalidArgument unless `size` is this library's
 * sizeof(mccsCommConfig), so a caller built against another header can never
 * have bytes written past its struct. */
mccsResult_t mccsCommConfigDefaultSized(mccsCommConfig *cfg, size_t size);

/* One process drives `nranks` ranks (the reference service model: one mccs
 * process owns every GPU of the host).  devices[r] is rank r's GPU; devices
 * may repeat (several ranks on one GPU: their collectives must be issued
 * inside one mccsGroupStart/End so they run as one launch). */
mccsResult_t mccsCommInitAll(mccsComm_t *comms, int nranks, const int *devices, const mccsCommConfig *cfg);

/* One rank per process: SetupRank allocates this rank's FIFO arena and writes
 * a connect handle (IPC memory handle + layout, mccsConnectHandleSize()
 * bytes); the caller all-gathers the handles out of band (the reference's
 * bootstrap/exchange engines) and passes all nranks of them, concatenated in
 * rank order, to Connect. */
size_t mccsConnectHandleSize(void);
mccsResult_t mccsCommSetupRank(mccsComm_t *comm, int rank, int nranks, int device, const mccsCommConfig *cfg,
                               void *handle_out);
mccsResult_t mccsCommConnect(mccsComm_t comm, const void *all_handles);

/* libmccs::all_reduce (src/libmccs/src/collectives.rs:75-138): count in
 * elements of dtype, stream-ordered on `stream`, returns after launch.
 * A communicator's collectives run in the order they are issued, whatever
 * stream each is issued on (a launch on another stream than the comm's
 * previous one waits for it), as on the reference's one private comm stream.
 * Exception: a collective captured into a HIP graph runs when the graph is
 * replayed, and a replay makes no library call, so it is not ordered against
 * the comm's other launches by issue.  Instead every launch of a communicator,
 * replayed or not, takes the communicator's launch guard on the GPU before it
 * touches the comm's FIFO state, so two of its kernels never run at once: a
 * replay and a launch on another stream with no dependency between them run
 * one after the other, in either order.  Across processes each rank decides
 * that order on its own, so ranks whose replays race other launches of the
 * comm must order those streams themselves (a captured and an eager collective
 * of the same shape could otherwise pair up differently on different ranks).
 * A launch waiting for the guard keeps its workgroup slots: launches of one
 * comm pending together on different hardware queues whose grids exceed the
 * device's co-resident slots can stall until the watchdog (an error, never a
 * wrong sum).
 * Calls on ONE communicator must come from one thread at a time (group state
 * is per thread); different communicators may be driven from different
 * threads at once. */
mccsResult_t mccsAllReduce(const void *sendbuff, void *recvbuff, size_t count, int dtype, int op, mccsComm_t comm,
                           hipStream_t stream);
/* libmccs::all_gather: sendbytes per rank; recvbuff holds nranks*sendbytes. */
mccsResult_t mccsAllGather(const void *sendbuff, void *recvbuff, size_t sendbytes, mccsComm_t comm,
                           hipStream_t stream);
/* Ring ReduceScatter.  Not in the reference: it declares the function
 * (mccsFuncReduceScatter = 3, src/collectives/include/devcomm.h:14 and
 * src/mccs/src/proxy/task.rs:12) but stops at unimplemented!() in
 * CollTask::total_bytes (task.rs:95-102) and ships no kernel for it.
 * sendbuff holds nranks * recvcount elements of dtype, block D at element
 * D * recvcount; rank r receives in recvbuff (recvcount elements) the
 * reduction over all ranks of block r.  dtype: any mccsDevDataType_t; op:
 * mccsDevSum / Prod / Max / Min.  For block D on a channel the value is
 * acc = x[s1], then acc = fn(x[sk], acc) for k = 2..n, each hop rounded in
 * dtype, where s1..sn are the successors of D along that channel's ring and
 * sn = D (the operand order of the AllReduce ring).  Which channel an element
 * belongs to follows the ring walk.
 * Stream-ordered, returns after launch.  As for mccsAllReduce: a
 * communicator's collectives run in issue order whatever stream each is issued
 * on; every launch takes the communicator's launch guard; several
 * ReduceScatters of one comm in one group are batched into one launch (mixing
 * functions, dtypes or ops on one comm in a group is refused with
 * mccsInvalidUsage at mccsGroupEnd); ranks sharing a GPU run as one fused
 * launch; the call may be captured into a HIP graph; the watchdog and
 * mccsCommAbort end a stuck kernel.  The ring (mccsCommLastAlgo reports
 * MCCS_ALGO_RING) at every size, unless the communicator opted in to the direct
 * ReduceScatter (mccsCommSetReduceScatterDirect, below): a small block then
 * takes one exchange instead of n-1 hops, with the ring's result bit for bit.
 * In place means recvbuff == sendbuff + rank * recvcount (in elements) and is
 * supported; no other overlap of the two buffers is.  Out of place, sendbuff
 * is never written.  Nothing outside [recvbuff, recvbuff + recvcount) is
 * written.  recvcount == 0 succeeds and launches nothing; an unknown dtype or
 * op and null buffers are refused with mccsInvalidArgument; nranks == 1 is a
 * local copy. */
mccsResult_t mccsReduceScatter(const void *sendbuff, void *recvbuff, size_t recvcount, int dtype, int op,
                               mccsComm_t comm, hipStream_t stream);
/* Ring Broadcast and Reduce, the two rooted collectives.  Not in the
 * reference: it declares the functions (mccsFuncBoadcast = 0, sic, and
 * mccsFuncReduce = 1, src/collectives/include/devcomm.h:11-12) and carries
 * mccsDevWorkElem.root, but ships no kernel for either.
 * mccsBroadcast is byte-typed like mccsAllGather: every rank's
 * recvbuff[0, nbytes) becomes the root's sendbuff[0, nbytes).  sendbuff is
 * read on the root only; elsewhere it may be NULL and is never dereferenced.
 * In place on the root means recvbuff == sendbuff; out of place the root's
 * recvbuff is written too and its sendbuff is never written.
 * mccsReduce: dtype any mccsDevDataType_t, op mccsDevSum / Prod / Max / Min.
 * The root's recvbuff[0, count) receives the reduction over all ranks of
 * sendbuff[0, count); recvbuff is neither read nor written on the other ranks
 * and may be NULL there.  In place on the root, recvbuff == sendbuff, is
 * supported; no other overlap is.  On a channel the value is acc = x[s1], then
 * acc = fn(x[sk], acc) for k = 2..n, each hop rounded in dtype, where s1..sn
 * are the successors of root along that channel's ring and sn = root: the
 * operand order mccsReduceScatter has for block `root`, and the AllReduce
 * ring's.  Which channel an element belongs to follows the ring walk of the
 * whole buffer cut like a block.
 * Both are a chain along each channel's ring, from the root (Broadcast) or to
 * it (Reduce); the connection between the chain's two ends carries nothing, so
 * after a rooted call the communicator's connections stand at different FIFO
 * steps (each connection's two ends still agree).
 * Otherwise as for mccsReduceScatter: stream-ordered, returns after launch; a
 * communicator's collectives run in issue order whatever stream each is issued
 * on; every launch takes the communicator's launch guard; several calls of one
 * function, dtype and op on one comm in one group are batched into one launch,
 * and their roots may differ (the root is per work element); mixing functions,
 * dtypes or ops on one comm in a group is refused with mccsInvalidUsage at
 * mccsGroupEnd; ranks sharing a GPU run as one fused launch; the call may be
 * captured into a HIP graph; the watchdog and mccsCommAbort end a stuck
 * kernel.  The ring (mccsCommLastAlgo reports MCCS_ALGO_RING) at every size,
 * unless the communicator opted in to the direct Broadcast / Reduce
 * (mccsCommSetRootedDirect, below): a small buffer then takes one exchange
 * instead of the chain's n-1 hops, with the ring's result bit for bit; such a
 * call takes no FIFO step, so it leaves the connections where they were.
 * nbytes / count == 0 succeeds and launches nothing; a root outside
 * [0, nranks) is refused with mccsInvalidArgument (mccsGetLastErrorString names
 * it), as are an unknown dtype or op and a NULL buffer where the rank's role
 * uses it; nranks == 1 is a local copy.  Every rank must name the same root:
 * ranks that disagree stall until the watchdog (mccsTimeout from
 * mccsCommSync); this is not detected earlier.  Nothing outside
 * [recvbuff, recvbuff + size) is written on any rank. */
mccsResult_t mccsBroadcast(const void *sendbuff, void *recvbuff, size_t nbytes, int root, mccsComm_t comm,
                           hipStream_t stream);
mccsResult_t mccsReduce(const void *sendbuff, void *recvbuff, size_t count, int dtype, int op, int root,
                        mccsComm_t comm, hipStream_t stream);
/* AllToAll on the ring connections.  Not in the reference (its device ABI
 * reserves point-to-point function ids only).  Byte-typed like mccsAllGather
 * and mccsBroadcast: both buffers hold nranks * bytes_per_peer bytes, and after
 * the call rank r's recvbuff[s*B + i] == rank s's sendbuff[r*B + i] for every
 * rank s, s == r included (B = bytes_per_peer).
 * Route, fixed when the communicator is created from its rings (DESIGN.md
 * §3.2; mccsCommAllToAllRoute reports it).  One hop: when every ordered pair of
 * ranks (s, t) is the arc s -> next of exactly m >= 1 channels, the same m for
 * every pair -- the default rings of 2, 3, 4, 5, 7 and 8 ranks -- each channel
 * carries only the block for its ring successor, the pair's block cut over its
 * m channels as mccsAllGather cuts a block over m channels; every link carries
 * only its own pair's bytes, and the call uses all the comm's channels
 * whatever its size.  Relay: on any other ring set (the default rings of 6
 * ranks, fewer channels than nranks - 1), or with MCCS_ALLTOALL_HOPS=relay in
 * the environment when the communicator is created (every rank must agree, as
 * for MCCS_GATE; mccsCommConnect refuses a mismatch), every channel the call
 * selects (as mccsAllGather selects them) carries every pair's block hop by hop
 * along its ring, FIFO slot to FIFO slot, touching no user buffer on the way.
 * Rank r's own block is copied locally.
 * Out of place only: overlapping sendbuff and recvbuff ranges are refused with
 * mccsInvalidArgument (mccsGetLastErrorString names it).  sendbuff is never
 * written; nothing outside [recvbuff, recvbuff + nranks*B) is written, at any
 * alignment of either buffer.  bytes_per_peer == 0 succeeds and launches
 * nothing; NULL buffers are refused with mccsInvalidArgument; nranks == 1 is a
 * local copy.
 * Otherwise as for mccsReduceScatter: stream-ordered, returns after launch; a
 * communicator's collectives run in issue order whatever stream each is issued
 * on; every launch takes the communicator's launch guard; ranks sharing a GPU
 * run as one fused launch; the call may be captured into a HIP graph (the
 * route lives in the captured work list); the watchdog and mccsCommAbort end a
 * stuck kernel; several AllToAlls of one comm in one group are batched into one
 * launch, and mixing it with another function on one comm in a group is refused
 * with mccsInvalidUsage at mccsGroupEnd.  The ring (mccsCommLastAlgo reports
 * MCCS_ALGO_RING) whatever the direct / one-shot / LL thresholds, unless the
 * communicator opted in to the LL all-to-all (mccsCommSetAllToAllLL, below):
 * then a call of at most that limit per peer which is its communicator's only
 * call of the launch takes the LL kernel (MCCS_ALGO_LL), on any route. */
mccsResult_t mccsAllToAll(const void *sendbuff, void *recvbuff, size_t bytes_per_peer, mccsComm_t comm,
                          hipStream_t stream);
/* The comm's AllToAll route: info2[0] hops (1: one hop; nranks - 1: relay; 0
 * for one rank), info2[1] m, the channels carrying each pair's block (one hop;
 * 0 for the relay, where the call's size selects them). */
mccsResult_t mccsCommAllToAllRoute(mccsComm_t comm, int *info2);
/* AllToAllv: AllToAll with per-peer byte counts and displacements (MPI's
 * Alltoallv, in bytes).  Each of the four arrays has nranks entries, read by
 * the host during the call (the caller may free them afterwards).  Rank r sends
 * sendcounts[t] bytes from sendbuff + sdispls[t] to rank t and receives
 * recvcounts[s] bytes from rank s at recvbuff + rdispls[s]; the self block
 * (sendcounts[r] bytes) moves from sendbuff + sdispls[r] to recvbuff +
 * rdispls[r] without a FIFO step.  The contract is MPI's: rank s's
 * sendcounts[t] equals rank t's recvcounts[s].  Ranks that disagree stall until
 * the watchdog or receive wrong bytes; like disagreeing roots this is not
 * detected.  sendbuff is never written, and no byte of recvbuff outside the
 * nranks receive segments is written, at any alignment.
 * One hop only.  The call needs the one-hop AllToAll route (above): a channel
 * then carries only its successor's block, so a pair's size is known to its
 * two ranks and to nobody else.  On a relay route (the default rings of 6
 * ranks, fewer channels than the one-hop set needs, a user ring set without
 * the equal-m property, MCCS_ALLTOALL_HOPS=relay) a relaying rank would need
 * the sizes of blocks that are neither its row nor its column, and the call is
 * refused with mccsInvalidUsage; mccsGetLastErrorString names the route.
 * Refused with mccsInvalidArgument: a NULL array; a NULL buffer with a non-zero
 * count on that side; sendcounts[rank] != recvcounts[rank]; two receive
 * segments of non-zero length that overlap; a receive segment that overlaps a
 * send segment of non-zero length (the call is out of place).  Send segments
 * may overlap each other: the same bytes may go to two peers.
 * All counts zero: success, nothing is launched.  nranks == 1: the self copy
 * only.  The ring, and no direct threshold applies, unless the communicator
 * opted in to the LL all-to-all for the v calls (mccsCommSetAllToAllLL, below,
 * which changes four of the rules above).  Every ring element runs
 * with the schema's largest thread count (a pair's two ends know no common
 * byte total to derive a smaller one from).  Graph capture: counts and
 * displacements are baked into the captured work elements, and a replay
 * repeats them; mccsAllToAllvDev (below) reads them on the device at every
 * replay.  Several calls of one comm in one group are batched into one
 * launch; mixing with another function is refused as for mccsAllToAll.
 * Otherwise as mccsAllToAll. */
mccsResult_t mccsAllToAllv(const void *sendbuff, const size_t *sendcounts, const size_t *sdispls, void *recvbuff,
                           const size_t *recvcounts, const size_t *rdispls, mccsComm_t comm, hipStream_t stream);
/* AllToAllvDev: mccsAllToAllv with the sizes in device memory, read by the
 * kernel when it runs.  `table` is 8-byte aligned memory the rank's GPU can
 * read, 4 * nranks unsigned 64-bit words, all in bytes, row * nranks + peer:
 *   row 0  sendcounts[t]     row 2  recvcounts[s]
 *   row 1  sdispls[t]        row 3  rdispls[s]
 * with mccsAllToAllv's meaning: rank r sends sendcounts[t] bytes from sendbuff +
 * sdispls[t] to rank t and receives recvcounts[s] bytes from rank s at recvbuff
 * + rdispls[s]; the self block moves sendcounts[r] bytes without a FIFO step.
 * The host never reads the table.  The caller's contract:
 *   - the table is complete before the call's position in stream order and is
 *     not modified until the call has completed on the stream;
 *   - rank s's sendcounts[t] equals rank t's recvcounts[s], and sendcounts[r]
 *     == recvcounts[r];
 *   - receive segments overlap neither each other nor a send segment;
 *   - every segment lies inside its buffer.
 * None of this can be checked by the host and none is checked on the device:
 * the count and displacement checks mccsAllToAllv makes are the caller's here.
 * Ranks that disagree stall until the watchdog or receive wrong bytes, as for
 * disagreeing roots; a displacement outside a buffer is an out-of-bounds
 * access.
 * One hop only: a relay route is refused with mccsInvalidUsage exactly as for
 * mccsAllToAllv.  Refused with mccsInvalidArgument: a NULL table, a table that
 * is not 8-byte aligned, a NULL buffer (the host knows no count that would
 * excuse one).
 * The call always launches, on every channel of the comm, also when every count
 * turns out to be zero (a zero count makes no FIFO call and takes no step on
 * that side).  Its works always go through the work FIFO or, in a capture, the
 * graph work arena, never in the launch arguments.  nranks == 1: the self copy,
 * its size and both offsets read from the table.  The ring, unless the
 * communicator opted in to the LL all-to-all for the v calls
 * (mccsCommSetAllToAllLL, below).
 * Graph capture: the captured elements hold the table's address and the two
 * base pointers, and every replay reads the table anew, so a graph captured once
 * moves each step's own sizes (write the table, or have a kernel write it,
 * earlier on the stream).  Several calls of one comm in one group are batched
 * into one launch; mixing with another function, mccsAllToAllv included, is
 * refused as for mccsAllToAll.  Otherwise as mccsAllToAllv. */
mccsResult_t mccsAllToAllvDev(const void *sendbuff, void *recvbuff, const uint64_t *table, mccsComm_t comm,
                              hipStream_t stream);
/* The LL all-to-all: mccsAllToAll, mccsAllToAllv and mccsAllToAllvDev at small
 * sizes through the flag-carrying 16-byte lines of the LL one-shot (DESIGN.md
 * §3.4) instead of the ring FIFOs.  Opt-in per communicator; both limits
 * default to 0 = off, and with both off every call plans exactly as without
 * this entry point.  MCCS_A2A_LL_BYTES / MCCS_A2AV_LL_BYTES in the environment
 * set them when the communicator is created (clamped to the maximum below).
 * mccsCommAllToAllLLMax: the most bytes one ordered pair can move in one
 * launch, ll_slot / 2 - 8 with ll_slot = 2 x ll_bytes (a header line, then 8
 * data bytes per 16-byte line); 0 where the lines cannot be used: no LL slots
 * (ll_bytes < 0, nranks outside 2..8), a cached FIFO arena, system-scope
 * fences.
 * mccsCommSetAllToAllLL: a value above that maximum is refused with
 * mccsInvalidArgument; a call while the communicator has a group open or a
 * call pending, with mccsInvalidUsage.  EVERY RANK MUST SET THE SAME TWO
 * VALUES: ranks that disagree pick different kernels for one call and stall
 * until the watchdog; like disagreeing roots this is not detected.
 * bytes_per_peer > 0: an mccsAllToAll of at most that many bytes per peer that
 * is its communicator's only call of the launch takes the LL kernel
 * (mccsCommLastAlgo reports MCCS_ALGO_LL); a larger one, or one sharing a
 * group with a second call of the communicator, takes the ring as before.
 * Every rank knows the size, so every rank decides alike.  No route is needed:
 * 6 ranks and MCCS_ALLTOALL_HOPS=relay take it too.
 * v_bytes_per_peer > 0 is the caller's PROMISE that no count of any
 * mccsAllToAllv / mccsAllToAllvDev call on any rank of the communicator exceeds
 * it (a rank sees only its own row and column, so it cannot decide from its
 * counts): for example a MoE capacity bound.  Then
 *   - every v / Dev call that is its communicator's only call of the launch
 *     takes the LL kernel, whatever its counts;
 *   - it always launches, also with every count zero: the peers wait for this
 *     rank's header lines;
 *   - the relay-route refusal does not apply to it;
 *   - a host count above the limit is refused with mccsInvalidArgument
 *     (mccsGetLastErrorString names the peer); a Dev count above it is clamped
 *     in the kernel, on both sides, to the maximum above: the bytes are
 *     truncated and nothing is written past a slot;
 *   - every other argument rule stays;
 *   - a v call sharing a group with a second call of its communicator falls
 *     back to the ring, under the ring's rules (the relay refusal included).
 * Ranks sharing a GPU are fused into one launch as always; their counts may
 * differ.  A captured launch bakes host counts and displacements in; a Dev
 * launch re-reads its table at every replay.  The node gate does not cover
 * this path. */
mccsResult_t mccsCommSetAllToAllLL(mccsComm_t comm, size_t bytes_per_peer, size_t v_bytes_per_peer);
mccsResult_t mccsCommAllToAllLLMax(mccsComm_t comm, size_t *cap);
/* The direct ReduceScatter: every rank writes each foreign block of its input
 * once, straight into the owner's slot of the direct region, and every owner
 * reduces its own block -- one exchange instead of the ring's n-1 hops, the
 * same link bytes.  The result is the ring's, bit for bit:
 * the same channels, chunks and summation order.  Opt-in per communicator;
 * both limits are bytes PER BLOCK (recvcount x element size), default to 0 =
 * off, and with both off every call plans exactly as without this entry
 * point.  MCCS_RS_DIRECT_BYTES / MCCS_RS_LL_BYTES in the environment set them
 * when the communicator is created (clamped to the maxima below).
 * mccsCommReduceScatterDirectMax: *cap, the largest block of the count-based
 * variant (one one-shot slot: oneshot_bytes rounded up to 64 KiB; 0 without
 * one-shot slots -- oneshot_bytes < 0, nranks outside 2..8 -- or without peer
 * atomics); *ll_cap, the largest block of the LL variant (ll_slot / 2 =
 * ll_bytes rounded up to 8; 0 where the lines cannot be used: no LL slots, a
 * cached FIFO arena, system-scope fences).
 * mccsCommSetReduceScatterDirect: a value above its maximum is refused with
 * mccsInvalidArgument; a call while the communicator has a group open or a
 * call pending, with mccsInvalidUsage.  EVERY RANK MUST SET THE SAME TWO
 * VALUES: ranks that disagree pick different kernels for one call and stall
 * until the watchdog; like disagreeing roots this is not detected.
 * A mccsReduceScatter of Sum / Prod / Max / Min whose block is within
 * ll_block_bytes takes the LL variant (mccsCommLastAlgo reports MCCS_ALGO_LL),
 * else one within block_bytes the count-based variant (MCCS_ALGO_ONESHOT),
 * when it is its communicator's only call of the launch; a larger one, one
 * sharing a group with a second call of the communicator, and every
 * PreMulSum / SumPostDiv (mccsReduceScatterOpArg, the average) take the ring
 * as before.  In place (recvbuff == sendbuff + rank * recvcount) is
 * supported.  Ranks sharing a GPU are fused into one launch as always; the
 * call may be captured into a HIP graph.  The node gate does not cover this
 * path. */
mccsResult_t mccsCommSetReduceScatterDirect(mccsComm_t comm, size_t block_bytes, size_t ll_block_bytes);
mccsResult_t mccsCommReduceScatterDirectMax(mccsComm_t comm, size_t *cap, size_t *ll_cap);
/* The direct Broadcast and Reduce: the root writes its bytes once into every
 * peer's slot of the direct region (Broadcast), or every rank writes its input
 * once into the root's slot and the root folds them (Reduce) -- one exchange
 * instead of the ring chain's n-1 serial hops.  The result is
 * the ring's, bit for bit: Reduce keeps the ring's channels, chunks and
 * summation order.  Opt-in per communicator; the four limits are bytes of the
 * WHOLE BUFFER (nbytes; count x element size), two per function because their
 * crossovers need not agree; all default to 0 = off, and with all four off
 * every call plans exactly as without this entry point.  MCCS_BC_DIRECT_BYTES /
 * MCCS_BC_LL_BYTES / MCCS_RD_DIRECT_BYTES / MCCS_RD_LL_BYTES in the environment
 * set them when the communicator is created (clamped to the maxima below).
 * mccsCommRootedDirectMax: the direct ReduceScatter's maxima, over the whole
 * buffer: *cap, the largest buffer of the count-based variant (one one-shot
 * slot: oneshot_bytes rounded up to 64 KiB; 0 without one-shot slots --
 * oneshot_bytes < 0, nranks outside 2..8 -- or without peer atomics); *ll_cap,
 * the largest buffer of the LL variant (ll_slot / 2 = ll_bytes rounded up to
 * 8; 0 where the lines cannot be used: no LL slots, a cached FIFO arena,
 * system-scope fences).
 * mccsCommSetRootedDirect: a value above its maximum is refused with
 * mccsInvalidArgument; a call while the communicator has a group open or a
 * call pending, with mccsInvalidUsage.  EVERY RANK MUST SET THE SAME FOUR
 * VALUES: ranks that disagree pick different kernels for one call and stall
 * until the watchdog; like disagreeing roots this is not detected.
 * A mccsBroadcast, or a mccsReduce of Sum / Prod / Max / Min, within its
 * function's LL limit takes the LL variant (mccsCommLastAlgo reports
 * MCCS_ALGO_LL), else one within its count-based limit that variant
 * (MCCS_ALGO_ONESHOT), when it is its communicator's only call of the launch;
 * a larger one, one sharing a group with a second call of the communicator
 * (both keep their roots), and every PreMulSum / SumPostDiv (mccsReduceOpArg,
 * the average) take the ring as before.  Every argument check of the two calls
 * comes first and is unchanged.  In place on the root is supported; a
 * non-root's recvbuff (Reduce) and sendbuff (Broadcast) are never touched and
 * may be NULL.  A direct rooted call takes no FIFO step: the connections stay
 * where they were.  Ranks sharing a GPU are fused into one launch as always;
 * the call may be captured into a HIP graph.  The node gate does not cover
 * this path. */
mccsResult_t mccsCommSetRootedDirect(mccsComm_t comm, size_t bcast_bytes, size_t bcast_ll_bytes, size_t reduce_bytes,
                                     size_t reduce_ll_bytes);
mccsResult_t mccsCommRootedDirectMax(mccsComm_t comm, size_t *cap, size_t *ll_cap);
/* Send / Recv: grouped point-to-point (torch's batch_isend_irecv; the pieces of
 * a Gather or Scatter).  mccsSend moves count * elem_bytes(dtype) bytes from
 * sendbuff to rank `peer`, mccsRecv receives as many from rank `peer` into
 * recvbuff; the data path is byte-typed, dtype only scales count.  A message
 * involves its two ranks only: no other rank of the communicator enters a call.
 * Matching is NCCL's: on each ordered pair (s, t) the k-th send of s to t over
 * the communicator's life matches the k-th receive of t from s.  A size that
 * differs between the two ends, or a call whose partner never comes, stalls
 * until the watchdog; like disagreeing roots this is not detected.
 * Groups.  The sends and receives of one communicator inside mccsGroupStart /
 * mccsGroupEnd form one launch; outside a group each call is a launch of its
 * own.  A zero-byte call succeeds and takes no FIFO step (inside a group it
 * still holds its place in the order of its pair); a group whose calls are all
 * empty launches nothing.
 * One hop only.  A message s -> t travels on the m channels whose ring has t
 * right after s, cut over them as mccsAllToAllv cuts a pair's block, which
 * needs the one-hop AllToAll route (mccsCommAllToAllRoute).  On a relay route
 * (the default rings of 6 ranks, fewer channels than the one-hop set needs, a
 * user ring set without the equal-m property, MCCS_ALLTOALL_HOPS=relay) the
 * call is refused with mccsInvalidUsage, in mccsAllToAllv's words;
 * mccsGetLastErrorString names the route.
 * Refused with mccsInvalidArgument: peer outside 0 .. nranks - 1; peer == the
 * calling rank (a self send is out of scope: copy the buffer); an unknown
 * dtype; a NULL buffer with a non-zero count; a communicator of one rank (it
 * has no peer).  Mixing with another function in one group on one communicator
 * is refused with mccsInvalidUsage, as for every function.
 * Stricter than NCCL: group what you exchange.  One workgroup walks a
 * channel's send and its receive in lockstep (call i of the send, then call i
 * of the receive), and the j-th send and the j-th receive of a group that
 * share a channel share an element.  Ranks that exchange messages with each
 * other must therefore issue those calls in one group each, on both sides.  If
 * rank A groups its send to B with its receive from B while B issues the same
 * two calls ungrouped, as two launches, the pair can stall where NCCL would
 * not.  An ungrouped send larger than the FIFO's free space (buffer_size)
 * completes only once the peer's receive runs.
 * Always the ring (mccsCommLastAlgo reports it); every element runs with the
 * schema's largest thread count, as mccsAllToAllv's.  Graph capture: pointers
 * and sizes are baked into the captured work elements. */
mccsResult_t mccsSend(const void *sendbuff, size_t count, int dtype, int peer, mccsComm_t comm, hipStream_t stream);
mccsResult_t mccsRecv(void *recvbuff, size_t count, int dtype, int peer, mccsComm_t comm, hipStream_t stream);
/* PreMulSum, SumPostDiv and the average: the three reducing ring collectives
 * with an op argument.  The reference declares both ops (mccsDevPreMulSum = 4,
 * mccsDevSumPostDiv = 5, collectives.h:28-32; DECL2(AllReduce, PreMulSum /
 * SumPostDiv), collectives.h:101-102; AllReduceOpType, command.rs:40-41; the
 * functors FuncPreMulSum / FuncSumPostDiv, reduce_kernel.h:478-697) and carries
 * the scalar in mccsDevWorkElem.redOpArg; the semantics below are those
 * functors'.
 * op: any of the six mccsDevRedOp_t.  With mccsDevSum / Prod / Max / Min op_arg
 * must be 0 and the call is exactly the plain one (which keeps refusing ops 4
 * and 5).
 * mccsDevPreMulSum, every dtype: op_arg holds the scalar s, an element of
 * dtype, in its low sizeof(T) bytes (*(T*)&op_arg; the bits above must be
 * zero).  Every rank's own input element x is replaced by pre(x) = x * s,
 * rounded ONCE in dtype (integers: modulo 2^w; half / bfloat16: the exact
 * product rounded once to the type), before its first use; the reduction then
 * is Sum.  The product and the sum are two roundings, never one fused
 * multiply-add.
 * mccsDevSumPostDiv, the six integer dtypes only: n = (int)op_arg, 1 <= n <=
 * INT32_MAX.  The reduction is Sum, wrapping in dtype; the finished sum goes
 * through post(x) = T(x / n), C division truncating toward zero after the
 * usual promotions (n converts to unsigned for uint32 / uint64).
 * With the operand order of the plain calls the value is acc = pre(x[s1]),
 * then acc = pre(x[sk]) + acc for k = 2..n, result = post(acc).  So a
 * PreMulSum collective equals, bit for bit, the Sum collective over inputs
 * pre-scaled elementwise, and a SumPostDiv collective equals post applied
 * elementwise to the Sum collective's output.  pre is applied where a call
 * reads the user input, post on the call that finishes the reduction
 * (AllReduce's recvReduceCopySend, the closing recvReduceCopy of ReduceScatter
 * and of Reduce's root), whose posted value goes to every destination: the
 * FIFO never carries a pre-less input or a posted partial.  nranks == 1:
 * recvbuff = post(pre(sendbuff)), in place too.
 * Otherwise as the plain calls (buffers, in place, counts, roots, groups:
 * several calls of one function, dtype and op on one comm in one group are
 * batched into one launch and may differ in op_arg, which is per work element
 * like the root; mixing ops, e.g. Sum and PreMulSum, is refused with
 * mccsInvalidUsage at mccsGroupEnd; fused launches of ranks sharing a GPU,
 * graph capture -- the scalar lives in the captured work list --, the launch
 * guard, the watchdog and mccsCommAbort).  PreMulSum and SumPostDiv always take
 * the ring (mccsCommLastAlgo reports MCCS_ALGO_RING), whatever the size and the
 * direct / one-shot / LL thresholds: those kernels know neither step.
 * Refused with mccsInvalidArgument (mccsGetLastErrorString names the problem):
 * a nonzero op_arg with Sum / Prod / Max / Min, PreMulSum bits above the element
 * width, SumPostDiv on a floating dtype or with op_arg outside 1..INT32_MAX. */
mccsResult_t mccsAllReduceOpArg(const void *sendbuff, void *recvbuff, size_t count, int dtype, int op,
                                uint64_t op_arg, mccsComm_t comm, hipStream_t stream);
mccsResult_t mccsReduceScatterOpArg(const void *sendbuff, void *recvbuff, size_t recvcount, int dtype, int op,
                                    uint64_t op_arg, mccsComm_t comm, hipStream_t stream);
mccsResult_t mccsReduceOpArg(const void *sendbuff, void *recvbuff, size_t count, int dtype, int op, uint64_t op_arg,
                             int root, mccsComm_t comm, hipStream_t stream);
/* The average over nranks as (op, op_arg) for the calls above (host only).
 * Floating dtypes: mccsDevPreMulSum with s = 1/nranks (double: 1.0 / n; float:
 * 1.0f / (float)n; half / bfloat16: that binary32 value rounded to nearest even
 * once to the type).  Integer dtypes: mccsDevSumPostDiv with n = nranks (NCCL's
 * mapping). */
mccsResult_t mccsAvgOp(int dtype, int nranks, int *op, uint64_t *op_arg);
/* Encodes v as a PreMulSum scalar of dtype (host only).  double: v as is;
 * float: (float)v; half / bfloat16: (float)v rounded to nearest even to the
 * type -- two roundings, so a v within half a binary32 ulp of a 16-bit tie may
 * land one ulp from the directly rounded value; pass a v the type holds exactly
 * where that matters.  Integer dtypes: v must be integral and in the type's
 * range (else mccsInvalidArgument); negative values are two's complement in the
 * element's width. */
mccsResult_t mccsRedOpArgFromDouble(int dtype, double v, uint64_t *op_arg);
/* Group calls (ProxyCommand::GroupCall): collectives issued between Start and
 * End are planned together and launched at End (one launch per device). */
mccsResult_t mccsGroupStart(void);
mccsResult_t mccsGroupEnd(void);

/* Waits for the comm's stream and reports a device-side failure (watchdog
 * timeout / abort) as mccsTimeout / mccsRemoteError. */
mccsResult_t mccsCommSync(mccsComm_t comm);
/* Raises the comm's abortFlag: in-flight kernels exit at their next poll. */
mccsResult_t mccsCommAbort(mccsComm_t comm);
/* Frees the comm after its last launch completed; no barrier with the peers
 * is needed.  A peer's kernel may still post into this rank's FIFO arena after
 * this rank's own kernel finished, so the arena goes back to a per-process pool
 * but is handed to a new communicator only once every peer has destroyed its
 * side too (each peer's destroy writes a release word into the arena, after
 * its own kernels ended) or has exited: a peer process that never destroys
 * (it crashed, or its mccsCommConnect failed) stops being awaited once it has
 * exited and been reaped, where this process can see that (same host and pid
 * namespace); otherwise the arena stays pooled and unused. */
mccsResult_t mccsCommDestroy(mccsComm_t comm);
/* rank, nranks, device, channels, lanes, block threads, fifo memory kind
 * (MCCS_FIFO_*: the hand-off mode the comm's launches run). */
mccsResult_t mccsCommInfo(mccsComm_t comm, int *info7);
/* ring send order of channel ch (nranks ints). */
mccsResult_t mccsCommRing(mccsComm_t comm, int ch, int *order);
/* Algorithm of the comm's latest launch: MCCS_ALGO_RING, MCCS_ALGO_DIRECT
 * (two-shot), MCCS_ALGO_ONESHOT or MCCS_ALGO_LL (LL one-shot) (-1 before the first). */
#define MCCS_ALGO_RING 0
#define MCCS_ALGO_DIRECT 1
#define MCCS_ALGO_ONESHOT 2
#define MCCS_ALGO_LL 3
int mccsCommLastAlgo(mccsComm_t comm);
/* 1 when the comm may run the direct kernel: a direct region was configured
 * and every device of the communicator can perform atomics on every other's
 * memory (hipDevP2PAttrNativeAtomicSupported; the hand-off counts are remote
 * atomics).  Otherwise every AllReduce takes the ring, except buckets up to
 * ll_bytes, whose LL one-shot makes no remote atomics. */
int mccsCommDirectEnabled(mccsComm_t comm);
/* Node gate (connect-time self-test, run when a communicator spans two or
 * more GPUs; MCCS_GATE=0 skips it, MCCS_GATE=1 forces it): one exact-sum
 * AllReduce through the ring in its configured hand-off and through each
 * enabled direct variant, with every rank agreeing on the verdicts.  A wrong
 * ring sum steps every rank down uncached -> uncached + release -> cached
 * (system-scope fences); a wrong direct sum disables that variant.
 * info4[0] 1 if the gate ran, [1] the hand-off the comm now runs (MCCS_FIFO_*),
 * [2] MCCS_GATE_* bits that failed, [3] MCCS_GATE_* direct variants disabled. */
#define MCCS_GATE_RING_UNCACHED 0x1 /* ring, relaxed hand-off on uncached FIFOs */
#define MCCS_GATE_RING_RELEASE 0x2  /* ring, release fence before each post */
#define MCCS_GATE_RING_SYSTEM 0x4   /* ring, system-scope release/acquire (reference) */
#define MCCS_GATE_LL 0x8            /* LL one-shot */
#define MCCS_GATE_ONESHOT 0x10      /* one-shot */
#define MCCS_GATE_TWOSHOT 0x20      /* two-shot */
#define MCCS_GATE_NO_ATOMICS 0x40   /* some rank cannot perform peer atomics (direct kernel off) */
mccsResult_t mccsCommGateInfo(mccsComm_t comm, int *info4);
/* The comm's launch guard (inspection, tests): out4[0] the token of the launch
 * holding it (0 = free), [1] 1 once a fused launch holds every rank slot's
 * guard, [2] workgroups of the holder that have finished, [3] workgroups that
 * ever found it held by another launch of the comm and waited.  Copies from
 * device memory (synchronous). */
mccsResult_t mccsCommGuardInfo(mccsComm_t comm, uint64_t *out4);
/* 1 when this process's HIP runtime tells streams apart by hipStreamGetId,
 * 0 when by address (a runtime older than ROCm 7.1 loaded first, e.g. torch's).
 * The cross-stream issue order above keys on it. */
int mccs_stream_id_native(void);
/* Device pointer of the comm's mccsDevCommAndChannels (for inspection). */
mccsResult_t mccsCommDevComm(mccsComm_t comm, void **dev_comm);
const char *mccsGetErrorString(mccsResult_t r);
/* Diagnosis of the calling thread's latest failed library call: the step it
 * failed in, the failing runtime call and its hipError_t name and text, e.g.
 * "mccsCommSetupRank(rank 2/4, device 0) > comm_alloc_local > work FIFO:
 * HostMallocMapped -> hipErrorOutOfMemory (out of memory) at comm.cpp:318".
 * "" when the latest communicator / collective call succeeded (each one clears
 * it on entry).  The pointer stays valid until this thread's next library
 * call.  The reference returns one code per failure and logs the CUDA error
 * (cuda_warning!, src/mccs/src/utils/mod.rs:7-26); this adds where it failed. */
const char *mccsGetLastErrorString(void);
/* The hipError_t of that failure (0 when the failure was not a HIP call, e.g.
 * a refused argument or mismatched peers). */
int mccsGetLastHipError(void);
/* Ring timing counters of `device` (armed by MCCS_RING_PROFILE=1 at
 * communicator init): out4[0] slices, [1] ticks waiting for peer flags,
 * [2] ticks streaming + draining (s_memrealtime, 100 MHz), [3] reserved.
 * reset != 0 zeroes them after reading. */
mccsResult_t mccs_ring_profile(int device, unsigned long long *out4, int reset);

/* ----------------------------------------------------------------------
 * Application <-> backend bridge (the reference's mCCS service model: the
 * collectives run in a backend process; the application shares buffers and
 * stream order with it through IPC handles).  Handles are the 64-byte
 * hipIpcMemHandle_t / hipIpcEventHandle_t as opaque bytes.
 * ---------------------------------------------------------------------- */
#define MCCS_IPC_HANDLE_BYTES 64
/* libmccs cuda_malloc (src/libmccs/src/memory.rs:12-37): the backend
 * allocates and exports; the application opens the handle. */
mccsResult_t mccsMemAllocShared(int device, size_t bytes, void **dptr, void *handle_out);
mccsResult_t mccsMemFreeShared(int device, void *dptr);
mccsResult_t mccsMemOpenShared(int device, const void *handle, void **dptr);
mccsResult_t mccsMemCloseShared(int device, void *dptr);
/* libmccs register_stream (communicator.rs:47-66): the application creates an
 * interprocess event per stream; the backend opens it. */
mccsResult_t mccsEventCreateShared(int device, void **event, void *handle_out);
mccsResult_t mccsEventOpenShared(int device, const void *handle, void **event);
mccsResult_t mccsEventDestroyShared(void *event);
/* The comm's completion event (recorded after every launch) exported for the
 * application (InitCommunicator's event handle, communicator.rs:35-38). */
mccsResult_t mccsCommEventHandle(mccsComm_t comm, void *handle_out);
/* The comm's own stream, and wait_user_event (proxy/engine.rs:1185-1189):
 * the comm stream waits on an (opened) application event. */
mccsResult_t mccsCommStream(mccsComm_t comm, hipStream_t *stream);
mccsResult_t mccsCommWaitEvent(mccsComm_t comm, void *event);
/* Application side of the bridge (collectives.rs:86,134): record the user
 * event on its stream before a request; wait on the backend event after. */
mccsResult_t mccsEventRecordShared(void *event, hipStream_t stream);
mccsResult_t mccsStreamWaitShared(hipStream_t stream, void *event);

/* Host-only helpers (no GPU needed). */
/* BASELINE configs[0] plumbing: the same ring schedule and FIFO protocol run
 * by nranks x nchannels host threads over host memory (no GPU).  rings as in
 * mccsCommConfig (NULL = identity order on every channel). */
mccsResult_t mccs_host_ring_allreduce(int nranks, const void *const *sendbufs, void *const *recvbufs, size_t count,
                                      int dtype, int op, int nchannels, int nthreads_ref, int buff_size,
                                      const int *rings);
/* The ring ReduceScatter schedule (mccsReduceScatter) and FIFO protocol on
 * host threads over host memory: sendbufs[r] holds nranks * recvcount
 * elements, recvbufs[r] recvcount; in place as for mccsReduceScatter. */
mccsResult_t mccs_host_ring_reduce_scatter(int nranks, const void *const *sendbufs, void *const *recvbufs,
                                           size_t recvcount, int dtype, int op, int nchannels, int nthreads_ref,
                                           int buff_size, const int *rings);
/* The ring Broadcast and Reduce schedules (mccsBroadcast, mccsReduce) and the
 * FIFO protocol on host threads over host memory.  Buffers as for the device
 * calls: sendbufs[r] of a Broadcast may be NULL for r != root, recvbufs[r] of
 * a Reduce for r != root. */
mccsResult_t mccs_host_ring_broadcast(int nranks, const void *const *sendbufs, void *const *recvbufs, size_t nbytes,
                                      int root, int nchannels, int nthreads_ref, int buff_size, const int *rings);
mccsResult_t mccs_host_ring_reduce(int nranks, const void *const *sendbufs, void *const *recvbufs, size_t count,
                                   int dtype, int op, int root, int nchannels, int nthreads_ref, int buff_size,
                                   const int *rings);
/* The AllToAll route of a ring set (rings: nchannels x nranks send orders, NULL
 * = identity order on every channel), as mccsAllToAll derives it: hops and m
 * as mccsCommAllToAllRoute reports them, and two nranks x nchannels tables (may
 * be NULL): send_bid[r*nchannels + c] is the part of its successor's block rank
 * r sends on channel c, recv_bid the part of its predecessor's block it
 * receives there (one hop: the number of earlier channels with the same arc,
 * so a connection's sender and receiver name the same part; relay: c). */
mccsResult_t mccs_alltoall_route(int nranks, int nchannels, const int *rings, int force_relay, int *hops, int *m,
                                 int *send_bid, int *recv_bid);
/* The AllToAll schedule (mccsAllToAll) and the FIFO protocol on host threads
 * over host memory: sendbufs[r] and recvbufs[r] hold nranks * bytes_per_peer
 * bytes.  The route is mccs_alltoall_route's for these rings; a relay uses all
 * nchannels. */
mccsResult_t mccs_host_ring_all_to_all(int nranks, const void *const *sendbufs, void *const *recvbufs,
                                       size_t bytes_per_peer, int nchannels, int nthreads_ref, int buff_size,
                                       const int *rings, int force_relay);
/* The AllToAllv schedule (mccsAllToAllv) on host threads over host memory:
 * counts is the nranks x nranks byte matrix (counts[s*nranks + t]: what s sends
 * to t), sdispls[r*nranks + t] and rdispls[r*nranks + s] each rank's
 * displacement rows.  Refuses a ring set whose route is not one hop
 * (mccsInvalidUsage). */
mccsResult_t mccs_host_ring_all_to_all_v(int nranks, const void *const *sendbufs, void *const *recvbufs,
                                         const size_t *counts, const size_t *sdispls, const size_t *rdispls,
                                         int nchannels, int nthreads_ref, int buff_size, const int *rings,
                                         int force_relay);
/* The AllToAllvDev schedule on host threads: tables[r] is rank r's size table
 * (mccsAllToAllvDev's layout) in host memory.  Each channel's element is
 * resolved from the table by the arithmetic the kernel uses, then walked as
 * mccs_host_ring_all_to_all_v walks it. */
mccsResult_t mccs_host_ring_all_to_all_v_tables(int nranks, const void *const *sendbufs, void *const *recvbufs,
                                                const uint64_t *const *tables, int nchannels, int nthreads_ref,
                                                int buff_size, const int *rings, int force_relay);
/* Index of the word of `row` (0 sendcounts, 1 sdispls, 2 recvcounts, 3
 * rdispls) for `peer` in a size table of nranks ranks, as the kernel and the
 * host-thread ring compute it; -1 for an argument out of range. */
long long mccs_a2avd_index(int row, int nranks, int peer);
/* The Send/Recv schedule (mccsSend / mccsRecv) on host threads over host
 * memory.  Op i is a send (op_is_send[i] != 0) or a receive of op_bytes[i]
 * bytes at op_buf[i], issued by rank op_rank[i] with rank op_peer[i]; each
 * rank's ops, in list order, form one group.  The elements are built by the
 * planner's own pairing rule and walked as mccs_host_ring_all_to_all_v walks
 * its elements.  A relay route is refused (mccsInvalidUsage).  Seeing all
 * ranks, it refuses with mccsInvalidArgument what the device path cannot
 * detect: a send without its receive or of another size; and fewer than two
 * ranks, a rank or peer out of range, peer == rank, a NULL buffer with bytes. */
mccsResult_t mccs_host_ring_send_recv(int nranks, int nops, const int *op_rank, const int *op_is_send,
                                      const int *op_peer, void *const *op_buf, const size_t *op_bytes, int nchannels,
                                      int nthreads_ref, int buff_size, const int *rings);
/* The three reducing schedules with an op argument (mccsAllReduceOpArg,
 * mccsReduceScatterOpArg, mccsReduceOpArg): all six ops, the same argument
 * rules, pre and post applied where the kernels apply them and rounded as they
 * round.  The three functions above keep refusing ops 4 and 5. */
mccsResult_t mccs_host_ring_allreduce_oparg(int nranks, const void *const *sendbufs, void *const *recvbufs,
                                            size_t count, int dtype, int op, int nchannels, int nthreads_ref,
                                            int buff_size, const int *rings, uint64_t op_arg);
mccsResult_t mccs_host_ring_reduce_scatter_oparg(int nranks, const void *const *sendbufs, void *const *recvbufs,
                                                 size_t recvcount, int dtype, int op, int nchannels,
                                                 int nthreads_ref, int buff_size, const int *rings, uint64_t op_arg);
mccsResult_t mccs_host_ring_reduce_oparg(int nranks, const void *const *sendbufs, void *const *recvbufs, size_t count,
                                         int dtype, int op, int root, int nchannels, int nthreads_ref, int buff_size,
                                         const int *rings, uint64_t op_arg);
/* Default ring orders for an n-rank node (edge-disjoint Hamiltonian cycles,
 * both directions); writes up to max_channels x nranks ints, returns count. */
int mccs_default_rings(int nranks, int nch_req, int *out, int max_channels);
/* The library's default direct thresholds for an n-rank communicator (what
 * mccsCommConfig.oneshot_bytes / direct_bytes = 0 resolve to without the
 * MCCS_* overrides; -1 = off). */
void mccs_direct_defaults(int nranks, int *oneshot_bytes, int *direct_bytes);
/* mccsCommConfig.ll_bytes = 0 resolves to this (without the environment override). */
int mccs_ll_default(int nranks);
/* get_task_schema (plan.rs:602-635): channels and threads for total_bytes. */
void mccs_task_schema(size_t total_bytes, int nch_cfg, int *nch, int *nthreads);
/* The chunk walk of one work element, as every kernel and host path cuts it:
 * func = mccsFuncAllReduce (count = the buffer's elements), mccsFuncAllGather
 * (elem_bytes = 1, count = bytes per rank) or mccsFuncReduceScatter (count =
 * elements per block); width = 64 (the ring's arithmetic) or 32 (the direct
 * kernels'; count < 2^31).  Writes the first max_rows rows of four values
 * {gridOffset, realChunkSize, chunk offset, nelem}, one row per loop and part
 * (AllReduce: part = bid * nranks + ring chunk; otherwise part = bid), nelem
 * 0 for a part past the end.  Returns the walk's row count, -1 for invalid
 * arguments. */
long long mccs_ring_walk(int func, int nranks, int nchannels, int elem_bytes, int nthreads_ref, int buff_size,
                         size_t count, int width, long long *rows, long long max_rows);

/* Library identification. */
const char *mccs_hip_version(void);

#ifdef __cplusplus
}
#endif

#endif /* MCCS_AMD_HIP_H_ */
