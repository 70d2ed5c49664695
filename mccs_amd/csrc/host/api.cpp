// api.cpp — extern "C" communicator / collective API of libmccs_hip.so.
//
// The reference splits this across libmccs (app shim, src/libmccs/src/*.rs),
// the daemon relay and the proxy engine; here the app calls the planner
// directly (no daemon process on the hot path: the reference's WR/WC shared
// memory queues only relay the same arguments, collectives.rs:88-131).
#include <hip/hip_runtime.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "comm.h"
#include "dtypes.h"
#include "half_bits.h"
#include "ring_walk.h"

namespace mccs {
void task_schema(size_t total_bytes, int nch_cfg, int* nch_out, int* nthreads_out);

struct GroupState {
  int depth = 0;
  mccsResult_t error = mccsSuccess;  // first failure inside the group
  std::vector<Comm*> comms;
  std::vector<hipStream_t> streams;
};
static thread_local GroupState g_group;

// Drops every plan queued in the current group (error path).
static void group_discard() {
  for (Comm* c : g_group.comms) plan_discard(c);
  g_group.comms.clear();
  g_group.streams.clear();
}

// Direct AllReduce thresholds when the config leaves them 0 (MCCS_DIRECT_BYTES /
// MCCS_ONESHOT_BYTES override): buckets up to this many bytes per rank take
// the one-shot / two-shot kernel (bit-identical to the ring either way).
// Virtual node, graph replay, fp16 (profiles/r03_direct_vnode*.json): one-shot
// beat the ring to 2 MiB at n = 2, and beat two-shot to ~1 MiB at n = 3 / 4
// and to 512 KiB at n = 8; two-shot beat the ring to 2 MiB at n = 3 and to
// 8 MiB at n = 4 / 8 and only tied it at n = 2 (the ring is two hops there).  Over xGMI
// the ring's 2(n-1) sequential hops cost more than here, so these are
// conservative; the node's sweep (bench config.direct_sweep_fp16) refines them.
static int default_oneshot_bytes(int nranks) {
  return nranks == 2 ? 2 << 20 : nranks <= 4 ? 1 << 20 : 256 << 10;
}
static int default_direct_bytes(int nranks) { return nranks >= 4 ? 8 << 20 : nranks == 3 ? 4 << 20 : -1; }
// LL one-shot (ring_cfg.h): buckets whose hand-off round trips cost more than
// their bytes; its lines carry 8 data bytes per 16, so it stays small.
// Virtual node, graph replay, fp16 (profiles/r03_direct_ll_vnode.json): LL
// beat the one-shot at every n up to 128 KiB (n = 8: 32 KiB 15.1 -> 8.6 us,
// 128 KiB 22.0 -> 14.2; n = 2: 32 KiB 8.4 -> 5.0) and lost at n = 8 from
// 512 KiB.  Over xGMI its doubled line bytes cost link time
// (2 x 128 KiB per peer link ~ 4 us at ~64 GB/s, about the round trips it
// saves), so the default stays at 128 KiB for every n.
static int default_ll_bytes(int nranks) {
  (void)nranks;
  return 128 << 10;
}

static void fill_defaults(mccsCommConfig* c, int nranks) {
  if (c->buffer_size <= 0) c->buffer_size = 1 << 22;  // mccs.toml:19
  if (c->block_threads <= 0) c->block_threads = MCCS_RING_MAX_THREADS;
  if (c->work_fifo_depth <= 0) c->work_fifo_depth = 4096;
  // launch on the caller's stream (stream order is the same as libmccs's
  // user-event -> comm-stream -> backend-event bridge, without the ~10 us per
  // cross-stream wait measured on MI355X); 1 keeps the two-stream bridge
  if (c->bridge_streams == 0) c->bridge_streams = -1;
  // 16 slots: four 4-step slices in flight per lane instead of two (n = 8
  // virtual node +5 % at 128 MiB, +10 % at 16 MiB; n = 2 / 4 unchanged), more
  // bytes in flight per lane to cover an xGMI hop; 2 x the FIFO memory
  // (8 MiB per connection)
  if (c->fifo_slots == 0) c->fifo_slots = 2 * MCCS_BUFFER_SLOTS;
  if (c->direct_bytes == 0) c->direct_bytes = default_direct_bytes(nranks);
  if (c->oneshot_bytes == 0) c->oneshot_bytes = default_oneshot_bytes(nranks);
  if (c->ll_bytes == 0) c->ll_bytes = default_ll_bytes(nranks);
}

static mccsResult_t validate_cfg(const mccsCommConfig& c, int nranks) {
  StepScope st("config");
  // a chunk (buffer_size/2 bytes) must be a multiple of the largest thread
  // granule (512 x 8 B, all_reduce.h:34-35) so a rounded chunk fits 4 steps
  if (c.buffer_size < 8192 || c.buffer_size % 8192 != 0)
    MCCS_FAIL(mccsInvalidArgument, "buffer_size %d is not a multiple of 8192", c.buffer_size);
  // multiples of 32 keep the reference's nWarps*32 blocks (e.g. 544) valid;
  // at least one data wave next to the control wave (ring_kernel.h), like
  // the reference's smallest block (96 threads, plan.rs:602-635)
  if (c.block_threads < 96 || c.block_threads > MCCS_RING_MAX_THREADS || c.block_threads % 32)
    MCCS_FAIL(mccsInvalidArgument, "block_threads %d outside 96..%d or not a multiple of 32", c.block_threads,
              MCCS_RING_MAX_THREADS);
  if (c.lanes < 0 || c.lanes > MCCS_MAX_LANES) MCCS_FAIL(mccsInvalidArgument, "lanes %d outside 0..%d", c.lanes, MCCS_MAX_LANES);
  if (c.channel_count < 0 || c.channel_count > MCCS_MAX_NCHANNELS)
    MCCS_FAIL(mccsInvalidArgument, "channel_count %d outside 0..%d", c.channel_count, MCCS_MAX_NCHANNELS);
  if (c.work_fifo_depth & (c.work_fifo_depth - 1))
    MCCS_FAIL(mccsInvalidArgument, "work_fifo_depth %d is not a power of two", c.work_fifo_depth);
  if (c.locality != MCCS_LOCALITY_SENDER && c.locality != MCCS_LOCALITY_RECEIVER)
    MCCS_FAIL(mccsInvalidArgument, "locality %d unknown", c.locality);
  if (c.fifo_memory != MCCS_FIFO_UNCACHED && c.fifo_memory != MCCS_FIFO_DEVICE &&
      c.fifo_memory != MCCS_FIFO_UNCACHED_RELEASE)
    MCCS_FAIL(mccsInvalidArgument, "fifo_memory %d unknown", c.fifo_memory);
  if (nranks < 1 || nranks > 64) MCCS_FAIL(mccsInvalidArgument, "nranks %d outside 1..64", nranks);
  if (c.fifo_slots != 8 && c.fifo_slots != 16 && c.fifo_slots != 32)
    MCCS_FAIL(mccsInvalidArgument, "fifo_slots %d is not 8, 16 or 32", c.fifo_slots);
  // 9 slots of direct_bytes, 16 of oneshot_bytes and 16 of twice ll_bytes live in every rank's arena
  if (c.direct_bytes > (1 << 30)) MCCS_FAIL(mccsInvalidArgument, "direct_bytes %d above 1 GiB", c.direct_bytes);
  if (c.oneshot_bytes > (64 << 20)) MCCS_FAIL(mccsInvalidArgument, "oneshot_bytes %d above 64 MiB", c.oneshot_bytes);
  if (c.ll_bytes > (1 << 20)) MCCS_FAIL(mccsInvalidArgument, "ll_bytes %d above 1 MiB", c.ll_bytes);
  return mccsSuccess;
}

static mccsResult_t make_comm(int rank, int nranks, int device, const mccsCommConfig* user_cfg, Comm** out) {
  StepScope st("make_comm");
  mccsCommConfig cfg;
  mccsCommConfigDefault(&cfg);
  if (user_cfg) cfg = *user_cfg;
  for (int w : cfg.reserved)
    if (w != 0) MCCS_FAIL(mccsInvalidArgument, "a reserved config word is not zero");  // a field this library does not know
  fill_defaults(&cfg, nranks);
  MCCS_CHECK(validate_cfg(cfg, nranks));
  if (rank < 0 || rank >= nranks) MCCS_FAIL(mccsInvalidArgument, "rank %d outside 0..%d", rank, nranks - 1);
  int ndev = 0;
  MCCS_HIP(rt().GetDeviceCount(&ndev));
  if (device < 0 || device >= ndev) MCCS_FAIL(mccsInvalidArgument, "device %d not visible (%d devices)", device, ndev);
  Comm* c = new Comm();
  c->rank = rank;
  c->nranks = nranks;
  c->device = device;
  c->cfg = cfg;
  if (cfg.rings) {
    const int nch = cfg.channel_count > 0 ? cfg.channel_count : 1;
    for (int ch = 0; ch < nch; ++ch) {
      std::vector<int> r(cfg.rings + (size_t)ch * nranks, cfg.rings + (size_t)(ch + 1) * nranks);
      std::vector<int> s = r;
      std::sort(s.begin(), s.end());
      for (int i = 0; i < nranks; ++i)
        if (s[i] != i) {
          delete c;
          // not a permutation (engine.rs:274-279 asserts)
          MCCS_FAIL(mccsInvalidArgument, "rings[%d] is not a permutation of 0..%d", ch, nranks - 1);
        }
      c->rings.push_back(r);
    }
  } else {
    default_rings(nranks, cfg.channel_count, &c->rings);
  }
  c->cfg.rings = nullptr;  // not owned
  c->nch = (int)c->rings.size();
  if (const char* v = std::getenv("MCCS_SLICE_STEPS")) c->slice_steps = std::atoi(v) == 2 ? 2 : ALLREDUCE_CHUNKSTEPS;
  if (const char* v = std::getenv("MCCS_INLINE_WORKS")) c->inline_works = std::atoi(v) != 0;
  // (at most 4096: a launch guard counts a slot's workgroups in 16 bits)
  if (const char* v = std::getenv("MCCS_DIRECT_BLOCKS")) c->direct_blocks = std::atoi(v) > 0 ? std::min(std::atoi(v), 4096) : 128;
  // MCCS_ALLTOALL_HOPS=relay: AllToAll relays along the rings even where they
  // allow one hop (read here, carried in the connect handle: every rank agrees)
  if (const char* v = std::getenv("MCCS_ALLTOALL_HOPS")) c->a2a_force_relay = v[0] == 'r' || v[0] == 'R';
  {
    std::vector<int> flat, sb((size_t)nranks * c->nch), rb((size_t)nranks * c->nch);
    for (const auto& r : c->rings) flat.insert(flat.end(), r.begin(), r.end());
    alltoall_route(nranks, c->nch, flat.data(), c->a2a_force_relay, &c->a2a_hops, &c->a2a_m, sb.data(), rb.data());
    for (int ch = 0; ch < c->nch; ++ch) {
      c->a2a_send_bid.push_back((uint8_t)sb[(size_t)rank * c->nch + ch]);
      c->a2a_recv_bid.push_back((uint8_t)rb[(size_t)rank * c->nch + ch]);
    }
  }
  c->block_threads = cfg.block_threads;
  // auto lanes: ~64 streaming workgroups per rank (128 at n = 2).  A lane's
  // throughput is bound by its per-slice latency chain (flag poll, loads,
  // store drain), not by bandwidth: the 2-rank virtual node at 128 MiB runs
  // 335 / 488 / 499 GB/s at 2 channels x 16 / 32 / 64 lanes and 754 at
  // 4 x 32 (comm.cpp default_rings); an 8-GPU rank must feed 7 links x
  // ~77 GB/s per direction (7 channels x 9 lanes).
  const int wgs = nranks == 2 ? 128 : 64;
  c->lanes = cfg.lanes > 0 ? cfg.lanes : (nranks == 1 ? 1 : std::max(1, std::min(MCCS_MAX_LANES, wgs / c->nch)));
  // every lane owns a >= 256-byte region of each 2-step slot pair (ring.hip)
  while (c->lanes > 1 && (size_t)cfg.buffer_size / MCCS_BUFFER_SLOTS * 2 / c->lanes < 256) {
    if (cfg.lanes > 0) {
      delete c;
      MCCS_FAIL(mccsInvalidArgument, "lanes %d leave under 256 bytes of a slot pair per lane", cfg.lanes);
    }
    c->lanes /= 2;
  }
  *out = c;
  return mccsSuccess;
}

static mccsResult_t enable_peer(int a, int b) {
  if (a == b) return mccsSuccess;
  StepScope st("peer access " + std::to_string(a) + " -> " + std::to_string(b));
  int can = 0;
  MCCS_HIP(rt().CanAccessPeer(&can, a, b));
  if (!can) MCCS_FAIL(mccsSystemError, "device %d cannot access device %d", a, b);
  DeviceGuard g(a);
  MCCS_HIP(rt().EnablePeerAccess(b));
  return mccsSuccess;
}

// op_arg: nullptr from the plain entry points (Sum / Prod / Max / Min only), the
// argument of an mccs*OpArg entry point otherwise (all six ops).
static mccsResult_t launch_single(Comm* c, int func, int dtype, int op, const void* send, void* recv, size_t count,
                                  hipStream_t stream, int root = 0, const uint64_t* op_arg = nullptr) {
  // inside a group the diagnosis of a rejected call must survive to GroupEnd
  // (the group was cleared at GroupStart)
  if (g_group.depth == 0) err_clear();
  auto reject = [](mccsResult_t e, const char* why) {
    const bool first = g_group.depth == 0 || g_group.error == mccsSuccess;  // a group keeps its first failure
    if (g_group.depth > 0 && first) g_group.error = e;
    if (first) err_note(__FILE__, __LINE__, "%s", why);
    return e;
  };
  if (!c || !c->connected) return reject(mccsInvalidUsage, "the communicator is not connected");
  if (c->failed) return reject(mccsRemoteError, "the communicator failed earlier (watchdog or abort): destroy it");
  if (count == 0) return mccsSuccess;
  const bool rooted = func == mccsFuncBoadcast || func == mccsFuncReduce;
  if (rooted && (root < 0 || root >= c->nranks)) {
    char why[96];
    std::snprintf(why, sizeof(why), "root %d outside 0..%d", root, c->nranks - 1);
    return reject(mccsInvalidArgument, why);
  }
  // a rooted call's buffers are needed where the rank's role uses them:
  // Broadcast reads sendbuff on the root only, Reduce writes recvbuff there only
  const bool need_send = func != mccsFuncBoadcast || c->rank == root;
  const bool need_recv = func != mccsFuncReduce || c->rank == root;
  if ((need_send && !send) || (need_recv && !recv)) return reject(mccsInvalidArgument, "null send or recv buffer");
  if (func == MCCS_FUNC_ALLTOALL) {
    // out of place only: the schedule reads blocks of sendbuff after it wrote others of recvbuff
    const uintptr_t s0 = (uintptr_t)send, r0 = (uintptr_t)recv, len = (uintptr_t)count * (uintptr_t)c->nranks;
    if (s0 < r0 + len && r0 < s0 + len)
      return reject(mccsInvalidArgument, "mccsAllToAll: sendbuff and recvbuff overlap (the call is out of place only)");
  }
  if ((func == mccsFuncAllReduce || func == mccsFuncReduceScatter || func == mccsFuncReduce) &&
      (dtype < 0 || dtype >= mccsNumTypes || op < 0 || op > (op_arg ? mccsDevSumPostDiv : mccsDevMin)))
    return reject(mccsInvalidArgument, "unknown dtype or reduction op");
  const uint64_t arg = op_arg ? *op_arg : 0;
  if (op_arg) {
    const int es = elem_bytes(dtype);
    if (op <= mccsDevMin && arg != 0)
      return reject(mccsInvalidArgument, "op_arg must be 0 for Sum / Prod / Max / Min");
    if (op == mccsDevPreMulSum && es < 8 && (arg >> (8 * es)) != 0)
      return reject(mccsInvalidArgument, "PreMulSum: op_arg has bits set above the element width");
    if (op == mccsDevSumPostDiv && !is_integer_dtype(dtype))
      return reject(mccsInvalidArgument, "SumPostDiv needs an integer dtype");
    if (op == mccsDevSumPostDiv && (arg < 1 || arg > (uint64_t)INT32_MAX))
      return reject(mccsInvalidArgument, "SumPostDiv: op_arg (the divisor) outside 1..INT32_MAX");
  }
  const char* const name = func == MCCS_FUNC_ALLTOALL      ? "mccsAllToAll"
                           : func == mccsFuncAllGather     ? "mccsAllGather"
                           : func == mccsFuncReduceScatter ? (op_arg ? "mccsReduceScatterOpArg" : "mccsReduceScatter")
                           : func == mccsFuncBoadcast      ? "mccsBroadcast"
                           : func == mccsFuncReduce        ? (op_arg ? "mccsReduceOpArg" : "mccsReduce")
                                                           : (op_arg ? "mccsAllReduceOpArg" : "mccsAllReduce");
  if (std::find(g_group.comms.begin(), g_group.comms.end(), c) == g_group.comms.end()) {
    g_group.comms.push_back(c);
    g_group.streams.push_back(stream);
  }
  mccsResult_t er;
  {
    StepScope st(name);
    er = plan_enqueue(c, func, dtype, op, send, recv, count, rooted ? root : 0, arg);
  }
  if (er != mccsSuccess) {
    if (g_group.depth == 0) group_discard();
    else if (g_group.error == mccsSuccess) g_group.error = er;
    return er;
  }
  if (g_group.depth == 0) {
    StepScope st(std::string(name) + " launch");
    mccsResult_t r = plan_launch_group(g_group.comms, g_group.streams);
    group_discard();
    return r;
  }
  return mccsSuccess;
}

// A rejected call's diagnosis: inside a group the first failure is kept to GroupEnd.
static mccsResult_t reject_call(mccsResult_t e, const char* why) {
  const bool first = g_group.depth == 0 || g_group.error == mccsSuccess;
  if (g_group.depth > 0 && first) g_group.error = e;
  if (first) err_note(__FILE__, __LINE__, "%s", why);
  return e;
}

// The v calls' ring path runs on the one-hop AllToAll route only (a2av_needs_relay, plan.cpp); a
// call the LL kernel takes (a2av_takes_ll) needs no route.
static mccsResult_t reject_relay(const Comm* c) {
  char why[256];
  std::snprintf(why, sizeof(why),
                "the AllToAll route is not one hop (%s: hops = %d over %d channels of %d ranks); a relaying rank "
                "would need the sizes of blocks that are neither its row nor its column",
                c->a2a_force_relay ? "MCCS_ALLTOALL_HOPS=relay" : "relay", c->a2a_hops, c->nch, c->nranks);
  return reject_call(mccsInvalidUsage, why);
}

// mccsAllToAllv: the argument rules of mccs_hip.h, then the plan.  *planned: something to launch.
static mccsResult_t a2av_check_and_plan(Comm* c, const void* send, const size_t* sendcounts, const size_t* sdispls,
                                        void* recv, const size_t* recvcounts, const size_t* rdispls,
                                        hipStream_t stream, bool* planned) {
  if (!sendcounts || !sdispls || !recvcounts || !rdispls)
    return reject_call(mccsInvalidArgument, "null count or displacement array");
  const int n = c->nranks, r = c->rank;
  const bool ll = a2av_takes_ll(c);
  if (!ll && a2av_needs_relay(c)) return reject_relay(c);
  size_t any_send = 0, any_recv = 0;
  for (int i = 0; i < n; ++i) {
    any_send |= sendcounts[i];
    any_recv |= recvcounts[i];
  }
  if ((any_send && !send) || (any_recv && !recv))
    return reject_call(mccsInvalidArgument, "null buffer with a non-zero count");
  if (sendcounts[r] != recvcounts[r])
    return reject_call(mccsInvalidArgument, "sendcounts[rank] != recvcounts[rank]");
  const uintptr_t s0 = (uintptr_t)send, r0 = (uintptr_t)recv;
  for (int i = 0; i < n; ++i) {
    if (!recvcounts[i]) continue;
    const uintptr_t a = r0 + rdispls[i], ae = a + recvcounts[i];
    for (int j = 0; j < n; ++j) {
      if (j > i && recvcounts[j] && a < r0 + rdispls[j] + recvcounts[j] && r0 + rdispls[j] < ae)
        return reject_call(mccsInvalidArgument, "two receive segments overlap");
      if (sendcounts[j] && a < s0 + sdispls[j] + sendcounts[j] && s0 + sdispls[j] < ae)
        return reject_call(mccsInvalidArgument,
                           "a receive segment overlaps a send segment (the call is out of place only)");
    }
  }
  // the LL limit is the caller's promise for every count on every rank: a count above it is refused
  if (c->a2av_ll_bytes > 0)
    for (int i = 0; i < n; ++i)
      if (sendcounts[i] > c->a2av_ll_bytes || recvcounts[i] > c->a2av_ll_bytes) {
        char why[160];
        std::snprintf(why, sizeof(why), "%s[%d] = %zu is above the AllToAllv LL limit of %zu bytes per peer",
                      sendcounts[i] > c->a2av_ll_bytes ? "sendcounts" : "recvcounts", i,
                      sendcounts[i] > c->a2av_ll_bytes ? sendcounts[i] : recvcounts[i], c->a2av_ll_bytes);
        return reject_call(mccsInvalidArgument, why);
      }
  // nothing moves: nothing is launched -- except on the LL path, where the peers wait for this rank's headers
  if (!any_send && !any_recv && !ll) return mccsSuccess;
  if (std::find(g_group.comms.begin(), g_group.comms.end(), c) == g_group.comms.end()) {
    g_group.comms.push_back(c);
    g_group.streams.push_back(stream);
  }
  *planned = true;
  const mccsResult_t er = plan_enqueue_a2av(c, send, sendcounts, sdispls, recv, recvcounts, rdispls);
  if (er != mccsSuccess) {
    if (g_group.depth == 0) group_discard();
    else if (g_group.error == mccsSuccess) g_group.error = er;
  }
  return er;
}

static mccsResult_t launch_a2av(Comm* c, const void* send, const size_t* sendcounts, const size_t* sdispls, void* recv,
                                const size_t* recvcounts, const size_t* rdispls, hipStream_t stream) {
  if (g_group.depth == 0) err_clear();
  if (!c || !c->connected) return reject_call(mccsInvalidUsage, "the communicator is not connected");
  if (c->failed) return reject_call(mccsRemoteError, "the communicator failed earlier (watchdog or abort): destroy it");
  bool planned = false;
  {
    StepScope st("mccsAllToAllv");  // names the call in every diagnosis
    const mccsResult_t er =
        a2av_check_and_plan(c, send, sendcounts, sdispls, recv, recvcounts, rdispls, stream, &planned);
    if (er != mccsSuccess || !planned) return er;
  }
  if (g_group.depth == 0) {
    StepScope st("mccsAllToAllv launch");
    const mccsResult_t r = plan_launch_group(g_group.comms, g_group.streams);
    group_discard();
    return r;
  }
  return mccsSuccess;
}

// mccsAllToAllvDev: the sizes are on the device, so the host checks the three
// pointers and the route and nothing else; the call always plans and launches.
static mccsResult_t launch_a2av_dev(Comm* c, const void* send, void* recv, const uint64_t* table, hipStream_t stream) {
  if (g_group.depth == 0) err_clear();
  if (!c || !c->connected) return reject_call(mccsInvalidUsage, "the communicator is not connected");
  if (c->failed) return reject_call(mccsRemoteError, "the communicator failed earlier (watchdog or abort): destroy it");
  {
    StepScope st("mccsAllToAllvDev");  // names the call in every diagnosis
    if (!table) return reject_call(mccsInvalidArgument, "null size table");
    if ((uintptr_t)table % 8) return reject_call(mccsInvalidArgument, "the size table is not 8-byte aligned");
    if (!send || !recv) return reject_call(mccsInvalidArgument, "null buffer (the host knows no count to excuse it)");
    if (!a2av_takes_ll(c) && a2av_needs_relay(c)) return reject_relay(c);
    if (std::find(g_group.comms.begin(), g_group.comms.end(), c) == g_group.comms.end()) {
      g_group.comms.push_back(c);
      g_group.streams.push_back(stream);
    }
    const mccsResult_t er = plan_enqueue_a2av_dev(c, send, recv, table);
    if (er != mccsSuccess) {
      if (g_group.depth == 0) group_discard();
      else if (g_group.error == mccsSuccess) g_group.error = er;
      return er;
    }
  }
  if (g_group.depth == 0) {
    StepScope st("mccsAllToAllvDev launch");
    const mccsResult_t r = plan_launch_group(g_group.comms, g_group.streams);
    group_discard();
    return r;
  }
  return mccsSuccess;
}

// mccsSend / mccsRecv: the argument rules of mccs_hip.h; the call then joins
// its comm's pending group (plan.cpp pairs a group's calls into elements when
// it launches).  Outside a group the call is a group of its own.
static mccsResult_t launch_sendrecv(Comm* c, bool is_send, void* buf, size_t count, int dtype, int peer,
                                    hipStream_t stream) {
  if (g_group.depth == 0) err_clear();
  const char* const name = is_send ? "mccsSend" : "mccsRecv";
  if (!c || !c->connected) return reject_call(mccsInvalidUsage, "the communicator is not connected");
  if (c->failed) return reject_call(mccsRemoteError, "the communicator failed earlier (watchdog or abort): destroy it");
  {
    StepScope st(name);  // names the call in every diagnosis
    char why[128];
    if (c->nranks == 1) return reject_call(mccsInvalidArgument, "a communicator of one rank has no peer");
    if (peer < 0 || peer >= c->nranks) {
      std::snprintf(why, sizeof(why), "peer %d outside 0..%d", peer, c->nranks - 1);
      return reject_call(mccsInvalidArgument, why);
    }
    if (peer == c->rank) return reject_call(mccsInvalidArgument, "peer is the calling rank (a self send is out of scope)");
    if (dtype < 0 || dtype >= mccsNumTypes) return reject_call(mccsInvalidArgument, "unknown dtype");
    if (!buf && count) return reject_call(mccsInvalidArgument, "null buffer with a non-zero count");
    if (a2av_needs_relay(c)) return reject_relay(c);
    if (std::find(g_group.comms.begin(), g_group.comms.end(), c) == g_group.comms.end()) {
      g_group.comms.push_back(c);
      g_group.streams.push_back(stream);
    }
    const mccsResult_t er = plan_enqueue_sendrecv(c, is_send, buf, count * (size_t)elem_bytes(dtype), peer);
    if (er != mccsSuccess) {
      if (g_group.depth == 0) group_discard();
      else if (g_group.error == mccsSuccess) g_group.error = er;
      return er;
    }
  }
  if (g_group.depth == 0) {
    StepScope st(std::string(name) + " launch");
    const mccsResult_t r = plan_launch_group(g_group.comms, g_group.streams);
    group_discard();
    return r;
  }
  return mccsSuccess;
}

}  // namespace mccs

using namespace mccs;

extern "C" void mccsCommConfigDefault(mccsCommConfig* cfg) {
  std::memset(cfg, 0, sizeof(*cfg));
  cfg->buffer_size = 1 << 22;
  // 8 data waves + the control wave (ring_kernel.h workgroup roles)
  cfg->block_threads = MCCS_RING_MAX_THREADS;
  // FIFO data lives with the receiver: the sender's stores cross xGMI as
  // posted writes and every read is local HBM (the reference SHM default was
  // Sender for host-pinned memory; both remain selectable)
  cfg->locality = MCCS_LOCALITY_RECEIVER;
  cfg->fifo_memory = MCCS_FIFO_UNCACHED;
  cfg->work_fifo_depth = 4096;
  cfg->bridge_streams = -1;
  // operator overrides (no rebuild needed): MCCS_LOCALITY=sender|receiver,
  // MCCS_LANES, MCCS_BLOCK_THREADS, MCCS_CHANNELS, MCCS_BUFFER_SIZE,
  // MCCS_BRIDGE_STREAMS, MCCS_FIFO_MEMORY=uncached|release|device,
  // MCCS_FIFO_SLOTS, MCCS_DIRECT_BYTES, MCCS_ONESHOT_BYTES, MCCS_TIMEOUT_MS
  if (const char* v = std::getenv("MCCS_LOCALITY"))
    cfg->locality = (v[0] == 's' || v[0] == 'S') ? MCCS_LOCALITY_SENDER : MCCS_LOCALITY_RECEIVER;
  if (const char* v = std::getenv("MCCS_LANES")) cfg->lanes = std::atoi(v);
  if (const char* v = std::getenv("MCCS_BRIDGE_STREAMS")) cfg->bridge_streams = std::atoi(v);
  if (const char* v = std::getenv("MCCS_FIFO_MEMORY"))
    cfg->fifo_memory = (v[0] == 'd' || v[0] == 'D')   ? MCCS_FIFO_DEVICE
                       : (v[0] == 'r' || v[0] == 'R') ? MCCS_FIFO_UNCACHED_RELEASE
                                                      : MCCS_FIFO_UNCACHED;
  if (const char* v = std::getenv("MCCS_BLOCK_THREADS")) cfg->block_threads = std::atoi(v);
  if (const char* v = std::getenv("MCCS_CHANNELS")) cfg->channel_count = std::atoi(v);
  if (const char* v = std::getenv("MCCS_BUFFER_SIZE")) cfg->buffer_size = std::atoi(v);
  if (const char* v = std::getenv("MCCS_FIFO_SLOTS")) cfg->fifo_slots = std::atoi(v);
  if (const char* v = std::getenv("MCCS_DIRECT_BYTES")) cfg->direct_bytes = std::atoi(v);
  if (const char* v = std::getenv("MCCS_ONESHOT_BYTES")) cfg->oneshot_bytes = std::atoi(v);
  if (const char* v = std::getenv("MCCS_LL_BYTES")) cfg->ll_bytes = std::atoi(v);
  if (const char* v = std::getenv("MCCS_TIMEOUT_MS")) cfg->timeout_ms = std::atoi(v);
}

extern "C" mccsResult_t mccsCommInitAll(mccsComm_t* comms, int nranks, const int* devices, const mccsCommConfig* cfg) {
  err_clear();
  StepScope st0("mccsCommInitAll(" + std::to_string(nranks) + " ranks)");
  if (!comms || !devices || nranks < 1) MCCS_FAIL(mccsInvalidArgument, "null comms/devices or nranks < 1");
  std::vector<Comm*> cs(nranks, nullptr);
  mccsResult_t r = mccsSuccess;
  for (int i = 0; i < nranks && r == mccsSuccess; ++i) {
    StepScope st("rank " + std::to_string(i));
    r = make_comm(i, nranks, devices[i], cfg, &cs[i]);
  }
  // ranks sharing a GPU run as one fused launch that must be co-resident:
  // shrink automatic lanes to fit (explicit lanes are checked at launch)
  for (int i = 0; i < nranks && r == mccsSuccess; ++i) {
    Comm* c = cs[i];
    int share = 0;
    for (int j = 0; j < nranks; ++j) share += devices[j] == devices[i];
    c->share = share;
    if (share < 2 || c->cfg.lanes > 0) continue;
    const int cap = coresident_ring_blocks(c->block_threads, c->device);
    const int fit = cap / (share * c->nch);
    if (fit < 1) {
      err_note(__FILE__, __LINE__, "%d ranks x %d channels do not fit %d co-resident workgroups on device %d", share,
               c->nch, cap, c->device);
      r = mccsInvalidUsage;
    } else {
      c->lanes = std::min(c->lanes, fit);
    }
  }
  for (int i = 0; i < nranks && r == mccsSuccess; ++i) {
    StepScope st("rank " + std::to_string(i));
    r = comm_alloc_local(cs[i]);
  }
  for (int i = 0; i < nranks && r == mccsSuccess; ++i)
    for (int j = 0; j < nranks && r == mccsSuccess; ++j) r = enable_peer(devices[i], devices[j]);
  if (r == mccsSuccess)  // every rank's arena is every peer's to write (released at comm_free)
    for (int i = 0; i < nranks; ++i) {
      cs[i]->arena_shared = nranks > 1;
      for (int j = 0; j < nranks; ++j) cs[i]->peer_epoch[j] = j == i ? 0 : cs[j]->arena_epoch;
    }
  if (r == mccsSuccess) {
    bool all_uc = true, release = false;
    for (int i = 0; i < nranks; ++i) {
      all_uc = all_uc && cs[i]->own_arena_uncached;
      release = release || cs[i]->cfg.fifo_memory == MCCS_FIFO_UNCACHED_RELEASE;
    }
    const bool atomics = devices_p2p_atomics(std::vector<int>(devices, devices + nranks));
    for (int i = 0; i < nranks; ++i) {
      for (int j = 0; j < nranks; ++j) cs[i]->peer_arena[j] = cs[j]->own_arena;
      cs[i]->all_uncached = all_uc;
      cs[i]->fifo_release = release;
      cs[i]->direct_ok = atomics;
    }
    for (int i = 0; i < nranks && r == mccsSuccess; ++i) {
      StepScope st("rank " + std::to_string(i));
      r = comm_build_device(cs[i]);
    }
    // node gate: one process sees every rank, so the host combines their verdicts
    bool distinct = false;
    for (int i = 1; i < nranks; ++i) distinct = distinct || devices[i] != devices[0];
    if (r == mccsSuccess && nranks > 1 && gate_wanted(distinct)) {
      StepScope st("node gate");
      std::vector<bool> atomics_ok(nranks, atomics);
      r = comm_gate(cs, atomics_ok);
    }
  }
  if (r != mccsSuccess) {
    for (auto c : cs)
      if (c) {
        comm_free(c);
        delete c;
      }
    return r;
  }
  for (int i = 0; i < nranks; ++i) comms[i] = (mccsComm_t)cs[i];
  return mccsSuccess;
}

// This process's pid namespace (the inode of /proc/self/ns/pid), 0 if unknown.
static uint64_t pid_namespace() {
  struct stat st;
  return stat("/proc/self/ns/pid", &st) == 0 ? (uint64_t)st.st_ino : 0;
}

// Two connect handles name the same GPU: same host and PCI bus id (ordinals
// are local to a process, so they would match across different GPUs).
static bool same_gpu(const ConnectHandle& a, const ConnectHandle& b) {
  return std::strncmp(a.host, b.host, sizeof(a.host)) == 0 && std::strncmp(a.pci, b.pci, sizeof(a.pci)) == 0;
}

extern "C" size_t mccsConnectHandleSize(void) { return sizeof(ConnectHandle); }

// Exports the comm's FIFO arena for its peers.  An uncached arena whose
// export is refused falls back to a plain device arena (system fences).
static mccsResult_t export_arena(Comm* c, hipIpcMemHandle_t* h) {
  StepScope st("IPC export of the FIFO arena");
  DeviceGuard g(c->device);
  hipError_t e = rt().IpcGetMemHandle(h, c->own_arena);
  if (e == hipSuccess || !c->own_arena_uncached) {
    MCCS_HIP(e);
    return mccsSuccess;
  }
  MCCS_LOG("hipIpcGetMemHandle(uncached arena): %s; retrying with hipMalloc", hipGetErrorString(e));
  MCCS_CHECK(comm_switch_to_device_arena(c));
  MCCS_HIP(rt().IpcGetMemHandle(h, c->own_arena));
  return mccsSuccess;
}

extern "C" mccsResult_t mccsCommSetupRank(mccsComm_t* out, int rank, int nranks, int device, const mccsCommConfig* cfg,
                                          void* handle_out) {
  err_clear();
  StepScope st0("mccsCommSetupRank(rank " + std::to_string(rank) + "/" + std::to_string(nranks) + ", device " +
                std::to_string(device) + ")");
  if (!out || !handle_out) MCCS_FAIL(mccsInvalidArgument, "null comm or handle pointer");
  Comm* c = nullptr;
  MCCS_CHECK(make_comm(rank, nranks, device, cfg, &c));
  ConnectHandle h;
  std::memset(&h, 0, sizeof(h));
  mccsResult_t r = comm_alloc_local(c);
  if (r == mccsSuccess) r = export_arena(c, &h.ipc);
  if (r != mccsSuccess) {
    comm_free(c);
    delete c;
    return r;
  }
  c->arena_shared = nranks > 1;  // exported: any peer may map it from now on
  h.arena_epoch = c->arena_epoch;
  h.magic = kHandleMagic;
  h.rank = rank;
  h.nranks = nranks;
  h.device = device;
  h.pid = (int32_t)getpid();
  h.pidns = pid_namespace();
  h.fifo_memory = !c->own_arena_uncached                              ? MCCS_FIFO_DEVICE
                  : c->cfg.fifo_memory == MCCS_FIFO_UNCACHED_RELEASE ? MCCS_FIFO_UNCACHED_RELEASE
                                                                     : MCCS_FIFO_UNCACHED;
  h.nch = c->nch;
  h.lanes = c->lanes;
  h.lanes_auto = c->cfg.lanes > 0 ? 0 : 1;
  h.ring_cap = coresident_ring_blocks(c->block_threads, device);
  h.arena_bytes = c->layout.total();
  h.buffer_size = c->layout.buffer_size;
  h.direct_bytes = c->cfg.direct_bytes;
  h.oneshot_bytes = c->cfg.oneshot_bytes;
  h.ll_bytes = c->cfg.ll_bytes;
  h.fifo_slots = c->cfg.fifo_slots;
  h.slice_steps = c->slice_steps;
  h.block_threads = c->block_threads;
  h.gate_env = gate_env();
  h.a2a_relay = c->a2a_force_relay ? 1 : 0;
  if (rt().DeviceGetPCIBusId(h.pci, sizeof(h.pci) - 1, device) != hipSuccess)
    std::snprintf(h.pci, sizeof(h.pci), "ordinal:%d", device);
  gethostname(h.host, sizeof(h.host) - 1);
  std::memcpy(handle_out, &h, sizeof(h));
  *out = (mccsComm_t)c;
  return mccsSuccess;
}

// Why rank r's handle cannot join this communicator ("" if it can).
static std::string handle_mismatch(const Comm* c, const ConnectHandle& h, const ConnectHandle& mine, int r) {
  char b[200];
  auto diff = [&](const char* what, long long theirs, long long ours) {
    std::snprintf(b, sizeof(b), "rank %d's %s %lld differs from this rank's %lld", r, what, theirs, ours);
    return std::string(b);
  };
  if (h.magic != kHandleMagic) return "rank " + std::to_string(r) + "'s handle is not a connect handle";
  if (h.rank != r) return diff("handle rank", h.rank, r);
  if (h.nranks != c->nranks) return diff("nranks", h.nranks, c->nranks);
  if (h.nch != c->nch) return diff("channel count", h.nch, c->nch);
  if (h.arena_bytes != c->layout.total()) return diff("arena bytes", (long long)h.arena_bytes, (long long)c->layout.total());
  if (h.buffer_size != c->layout.buffer_size) return diff("buffer_size", (long long)h.buffer_size, (long long)c->layout.buffer_size);
  // ... or on which kernel / slice shape a call takes (both ends of every
  // connection must run the same one: ADVICE r03)
  if (h.direct_bytes != c->cfg.direct_bytes) return diff("direct_bytes", h.direct_bytes, c->cfg.direct_bytes);
  if (h.oneshot_bytes != c->cfg.oneshot_bytes) return diff("oneshot_bytes", h.oneshot_bytes, c->cfg.oneshot_bytes);
  if (h.ll_bytes != c->cfg.ll_bytes) return diff("ll_bytes", h.ll_bytes, c->cfg.ll_bytes);
  if (h.fifo_slots != c->cfg.fifo_slots) return diff("fifo_slots", h.fifo_slots, c->cfg.fifo_slots);
  if (h.slice_steps != c->slice_steps) return diff("slice steps", h.slice_steps, c->slice_steps);
  if (h.block_threads != c->block_threads) return diff("block_threads", h.block_threads, c->block_threads);
  // the node gate's collectives need every rank (a rank that skipped it
  // would leave the others in its vote until the watchdog)
  if (h.gate_env != mine.gate_env) return diff("MCCS_GATE", h.gate_env, mine.gate_env);
  // both ends of every connection must walk the same AllToAll route
  if (h.a2a_relay != mine.a2a_relay) return diff("MCCS_ALLTOALL_HOPS=relay", h.a2a_relay, mine.a2a_relay);
  return "";
}

extern "C" mccsResult_t mccsCommConnect(mccsComm_t comm, const void* all_handles) {
  err_clear();
  Comm* c = (Comm*)comm;
  if (!c || !all_handles || c->connected) {
    StepScope st0("mccsCommConnect");
    MCCS_FAIL(mccsInvalidUsage, "null comm or handles, or the comm is already connected");
  }
  StepScope st0("mccsCommConnect(rank " + std::to_string(c->rank) + "/" + std::to_string(c->nranks) + ")");
  const ConnectHandle* hs = (const ConnectHandle*)all_handles;
  bool all_uc = true, release = false;
  {
    StepScope st("handle check");
    // A refused handle set is refused by every rank: each compares every
    // handle with its own and with rank 0's, and any disagreement between two
    // ranks shows up at every rank.  So no rank goes on to map this rank's
    // arena, and it need not wait for peers' release words when it is
    // destroyed (a service retrying failed connects lost one FIFO
    // arena per attempt on every rank).  Failures after this point keep the
    // wait: a peer past its own check may have mapped the arena, and its ring
    // sender writes up to fifo_slots steps into it before any credit.
    auto refuse = [&](const char* why) {
      c->arena_shared = false;
      err_note(__FILE__, __LINE__, "%s", why);
      return mccsInvalidArgument;
    };
    for (int r = 0; r < c->nranks; ++r) {
      const ConnectHandle& h = hs[r];
      const std::string why = handle_mismatch(c, h, hs[c->rank], r);
      // ranks disagree on the communicator profile
      if (!why.empty()) return refuse(why.c_str());
      all_uc = all_uc && h.fifo_memory != MCCS_FIFO_DEVICE;
      release = release || h.fifo_memory == MCCS_FIFO_UNCACHED_RELEASE;
      if (h.lanes != hs[0].lanes || h.lanes_auto != hs[0].lanes_auto) {
        char b[160];
        std::snprintf(b, sizeof(b), "rank %d's lanes %d (auto %d) differ from rank 0's %d (auto %d)", r, h.lanes,
                      h.lanes_auto, hs[0].lanes, hs[0].lanes_auto);
        return refuse(b);
      }
    }
    // From here a peer may map this rank's arena, so its destroy awaits every
    // peer's release word -- or, for a peer whose exit this process can see
    // (same host and pid namespace), that peer's exit: a peer that crashed, or
    // whose Connect failed before it mapped the arena, never writes the word
    // (ADVICE r05), and once it has exited none of its kernels can write here.
    const ConnectHandle& me = hs[c->rank];
    c->peer_pid.assign(c->nranks, 0);
    for (int r = 0; r < c->nranks; ++r)
      if (r != c->rank && hs[r].pidns && hs[r].pidns == me.pidns && hs[r].pid > 0 &&
          std::strncmp(hs[r].host, me.host, sizeof(me.host)) == 0)
        c->peer_pid[r] = hs[r].pid;
  }
  // Ranks of this communicator that share a GPU as separate processes run
  // separate launches that spin on each other's flags, so all of them must be
  // resident together.  Unlike one fused launch (mccsCommInitAll), the GPU
  // does not co-schedule separate processes' grids as a unit (4 processes x
  // 60 workgroups = 240 of 256 slots timed out on MI355X), so automatic lanes
  // shrink to half the slots; explicit lanes that cannot fit at all are
  // refused instead of deadlocking.  Every rank derives the same lane count
  // from the same handles (a connection's two ends must agree on lanes).
  {
    StepScope st("co-residency");
    int max_share = 1, cap = 1 << 30;
    for (int r = 0; r < c->nranks; ++r) {
      int share = 0;
      for (int q = 0; q < c->nranks; ++q) share += same_gpu(hs[q], hs[r]);
      max_share = std::max(max_share, share);
      if (hs[r].ring_cap > 0) cap = std::min(cap, (int)hs[r].ring_cap);
    }
    c->share = max_share;
    if (max_share > 1 && cap < (1 << 30)) {
      if (hs[0].lanes_auto) {
        const int fit = cap / 2 / (max_share * c->nch);
        if (fit < 1)
          MCCS_FAIL(mccsInvalidUsage, "%d ranks x %d channels per GPU do not fit half of %d workgroup slots", max_share,
                    c->nch, cap);
        c->lanes = std::min(c->lanes, fit);
      } else if ((long)max_share * c->nch * c->lanes > cap) {
        MCCS_FAIL(mccsInvalidUsage, "%d ranks x %d channels x %d lanes per GPU exceed %d workgroup slots", max_share,
                  c->nch, c->lanes, cap);
      }
    }
  }
  DeviceGuard g(c->device);
  for (int r = 0; r < c->nranks; ++r) {
    if (r == c->rank) continue;
    StepScope st("IPC open of rank " + std::to_string(r) + "'s arena");
    const ConnectHandle& h = hs[r];
    if (h.pid == (int32_t)getpid())  // same process: use mccsCommInitAll
      MCCS_FAIL(mccsInvalidUsage, "rank %d is in this process (pid %d): use mccsCommInitAll", r, (int)h.pid);
    int peer_dev = -1;  // the peer's GPU as this process numbers it
    if (rt().DeviceGetByPCIBusId(&peer_dev, h.pci) != hipSuccess) peer_dev = -1;
    if (peer_dev >= 0 && enable_peer(c->device, peer_dev) != mccsSuccess)
      err_clear();  // best effort; IPC maps regardless
    void* p = nullptr;
    MCCS_HIP(rt().IpcOpenMemHandle(&p, h.ipc));
    c->peer_arena[r] = (char*)p;
    c->peer_opened_ipc[r] = true;
    c->peer_epoch[r] = h.arena_epoch;
  }
  c->all_uncached = all_uc;
  c->fifo_release = release;
  // Peer atomics as THIS process sees them: every peer's GPU looked up by PCI
  // bus id (ordinals are per process).  A peer GPU this process cannot see,
  // or cannot do atomics on, turns the count-based direct variants off here;
  // the node gate's vote then turns them off on every rank alike.
  bool atomics = true, distinct = false;
  for (int r = 0; r < c->nranks; ++r) {
    if (same_gpu(hs[r], hs[c->rank])) continue;
    distinct = true;
    int dev = -1, ok = 0;
    if (rt().DeviceGetByPCIBusId(&dev, hs[r].pci) != hipSuccess || dev < 0) atomics = false;
    else if (rt().P2PAtomics(&ok, c->device, dev) != hipSuccess || !ok) atomics = false;
  }
  c->direct_ok = atomics;
  {
    StepScope st("device structures");
    MCCS_CHECK(comm_build_device(c));
  }
  if (gate_wanted(distinct)) {
    StepScope st("node gate");
    std::vector<Comm*> cs{c};
    mccsResult_t r = comm_gate(cs, std::vector<bool>{atomics});
    if (r != mccsSuccess) {
      c->connected = false;  // the caller destroys it; no collective may run on it
      return r;
    }
  } else if (distinct) {
    // no gate, no vote: keep the count-based direct variants only where every
    // rank can be trusted to decide alike (they cannot tell without a vote)
    c->direct_ok = false;
  }
  return mccsSuccess;
}

extern "C" mccsResult_t mccsAllReduce(const void* sendbuff, void* recvbuff, size_t count, int dtype, int op,
                                      mccsComm_t comm, hipStream_t stream) {
  return launch_single((Comm*)comm, mccsFuncAllReduce, dtype, op, sendbuff, recvbuff, count, stream);
}

extern "C" mccsResult_t mccsAllGather(const void* sendbuff, void* recvbuff, size_t sendbytes, mccsComm_t comm,
                                      hipStream_t stream) {
  return launch_single((Comm*)comm, mccsFuncAllGather, mccsInt8, mccsDevSum, sendbuff, recvbuff, sendbytes, stream);
}

extern "C" mccsResult_t mccsReduceScatter(const void* sendbuff, void* recvbuff, size_t recvcount, int dtype, int op,
                                          mccsComm_t comm, hipStream_t stream) {
  return launch_single((Comm*)comm, mccsFuncReduceScatter, dtype, op, sendbuff, recvbuff, recvcount, stream);
}

extern "C" mccsResult_t mccsBroadcast(const void* sendbuff, void* recvbuff, size_t nbytes, int root, mccsComm_t comm,
                                      hipStream_t stream) {
  return launch_single((Comm*)comm, mccsFuncBoadcast, mccsInt8, mccsDevSum, sendbuff, recvbuff, nbytes, stream, root);
}

extern "C" mccsResult_t mccsReduce(const void* sendbuff, void* recvbuff, size_t count, int dtype, int op, int root,
                                   mccsComm_t comm, hipStream_t stream) {
  return launch_single((Comm*)comm, mccsFuncReduce, dtype, op, sendbuff, recvbuff, count, stream, root);
}

extern "C" mccsResult_t mccsAllToAll(const void* sendbuff, void* recvbuff, size_t bytes_per_peer, mccsComm_t comm,
                                     hipStream_t stream) {
  return launch_single((Comm*)comm, MCCS_FUNC_ALLTOALL, mccsInt8, mccsDevSum, sendbuff, recvbuff, bytes_per_peer,
                       stream);
}

extern "C" mccsResult_t mccsAllToAllv(const void* sendbuff, const size_t* sendcounts, const size_t* sdispls,
                                      void* recvbuff, const size_t* recvcounts, const size_t* rdispls, mccsComm_t comm,
                                      hipStream_t stream) {
  return launch_a2av((Comm*)comm, sendbuff, sendcounts, sdispls, recvbuff, recvcounts, rdispls, stream);
}

extern "C" mccsResult_t mccsAllToAllvDev(const void* sendbuff, void* recvbuff, const uint64_t* table, mccsComm_t comm,
                                         hipStream_t stream) {
  return launch_a2av_dev((Comm*)comm, sendbuff, recvbuff, table, stream);
}

extern "C" mccsResult_t mccsSend(const void* sendbuff, size_t count, int dtype, int peer, mccsComm_t comm,
                                 hipStream_t stream) {
  return launch_sendrecv((Comm*)comm, true, const_cast<void*>(sendbuff), count, dtype, peer, stream);
}

extern "C" mccsResult_t mccsRecv(void* recvbuff, size_t count, int dtype, int peer, mccsComm_t comm,
                                 hipStream_t stream) {
  return launch_sendrecv((Comm*)comm, false, recvbuff, count, dtype, peer, stream);
}

// The word of a size table (ring_walk.h a2avd_index), for the tests' own table builder.
extern "C" long long mccs_a2avd_index(int row, int nranks, int peer) {
  if (row < 0 || row >= kA2AvdRows || nranks < 1 || peer < 0 || peer >= nranks) return -1;
  return (long long)a2avd_index(row, nranks, peer);
}

extern "C" mccsResult_t mccsCommAllToAllLLMax(mccsComm_t comm, size_t* cap) {
  err_clear();
  const Comm* c = (const Comm*)comm;
  if (!c || !cap) MCCS_FAIL(mccsInvalidArgument, "mccsCommAllToAllLLMax: null communicator or output");
  *cap = c->connected ? a2a_ll_cap(c) : 0;
  return mccsSuccess;
}

extern "C" mccsResult_t mccsCommSetAllToAllLL(mccsComm_t comm, size_t bytes_per_peer, size_t v_bytes_per_peer) {
  err_clear();
  StepScope st("mccsCommSetAllToAllLL");
  Comm* c = (Comm*)comm;
  if (!c || !c->connected) MCCS_FAIL(mccsInvalidUsage, "the communicator is not connected");
  if (g_group.depth > 0 || c->plan_pending)
    MCCS_FAIL(mccsInvalidUsage, "the communicator has a group open or a call pending: set the limits between launches");
  const size_t cap = a2a_ll_cap(c);
  if (bytes_per_peer > cap || v_bytes_per_peer > cap)
    MCCS_FAIL(mccsInvalidArgument, "%s %zu is above the %zu bytes one pair can move through its LL slot%s",
              bytes_per_peer > cap ? "bytes_per_peer" : "v_bytes_per_peer",
              bytes_per_peer > cap ? bytes_per_peer : v_bytes_per_peer, cap,
              cap ? "" : " (no LL slots, a cached arena or system-scope fences: the LL path is closed here)");
  c->a2a_ll_bytes = bytes_per_peer;
  c->a2av_ll_bytes = v_bytes_per_peer;
  a2a_ll_prepare(c);
  return mccsSuccess;
}

extern "C" mccsResult_t mccsCommReduceScatterDirectMax(mccsComm_t comm, size_t* cap, size_t* ll_cap) {
  err_clear();
  const Comm* c = (const Comm*)comm;
  if (!c || !cap || !ll_cap) MCCS_FAIL(mccsInvalidArgument, "mccsCommReduceScatterDirectMax: null communicator or output");
  *cap = c->connected ? rs_direct_cap(c) : 0;
  *ll_cap = c->connected ? rs_ll_cap(c) : 0;
  return mccsSuccess;
}

extern "C" mccsResult_t mccsCommSetReduceScatterDirect(mccsComm_t comm, size_t block_bytes, size_t ll_block_bytes) {
  err_clear();
  StepScope st("mccsCommSetReduceScatterDirect");
  Comm* c = (Comm*)comm;
  if (!c || !c->connected) MCCS_FAIL(mccsInvalidUsage, "the communicator is not connected");
  if (g_group.depth > 0 || c->plan_pending)
    MCCS_FAIL(mccsInvalidUsage, "the communicator has a group open or a call pending: set the limits between launches");
  const size_t cap = rs_direct_cap(c), ll_cap = rs_ll_cap(c);
  if (block_bytes > cap)
    MCCS_FAIL(mccsInvalidArgument, "block_bytes %zu is above the %zu bytes of a one-shot slot%s", block_bytes, cap,
              cap ? "" : " (no one-shot slots or no peer atomics: the count-based path is closed here)");
  if (ll_block_bytes > ll_cap)
    MCCS_FAIL(mccsInvalidArgument, "ll_block_bytes %zu is above the %zu bytes one block can move through an LL slot%s",
              ll_block_bytes, ll_cap,
              ll_cap ? "" : " (no LL slots, a cached arena or system-scope fences: the LL path is closed here)");
  c->rs_direct_bytes = block_bytes;
  c->rs_ll_bytes = ll_block_bytes;
  rs_direct_prepare(c);
  return mccsSuccess;
}

extern "C" mccsResult_t mccsCommRootedDirectMax(mccsComm_t comm, size_t* cap, size_t* ll_cap) {
  err_clear();
  const Comm* c = (const Comm*)comm;
  if (!c || !cap || !ll_cap) MCCS_FAIL(mccsInvalidArgument, "mccsCommRootedDirectMax: null communicator or output");
  *cap = c->connected ? rs_direct_cap(c) : 0;
  *ll_cap = c->connected ? rs_ll_cap(c) : 0;
  return mccsSuccess;
}

extern "C" mccsResult_t mccsCommSetRootedDirect(mccsComm_t comm, size_t bcast_bytes, size_t bcast_ll_bytes,
                                                size_t reduce_bytes, size_t reduce_ll_bytes) {
  err_clear();
  StepScope st("mccsCommSetRootedDirect");
  Comm* c = (Comm*)comm;
  if (!c || !c->connected) MCCS_FAIL(mccsInvalidUsage, "the communicator is not connected");
  if (g_group.depth > 0 || c->plan_pending)
    MCCS_FAIL(mccsInvalidUsage, "the communicator has a group open or a call pending: set the limits between launches");
  const size_t cap = rs_direct_cap(c), ll_cap = rs_ll_cap(c);
  const struct {
    const char* name;
    size_t v;
    bool ll;
  } lim[4] = {{"bcast_bytes", bcast_bytes, false},
              {"bcast_ll_bytes", bcast_ll_bytes, true},
              {"reduce_bytes", reduce_bytes, false},
              {"reduce_ll_bytes", reduce_ll_bytes, true}};
  for (const auto& l : lim) {
    if (!l.ll && l.v > cap)
      MCCS_FAIL(mccsInvalidArgument, "%s %zu is above the %zu bytes of a one-shot slot%s", l.name, l.v, cap,
                cap ? "" : " (no one-shot slots or no peer atomics: the count-based path is closed here)");
    if (l.ll && l.v > ll_cap)
      MCCS_FAIL(mccsInvalidArgument, "%s %zu is above the %zu bytes one buffer can move through an LL slot%s", l.name,
                l.v, ll_cap,
                ll_cap ? "" : " (no LL slots, a cached arena or system-scope fences: the LL path is closed here)");
  }
  c->bc_direct_bytes = bcast_bytes;
  c->bc_ll_bytes = bcast_ll_bytes;
  c->rd_direct_bytes = reduce_bytes;
  c->rd_ll_bytes = reduce_ll_bytes;
  rs_direct_prepare(c);
  return mccsSuccess;
}

extern "C" mccsResult_t mccsCommAllToAllRoute(mccsComm_t comm, int* info2) {
  const Comm* c = (const Comm*)comm;
  if (!c || !info2) return mccsInvalidArgument;
  info2[0] = c->a2a_hops;
  info2[1] = c->a2a_m;
  return mccsSuccess;
}

extern "C" mccsResult_t mccsAllReduceOpArg(const void* sendbuff, void* recvbuff, size_t count, int dtype, int op,
                                           uint64_t op_arg, mccsComm_t comm, hipStream_t stream) {
  return launch_single((Comm*)comm, mccsFuncAllReduce, dtype, op, sendbuff, recvbuff, count, stream, 0, &op_arg);
}

extern "C" mccsResult_t mccsReduceScatterOpArg(const void* sendbuff, void* recvbuff, size_t recvcount, int dtype,
                                               int op, uint64_t op_arg, mccsComm_t comm, hipStream_t stream) {
  return launch_single((Comm*)comm, mccsFuncReduceScatter, dtype, op, sendbuff, recvbuff, recvcount, stream, 0,
                       &op_arg);
}

extern "C" mccsResult_t mccsReduceOpArg(const void* sendbuff, void* recvbuff, size_t count, int dtype, int op,
                                        uint64_t op_arg, int root, mccsComm_t comm, hipStream_t stream) {
  return launch_single((Comm*)comm, mccsFuncReduce, dtype, op, sendbuff, recvbuff, count, stream, root, &op_arg);
}

extern "C" mccsResult_t mccsRedOpArgFromDouble(int dtype, double v, uint64_t* op_arg) {
  err_clear();
  if (!op_arg || dtype < 0 || dtype >= mccsNumTypes) MCCS_FAIL(mccsInvalidArgument, "unknown dtype or null op_arg");
  uint64_t bits = 0;
  switch (dtype) {
    case mccsFloat64: std::memcpy(&bits, &v, 8); break;
    case mccsFloat32: {
      const float f = (float)v;
      std::memcpy(&bits, &f, 4);
      break;
    }
    // two roundings: to binary32, then to the 16-bit type (nearest even both times)
    case mccsFloat16: bits = f2h((float)v); break;
    case mccsBfloat16: bits = f2b((float)v); break;
    default: {
      const int w = 8 * elem_bytes(dtype);
      const bool sgn = dtype == mccsInt8 || dtype == mccsInt32 || dtype == mccsInt64;
      const double lo = sgn ? -std::ldexp(1.0, w - 1) : 0.0, hi = std::ldexp(1.0, sgn ? w - 1 : w);  // [lo, hi)
      if (!(v >= lo && v < hi) || v != std::floor(v))
        MCCS_FAIL(mccsInvalidArgument, "%g is not an integer the dtype can hold", v);
      bits = sgn ? (uint64_t)(int64_t)v : (uint64_t)v;
      if (w < 64) bits &= (1ull << w) - 1;
    }
  }
  *op_arg = bits;
  return mccsSuccess;
}

extern "C" mccsResult_t mccsAvgOp(int dtype, int nranks, int* op, uint64_t* op_arg) {
  err_clear();
  if (!op || !op_arg || dtype < 0 || dtype >= mccsNumTypes || nranks < 1)
    MCCS_FAIL(mccsInvalidArgument, "unknown dtype, nranks < 1 or null output");
  if (is_integer_dtype(dtype)) {  // NCCL's mapping: integers divide the finished sum
    *op = mccsDevSumPostDiv;
    *op_arg = (uint64_t)nranks;
    return mccsSuccess;
  }
  *op = mccsDevPreMulSum;
  if (dtype == mccsFloat64) {
    const double s = 1.0 / nranks;
    std::memcpy(op_arg, &s, 8);
    return mccsSuccess;
  }
  const float s = 1.0f / (float)nranks;
  uint32_t b;
  std::memcpy(&b, &s, 4);
  *op_arg = dtype == mccsFloat32 ? b : dtype == mccsFloat16 ? f2h(s) : f2b(s);
  return mccsSuccess;
}

extern "C" mccsResult_t mccsGroupStart(void) {
  if (g_group.depth++ == 0) err_clear();
  return mccsSuccess;
}

extern "C" mccsResult_t mccsGroupEnd(void) {
  if (g_group.depth <= 0) {
    err_clear();
    MCCS_FAIL(mccsInvalidUsage, "mccsGroupEnd without mccsGroupStart");
  }
  if (--g_group.depth > 0) return mccsSuccess;
  if (g_group.error != mccsSuccess) {  // a collective of the group was rejected: launch none
    const mccsResult_t e = g_group.error;
    g_group.error = mccsSuccess;
    group_discard();
    return e;
  }
  StepScope st("mccsGroupEnd launch");
  mccsResult_t r = plan_launch_group(g_group.comms, g_group.streams);
  group_discard();  // plans not launched after an error are dropped, not left queued
  return r;
}

extern "C" mccsResult_t mccsCommSync(mccsComm_t comm) {
  err_clear();
  StepScope st0("mccsCommSync");
  Comm* c = (Comm*)comm;
  if (!c) return mccsInvalidArgument;
  DeviceGuard g(c->device);
  // the latest launch recorded the comm event only if something consumes it
  // (plan.cpp); else the event of the comm it was fused with; else wait for
  // every stream of the device, a superset
  MCCS_HIP(comm_wait_last_launch(c));
  if (c->stream) MCCS_HIP(rt().StreamSynchronize(c->stream));
  // the communicator's abort line: word 0 abortFlag, word 1 the error bits its
  // kernels reported (ring_cfg.h), so another communicator's failure never
  // shows up here
  const uint32_t abort_val = __atomic_load_n(c->h_abort, __ATOMIC_ACQUIRE);
  const uint32_t err = __atomic_load_n(c->h_abort + 1, __ATOMIC_ACQUIRE);
  if (err || abort_val) c->failed = true;
  if (err & MCCS_ERR_TIMEOUT)
    MCCS_FAIL(mccsTimeout, "rank %d: a FIFO wait passed the %d ms watchdog (error bits 0x%x)", c->rank,
              c->cfg.timeout_ms == 0 ? kDefaultTimeoutMs : c->cfg.timeout_ms, err);
  if (err || abort_val) MCCS_FAIL(mccsRemoteError, "rank %d: abortFlag %u, error bits 0x%x", c->rank, abort_val, err);
  return mccsSuccess;
}

extern "C" mccsResult_t mccsCommAbort(mccsComm_t comm) {
  Comm* c = (Comm*)comm;
  if (!c) return mccsInvalidArgument;
  c->failed = true;
  // a CPU store into the host-mapped line: no stream, so nothing can queue it
  // behind the kernel it must stop (comm.cpp place_abort_line)
  if (c->h_abort) __atomic_store_n(c->h_abort, 1u, __ATOMIC_SEQ_CST);
  return mccsSuccess;
}

extern "C" mccsResult_t mccsCommDestroy(mccsComm_t comm) {
  Comm* c = (Comm*)comm;
  if (!c) return mccsInvalidArgument;
  comm_free(c);
  delete c;
  return mccsSuccess;
}

extern "C" mccsResult_t mccsCommInfo(mccsComm_t comm, int* info) {
  Comm* c = (Comm*)comm;
  if (!c || !info) return mccsInvalidArgument;
  info[0] = c->rank;
  info[1] = c->nranks;
  info[2] = c->device;
  info[3] = c->nch;
  info[4] = c->lanes;
  info[5] = c->block_threads;
  // the hand-off the launches run (after any node-gate step-down)
  info[6] = c->kcfg.fence_mode == MCCS_FENCE_SYSTEM             ? MCCS_FIFO_DEVICE
            : c->kcfg.fence_mode == MCCS_FENCE_UNCACHED_RELEASE ? MCCS_FIFO_UNCACHED_RELEASE
                                                                : MCCS_FIFO_UNCACHED;
  return mccsSuccess;
}

extern "C" mccsResult_t mccsCommRing(mccsComm_t comm, int ch, int* order) {
  Comm* c = (Comm*)comm;
  if (!c || !order || ch < 0 || ch >= c->nch) return mccsInvalidArgument;
  for (int i = 0; i < c->nranks; ++i) order[i] = c->rings[ch][i];
  return mccsSuccess;
}

extern "C" int mccsCommLastAlgo(mccsComm_t comm) {
  const Comm* c = (const Comm*)comm;
  return c ? c->last_algo : -1;
}

extern "C" int mccsCommDirectEnabled(mccsComm_t comm) {
  const Comm* c = (const Comm*)comm;
  return c && c->direct_ok && (c->layout.direct_slot > 0 || c->layout.oneshot_slot > 0 || c->layout.ll_slot > 0);
}

extern "C" mccsResult_t mccsCommGuardInfo(mccsComm_t comm, uint64_t* out4) {
  Comm* c = (Comm*)comm;
  if (!c || !out4 || !c->d_guard) return mccsInvalidArgument;
  DeviceGuard g(c->device);
  mccsLaunchGuard line;
  MCCS_HIP(rt().Memcpy(&line, c->d_guard, sizeof(line), hipMemcpyDeviceToHost));
  out4[0] = line.word >> MCCS_GUARD_TOK_SHIFT;
  out4[1] = (line.word & MCCS_GUARD_CONFIRMED) ? 1 : 0;
  out4[2] = line.word & MCCS_GUARD_FIN_MASK;
  out4[3] = line.waits;
  return mccsSuccess;
}

extern "C" mccsResult_t mccsCommDevComm(mccsComm_t comm, void** dev_comm) {
  Comm* c = (Comm*)comm;
  if (!c || !dev_comm) return mccsInvalidArgument;
  *dev_comm = c->d_comm;
  return mccsSuccess;
}

extern "C" const char* mccsGetErrorString(mccsResult_t r) {
  switch (r) {
    case mccsSuccess: return "no error";
    case mccsUnhandledCudaError: return "unhandled HIP error";
    case mccsSystemError: return "system error";
    case mccsInternalError: return "internal error";
    case mccsInvalidArgument: return "invalid argument";
    case mccsInvalidUsage: return "invalid usage";
    case mccsRemoteError: return "remote process exited or the kernel aborted";
    case mccsInProgress: return "in progress";
    case mccsTimeout: return "FIFO watchdog timeout";
    default: return "unknown result";
  }
}

// Pure host helpers, usable without a GPU (tests, tools).
extern "C" int mccs_default_rings(int nranks, int nch_req, int* out, int max_channels) {
  std::vector<std::vector<int>> rings;
  default_rings(nranks, nch_req, &rings);
  int n = std::min((int)rings.size(), max_channels);
  for (int c = 0; c < n; ++c)
    for (int i = 0; i < nranks; ++i) out[c * nranks + i] = rings[c][i];
  return n;
}

extern "C" mccsResult_t mccs_alltoall_route(int nranks, int nchannels, const int* rings, int force_relay, int* hops,
                                            int* m, int* send_bid, int* recv_bid) {
  if (nranks < 1 || nranks > 64 || nchannels < 1 || nchannels > MCCS_MAX_NCHANNELS || !hops || !m)
    return mccsInvalidArgument;
  std::vector<int> ident;
  if (!rings) {  // identity order on every channel, as for the host rings
    for (int c = 0; c < nchannels; ++c)
      for (int i = 0; i < nranks; ++i) ident.push_back(i);
    rings = ident.data();
  }
  for (int c = 0; c < nchannels; ++c) {
    std::vector<int> s(rings + (size_t)c * nranks, rings + (size_t)(c + 1) * nranks);
    std::sort(s.begin(), s.end());
    for (int i = 0; i < nranks; ++i)
      if (s[i] != i) return mccsInvalidArgument;  // not a permutation
  }
  alltoall_route(nranks, nchannels, rings, force_relay != 0, hops, m, send_bid, recv_bid);
  return mccsSuccess;
}

extern "C" int mccs_ll_default(int nranks) { return default_ll_bytes(nranks); }

extern "C" void mccs_direct_defaults(int nranks, int* oneshot_bytes, int* direct_bytes) {
  if (oneshot_bytes) *oneshot_bytes = default_oneshot_bytes(nranks);
  if (direct_bytes) *direct_bytes = default_direct_bytes(nranks);
}

extern "C" void mccs_task_schema(size_t total_bytes, int nch_cfg, int* nch, int* nthreads) {
  task_schema(total_bytes, nch_cfg, nch, nthreads);
}

// The chunk walk of one work element as every kernel and host path takes it
// (ring_walk.h), one row {gridOffset, realChunkSize, chunk offset, nelem} per
// loop and part; nelem is 0 for a part past the end of the buffer.
template <typename I>
static long long ring_walk_rows(int func, int nranks, int nch, int esize, int nthr, int buff_size, size_t count,
                                long long* rows, long long max_rows) {
  RingWalk<I> w;
  ring_walk<I>(w, func, nranks, nch, esize, nthr, buff_size, (I)count);
  walk_guard(w);
  const I parts = walk_parts<I>(func, nch, nranks);
  long long n = 0;
  for (I g = 0; g < w.size; g += w.loopSize) {
    const I rcs = real_chunk_size(w, g, parts);
    for (I c = 0; c < parts; ++c, ++n) {
      const I off = func == mccsFuncAllReduce ? allreduce_chunk_offset(g, c, rcs) : block_chunk_offset(g, c, rcs);
      if (n >= max_rows) continue;
      const long long row[4] = {(long long)g, (long long)rcs, (long long)off,
                                off < w.size ? (long long)chunk_nelem(w.size, off, rcs) : 0};
      std::memcpy(rows + 4 * n, row, sizeof(row));
    }
  }
  return n;
}

extern "C" long long mccs_ring_walk(int func, int nranks, int nchannels, int elem_bytes, int nthreads_ref,
                                    int buff_size, size_t count, int width, long long* rows, long long max_rows) {
  if ((func != mccsFuncAllReduce && func != mccsFuncAllGather && func != mccsFuncReduceScatter) || nranks < 1 ||
      nchannels < 1 || nchannels > MCCS_MAX_NCHANNELS || elem_bytes < 1 || nthreads_ref <= WARP_SIZE ||
      buff_size < 8192 || buff_size % 8192 || (width != 32 && width != 64) || (max_rows > 0 && !rows) ||
      (width == 32 && count > 0x7fffffffu))
    return -1;
  return width == 32 ? ring_walk_rows<uint32_t>(func, nranks, nchannels, elem_bytes, nthreads_ref, buff_size, count,
                                                rows, max_rows)
                     : ring_walk_rows<int64_t>(func, nranks, nchannels, elem_bytes, nthreads_ref, buff_size, count,
                                               rows, max_rows);
}

// Ring profile counters of `device` (MCCS_RING_PROFILE=1 at communicator
// init arms them): out[0] slices, out[1] wait ticks, out[2] work ticks
// (s_memrealtime, 100 MHz), out[3] reserved.
extern "C" mccsResult_t mccs_ring_profile(int device, unsigned long long* out4, int reset) {
  if (!out4) return mccsInvalidArgument;
  DeviceGuard g(device);
  MCCS_HIP(ring_read_profile(out4, reset != 0));
  return mccsSuccess;
}
