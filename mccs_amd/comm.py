"""Communicators and collectives: the Python face of libmccs.

Mirrors the reference application API (src/libmccs/src/lib.rs:19-27):

  reference (Rust libmccs)                      here
  ------------------------------------------    ---------------------------------------------
  init_communicator_rank(id, rank, n, dev, ip)  init_communicator_rank(rank, n, dev, exchange)
  all_reduce(comm, send, recv, size, dtype,     all_reduce(comm, send, recv, size, dtype,
             op, stream) -> Result<(), Error>              op, stream)  (raises MccsError)
  all_gather(comm, send, recv, size, stream)    all_gather(comm, send, recv, size, stream)
  (none: ReduceScatter is declared but          reduce_scatter(comm, send, recv, recv_count, dtype,
   unimplemented, task.rs:95-102)                              op, stream)
  (none: no all-to-all)                         all_to_all(comm, send, recv, nbytes, stream)
  (none)                                        all_to_all_v(comm, send, scounts, sdispls, recv, rcounts, rdispls, stream)
  (none)                                        all_to_all_v_dev(comm, send, recv, table, stream): sizes on the device
  (none: SendRecv ids reserved, no kernel)      send / recv(comm, buf, count, dtype, peer, stream), batch_send_recv
  (none: Broadcast and Reduce are declared,     broadcast(comm, send, recv, nbytes, root, stream)
   devcomm.h:11-12, and have no kernel)         reduce(comm, send, recv, count, dtype, op, root, stream)
  AllReduceDataType {Float16, Int32}            AllReduceDataType (+ Float32: the one API delta,
                                                SURVEY §8(b); + the other kernel dtypes)
  AllReduceOpType {Sum, Prod, ...}              AllReduceOpType

`size` is an element count (src/ipc/mccs/src/command.rs:71-80).  Everything
below is a thin ctypes layer over include/mccs_hip.h; the work happens in
libmccs_hip.so (HIP kernels + C++ planner).  There is no fallback path.
"""
from __future__ import annotations

import contextlib
import ctypes
import math
import enum
import time
from dataclasses import dataclass

from . import _lib
from ._lib import DataType, RedOp, _CommConfig

_P = ctypes.POINTER
_vp, _ci, _sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t


class AllReduceDataType(enum.IntEnum):
    """ipc::mccs::command::AllReduceDataType (command.rs:28-31) + Float32 and the
    remaining kernel dtypes; values are mccsDevDataType_t codes."""

    Float16 = DataType.Float16
    Int32 = DataType.Int32
    Float32 = DataType.Float32
    Int8 = DataType.Int8
    Uint8 = DataType.Uint8
    Uint32 = DataType.Uint32
    Int64 = DataType.Int64
    Uint64 = DataType.Uint64
    Float64 = DataType.Float64
    Bfloat16 = DataType.Bfloat16


class AllReduceOpType(enum.IntEnum):
    """command.rs:33-42.  PreMulSum and SumPostDiv take an argument (`op_arg=`
    of all_reduce / reduce_scatter / reduce: the scalar in the element type's
    bits, red_op_arg(); the divisor): the ring kernels implement both
    (PreMulSum for every dtype, SumPostDiv for the integer ones).  avg_op()
    maps the average onto them."""

    Sum = 0
    Prod = 1
    Max = 2
    Min = 3
    PreMulSum = 4
    SumPostDiv = 5


LOCALITY_SENDER, LOCALITY_RECEIVER = 0, 1
# MCCS_FIFO_*: uncached arena (relaxed hand-offs), plain device arena
# (system-scope release/acquire), uncached arena + release fence before posts
FIFO_UNCACHED, FIFO_DEVICE, FIFO_UNCACHED_RELEASE = 0, 1, 2


@dataclass
class CommConfig:
    """comm_default_config (mccs.toml:18-20) + MI355X knobs.  None = the
    library default (mccsCommConfigDefault, which also honours the MCCS_*
    environment overrides)."""

    channel_count: int | None = None
    buffer_size: int | None = None
    lanes: int | None = None
    block_threads: int | None = None
    locality: int | None = None
    fifo_memory: int | None = None
    timeout_ms: int | None = None
    work_fifo_depth: int | None = None
    bridge_streams: int | None = None
    rings: list | None = None  # comm_patterns_override: channel_count x nranks send orders
    fifo_slots: int | None = None  # FIFO slots per connection: 8 (reference), 16, 32
    direct_bytes: int | None = None  # largest bucket (bytes per rank) for the direct two-shot kernel; < 0 never
    oneshot_bytes: int | None = None  # largest bucket for the one-shot variant; < 0 never
    ll_bytes: int | None = None  # largest bucket for the LL one-shot (uncached arenas); < 0 never

    def to_c(self, nranks: int):
        c = _CommConfig()
        _lib.load().mccsCommConfigDefault(ctypes.byref(c))
        for f, _ in _CommConfig._fields_:
            if f in ("rings", "reserved"):
                continue
            v = getattr(self, f)
            if v is not None:
                setattr(c, f, int(v))
        keep = None
        if self.rings is not None:
            flat = [int(x) for ring in self.rings for x in ring]
            if len(flat) != len(self.rings) * nranks:
                raise ValueError("each ring must list every rank once")
            keep = (_ci * len(flat))(*flat)
            c.rings = ctypes.cast(keep, _P(_ci))
            c.channel_count = len(self.rings)
        return c, keep


def _sig():
    return _lib.load()


def _ptr(x) -> int:
    if x is None:  # the buffer a rooted collective's role does not use
        return 0
    return x.data_ptr() if hasattr(x, "data_ptr") else int(x)


def _u64(x) -> int:
    """An op argument as the C-ABI's uint64_t (a negative Python int is taken in two's complement)."""
    return int(x) & 0xFFFFFFFFFFFFFFFF


def _stream(s) -> int:
    if s is None:
        import torch

        return torch.cuda.current_stream().cuda_stream
    return s.cuda_stream if hasattr(s, "cuda_stream") else int(s)


class Communicator:
    """One rank of a communicator (reference: MccsCommunicatorHandle)."""

    def __init__(self, handle: int):
        self._h = ctypes.c_void_p(handle)
        self._load_info()

    def _load_info(self) -> None:
        """(Re)reads the comm's profile; mccsCommConnect may shrink the lanes of
        co-located processes and settle the hand-off mode."""
        info = (_ci * 7)()
        _lib.check(_sig().mccsCommInfo(self._h, info), "mccsCommInfo")
        (self.rank, self.nranks, self.device, self.nchannels, self.lanes, self.block_threads,
         self.fifo_memory) = list(info)

    @property
    def handle(self) -> int:
        return self._h.value

    def gate_info(self) -> dict:
        """Outcome of the node gate (mccsCommGateInfo): whether it ran, the
        hand-off the comm now runs (MCCS_FIFO_*), the MCCS_GATE_* bits that
        failed and the direct variants it disabled."""
        info = (ctypes.c_int * 4)()
        _lib.check(_sig().mccsCommGateInfo(self._h, info), "mccsCommGateInfo")
        return {"ran": bool(info[0]), "fifo_mode": info[1], "failed": info[2], "disabled": info[3]}

    def guard_info(self) -> dict:
        """The comm's launch guard (mccsCommGuardInfo, launch_guard.h): the
        holder's token (0 = free), the fused-launch confirm word, finished
        workgroups of the holder, and how many workgroups ever waited for
        another launch of this comm."""
        out = (ctypes.c_uint64 * 4)()
        _lib.check(_sig().mccsCommGuardInfo(self._h, out), "mccsCommGuardInfo")
        return {"owner": out[0], "confirm": out[1], "fin": out[2], "waits": out[3]}

    def rings(self) -> list[list[int]]:
        out = []
        for ch in range(self.nchannels):
            arr = (_ci * self.nranks)()
            _lib.check(_sig().mccsCommRing(self._h, ch, arr), "mccsCommRing")
            out.append(list(arr))
        return out

    def last_algo(self) -> str | None:
        """"ring", "direct" (two-shot) or "oneshot": the algorithm of the latest
        launch (None before one)."""
        a = _sig().mccsCommLastAlgo(self._h)
        return {0: "ring", 1: "direct", 2: "oneshot", 3: "ll"}.get(a)

    def direct_enabled(self) -> bool:
        """Whether AllReduces may take the direct kernel (a direct region is
        configured and every device pair supports peer atomics)."""
        return bool(_sig().mccsCommDirectEnabled(self._h))

    def dev_comm(self) -> int:
        p = ctypes.c_void_p()
        _lib.check(_sig().mccsCommDevComm(self._h, ctypes.byref(p)), "mccsCommDevComm")
        return p.value

    def all_reduce(self, send_buf, recv_buf, size: int, data_type=AllReduceDataType.Float32,
                   op_type=AllReduceOpType.Sum, stream=None, op_arg: int | None = None) -> None:
        all_reduce(self, send_buf, recv_buf, size, data_type, op_type, stream, op_arg=op_arg)

    def all_gather(self, send_buf, recv_buf, size: int, stream=None) -> None:
        all_gather(self, send_buf, recv_buf, size, stream)

    def reduce_scatter(self, send_buf, recv_buf, recv_count: int, data_type=AllReduceDataType.Float32,
                       op_type=AllReduceOpType.Sum, stream=None, op_arg: int | None = None) -> None:
        reduce_scatter(self, send_buf, recv_buf, recv_count, data_type, op_type, stream, op_arg=op_arg)

    def broadcast(self, send_buf, recv_buf, nbytes: int, root: int, stream=None) -> None:
        broadcast(self, send_buf, recv_buf, nbytes, root, stream)

    def reduce(self, send_buf, recv_buf, count: int, data_type=AllReduceDataType.Float32,
               op_type=AllReduceOpType.Sum, root: int = 0, stream=None, op_arg: int | None = None) -> None:
        reduce(self, send_buf, recv_buf, count, data_type, op_type, root, stream, op_arg=op_arg)

    def all_to_all(self, send_buf, recv_buf, nbytes: int, stream=None) -> None:
        all_to_all(self, send_buf, recv_buf, nbytes, stream)

    def all_to_all_v(self, send_buf, send_counts, send_displs, recv_buf, recv_counts, recv_displs,
                     stream=None) -> None:
        all_to_all_v(self, send_buf, send_counts, send_displs, recv_buf, recv_counts, recv_displs, stream)

    def all_to_all_v_dev(self, send_buf, recv_buf, table, stream=None) -> None:
        all_to_all_v_dev(self, send_buf, recv_buf, table, stream)

    def exchange_counts(self, table, stream=None) -> None:
        exchange_counts(self, table, stream)

    def send(self, buf, count: int, data_type=AllReduceDataType.Uint8, peer: int = 0, stream=None) -> None:
        send(self, buf, count, data_type, peer, stream)

    def recv(self, buf, count: int, data_type=AllReduceDataType.Uint8, peer: int = 0, stream=None) -> None:
        recv(self, buf, count, data_type, peer, stream)

    def set_all_to_all_ll(self, bytes_per_peer: int = 0, v_bytes_per_peer: int = 0) -> None:
        """mccsCommSetAllToAllLL: opts the communicator in to the LL all-to-all
        (0 = off, the default).  bytes_per_peer: an all_to_all of at most that
        many bytes per peer that is the communicator's only call of its launch
        takes the LL kernel (last_algo() == "ll").  v_bytes_per_peer: the
        caller's promise that no count of any all_to_all_v / all_to_all_v_dev
        call on any rank exceeds it; every such single call then takes the LL
        kernel, on any route, and always launches.  Every rank must set the
        same two values, each at most all_to_all_ll_max()."""
        rc = _sig().mccsCommSetAllToAllLL(self._h, int(bytes_per_peer), int(v_bytes_per_peer))
        _lib.check(rc, "mccsCommSetAllToAllLL")

    def all_to_all_ll_max(self) -> int:
        """mccsCommAllToAllLLMax: the most bytes one pair can move through its
        LL slot in one launch (ll_bytes - 8); 0 where the LL lines cannot be
        used (no LL slots, a cached arena, system-scope fences)."""
        cap = ctypes.c_size_t(0)
        _lib.check(_sig().mccsCommAllToAllLLMax(self._h, ctypes.byref(cap)), "mccsCommAllToAllLLMax")
        return int(cap.value)

    def set_reduce_scatter_direct(self, block_bytes: int = 0, ll_block_bytes: int = 0) -> None:
        """mccsCommSetReduceScatterDirect: opts the communicator in to the direct
        ReduceScatter (0 = off, the default).  Both limits are bytes per block
        (recv_count x element size).  A reduce_scatter of Sum / Prod / Max / Min
        that is the communicator's only call of its launch takes the LL kernel
        when its block is within ll_block_bytes (last_algo() == "ll"), else the
        count-based one within block_bytes ("oneshot"); the result is the
        ring's bit for bit.  Every rank must set the same two values, each at
        most its reduce_scatter_direct_max()."""
        rc = _sig().mccsCommSetReduceScatterDirect(self._h, int(block_bytes), int(ll_block_bytes))
        _lib.check(rc, "mccsCommSetReduceScatterDirect")

    def reduce_scatter_direct_max(self) -> tuple[int, int]:
        """mccsCommReduceScatterDirectMax: (cap, ll_cap), the largest block in
        bytes of the count-based and of the LL variant; 0 where one cannot be
        used (no slots or no peer atomics; no LL slots, a cached arena,
        system-scope fences)."""
        cap, ll_cap = ctypes.c_size_t(0), ctypes.c_size_t(0)
        _lib.check(_sig().mccsCommReduceScatterDirectMax(self._h, ctypes.byref(cap), ctypes.byref(ll_cap)),
                   "mccsCommReduceScatterDirectMax")
        return int(cap.value), int(ll_cap.value)

    def set_rooted_direct(self, bcast_bytes: int = 0, bcast_ll_bytes: int = 0, reduce_bytes: int = 0,
                          reduce_ll_bytes: int = 0) -> None:
        """mccsCommSetRootedDirect: opts the communicator in to the direct
        Broadcast and Reduce (0 = off, the default).  The four limits are bytes
        of the whole buffer.  A broadcast, or a reduce of Sum / Prod / Max / Min,
        that is the communicator's only call of its launch takes the LL kernel
        when it is within its function's LL limit (last_algo() == "ll"), else
        the count-based one within the other ("oneshot"); the result is the
        ring's bit for bit.  Every rank must set the same four values, each at
        most its rooted_direct_max()."""
        rc = _sig().mccsCommSetRootedDirect(self._h, int(bcast_bytes), int(bcast_ll_bytes), int(reduce_bytes),
                                            int(reduce_ll_bytes))
        _lib.check(rc, "mccsCommSetRootedDirect")

    def rooted_direct_max(self) -> tuple[int, int]:
        """mccsCommRootedDirectMax: (cap, ll_cap), the largest buffer in bytes
        of the count-based and of the LL variant; 0 where one cannot be used
        (no slots or no peer atomics; no LL slots, a cached arena, system-scope
        fences)."""
        cap, ll_cap = ctypes.c_size_t(0), ctypes.c_size_t(0)
        _lib.check(_sig().mccsCommRootedDirectMax(self._h, ctypes.byref(cap), ctypes.byref(ll_cap)),
                   "mccsCommRootedDirectMax")
        return int(cap.value), int(ll_cap.value)

    def all_to_all_route(self) -> dict:
        """The comm's AllToAll route (mccsCommAllToAllRoute): hops (1: every
        block goes straight to its ring successor; nranks - 1: relayed along the
        rings) and m, the channels carrying each pair's block (0 for the relay)."""
        info = (_ci * 2)()
        _lib.check(_sig().mccsCommAllToAllRoute(self._h, info), "mccsCommAllToAllRoute")
        return {"hops": info[0], "m": info[1]}

    def all_reduce_avg(self, send_buf, recv_buf, size: int, data_type=AllReduceDataType.Float32, stream=None) -> None:
        all_reduce_avg(self, send_buf, recv_buf, size, data_type, stream)

    def reduce_scatter_avg(self, send_buf, recv_buf, recv_count: int, data_type=AllReduceDataType.Float32,
                           stream=None) -> None:
        reduce_scatter_avg(self, send_buf, recv_buf, recv_count, data_type, stream)

    def reduce_avg(self, send_buf, recv_buf, count: int, data_type=AllReduceDataType.Float32, root: int = 0,
                   stream=None) -> None:
        reduce_avg(self, send_buf, recv_buf, count, data_type, root, stream)

    def sync(self) -> None:
        """Waits for the comm's launches; raises on a device-side timeout/abort."""
        _lib.check(_sig().mccsCommSync(self._h), "mccsCommSync")

    def abort(self) -> None:
        _lib.check(_sig().mccsCommAbort(self._h), "mccsCommAbort")

    def destroy(self) -> None:
        """mccsCommDestroy: frees the comm once its last launch completed.  No
        barrier with the peers is needed: the FIFO arena is reused only after
        every peer destroyed its side (include/mccs_hip.h)."""
        if self._h.value:
            _lib.check(_sig().mccsCommDestroy(self._h), "mccsCommDestroy")
            self._h = ctypes.c_void_p(0)


def init_all(devices: list[int], config: CommConfig | None = None) -> list[Communicator]:
    """One process drives len(devices) ranks (the reference's one-service-per-host
    model).  Devices may repeat: ranks sharing a GPU must issue collectives
    inside `group()` so they run as one launch."""
    lib = _sig()
    n = len(devices)
    cfg, keep = (config or CommConfig()).to_c(n)
    hs = (_vp * n)()
    devs = (_ci * n)(*devices)
    _lib.check(lib.mccsCommInitAll(hs, n, devs, ctypes.byref(cfg)), "mccsCommInitAll")
    del keep
    return [Communicator(hs[i]) for i in range(n)]


def init_communicator_rank(rank: int, nranks: int, device: int, exchange, config: CommConfig | None = None):
    """One rank per process.  `exchange(bytes) -> list[bytes]` all-gathers the
    per-rank connect handles (e.g. over torch.distributed/gloo); it replaces
    the reference's bootstrap ring + exchange engine."""
    lib = _sig()
    cfg, keep = (config or CommConfig()).to_c(nranks)
    hsize = lib.mccsConnectHandleSize()
    mine = (ctypes.c_char * hsize)()
    h = ctypes.c_void_p()
    t0 = time.perf_counter()
    rc = lib.mccsCommSetupRank(ctypes.byref(h), rank, nranks, device, ctypes.byref(cfg), mine)
    detail = _lib.last_error() if rc != 0 else ""
    t1 = time.perf_counter()
    del keep
    # every rank joins the exchange even after a local failure (its diagnosis
    # in place of a handle), so a peer's error never leaves the others blocked
    # in it, and every rank can say which rank failed and why
    allh = exchange(bytes(mine) if rc == 0 else b"ERR:" + detail.encode())
    if rc != 0:
        raise _lib.MccsError(rc, "mccsCommSetupRank", detail)
    comm = Communicator(h.value)
    if len(allh) != nranks or any(len(x) != hsize for x in allh):
        comm.destroy()
        failed = [(r, x[4:].decode(errors="replace")) for r, x in enumerate(allh) if x[:4] == b"ERR:"]
        if failed:
            raise RuntimeError("connect-handle exchange: " +
                               "; ".join(f"rank {r} failed mccsCommSetupRank: {d}" for r, d in failed))
        raise RuntimeError("connect-handle exchange: a peer sent malformed data")
    buf = ctypes.create_string_buffer(b"".join(allh), hsize * nranks)
    t2 = time.perf_counter()
    rc = lib.mccsCommConnect(h, buf)
    if rc != 0:
        detail = _lib.last_error()
        comm.destroy()
        raise _lib.MccsError(rc, "mccsCommConnect", detail)
    comm._load_info()
    # this rank's wall time per phase (the N > 1 bench line reports it per rank);
    # connect includes the node gate when it runs
    comm.connect_timing = {"setup_s": round(t1 - t0, 4), "exchange_s": round(t2 - t1, 4),
                           "connect_s": round(time.perf_counter() - t2, 4)}
    return comm


def all_reduce(comm: Communicator, send_buf, recv_buf, size: int, data_type=AllReduceDataType.Float32,
               op_type=AllReduceOpType.Sum, stream=None, op_arg: int | None = None) -> None:
    """libmccs::all_reduce (collectives.rs:75-138): stream-ordered, returns after launch.
    op_arg=None is mccsAllReduce (Sum / Prod / Max / Min); a value goes to
    mccsAllReduceOpArg, which also takes PreMulSum (op_arg: the scalar's bits,
    red_op_arg()) and SumPostDiv (op_arg: the divisor) and always runs those
    two on the ring."""
    if op_arg is None:
        rc = _sig().mccsAllReduce(_ptr(send_buf), _ptr(recv_buf), int(size), int(data_type), int(op_type),
                                  comm._h, _stream(stream))
        _lib.check(rc, "mccsAllReduce")
        return
    rc = _sig().mccsAllReduceOpArg(_ptr(send_buf), _ptr(recv_buf), int(size), int(data_type), int(op_type),
                                   _u64(op_arg), comm._h, _stream(stream))
    _lib.check(rc, "mccsAllReduceOpArg")


def all_gather(comm: Communicator, send_buf, recv_buf, size: int, stream=None) -> None:
    """libmccs::all_gather: `size` bytes per rank; recv holds nranks*size bytes."""
    rc = _sig().mccsAllGather(_ptr(send_buf), _ptr(recv_buf), int(size), comm._h, _stream(stream))
    _lib.check(rc, "mccsAllGather")


def reduce_scatter(comm: Communicator, send_buf, recv_buf, recv_count: int, data_type=AllReduceDataType.Float32,
                   op_type=AllReduceOpType.Sum, stream=None, op_arg: int | None = None) -> None:
    """mccsReduceScatter: send holds nranks * recv_count elements (block D at
    element D * recv_count); recv gets recv_count elements, the reduction of
    this rank's block over all ranks.  The ring, unless the communicator opted
    in with set_reduce_scatter_direct and the block is within a limit (then
    one direct exchange, same bits); stream-ordered.  op_arg as for all_reduce
    (mccsReduceScatterOpArg; PreMulSum / SumPostDiv always take the ring)."""
    if op_arg is None:
        rc = _sig().mccsReduceScatter(_ptr(send_buf), _ptr(recv_buf), int(recv_count), int(data_type),
                                      int(op_type), comm._h, _stream(stream))
        _lib.check(rc, "mccsReduceScatter")
        return
    rc = _sig().mccsReduceScatterOpArg(_ptr(send_buf), _ptr(recv_buf), int(recv_count), int(data_type),
                                       int(op_type), _u64(op_arg), comm._h, _stream(stream))
    _lib.check(rc, "mccsReduceScatterOpArg")


def broadcast(comm: Communicator, send_buf, recv_buf, nbytes: int, root: int, stream=None) -> None:
    """mccsBroadcast: every rank's recv[0, nbytes) becomes the root's
    send[0, nbytes).  send is read on the root only (None elsewhere); in place
    on the root is recv == send.  The ring, unless the communicator opted in
    with set_rooted_direct and nbytes is within a limit (then one direct
    exchange, same bytes); stream-ordered."""
    rc = _sig().mccsBroadcast(_ptr(send_buf), _ptr(recv_buf), int(nbytes), int(root), comm._h, _stream(stream))
    _lib.check(rc, "mccsBroadcast")


def reduce(comm: Communicator, send_buf, recv_buf, count: int, data_type=AllReduceDataType.Float32,
           op_type=AllReduceOpType.Sum, root: int = 0, stream=None, op_arg: int | None = None) -> None:
    """mccsReduce: the root's recv[0, count) gets the reduction of every rank's
    send[0, count).  recv is used on the root only (None elsewhere); in place on
    the root is recv == send.  The ring, unless the communicator opted in with
    set_rooted_direct and the buffer is within a limit (then one direct
    exchange, same bits); stream-ordered.  op_arg as for all_reduce
    (mccsReduceOpArg; PreMulSum / SumPostDiv always take the ring)."""
    if op_arg is None:
        rc = _sig().mccsReduce(_ptr(send_buf), _ptr(recv_buf), int(count), int(data_type), int(op_type), int(root),
                               comm._h, _stream(stream))
        _lib.check(rc, "mccsReduce")
        return
    rc = _sig().mccsReduceOpArg(_ptr(send_buf), _ptr(recv_buf), int(count), int(data_type), int(op_type),
                                _u64(op_arg), int(root), comm._h, _stream(stream))
    _lib.check(rc, "mccsReduceOpArg")


def all_to_all(comm: Communicator, send_buf, recv_buf, nbytes: int, stream=None) -> None:
    """mccsAllToAll: `nbytes` bytes per peer; both buffers hold nranks * nbytes
    bytes.  Afterwards rank r's recv[s*nbytes + i] is rank s's send[r*nbytes + i].
    Out of place only; stream-ordered.  The ring connections, unless the
    communicator opted in with set_all_to_all_ll and nbytes is within its
    limit: then the LL kernel (last_algo() == "ll")."""
    rc = _sig().mccsAllToAll(_ptr(send_buf), _ptr(recv_buf), int(nbytes), comm._h, _stream(stream))
    _lib.check(rc, "mccsAllToAll")


def _sizes(vals):
    if isinstance(vals, ctypes.Array) and vals._type_ is ctypes.c_size_t:  # marshalled once by the caller
        return vals
    vals = [int(v) for v in vals]
    return (ctypes.c_size_t * max(1, len(vals)))(*vals)


def all_to_all_v(comm: Communicator, send_buf, send_counts, send_displs, recv_buf, recv_counts, recv_displs,
                 stream=None) -> None:
    """mccsAllToAllv: per-peer byte counts and displacements (nranks entries
    each, in bytes).  Rank r sends send_counts[t] bytes from send + send_displs[t]
    to rank t and receives recv_counts[s] bytes from rank s at recv +
    recv_displs[s].  One-hop AllToAll routes only (all_to_all_route), unless
    set_all_to_all_ll(v_bytes_per_peer=...) sends the v calls through the LL
    kernel, which needs no route and refuses a count above that limit; out of
    place only; a buffer may be None when all its counts are 0.  A caller whose
    sizes repeat may pass ctypes c_size_t arrays, which are used as they are."""
    n = comm.nranks
    for name, a in (("send_counts", send_counts), ("send_displs", send_displs), ("recv_counts", recv_counts),
                    ("recv_displs", recv_displs)):
        if a is not None and len(a) != n:
            raise ValueError(f"{name} has {len(a)} entries for {n} ranks")
    arr = lambda a: None if a is None else _sizes(a)
    rc = _sig().mccsAllToAllv(_ptr(send_buf), arr(send_counts), arr(send_displs), _ptr(recv_buf), arr(recv_counts),
                              arr(recv_displs), comm._h, _stream(stream))
    _lib.check(rc, "mccsAllToAllv")


def _table_ptr(comm: Communicator, table) -> int:
    """A size table's address: a contiguous CUDA int64 / uint64 tensor of 4 * nranks elements, or a raw pointer."""
    if not hasattr(table, "data_ptr"):
        return 0 if table is None else int(table)
    import torch

    if table.dtype not in (torch.int64, torch.uint64):
        raise ValueError(f"the size table holds 64-bit integers, not {table.dtype}")
    if table.numel() != 4 * comm.nranks:
        raise ValueError(f"the size table has {table.numel()} elements, not 4 * {comm.nranks}")
    if not table.is_cuda or not table.is_contiguous():
        raise ValueError("the size table is a contiguous CUDA tensor")
    return table.data_ptr()


def all_to_all_v_dev(comm: Communicator, send_buf, recv_buf, table, stream=None) -> None:
    """mccsAllToAllvDev: all_to_all_v with the sizes in device memory.  table
    holds 4 * nranks 64-bit words in bytes: send counts, send displacements,
    receive counts, receive displacements (nranks each).  The kernel reads it
    when it runs, so a replayed graph moves what the table holds at that
    replay.  The host checks none of the sizes: the table must be complete
    earlier on the stream, stay unmodified until the call completes, agree
    with the peers' tables, and keep every segment inside its buffer.  Always
    launches; one-hop routes only, unless set_all_to_all_ll(v_bytes_per_peer=...)
    sends the v calls through the LL kernel (any route; a count above the
    limit is clamped on the device)."""
    rc = _sig().mccsAllToAllvDev(_ptr(send_buf), _ptr(recv_buf), _table_ptr(comm, table), comm._h, _stream(stream))
    _lib.check(rc, "mccsAllToAllvDev")


def exchange_counts(comm: Communicator, table, stream=None) -> None:
    """Fills row 2 of a size table (receive counts) from the peers' row 0
    (send counts) on the device: the uniform all_to_all of 8 bytes per peer.
    Issue it on every rank, before all_to_all_v_dev on the same stream.  Being
    an all_to_all of 8 bytes, it takes the LL kernel by itself once
    set_all_to_all_ll set a uniform limit (any bytes_per_peer >= 8)."""
    p = _table_ptr(comm, table)
    if not p:
        raise ValueError("exchange_counts needs a size table")
    all_to_all(comm, p, p + 2 * comm.nranks * 8, 8, stream)


def all_to_all_single(comm: Communicator, output, input, output_split_sizes=None, input_split_sizes=None,
                      stream=None) -> None:
    """torch.distributed.all_to_all_single's shape: splits run along dim 0 of
    contiguous tensors, packed in rank order.  No splits: dim 0 is cut evenly
    and the call is all_to_all."""
    n = comm.nranks
    if not (input.is_contiguous() and output.is_contiguous()):
        raise ValueError("all_to_all_single needs contiguous tensors")
    row = lambda t: math.prod(t.shape[1:]) * t.element_size()  # bytes of one dim-0 row
    if output_split_sizes is None and input_split_sizes is None:
        if input.shape[0] % n or output.numel() * output.element_size() != input.numel() * input.element_size():
            raise ValueError("without splits dim 0 must divide by nranks and both tensors hold the same bytes")
        all_to_all(comm, input, output, input.shape[0] // n * row(input), stream)
        return
    isp = [input.shape[0] // n] * n if input_split_sizes is None else [int(v) for v in input_split_sizes]
    osp = [output.shape[0] // n] * n if output_split_sizes is None else [int(v) for v in output_split_sizes]
    if len(isp) != n or len(osp) != n or sum(isp) != input.shape[0] or sum(osp) != output.shape[0]:
        raise ValueError("split sizes must have nranks entries that sum to dim 0")
    sc = [v * row(input) for v in isp]
    rc = [v * row(output) for v in osp]
    packed = lambda c: [sum(c[:i]) for i in range(n)]
    all_to_all_v(comm, input, sc, packed(sc), output, rc, packed(rc), stream)


def send(comm: Communicator, buf, count: int, dtype=AllReduceDataType.Uint8, peer: int = 0, stream=None) -> None:
    """mccsSend: count elements of dtype from buf to rank peer.  One-hop
    AllToAll routes only.  The k-th send of a pair matches its k-th recv;
    sends and receives inside one group() form one launch, and ranks that
    exchange with each other issue those calls in one group each."""
    _lib.check(_sig().mccsSend(_ptr(buf), int(count), int(dtype), int(peer), comm._h, _stream(stream)), "mccsSend")


def recv(comm: Communicator, buf, count: int, dtype=AllReduceDataType.Uint8, peer: int = 0, stream=None) -> None:
    """mccsRecv: count elements of dtype from rank peer into buf (see send)."""
    _lib.check(_sig().mccsRecv(_ptr(buf), int(count), int(dtype), int(peer), comm._h, _stream(stream)), "mccsRecv")


def batch_send_recv(comm: Communicator, ops, stream=None) -> None:
    """torch's batch_isend_irecv in one launch: ops is a list of ("send" |
    "recv", tensor_or_ptr, nbytes_or_count, dtype, peer), issued in order
    inside one group().  dtype None counts bytes."""
    with group():
        for kind, buf, count, dtype, peer in ops:
            if kind not in ("send", "recv"):
                raise ValueError(f"op kind {kind!r} is neither 'send' nor 'recv'")
            (send if kind == "send" else recv)(comm, buf, count, AllReduceDataType.Uint8 if dtype is None else dtype,
                                               peer, stream)


def avg_op(data_type, nranks: int) -> tuple[AllReduceOpType, int]:
    """mccsAvgOp: the (op, op_arg) that averages over nranks.  Floating types:
    PreMulSum with 1/nranks in the type's bits; integer types: SumPostDiv with
    nranks (truncating division of the finished sum).  Host-only."""
    op, arg = _ci(), ctypes.c_uint64()
    _lib.check(_sig().mccsAvgOp(int(data_type), int(nranks), ctypes.byref(op), ctypes.byref(arg)), "mccsAvgOp")
    return AllReduceOpType(op.value), int(arg.value)


def red_op_arg(data_type, value) -> int:
    """mccsRedOpArgFromDouble: `value` as a PreMulSum scalar of data_type (its
    bits in the low bytes).  float16 / bfloat16 round through binary32; an
    integer type needs an integral value in range.  Host-only."""
    arg = ctypes.c_uint64()
    _lib.check(_sig().mccsRedOpArgFromDouble(int(data_type), float(value), ctypes.byref(arg)),
               "mccsRedOpArgFromDouble")
    return int(arg.value)


def all_reduce_avg(comm: Communicator, send_buf, recv_buf, size: int, data_type=AllReduceDataType.Float32,
                   stream=None) -> None:
    """The average over the communicator's ranks (avg_op) as one AllReduce."""
    op, arg = avg_op(data_type, comm.nranks)
    all_reduce(comm, send_buf, recv_buf, size, data_type, op, stream, op_arg=arg)


def reduce_scatter_avg(comm: Communicator, send_buf, recv_buf, recv_count: int,
                       data_type=AllReduceDataType.Float32, stream=None) -> None:
    op, arg = avg_op(data_type, comm.nranks)
    reduce_scatter(comm, send_buf, recv_buf, recv_count, data_type, op, stream, op_arg=arg)


def reduce_avg(comm: Communicator, send_buf, recv_buf, count: int, data_type=AllReduceDataType.Float32,
               root: int = 0, stream=None) -> None:
    op, arg = avg_op(data_type, comm.nranks)
    reduce(comm, send_buf, recv_buf, count, data_type, op, root, stream, op_arg=arg)


@contextlib.contextmanager
def group():
    """ProxyCommand::GroupCall: collectives inside are launched together at exit."""
    lib = _sig()
    _lib.check(lib.mccsGroupStart(), "mccsGroupStart")
    try:
        yield
    finally:
        _lib.check(lib.mccsGroupEnd(), "mccsGroupEnd")


def default_rings(nranks: int, channels: int = 0) -> list[list[int]]:
    """Default ring orders (host-only; no GPU needed)."""
    out = (_ci * (32 * nranks))()
    k = _sig().mccs_default_rings(nranks, channels, out, 32)
    return [list(out[c * nranks:(c + 1) * nranks]) for c in range(k)]


def host_ring_allreduce(sendbufs, recvbufs, count: int, data_type, op_type=AllReduceOpType.Sum,
                        channels: int = 1, nthreads: int = 96, buffer_size: int = 1 << 22, rings=None,
                        op_arg: int | None = None) -> None:
    """BASELINE configs[0]: the ring protocol on host threads over host memory
    (numpy arrays or raw host pointers; no GPU)."""
    n = len(sendbufs)
    arr = ctypes.c_void_p * max(1, n)
    sp = arr(*[x.ctypes.data if hasattr(x, "ctypes") else int(x) for x in sendbufs])
    rp = arr(*[x.ctypes.data if hasattr(x, "ctypes") else int(x) for x in recvbufs])
    ro = None
    if rings is not None:
        flat = [int(v) for r in rings for v in r]
        ro = (_ci * len(flat))(*flat)
    if op_arg is not None:  # all six ops (mccs_host_ring_allreduce_oparg)
        rc = _sig().mccs_host_ring_allreduce_oparg(n, sp, rp, int(count), int(data_type), int(op_type), channels,
                                                   nthreads, buffer_size, ro, _u64(op_arg))
        _lib.check(rc, "mccs_host_ring_allreduce_oparg")
        return
    rc = _sig().mccs_host_ring_allreduce(n, sp, rp, int(count), int(data_type), int(op_type), channels, nthreads,
                                         buffer_size, ro)
    _lib.check(rc, "mccs_host_ring_allreduce")


def host_ring_reduce_scatter(sendbufs, recvbufs, recv_count: int, data_type, op_type=AllReduceOpType.Sum,
                             channels: int = 1, nthreads: int = 96, buffer_size: int = 1 << 22, rings=None,
                             op_arg: int | None = None) -> None:
    """The ring ReduceScatter schedule on host threads over host memory (numpy
    arrays or raw host pointers; no GPU): sendbufs[r] holds nranks * recv_count
    elements, recvbufs[r] recv_count."""
    n = len(sendbufs)
    arr = ctypes.c_void_p * max(1, n)
    sp = arr(*[x.ctypes.data if hasattr(x, "ctypes") else int(x) for x in sendbufs])
    rp = arr(*[x.ctypes.data if hasattr(x, "ctypes") else int(x) for x in recvbufs])
    ro = None
    if rings is not None:
        flat = [int(v) for r in rings for v in r]
        ro = (_ci * len(flat))(*flat)
    if op_arg is not None:
        rc = _sig().mccs_host_ring_reduce_scatter_oparg(n, sp, rp, int(recv_count), int(data_type), int(op_type),
                                                        channels, nthreads, buffer_size, ro, _u64(op_arg))
        _lib.check(rc, "mccs_host_ring_reduce_scatter_oparg")
        return
    rc = _sig().mccs_host_ring_reduce_scatter(n, sp, rp, int(recv_count), int(data_type), int(op_type), channels,
                                              nthreads, buffer_size, ro)
    _lib.check(rc, "mccs_host_ring_reduce_scatter")


def _host_ptrs(bufs):
    arr = ctypes.c_void_p * max(1, len(bufs))
    return arr(*[None if x is None else x.ctypes.data if hasattr(x, "ctypes") else int(x) for x in bufs])


def host_ring_broadcast(sendbufs, recvbufs, nbytes: int, root: int, channels: int = 1, nthreads: int = 96,
                        buffer_size: int = 1 << 22, rings=None) -> None:
    """The ring Broadcast schedule on host threads over host memory (numpy
    arrays or raw host pointers; no GPU).  sendbufs[r] may be None for r != root."""
    ro = None
    if rings is not None:
        flat = [int(v) for r in rings for v in r]
        ro = (_ci * len(flat))(*flat)
    rc = _sig().mccs_host_ring_broadcast(len(sendbufs), _host_ptrs(sendbufs), _host_ptrs(recvbufs), int(nbytes),
                                         int(root), channels, nthreads, buffer_size, ro)
    _lib.check(rc, "mccs_host_ring_broadcast")


def host_ring_reduce(sendbufs, recvbufs, count: int, data_type, op_type=AllReduceOpType.Sum, root: int = 0,
                     channels: int = 1, nthreads: int = 96, buffer_size: int = 1 << 22, rings=None,
                     op_arg: int | None = None) -> None:
    """The ring Reduce schedule on host threads over host memory (numpy arrays
    or raw host pointers; no GPU).  recvbufs[r] may be None for r != root."""
    ro = None
    if rings is not None:
        flat = [int(v) for r in rings for v in r]
        ro = (_ci * len(flat))(*flat)
    if op_arg is not None:
        rc = _sig().mccs_host_ring_reduce_oparg(len(sendbufs), _host_ptrs(sendbufs), _host_ptrs(recvbufs), int(count),
                                                int(data_type), int(op_type), int(root), channels, nthreads,
                                                buffer_size, ro, _u64(op_arg))
        _lib.check(rc, "mccs_host_ring_reduce_oparg")
        return
    rc = _sig().mccs_host_ring_reduce(len(sendbufs), _host_ptrs(sendbufs), _host_ptrs(recvbufs), int(count),
                                      int(data_type), int(op_type), int(root), channels, nthreads, buffer_size, ro)
    _lib.check(rc, "mccs_host_ring_reduce")


def alltoall_route(nranks: int, channels: int, rings=None, force_relay: bool = False) -> dict:
    """mccs_alltoall_route (host-only): the AllToAll route of a ring set
    (`channels` x nranks send orders; None = identity on every channel): hops,
    m, and the per rank and channel send / receive parts as nranks x channels
    lists."""
    ro = None
    if rings is not None:
        flat = [int(v) for r in rings for v in r]
        ro = (_ci * len(flat))(*flat)
    hops, m = _ci(), _ci()
    sb, rb = (_ci * (nranks * channels))(), (_ci * (nranks * channels))()
    rc = _sig().mccs_alltoall_route(int(nranks), int(channels), ro, 1 if force_relay else 0, ctypes.byref(hops),
                                    ctypes.byref(m), sb, rb)
    _lib.check(rc, "mccs_alltoall_route")
    cut = lambda t: [list(t[r * channels:(r + 1) * channels]) for r in range(nranks)]
    return {"hops": hops.value, "m": m.value, "send_bid": cut(sb), "recv_bid": cut(rb)}


def host_ring_all_to_all(sendbufs, recvbufs, nbytes: int, channels: int = 1, nthreads: int = 96,
                         buffer_size: int = 1 << 22, rings=None, force_relay: bool = False) -> None:
    """The AllToAll schedule on host threads over host memory (numpy arrays or
    raw host pointers; no GPU): every buffer holds nranks * nbytes bytes."""
    ro = None
    if rings is not None:
        flat = [int(v) for r in rings for v in r]
        ro = (_ci * len(flat))(*flat)
    rc = _sig().mccs_host_ring_all_to_all(len(sendbufs), _host_ptrs(sendbufs), _host_ptrs(recvbufs), int(nbytes),
                                          channels, nthreads, buffer_size, ro, 1 if force_relay else 0)
    _lib.check(rc, "mccs_host_ring_all_to_all")


def host_ring_all_to_all_v(sendbufs, recvbufs, counts, send_displs, recv_displs, channels: int = 1,
                           nthreads: int = 544, buffer_size: int = 1 << 22, rings=None,
                           force_relay: bool = False) -> None:
    """The AllToAllv schedule on host threads over host memory (no GPU).
    counts[s][t] bytes go from sendbufs[s] + send_displs[s][t] to recvbufs[t] +
    recv_displs[t][s].  A ring set whose route is not one hop is refused."""
    n = len(sendbufs)
    ro = None
    if rings is not None:
        flat = [int(v) for r in rings for v in r]
        ro = (_ci * len(flat))(*flat)
    flat2 = lambda m: _sizes([v for row in m for v in row])
    rc = _sig().mccs_host_ring_all_to_all_v(n, _host_ptrs(sendbufs), _host_ptrs(recvbufs), flat2(counts),
                                            flat2(send_displs), flat2(recv_displs), channels, nthreads, buffer_size,
                                            ro, 1 if force_relay else 0)
    _lib.check(rc, "mccs_host_ring_all_to_all_v")


def host_ring_all_to_all_v_tables(sendbufs, recvbufs, tables, channels: int = 1, nthreads: int = 544,
                                  buffer_size: int = 1 << 22, rings=None, force_relay: bool = False) -> None:
    """The AllToAllvDev schedule on host threads over host memory (no GPU).
    tables[r] is rank r's size table: a contiguous numpy uint64 / int64 array of
    4 * nranks words (or a raw host pointer), resolved by the kernel's own
    arithmetic.  A ring set whose route is not one hop is refused."""
    n = len(sendbufs)
    for t in tables:
        if hasattr(t, "ctypes") and (t.dtype.itemsize != 8 or t.dtype.kind not in "iu" or t.size != 4 * n or
                                     not t.flags["C_CONTIGUOUS"]):
            raise ValueError(f"a size table is a contiguous array of 4 * {n} 64-bit integers")
    ro = None
    if rings is not None:
        flat = [int(v) for r in rings for v in r]
        ro = (_ci * len(flat))(*flat)
    rc = _sig().mccs_host_ring_all_to_all_v_tables(n, _host_ptrs(sendbufs), _host_ptrs(recvbufs), _host_ptrs(tables),
                                                   channels, nthreads, buffer_size, ro, 1 if force_relay else 0)
    _lib.check(rc, "mccs_host_ring_all_to_all_v_tables")


def host_ring_send_recv(nranks: int, ops, channels: int = 1, nthreads: int = 544, buffer_size: int = 1 << 22,
                        rings=None) -> None:
    """The Send/Recv schedule on host threads over host memory (no GPU).  ops
    is a list of (rank, "send" | "recv", peer, buf, nbytes): buf a numpy array,
    a raw host pointer or None (nbytes 0).  Each rank's ops, in list order,
    form one group.  A ring set whose route is not one hop is refused."""
    k = len(ops)
    ints = lambda v: (_ci * max(1, k))(*v)
    ro = None
    if rings is not None:
        flat = [int(v) for r in rings for v in r]
        ro = (_ci * len(flat))(*flat)
    for o in ops:
        if o[1] not in ("send", "recv"):
            raise ValueError(f"op kind {o[1]!r} is neither 'send' nor 'recv'")
    rc = _sig().mccs_host_ring_send_recv(nranks, k, ints([int(o[0]) for o in ops]),
                                         ints([1 if o[1] == "send" else 0 for o in ops]),
                                         ints([int(o[2]) for o in ops]), _host_ptrs([o[3] for o in ops]),
                                         _sizes([o[4] for o in ops]), channels, nthreads, buffer_size, ro)
    _lib.check(rc, "mccs_host_ring_send_recv")


def ring_profile(device: int = 0, reset: bool = True) -> dict:
    """Per-slice timing of the ring kernels on `device` (MCCS_RING_PROFILE=1
    set before communicator init): slices, mean µs waiting for peer flags,
    mean µs streaming + draining (work_us), of which drain_us is the tail
    after thread 0's wave issued its last store (store drain + barrier)."""
    out = (ctypes.c_ulonglong * 4)()
    _lib.check(_sig().mccs_ring_profile(device, out, 1 if reset else 0), "mccs_ring_profile")
    n = max(1, out[0])
    return {"slices": out[0], "wait_us": out[1] / n / 100.0, "work_us": out[2] / n / 100.0,
            "drain_us": out[3] / n / 100.0}


def direct_defaults(nranks: int) -> tuple[int, int]:
    """(oneshot_bytes, direct_bytes) the library uses by default for n ranks
    (-1 = off); host-only."""
    a, b = _ci(), _ci()
    _sig().mccs_direct_defaults(int(nranks), ctypes.byref(a), ctypes.byref(b))
    return a.value, b.value


def ll_default(nranks: int) -> int:
    """ll_bytes the library uses by default for n ranks (-1 = off); host-only."""
    return int(_sig().mccs_ll_default(int(nranks)))


def task_schema(total_bytes: int, channels: int) -> tuple[int, int]:
    a, b = _ci(), _ci()
    _sig().mccs_task_schema(total_bytes, channels, ctypes.byref(a), ctypes.byref(b))
    return a.value, b.value


# mccsDevFunc_t (include/mccs_devcomm.h)
FUNC_BROADCAST, FUNC_REDUCE, FUNC_ALLGATHER, FUNC_REDUCE_SCATTER, FUNC_ALLREDUCE = 0, 1, 2, 3, 4


def ring_walk(func: int, nranks: int, channels: int, elem_bytes: int, nthreads: int, buffer_size: int, count: int,
              width: int = 64) -> list[tuple[int, int, int, int]]:
    """The chunk walk of one work element as the kernels and host paths cut it
    (csrc/ring_walk.h; host-only): one (gridOffset, realChunkSize, offset,
    nelem) per loop and part, in 64-bit or 32-bit arithmetic."""
    args = (int(func), int(nranks), int(channels), int(elem_bytes), int(nthreads), int(buffer_size), int(count),
            int(width))
    n = _sig().mccs_ring_walk(*args, None, 0)
    if n < 0:
        raise ValueError(f"mccs_ring_walk{args}: invalid argument")
    rows = (ctypes.c_longlong * (4 * max(1, n)))()
    assert _sig().mccs_ring_walk(*args, rows, n) == n
    vals = rows[:4 * n]
    return list(zip(vals[0::4], vals[1::4], vals[2::4], vals[3::4]))


__all__ = ["AllReduceDataType", "AllReduceOpType", "CommConfig", "Communicator", "init_all",
           "init_communicator_rank", "all_reduce", "all_gather", "reduce_scatter", "broadcast", "reduce", "all_to_all",
           "alltoall_route", "host_ring_all_to_all",
           "all_to_all_v", "all_to_all_single", "host_ring_all_to_all_v",
           "all_to_all_v_dev", "exchange_counts", "host_ring_all_to_all_v_tables",
           "send", "recv", "batch_send_recv", "host_ring_send_recv",
           "avg_op", "red_op_arg", "all_reduce_avg", "reduce_scatter_avg", "reduce_avg",
           "group", "default_rings", "task_schema",
           "direct_defaults", "ll_default", "ring_walk",
           "host_ring_allreduce", "host_ring_reduce_scatter", "host_ring_broadcast", "host_ring_reduce", "ring_profile",
           "FUNC_BROADCAST", "FUNC_REDUCE", "FUNC_ALLGATHER", "FUNC_REDUCE_SCATTER", "FUNC_ALLREDUCE",
           "RedOp", "DataType"]
