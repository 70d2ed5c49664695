"""GPU: Broadcast and Reduce inside sequences of collectives on one
communicator set, every result bit for bit.

A rooted collective is a chain: the connection between the chain's two ends
carries nothing (in a Broadcast the last -> root connection of each channel
stands still while all the others move), so after one the communicator's
connections no longer stand at the same FIFO step, and with rotating roots the
idle connection is a different one each time.  Everything a launch keeps for
the next one is per connection (the saved steps in the flag lines, the polled
head / tail counters, the slot index), and the sequences here are the test of
that: Broadcasts and Reduces with rotating roots between ring AllReduces,
direct-sized AllReduces (LL), AllGathers and ReduceScatters, no sync in
between.  A 64 KiB FIFO buffer makes most calls take several loops, so the
steps of the busy connections run many slots ahead of the idle one's.

The same sequence runs on one stream, across two streams, inside a replayed
HIP graph, and with one rank per process (tests/rooted_worker.py, fresh child
processes).  The sequence is a pure function of (seed, n);
tests/test_rooted_cases.py asserts on the CPU what it contains.
"""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from mccs_amd import comm as C
import rooted_ref
import rs_ref
import vnode

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
DIRECT_DEFAULTS = True  # the thresholds below are explicit; nothing here relies on the environment's

TIMEOUT_MS = 8000
BUFF = 1 << 16
# one-shot up to 256 KiB, LL up to 32 KiB, no two-shot: "ar" calls (above 256 KiB) take the ring, "ard" calls LL
CFG = dict(buffer_size=BUFF, oneshot_bytes=256 << 10, ll_bytes=32 << 10, direct_bytes=-1)
SEED = 31000
KINDS = ["bc"] * 4 + ["rd"] * 4 + ["ar"] * 2 + ["ard"] * 2 + ["ag", "rs"]  # 14 calls
MAX_BYTES = 400 << 10


def _sized(rng, esize, lo_bytes, hi_bytes):
    """Elements of `esize` bytes, log-uniform between the two byte sizes."""
    lo, hi = max(esize, lo_bytes), max(esize, hi_bytes)
    return max(1, int(lo * (hi / lo) ** float(rng.random())) // esize)


def sequence(seed, n):
    """The calls of one sequence for n ranks, the same on every rank: dicts
    with kind (bc, rd, ar = ring AllReduce, ard = direct-sized AllReduce, ag,
    rs), code, op, count (elements; bytes for bc / ag; elements per block for
    rs), and for the rooted ones root (rotating over the ranks) and inplace."""
    rng = np.random.default_rng([seed, n])
    kinds = [str(k) for k in rng.permutation(KINDS)]
    root0, k = int(rng.integers(0, n)), 0
    calls = []
    for kind in kinds:
        c = dict(kind=kind, code=0, op=0, root=None, inplace=False)
        if kind in ("bc", "rd"):
            c["root"] = (root0 + k) % n
            k += 1
            c["inplace"] = bool(rng.random() < 0.3)
        # rooted calls alternate between a few bytes .. 64 KiB and sizes of several loops on every channel
        lo, hi = (1, 64 << 10) if k % 2 else (256 << 10, 1 << 20)
        if kind == "bc":
            c["count"] = _sized(rng, 1, lo, hi)
        elif kind == "rd":
            c["code"], c["op"] = int(rng.choice([2, 6, 7, 9])), int(rng.choice([0, 0, 1, 2, 3]))
            c["count"] = _sized(rng, vnode.ESIZE[c["code"]], lo, hi)
        elif kind == "ar":
            c["code"] = int(rng.choice([6, 7]))
            c["count"] = _sized(rng, vnode.ESIZE[c["code"]], (256 << 10) + 8, 1 << 20)
        elif kind == "ard":
            c["code"] = 7
            c["count"] = _sized(rng, 4, 4, 16 << 10)
        elif kind == "ag":
            c["count"] = _sized(rng, 1, (256 << 10) + 1, MAX_BYTES)
        else:
            c["code"], c["op"] = int(rng.choice([2, 6, 7])), int(rng.choice([0, 2, 3]))
            c["count"] = _sized(rng, vnode.ESIZE[c["code"]], 1, MAX_BYTES // n)
        calls.append(c)
    return calls


def call_input(call, n, rng):
    """One rank's input of a call among n ranks."""
    if call["kind"] in ("bc", "ag"):
        return rng.integers(0, 256, call["count"], dtype=np.uint8)
    return vnode.gen(call["code"], (n if call["kind"] == "rs" else 1) * call["count"], rng)


def call_expected(orc, call, xs, nch_cfg, rings):
    """Per-rank expected outputs of one call (None: the rank has no output)."""
    n, kind, code, op, cnt = len(xs), call["kind"], call["code"], call["op"], call["count"]
    planner = vnode.Planner(nch_cfg, rings)  # every launch starts from idle channels
    if kind == "bc":
        return [rooted_ref.broadcast_expected(xs, call["root"])] * n
    if kind == "rd":
        exp = rooted_ref.reduce_expected_planned(orc, xs, code, op, call["root"], None, planner=planner, buff_size=BUFF)
        return [exp if r == call["root"] else None for r in range(n)]
    if kind == "ag":
        return [orc.ring_allgather(xs)] * n
    if kind == "rs":
        return rs_ref.expected_planned(orc, xs, code, op, None, planner=planner, buff_size=BUFF)
    nch, nthr, sel = planner.select(cnt * vnode.ESIZE[code], cnt * vnode.ESIZE[code])
    return [orc.ring_allreduce(code, op, xs, nchannels=nch, nthreads=nthr, buff_size=BUFF, ring_orders=sel)] * n


def rank_buffers(call, n, rank, x):
    """(send, recv, out) of one rank: device tensors or None for the buffer
    its role does not use; `out` is where its result lands (None: no result)."""
    kind, cnt, root = call["kind"], call["count"], call["root"]
    es = vnode.ESIZE[call["code"]]
    send = vnode.to_dev(x)
    if kind == "rd" and rank != root:
        return send, None, None
    if call["inplace"] and rank == root:
        return send, send, send
    recv = vnode.to_dev(np.zeros((n if kind == "ag" else 1) * cnt * es, np.uint8))
    return (None if kind == "bc" and rank != root else send), recv, recv


def issue_rank(comm, call, send, recv, stream=None):
    kind, cnt = call["kind"], call["count"]
    if kind == "bc":
        C.broadcast(comm, send, recv, cnt, call["root"], stream=stream)
    elif kind == "rd":
        C.reduce(comm, send, recv, cnt, call["code"], call["op"], call["root"], stream=stream)
    elif kind == "ag":
        C.all_gather(comm, send, recv, cnt, stream=stream)
    elif kind == "rs":
        C.reduce_scatter(comm, send, recv, cnt, call["code"], call["op"], stream=stream)
    else:
        C.all_reduce(comm, send, recv, cnt, call["code"], call["op"], stream=stream)


def expected_algo(call):
    return "ll" if call["kind"] == "ard" else "ring"


class Staged:
    """Device buffers of one call on the virtual node."""

    def __init__(self, call, n, xs):
        self.call, self.n = call, n
        self.bufs = [rank_buffers(call, n, r, xs[r]) for r in range(n)]
        self.xs = xs

    def refill(self, xs):
        import torch

        self.xs = xs
        for r in range(self.n):
            if self.bufs[r][0] is not None:
                self.bufs[r][0].copy_(torch.from_numpy(np.ascontiguousarray(xs[r]).view(np.uint8)).cuda())

    def issue(self, comms, stream=None):
        with C.group():
            for r in range(self.n):
                issue_rank(comms[r], self.call, self.bufs[r][0], self.bufs[r][1], stream)

    def check(self, orc, comm0, tag):
        exp = call_expected(orc, self.call, self.xs, comm0.nchannels, comm0.rings())
        for r in range(self.n):
            out = self.bufs[r][2]
            assert (out is None) == (exp[r] is None), (tag, self.call, r)
            if out is not None:
                assert out.cpu().numpy().tobytes() == exp[r].tobytes(), (tag, self.call, r)


def _stage(n, rng):
    return [Staged(call, n, [call_input(call, n, rng) for _ in range(n)]) for call in sequence(SEED, n)]


def _comms(n):
    comms = C.init_all([0] * n, C.CommConfig(timeout_ms=TIMEOUT_MS, **CFG))
    assert comms[0].fifo_memory != C.FIFO_DEVICE  # LL ("ard") needs the uncached arena
    return comms


def _finish(orc, comms, items, tag):
    import torch

    torch.cuda.synchronize()
    for c in comms:
        c.sync()
    for i, s in enumerate(items):
        s.check(orc, comms[0], (tag, i))


@pytest.mark.parametrize("n", [4, 8])
def test_sequence(orc, n):
    """14 calls, no sync in between, one sync, every output exact; every call
    took the kernel the sequence means it to take."""
    import torch

    comms = _comms(n)
    try:
        items = _stage(n, np.random.default_rng(n))
        torch.cuda.synchronize()
        took = []
        for s in items:
            s.issue(comms)
            took.append((s.call["kind"], comms[0].last_algo(), expected_algo(s.call)))
        _finish(orc, comms, items, ("sequence", n))
        print(f"n {n}:", " ".join(f"{k}:{a}" for k, a, _ in took))
        assert not [t for t in took if t[1] != t[2]], took
    finally:
        vnode.destroy(comms)


@pytest.mark.parametrize("n", [4, 8])
def test_sequence_across_two_streams(orc, n):
    """Every call on one of two streams, inputs staged and synchronised first:
    a communicator's launches still run in issue order."""
    import torch

    comms = _comms(n)
    streams = [torch.cuda.current_stream(), torch.cuda.Stream()]
    try:
        rng = np.random.default_rng(10 + n)
        items = _stage(n, rng)
        torch.cuda.synchronize()
        for s in items:
            s.issue(comms, streams[int(rng.integers(0, 2))])
        _finish(orc, comms, items, ("streams", n))
    finally:
        vnode.destroy(comms)


@pytest.mark.parametrize("n", [4, 8])
def test_sequence_graph_replay(orc, n):
    """The sequence issued once eagerly (the first launch of a kernel loads its
    code object, which a capture cannot), then captured into one HIP graph and
    replayed twice with fresh inputs: the replays pick every connection's steps
    up where the previous launch left them."""
    import torch

    comms = _comms(n)
    try:
        rng = np.random.default_rng(20 + n)
        items = _stage(n, rng)
        torch.cuda.synchronize()
        for s in items:
            s.issue(comms)
        _finish(orc, comms, items, ("eager", n))
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for s in items:
                s.issue(comms)
        for rep in range(2):
            for s in items:
                s.refill([call_input(s.call, n, rng) for _ in range(n)])
            torch.cuda.synchronize()
            g.replay()
            _finish(orc, comms, items, ("replay", n, rep))
        del g
    finally:
        vnode.destroy(comms)


def _free_port() -> int:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_sequence_one_rank_per_process():
    """n = 2, one rank per process: every call is the multi-rank kernel
    launched for a single rank, over IPC-mapped arenas."""
    world = 2
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.join(HERE, "rooted_worker.py")]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("MCCS_ONESHOT_BYTES", "MCCS_DIRECT_BYTES", "MCCS_LL_BYTES"):
        env.pop(k, None)
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=240, env=env, cwd=os.path.dirname(HERE))
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    lib_lines = "\n".join(l for l in (r.stdout + r.stderr).splitlines() if "mccs" in l.lower() or "hip" in l)[-3000:]
    assert r.returncode == 0 and lines, lib_lines + "\n----\n" + r.stdout[-2000:] + r.stderr[-2000:]
    res = json.loads(lines[-1])
    bad = [k for k, v in res["checks"].items() if not v]
    assert res["all_ok"] and not bad, bad
    kinds = {k.split("/")[1] for k in res["checks"]}
    assert {"bc", "rd", "ar", "ard", "ag", "rs"} <= kinds, sorted(res["checks"])
    print(f"{world} processes: {len(res['checks'])} checks")
