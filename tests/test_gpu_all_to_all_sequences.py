"""GPU: AllToAll between the other collectives on one communicator set, every
result exact.

An AllToAll moves every connection of a channel by the same number of steps,
but the calls before it do not: a Broadcast or Reduce leaves the connection
that closes its chain behind the others, with rotating roots a different one
each time, and ring AllReduces, AllGathers and ReduceScatters move the channels
they select and no others.  So the AllToAll that follows them starts from
connections at different FIFO steps and slots, and the relay's recvSend hands
slots of one connection to another that stands elsewhere.  The sequence is
tests/test_gpu_rooted_sequences.py's (its 14 calls, same seed) with an AllToAll
of a rotating size after every second call; a 64 KiB FIFO buffer makes the
larger ones take several loops.  It runs on one stream, across two streams,
inside a HIP graph replayed three times with new inputs, as one batched group,
and with one rank per process (tests/a2a_worker.py, fresh child processes).
"""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import a2a_ref
from mccs_amd import comm as C
import test_gpu_rooted_sequences as S
import vnode

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
DIRECT_DEFAULTS = True  # S.CFG sets every threshold

A2A_BYTES = [4099, 1, 70001, 15, 300000, 9, 65537]  # per peer, one after every second call of S.sequence


def sequence(n):
    """S.sequence with {"kind": "a2a", "count": bytes per peer} calls woven in."""
    out, k = [], 0
    for i, call in enumerate(S.sequence(S.SEED, n)):
        out.append(call)
        if i % 2 == 1:
            out.append(dict(kind="a2a", count=A2A_BYTES[k % len(A2A_BYTES)], salt=k, root=None))
            k += 1
    return out


class A2AStaged:
    """Device buffers of one AllToAll on the virtual node (the interface of S.Staged)."""

    def __init__(self, call, n, salt=None):
        self.call, self.n = call, n
        self.send = [vnode.to_dev(np.zeros(n * call["count"], np.uint8)) for _ in range(n)]
        self.recv = [vnode.to_dev(np.full(n * call["count"], a2a_ref.SENTINEL, np.uint8)) for _ in range(n)]
        self.refill(call["salt"] if salt is None else salt)

    def refill(self, salt):
        import torch

        self.xs = a2a_ref.make_inputs(self.n, self.call["count"], salt)
        for r in range(self.n):
            self.send[r].copy_(torch.from_numpy(self.xs[r]).cuda())

    def issue(self, comms, stream=None):
        with C.group():
            for r in range(self.n):
                C.all_to_all(comms[r], self.send[r], self.recv[r], self.call["count"], stream=stream)

    def check(self, orc, comm0, tag):
        want = a2a_ref.expected(self.xs, self.call["count"])
        for r in range(self.n):
            assert self.recv[r].cpu().numpy().tobytes() == want[r].tobytes(), (tag, self.call, r)
            assert self.send[r].cpu().numpy().tobytes() == self.xs[r].tobytes(), (tag, self.call, r, "send written")


def _stage(n, rng):
    return [A2AStaged(call, n) if call["kind"] == "a2a"
            else S.Staged(call, n, [S.call_input(call, n, rng) for _ in range(n)]) for call in sequence(n)]


def _refill(items, n, rng, rep):
    for s in items:
        if s.call["kind"] == "a2a":
            s.refill(100 + 10 * rep + s.call["salt"])
        else:
            s.refill([S.call_input(s.call, n, rng) for _ in range(n)])


def _algo(call):
    return "ring" if call["kind"] == "a2a" else S.expected_algo(call)


@pytest.mark.parametrize("n", [4, 8])
def test_sequence(orc, monkeypatch, n):
    import torch

    monkeypatch.delenv("MCCS_ALLTOALL_HOPS", raising=False)
    comms = S._comms(n)
    try:
        assert comms[0].all_to_all_route()["hops"] == 1
        items = _stage(n, np.random.default_rng(n))
        torch.cuda.synchronize()
        took = []
        for s in items:
            s.issue(comms)
            took.append((s.call["kind"], comms[0].last_algo(), _algo(s.call)))
        S._finish(orc, comms, items, ("a2a sequence", n))
        print(f"n {n}:", " ".join(f"{k}:{a}" for k, a, _ in took))
        assert not [t for t in took if t[1] != t[2]], took
        assert sum(1 for t in took if t[0] == "a2a") == 7
    finally:
        vnode.destroy(comms)


@pytest.mark.parametrize("n", [4, 8])
def test_sequence_relay(orc, monkeypatch, n):
    """The same with the relay forced: recvSend between connections at different steps."""
    import torch

    monkeypatch.setenv("MCCS_ALLTOALL_HOPS", "relay")
    comms = S._comms(n)
    try:
        assert comms[0].all_to_all_route() == {"hops": n - 1, "m": 0}
        items = _stage(n, np.random.default_rng(40 + n))
        torch.cuda.synchronize()
        for s in items:
            s.issue(comms)
        S._finish(orc, comms, items, ("a2a relay sequence", n))
    finally:
        vnode.destroy(comms)


@pytest.mark.parametrize("n", [4, 8])
def test_sequence_across_two_streams(orc, monkeypatch, n):
    import torch

    monkeypatch.delenv("MCCS_ALLTOALL_HOPS", raising=False)
    comms = S._comms(n)
    streams = [torch.cuda.current_stream(), torch.cuda.Stream()]
    try:
        rng = np.random.default_rng(10 + n)
        items = _stage(n, rng)
        torch.cuda.synchronize()
        for s in items:
            s.issue(comms, streams[int(rng.integers(0, 2))])
        S._finish(orc, comms, items, ("a2a streams", n))
    finally:
        vnode.destroy(comms)


@pytest.mark.parametrize("n", [4, 8])
def test_sequence_graph_replayed_three_times(orc, monkeypatch, n):
    """Issued once eagerly (the first launch of a kernel loads its code object,
    which a capture cannot), captured into one HIP graph, replayed three times
    with new inputs: the route rides in the captured work elements."""
    import torch

    monkeypatch.delenv("MCCS_ALLTOALL_HOPS", raising=False)
    comms = S._comms(n)
    try:
        rng = np.random.default_rng(20 + n)
        items = _stage(n, rng)
        torch.cuda.synchronize()
        for s in items:
            s.issue(comms)
        S._finish(orc, comms, items, ("eager", n))
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for s in items:
                s.issue(comms)
        for rep in range(3):
            _refill(items, n, rng, rep)
            torch.cuda.synchronize()
            g.replay()
            S._finish(orc, comms, items, ("replay", n, rep))
        del g
    finally:
        vnode.destroy(comms)


@pytest.mark.parametrize("n,relay", [(4, False), (8, False), (4, True)])
def test_batched_group(orc, monkeypatch, n, relay):
    """Several AllToAlls of one comm in one group are one launch; an AllReduce
    before and after leaves and finds the connections in step."""
    import torch

    if relay:
        monkeypatch.setenv("MCCS_ALLTOALL_HOPS", "relay")
    else:
        monkeypatch.delenv("MCCS_ALLTOALL_HOPS", raising=False)
    comms = S._comms(n)
    try:
        rng = np.random.default_rng(60 + n)
        ar = dict(kind="ar", code=7, op=0, root=None, inplace=False, count=100000)
        before = S.Staged(ar, n, [S.call_input(ar, n, rng) for _ in range(n)])
        after = S.Staged(ar, n, [S.call_input(ar, n, rng) for _ in range(n)])
        batch = [A2AStaged(dict(kind="a2a", count=B, salt=k, root=None), n) for k, B in enumerate((15, 4099, 300000))]
        torch.cuda.synchronize()
        before.issue(comms)
        with C.group():
            for s in batch:
                for r in range(n):
                    C.all_to_all(comms[r], s.send[r], s.recv[r], s.call["count"])
        after.issue(comms)
        S._finish(orc, comms, [before] + batch + [after], ("batched", n, relay))
    finally:
        vnode.destroy(comms)


def _free_port() -> int:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


@pytest.mark.parametrize("world", [2, 3])
def test_sequence_one_rank_per_process(world):
    """One rank per process: the multi-rank kernel launched for a single rank,
    over IPC-mapped arenas; n = 2 (m = 4) and n = 3 (two rings, m = 1)."""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.join(HERE, "a2a_worker.py")]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("MCCS_ONESHOT_BYTES", "MCCS_DIRECT_BYTES", "MCCS_LL_BYTES", "MCCS_ALLTOALL_HOPS"):
        env.pop(k, None)
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=240, env=env, cwd=os.path.dirname(HERE))
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    lib_lines = "\n".join(l for l in (r.stdout + r.stderr).splitlines() if "mccs" in l.lower() or "hip" in l)[-3000:]
    assert r.returncode == 0 and lines, lib_lines + "\n----\n" + r.stdout[-2000:] + r.stderr[-2000:]
    res = json.loads(lines[-1])
    bad = [k for k, v in res["checks"].items() if not v]
    assert res["all_ok"] and not bad, bad
    kinds = [k.split("/")[1] for k in res["checks"]]
    assert kinds.count("a2a") == 7 and {"bc", "rd", "ar", "ag", "rs"} <= set(kinds), sorted(res["checks"])
    assert res["route"] == {"hops": 1, "m": 4 if world == 2 else 1}
    print(f"{world} processes: {len(res['checks'])} checks")
