"""GPU: Send/Recv groups between the other collectives on one communicator set,
every result exact.

The sequence puts a Send/Recv group after every other call: ring AllReduces,
Broadcasts with rotating roots, an AllToAllv and an AllToAllvDev.  Those leave
the connections at different FIFO steps, a Send/Recv group moves only the
connections of its own pairs (by each message's loops alone, and several
elements on one channel), and the next call of any kind must find both ends of
every connection in step.  It runs on one stream, across two streams, inside a
HIP graph replayed three times with refilled payloads, and with one rank per
process (tests/sr_worker.py, fresh child processes), where each process groups
only its own calls and one 3C message is sent and received ungrouped.

On the virtual node a send and its receive are always issued in one group()
across the ranks' communicators (one fused launch).  ring only, buffer_size =
1 << 16, an 8 s watchdog.
"""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import a2av_ref as V
import sr_ref as SR
import test_gpu_all_to_all_v as G
import test_gpu_all_to_all_v_dev as D
import test_gpu_rooted_sequences as S
import test_gpu_send_recv as P
import vnode

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
DIRECT_DEFAULTS = True  # G._comms sets every threshold

assert S.BUFF == V.BUFF  # S.call_expected plans the AllReduces with the buffer size the comms get


def sequence(n):
    """The calls of one sequence for n ranks, the same on every rank."""
    bc = lambda root, count: dict(kind="bc", code=0, op=0, root=root % n, inplace=False, count=count)
    ar = lambda count: dict(kind="ar", code=7, op=0, root=None, inplace=False, count=count)
    sr = lambda pat, salt: dict(kind="sr", pat=pat, salt=salt, root=None, count=0)
    out = [bc(1, 70001), sr("b_shift_3C", 0), ar(100000), bc(2, 5), sr("d_fan", 1),
           dict(kind="a2av", mat="s1r3", layout="gaps", salt=2, root=None, count=0), sr("e_two_on_a_pair", 3),
           dict(kind="a2avd", mat="cyc5", layout="descending", salt=4, root=None, count=0), bc(3, 300001),
           sr("h_misaligned", 5), ar(70001), sr("c_pairwise", 6), sr("g_one_way", 7), bc(0, 4099),
           sr("e_zero_first", 8)]
    if n == 3:
        out += [sr("f_send_after_recvs", 9), bc(2, 33000)]
    if n <= 4:
        out += [sr("a_all_pairs", 10), ar(4099)]
    return out


def stage_call(call, n, rings, m, rng):
    if call["kind"] == "sr":
        return P.SRStaged(n, SR.patterns(n, m, rings)[call["pat"]], call["salt"], call=call)
    if call["kind"] == "a2av":
        return G.VStaged(n, V.matrices(n, m, rings)[call["mat"]], call["layout"], call["salt"], call=call)
    if call["kind"] == "a2avd":
        return D.DStaged(n, V.matrices(n, m, rings)[call["mat"]], call["layout"], call["salt"], call=call)
    return S.Staged(call, n, [S.call_input(call, n, rng) for _ in range(n)])


def _stage(n, rng, comms):
    rings, m = comms[0].rings(), comms[0].all_to_all_route()["m"]
    return [stage_call(call, n, rings, m, rng) for call in sequence(n)]


def _refill(items, n, rng, rep):
    for s in items:
        if s.call["kind"] in ("sr", "a2av", "a2avd"):
            s.refill(100 + 10 * rep + s.call["salt"])
        else:
            s.refill([S.call_input(s.call, n, rng) for _ in range(n)])


def _comms(n, monkeypatch):
    comms = G._comms(n, monkeypatch)
    assert comms[0].all_to_all_route()["hops"] == 1
    return comms


@pytest.mark.parametrize("n", [4, 8])
def test_sequence(orc, monkeypatch, n):
    import torch

    comms = _comms(n, monkeypatch)
    try:
        items = _stage(n, np.random.default_rng(n), comms)
        torch.cuda.synchronize()
        took = []
        for s in items:
            s.issue(comms)
            took.append((s.call["kind"], comms[0].last_algo()))
        S._finish(orc, comms, items, ("sr sequence", n))
        assert all(a == "ring" for _, a in took), took
        kinds = [k for k, _ in took]
        assert kinds.count("sr") >= 7 and {"bc", "ar", "a2av", "a2avd"} <= set(kinds)
    finally:
        vnode.destroy(comms)


@pytest.mark.parametrize("n", [4, 8])
def test_sequence_across_two_streams(orc, monkeypatch, n):
    import torch

    comms = _comms(n, monkeypatch)
    streams = [torch.cuda.current_stream(), torch.cuda.Stream()]
    try:
        rng = np.random.default_rng(10 + n)
        items = _stage(n, rng, comms)
        torch.cuda.synchronize()
        for s in items:
            s.issue(comms, streams[int(rng.integers(0, 2))])
        S._finish(orc, comms, items, ("sr streams", n))
    finally:
        vnode.destroy(comms)


@pytest.mark.parametrize("n", [4, 8])
def test_sequence_graph_replayed_three_times(orc, monkeypatch, n):
    """Issued once eagerly, captured into one HIP graph, replayed three times
    with refilled payloads: the pointers and sizes of every send and receive
    ride in the captured work elements."""
    import torch

    comms = _comms(n, monkeypatch)
    try:
        rng = np.random.default_rng(20 + n)
        items = _stage(n, rng, comms)
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


def _free_port() -> int:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


@pytest.mark.parametrize("world", [2, 3])
def test_sequence_one_rank_per_process(world):
    """One rank per process over IPC-mapped arenas, n = 2 (m = 4) and n = 3
    (m = 1, with pattern (f)).  Each process groups only its own calls; one 3C
    message goes from an ungrouped send to an ungrouped receive."""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.join(HERE, "sr_worker.py")]
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
    assert kinds.count("sr") >= 7 and kinds.count("sr1") == 1 and {"bc", "ar", "a2av", "a2avd"} <= set(kinds)
    assert ("f_send_after_recvs" in " ".join(res["checks"])) == (world == 3)
    assert res["route"] == {"hops": 1, "m": 4 if world == 2 else 1}
