"""GPU: AllToAllv between the other collectives on one communicator set, every
result exact.

The sequence is tests/test_gpu_rooted_sequences.py's (Broadcasts and Reduces
with rotating roots, ring and LL AllReduces, an AllGather and a ReduceScatter,
same seed) with a v call after every second call and one uniform AllToAll in
the middle.  The calls before a v call leave the connections at different FIFO
steps; a v call moves them further apart, since each connection advances by
its own pair's loops alone (0 to 3 here), and the next call of any kind must
find both ends of every connection in step.  It runs on one stream, across two
streams, inside a HIP graph replayed three times with new inputs, as a batched
group of two v calls with different matrices, and with one rank per process
(tests/a2av_worker.py, fresh child processes).
"""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import a2av_ref as V
from mccs_amd import comm as C
import test_gpu_all_to_all_sequences as A
import test_gpu_all_to_all_v as G
import test_gpu_rooted_sequences as S
import vnode

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
DIRECT_DEFAULTS = True  # S.CFG sets every threshold

MATS = ["s3r0", "s1r3", "cyc5", "zero_row", "s0r3", "zero_col", "s1r1"]  # one after every second call of S.sequence


def sequence(n):
    """S.sequence with {"kind": "a2av", "mat": name, "layout": kind} calls woven
    in, and one uniform AllToAll after the fourth v call."""
    out, k = [], 0
    for i, call in enumerate(S.sequence(S.SEED, n)):
        out.append(call)
        if i % 2 == 1:
            out.append(dict(kind="a2av", mat=MATS[k % len(MATS)], layout=V.LAYOUTS[k % 4], salt=k, root=None, count=0))
            k += 1
            if k == 4:
                out.append(dict(kind="a2a", count=70001, salt=k, root=None))
    return out


def stage_call(call, n, rings, m, rng):
    if call["kind"] == "a2av":
        return G.VStaged(n, V.matrices(n, m, rings)[call["mat"]], call["layout"], call["salt"], call=call)
    if call["kind"] == "a2a":
        return A.A2AStaged(call, n)
    return S.Staged(call, n, [S.call_input(call, n, rng) for _ in range(n)])


def _stage(n, rng, comms):
    rings, m = comms[0].rings(), comms[0].all_to_all_route()["m"]
    return [stage_call(call, n, rings, m, rng) for call in sequence(n)]


def _refill(items, n, rng, rep):
    for s in items:
        if s.call["kind"] in ("a2a", "a2av"):
            s.refill(100 + 10 * rep + s.call["salt"])
        else:
            s.refill([S.call_input(s.call, n, rng) for _ in range(n)])


def _algo(call):
    return "ring" if call["kind"] in ("a2a", "a2av") else S.expected_algo(call)


def _comms(n, monkeypatch):
    monkeypatch.delenv("MCCS_ALLTOALL_HOPS", raising=False)
    comms = S._comms(n)
    assert comms[0].all_to_all_route()["hops"] == 1 and S.CFG["buffer_size"] == V.BUFF
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
            took.append((s.call["kind"], comms[0].last_algo(), _algo(s.call)))
        S._finish(orc, comms, items, ("a2av sequence", n))
        assert not [t for t in took if t[1] != t[2]], took
        assert sum(1 for t in took if t[0] == "a2av") == 7 and sum(1 for t in took if t[0] == "a2a") == 1
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
        S._finish(orc, comms, items, ("a2av streams", n))
    finally:
        vnode.destroy(comms)


@pytest.mark.parametrize("n", [4, 8])
def test_sequence_graph_replayed_three_times(orc, monkeypatch, n):
    """Issued once eagerly, captured into one HIP graph, replayed three times
    with new inputs: counts and displacements ride in the captured work
    elements, and every replay advances each connection by its own pair's steps."""
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


@pytest.mark.parametrize("n", [4, 8])
def test_batched_group_of_two_matrices(orc, monkeypatch, n):
    """Two v calls with different matrices in one group are one launch; an
    AllReduce before and after leaves and finds the connections in step."""
    import torch

    comms = _comms(n, monkeypatch)
    try:
        rng = np.random.default_rng(60 + n)
        rings, m = comms[0].rings(), comms[0].all_to_all_route()["m"]
        mats = V.matrices(n, m, rings)
        ar = dict(kind="ar", code=7, op=0, root=None, inplace=False, count=100000)
        before = S.Staged(ar, n, [S.call_input(ar, n, rng) for _ in range(n)])
        after = S.Staged(ar, n, [S.call_input(ar, n, rng) for _ in range(n)])
        batch = [G.VStaged(n, mats["s1r3"], "gaps", 1), G.VStaged(n, mats["cyc5"], "descending", 2)]
        torch.cuda.synchronize()
        before.issue(comms)
        with C.group():
            for s in batch:
                for r in range(n):
                    s.issue_rank(comms[r], r)
        after.issue(comms)
        S._finish(orc, comms, [before] + batch + [after], ("batched", n))
    finally:
        vnode.destroy(comms)


def _free_port() -> int:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


@pytest.mark.parametrize("world", [2, 3])
def test_sequence_one_rank_per_process(world):
    """One rank per process: the multi-rank kernel launched for a single rank,
    over IPC-mapped arenas; n = 2 (m = 4) and n = 3 (m = 1)."""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.join(HERE, "a2av_worker.py")]
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
    assert kinds.count("a2av") == 7 and kinds.count("a2a") == 1 and {"bc", "rd", "ar", "ag", "rs"} <= set(kinds)
    assert res["route"] == {"hops": 1, "m": 4 if world == 2 else 1}
