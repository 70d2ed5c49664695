"""GPU: the direct and LL ReduceScatter between the launches that share their
slots, E_IN, the parity and the launch count, on one set of communicators;
every result bit for bit (expected values: tests/rs_ref.py and the oracle,
through tests/test_gpu_rooted_sequences.py's call_expected).

One sequence alternates count-based direct ReduceScatters (three in a row, of
different sizes and dtypes, and the cap itself), LL ReduceScatters (three in a
row, and the LL limit itself), one-shot, two-shot and LL AllReduces, a one-shot
and an LL AllGather, an LL AllToAll and a ring ReduceScatter above the cap, no
sync in between.  It runs on one stream, across two streams, in a HIP graph
replayed three times with rewritten inputs, and with one rank per process at
n = 2 and 3 (tests/rs_direct_worker.py).  Each sequence runs once.
64 KiB FIFO buffer (most blocks take several loops), one-shot slots of
256 KiB, LL to 32 KiB, two-shot to 2 MiB; the ReduceScatter limits are the
one-shot cap and 16 KiB (LL wins below it).
"""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from mccs_amd import comm as C
import test_gpu_all_to_all_sequences as A
import test_gpu_rooted_sequences as S
import vnode

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
DIRECT_DEFAULTS = True  # CFG sets every threshold

ONESHOT, LL_BYTES, TWOSHOT = 256 << 10, 32 << 10, 2 << 20
RS_LL = 16 << 10
CFG = dict(buffer_size=S.BUFF, oneshot_bytes=ONESHOT, ll_bytes=LL_BYTES, direct_bytes=TWOSHOT)
I32, F16, F32, BF16 = 2, 6, 7, 9
SUM, MAX = 0, 2


def opt_in(comm):
    cap, ll_cap = comm.reduce_scatter_direct_max()
    assert (cap, ll_cap) == (ONESHOT, LL_BYTES)
    comm.set_reduce_scatter_direct(block_bytes=cap, ll_block_bytes=RS_LL)
    comm.set_all_to_all_ll(bytes_per_peer=comm.all_to_all_ll_max())


def _comms(n):
    comms = C.init_all([0] * n, C.CommConfig(timeout_ms=S.TIMEOUT_MS, **CFG))
    for c in comms:
        opt_in(c)
    return comms


def sequence(n):
    """The calls of one sequence, the same on every rank: S's call dicts
    (count: elements, per block for rs; bytes for ag / a2a) plus `algo`, the
    kernel the call must take."""
    def call(kind, count, algo, code=F32, op=SUM, **kw):
        return dict(kind=kind, code=code, op=op, root=None, inplace=False, count=count, algo=algo, **kw)

    return [call("rs", 20000, "oneshot"), call("rs", 30011, "oneshot", F16), call("rs", 5001, "oneshot", I32, MAX),
            call("ar", 30000, "oneshot"),
            call("rs", 1000, "ll"), call("rs", 4099, "ll", F16), call("rs", 1, "ll", F32, MAX),
            call("ar", 2000, "ll"),
            call("rs", ONESHOT // 4, "oneshot"),
            call("ar", 200000, "direct"),
            call("ag", 100000, "oneshot", 0),
            call("rs", RS_LL // 4, "ll"),
            call("ag", 5000, "ll", 0),
            call("a2a", 4099, "ll", 0, salt=3),
            call("rs", ONESHOT // 4 + 1, "ring"),
            call("rs", 12345, "oneshot", BF16),
            call("rs", 333, "ll", F16)]


def _stage(n, rng):
    return [A.A2AStaged(call, n) if call["kind"] == "a2a"
            else S.Staged(call, n, [S.call_input(call, n, rng) for _ in range(n)]) for call in sequence(n)]


def _refill(items, n, rng, rep):
    for s in items:
        if s.call["kind"] == "a2a":
            s.refill(100 + 10 * rep + s.call["salt"])
        else:
            s.refill([S.call_input(s.call, n, rng) for _ in range(n)])


def _issue_all(items, comms, pick_stream=lambda: None):
    took = []
    for s in items:
        s.issue(comms, pick_stream())
        took.append((s.call["kind"], s.call["count"], comms[0].last_algo(), s.call["algo"]))
    return took


def check_took(took):
    assert not [t for t in took if t[2] != t[3]], took
    rs = "".join({"oneshot": "d", "ll": "l", "ring": "r"}[t[2]] if t[0] == "rs" else "." for t in took)
    assert "ddd" in rs and "lll" in rs and "r" in rs  # three consecutive of each variant, and the ring
    assert {(t[0], t[2]) for t in took} >= {("ar", "oneshot"), ("ar", "direct"), ("ar", "ll"), ("ag", "oneshot"),
                                            ("ag", "ll"), ("a2a", "ll")}


@pytest.mark.parametrize("n", [4, 8])
def test_sequence(orc, n):
    import torch

    comms = _comms(n)
    try:
        items = _stage(n, np.random.default_rng(n))
        torch.cuda.synchronize()
        took = _issue_all(items, comms)
        S._finish(orc, comms, items, ("rs sequence", n))
        check_took(took)
    finally:
        vnode.destroy(comms)


@pytest.mark.parametrize("n", [4, 8])
def test_sequence_across_two_streams(orc, n):
    import torch

    comms = _comms(n)
    streams = [torch.cuda.current_stream(), torch.cuda.Stream()]
    try:
        rng = np.random.default_rng(10 + n)
        items = _stage(n, rng)
        torch.cuda.synchronize()
        check_took(_issue_all(items, comms, lambda: streams[int(rng.integers(0, 2))]))
        S._finish(orc, comms, items, ("rs streams", n))
    finally:
        vnode.destroy(comms)


@pytest.mark.parametrize("n", [4, 8])
def test_sequence_graph_replayed_three_times(orc, n):
    """Issued once eagerly (the first launch of a kernel loads its code
    object, which a capture cannot), then captured into one HIP graph and
    replayed three times with rewritten inputs: E_IN, the launch count and the
    parity in the control block keep counting across the replays."""
    import torch

    comms = _comms(n)
    try:
        rng = np.random.default_rng(20 + n)
        items = _stage(n, rng)
        torch.cuda.synchronize()
        check_took(_issue_all(items, comms))
        S._finish(orc, comms, items, ("rs eager", n))
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            took = _issue_all(items, comms)
        check_took(took)
        for rep in range(3):
            _refill(items, n, rng, rep)
            torch.cuda.synchronize()
            g.replay()
            S._finish(orc, comms, items, ("rs graph", n, rep))
        del g
    finally:
        vnode.destroy(comms)


def _free_port() -> int:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


@pytest.mark.parametrize("world", [2, 3])
def test_sequence_one_rank_per_process(world):
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.join(HERE, "rs_direct_worker.py")]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("MCCS_ONESHOT_BYTES", "MCCS_DIRECT_BYTES", "MCCS_LL_BYTES", "MCCS_RS_DIRECT_BYTES", "MCCS_RS_LL_BYTES",
              "MCCS_A2A_LL_BYTES", "MCCS_A2AV_LL_BYTES"):
        env.pop(k, None)
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=240, env=env, cwd=os.path.dirname(HERE))
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    lib_lines = "\n".join(l for l in (r.stdout + r.stderr).splitlines() if "mccs" in l.lower() or "hip" in l)[-3000:]
    assert r.returncode == 0 and lines, lib_lines + "\n----\n" + r.stdout[-2000:] + r.stderr[-2000:]
    res = json.loads(lines[-1])
    bad = [k for k, v in res["checks"].items() if not v]
    assert res["all_ok"] and not bad, bad
    assert res["world"] == world and len(res["checks"]) == len(sequence(world))
    algos = [k.split("/")[1] + ":" + k.split("/")[-1] for k in res["checks"]]
    assert {"rs:oneshot", "rs:ll", "rs:ring", "ar:direct", "ag:ll", "a2a:ll"} <= set(algos), algos
