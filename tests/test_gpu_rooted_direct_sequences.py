"""GPU: the direct and LL Broadcast and Reduce between the launches that share
their slots, E_IN, the parity and the launch count, on one set of
communicators; every result byte for byte (expected values: tests/rooted_ref.py,
tests/rs_ref.py and the oracle, through tests/test_gpu_rooted_sequences.py's
call_expected).

A rooted call moves data on n-1 ordered pairs only; what keeps the slots'
parity reuse and the single E_IN word valid is that every pair hands off in
every launch all the same (csrc/ring_cfg.h, "Direct Broadcast and Reduce").
The sequence is the test of that: it opens with 2n consecutive direct rooted
calls whose root rotates on every call (0, 1, ..., n-1, 0, ...) through all
four modes with fresh payloads, so both parities are reused under every root
change; then rooted calls (the root still rotating) alternate with direct and
LL ReduceScatters, one-shot, two-shot and LL AllReduces, both AllGathers, an LL
AllToAll, an oversized ring Broadcast and an oversized ring Reduce; a ring
AllToAll closes it, which needs every FIFO connection in step -- a direct
rooted call takes no FIFO step (the two ring rooted calls run before it as
they would without this feature, and the ring AllToAll after a ring rooted call
is tests/test_gpu_all_to_all_sequences.py's ground).  No sync in between.

It runs on one stream, across two streams, in a HIP graph replayed three times
with rewritten inputs, and with one rank per process at n = 2 and 3
(tests/rooted_direct_worker.py).  64 KiB FIFO buffer, one-shot slots of
256 KiB, LL to 32 KiB, two-shot to 2 MiB; the rooted limits are the one-shot
cap and 16 KiB (LL wins below it), for both functions.
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
ROOTED_LL = 16 << 10
CFG = dict(buffer_size=S.BUFF, oneshot_bytes=ONESHOT, ll_bytes=LL_BYTES, direct_bytes=TWOSHOT)
I8, I32, F16, F32, BF16 = 0, 2, 6, 7, 9
SUM, PROD, MAX, MIN = 0, 1, 2, 3


def opt_in(comm):
    assert comm.rooted_direct_max() == (ONESHOT, LL_BYTES)
    comm.set_rooted_direct(bcast_bytes=ONESHOT, bcast_ll_bytes=ROOTED_LL, reduce_bytes=ONESHOT,
                           reduce_ll_bytes=ROOTED_LL)
    comm.set_reduce_scatter_direct(block_bytes=ONESHOT, ll_block_bytes=ROOTED_LL)
    comm.set_all_to_all_ll(bytes_per_peer=comm.all_to_all_ll_max())


def _comms(n):
    comms = C.init_all([0] * n, C.CommConfig(timeout_ms=S.TIMEOUT_MS, **CFG))
    for c in comms:
        opt_in(c)
    return comms


# (kind, variant) -> sizes in bytes the opening run cycles through
OPENING = {("bc", "oneshot"): [100001, 20000, ONESHOT, 16385], ("rd", "oneshot"): [80004, 17000, 262144, 120000],
           ("bc", "ll"): [4099, 1, 16384, 777], ("rd", "ll"): [4000, 8, 16384, 1028]}
RD_TYPES = [(F32, SUM), (F16, MAX), (I32, SUM), (BF16, MIN), (F32, PROD)]


def sequence(n):
    """The calls of one sequence, the same on every rank: S's call dicts
    (count: elements; bytes for bc / ag / a2a; per block for rs) plus `algo`,
    the kernel the call must take."""
    calls, k = [], [0]

    def call(kind, count, algo, code=F32, op=SUM, **kw):
        kw.setdefault("root", None)
        kw.setdefault("inplace", False)
        calls.append(dict(kind=kind, code=code, op=op, count=count, algo=algo, **kw))

    def rooted(kind, nbytes, algo, inplace=False):
        """The next rooted call: the root rotates on every one of them."""
        code, op = (I8, SUM) if kind == "bc" else RD_TYPES[k[0] % len(RD_TYPES)]
        call(kind, max(1, nbytes // vnode.ESIZE[code]), algo, code, op, root=k[0] % n, inplace=inplace)
        k[0] += 1

    modes = [("bc", "oneshot"), ("rd", "oneshot"), ("bc", "ll"), ("rd", "ll")]
    for i in range(2 * n):  # the mode shifts against the root every four calls
        kind, variant = modes[(i + i // 4) % 4]
        rooted(kind, OPENING[kind, variant][(i // 4) % 4], variant, inplace=i % 5 == 3)
    call("rs", 20000, "oneshot")
    rooted("rd", 50000, "oneshot")
    call("rs", 1000, "ll", F16)
    rooted("bc", 5000, "ll")
    call("ar", 30000, "oneshot")
    rooted("rd", 12000, "ll")
    call("ar", 200000, "direct")
    rooted("bc", 70001, "oneshot")
    call("ar", 2000, "ll")
    rooted("rd", 99996, "oneshot", inplace=True)
    call("ag", 100000, "oneshot", 0)
    rooted("bc", 333, "ll", inplace=True)
    call("ag", 5000, "ll", 0)
    rooted("rd", 16, "ll")
    call("a2a", 4099, "ll", 0, salt=3)
    rooted("bc", 31, "ll")
    rooted("bc", ONESHOT + 1, "ring")  # oversized: the ring chain
    rooted("rd", 40000, "oneshot")
    rooted("rd", ONESHOT + 4, "ring")
    rooted("bc", 200000, "oneshot")
    rooted("rd", 4, "ll")
    call("a2a", 40000, "ring", 0, salt=5)  # every FIFO connection in step
    return calls


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
        took.append((s.call["kind"], s.call["count"], comms[0].last_algo(), s.call["algo"], s.call["root"]))
    return took


def check_took(took, n):
    assert not [t for t in took if t[2] != t[3]], took
    opening = took[:2 * n]
    assert all(t[0] in ("bc", "rd") and t[2] in ("oneshot", "ll") for t in opening), opening
    assert [t[4] for t in opening] == [i % n for i in range(2 * n)]  # the root changes on every call
    assert {(t[0], t[2]) for t in took} >= {
        ("bc", "oneshot"), ("bc", "ll"), ("bc", "ring"), ("rd", "oneshot"), ("rd", "ll"), ("rd", "ring"),
        ("rs", "oneshot"), ("rs", "ll"), ("ar", "oneshot"), ("ar", "direct"), ("ar", "ll"), ("ag", "oneshot"),
        ("ag", "ll"), ("a2a", "ll"), ("a2a", "ring")}
    if n >= 4:
        assert {(t[0], t[2]) for t in opening} == {("bc", "oneshot"), ("bc", "ll"), ("rd", "oneshot"), ("rd", "ll")}
    assert took[-1][0] == "a2a" and took[-1][2] == "ring"


@pytest.mark.parametrize("n", [4, 8])
def test_sequence(orc, n):
    import torch

    comms = _comms(n)
    try:
        items = _stage(n, np.random.default_rng(n))
        torch.cuda.synchronize()
        took = _issue_all(items, comms)
        S._finish(orc, comms, items, ("rooted direct sequence", n))
        check_took(took, n)
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
        check_took(_issue_all(items, comms, lambda: streams[int(rng.integers(0, 2))]), n)
        S._finish(orc, comms, items, ("rooted direct streams", n))
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
        check_took(_issue_all(items, comms), n)
        S._finish(orc, comms, items, ("rooted direct eager", n))
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            took = _issue_all(items, comms)
        check_took(took, n)
        for rep in range(3):
            _refill(items, n, rng, rep)
            torch.cuda.synchronize()
            g.replay()
            S._finish(orc, comms, items, ("rooted direct graph", n, rep))
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
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()),
           os.path.join(HERE, "rooted_direct_worker.py")]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("MCCS_ONESHOT_BYTES", "MCCS_DIRECT_BYTES", "MCCS_LL_BYTES", "MCCS_RS_DIRECT_BYTES", "MCCS_RS_LL_BYTES",
              "MCCS_A2A_LL_BYTES", "MCCS_A2AV_LL_BYTES", "MCCS_BC_DIRECT_BYTES", "MCCS_BC_LL_BYTES",
              "MCCS_RD_DIRECT_BYTES", "MCCS_RD_LL_BYTES"):
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
    assert {"bc:oneshot", "bc:ll", "bc:ring", "rd:oneshot", "rd:ll", "rd:ring", "rs:oneshot", "rs:ll", "ar:direct",
            "ag:ll", "a2a:ll", "a2a:ring"} <= set(algos), algos
