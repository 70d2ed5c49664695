"""CPU: what the sequence of tests/test_gpu_rooted_sequences.py contains, and
that its expected values match the host ring.

The GPU tests take the sequence as given; here it is held to what they are
for: every function occurs, the rooted calls use at least three distinct roots
(so the connection left idle changes), AllReduces of both routes are present,
and most calls take more than one loop of the 64 KiB FIFO buffer.
"""
import numpy as np
import pytest

from mccs_amd import comm as C
import test_gpu_rooted_sequences as S
import vnode


@pytest.mark.parametrize("n", [2, 4, 8])
def test_sequence_contents(n):
    seq = S.sequence(S.SEED, n)
    assert seq == S.sequence(S.SEED, n)  # a pure function of (seed, n)
    assert len(seq) >= 12
    kinds = [c["kind"] for c in seq]
    assert set(kinds) == {"bc", "rd", "ar", "ard", "ag", "rs"}
    for kind in ("bc", "rd"):
        roots = {c["root"] for c in seq if c["kind"] == kind}
        assert all(0 <= r < n for r in roots)
    roots = {c["root"] for c in seq if c["kind"] in ("bc", "rd")}
    assert len(roots) >= min(3, n), roots
    assert any(c["inplace"] for c in seq) and any(not c["inplace"] for c in seq if c["kind"] in ("bc", "rd"))
    for c in seq:  # the route each AllReduce is meant to take under S.CFG
        nbytes = c["count"] * vnode.ESIZE[c["code"]]
        if c["kind"] == "ar":
            assert nbytes > S.CFG["oneshot_bytes"] and S.CFG["direct_bytes"] < 0
        if c["kind"] == "ard":
            assert nbytes <= S.CFG["ll_bytes"]
        if c["kind"] == "ag":
            assert nbytes > S.CFG["oneshot_bytes"]
    # several loops: a rooted call of more than channels x 32 KiB
    nch = len(C.default_rings(n))
    loop = nch * (S.BUFF // 2)
    assert sum(1 for c in seq if c["kind"] in ("bc", "rd") and c["count"] * vnode.ESIZE[c["code"]] > loop) >= 2


@pytest.mark.parametrize("n", [2, 4])
def test_rooted_expected_values_match_the_host_ring(orc, n):
    """call_expected for the sequence's Broadcasts and Reduces against
    mccs_host_ring_broadcast / mccs_host_ring_reduce with the planner's
    channels and threads."""
    rings = C.default_rings(n)
    rng = np.random.default_rng(n)
    for call in S.sequence(S.SEED, n):
        if call["kind"] not in ("bc", "rd"):
            continue
        xs = [S.call_input(call, n, rng) for _ in range(n)]
        exp = S.call_expected(orc, call, xs, len(rings), rings)
        nbytes = call["count"] * vnode.ESIZE[call["code"]]
        nch, nthr, sel = vnode.Planner(len(rings), rings).select(nbytes, nbytes)
        if call["kind"] == "bc":
            recvs = [np.zeros(nbytes, np.uint8) for _ in range(n)]
            sends = [xs[r] if r == call["root"] else None for r in range(n)]
            C.host_ring_broadcast(sends, recvs, nbytes, call["root"], channels=nch, nthreads=nthr, buffer_size=S.BUFF,
                                  rings=sel)
            for r in range(n):
                assert recvs[r].tobytes() == exp[r].tobytes(), (call, r)
        else:
            recvs = [np.zeros_like(xs[r]) if r == call["root"] else None for r in range(n)]
            C.host_ring_reduce(xs, recvs, call["count"], call["code"], call["op"], call["root"], channels=nch,
                               nthreads=nthr, buffer_size=S.BUFF, rings=sel)
            assert recvs[call["root"]].tobytes() == exp[call["root"]].tobytes(), call
