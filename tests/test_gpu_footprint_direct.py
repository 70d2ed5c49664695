"""GPU, virtual node: the direct and LL ReduceScatter, Reduce and Broadcast on
guarded buffers at every mix of alignments.

tests/test_gpu_footprint_collectives.py runs these cases on the ring only, and
the misalignment tests of the direct kernels (tests/test_gpu_reduce_scatter_direct.py,
tests/test_gpu_rooted_direct.py) put 32-byte bands of 0xA5 around the payload: a
store that lands 64 bytes past the output, or one that writes 0xA5-looking
bytes, is invisible to them.  Here the same cases (footprint_cases.rs_cases,
rooted_cases over roots(n)), inputs, expectations and `Buffers` run on
communicators opted in to each variant: every buffer a footprint.Guarded one
with 16 KiB pseudo-random pads, every destination prefilled with the NOT of its
expectation.  After each call `Buffers.check()` holds the result bit for bit,
every pad intact, every non-destination unchanged, and a non-root's recvbuff
(Reduce) and sendbuff (Broadcast) unchanged.

The configuration is the case's plus one-shot slots of 256 KiB and LL slots
for 128 KiB, opted in at the cap of the variant; the counts (1, n - 1, pack + 1,
4097, the alternation block) are far below both.  Every launch asserts
last_algo() on every rank; every communicator has an 8 s watchdog.
"""
import pytest

import footprint as F
import footprint_cases as K
import test_gpu_reduce_scatter_direct as D
import vnode
from mccs_amd import comm as C

pytestmark = pytest.mark.gpu
DIRECT_DEFAULTS = True  # the thresholds are set per communicator below

TIMEOUT_MS = 8000
DEV = "cuda"
VARIANTS = ["oneshot", "ll"]


def make_comms(case, variant):
    comms = C.init_all([0] * case.n, C.CommConfig(timeout_ms=TIMEOUT_MS, **D.CFG, **case.config()))
    try:  # the geometry the expectations were computed for is the communicators'
        assert comms[0].rings() == K.rings_of(case) and comms[0].lanes == case.lanes
        for c in comms:
            cap, ll_cap = c.reduce_scatter_direct_max()
            assert (cap, ll_cap) == c.rooted_direct_max() == (D.ONESHOT, D.LL_BYTES)
            if variant == "oneshot":
                c.set_reduce_scatter_direct(block_bytes=cap)
                c.set_rooted_direct(bcast_bytes=cap, reduce_bytes=cap)
            else:
                c.set_reduce_scatter_direct(ll_block_bytes=ll_cap)
                c.set_rooted_direct(bcast_ll_bytes=ll_cap, reduce_ll_bytes=ll_cap)
    except BaseException:
        vnode.destroy(comms)
        raise
    return comms


def launch(comms, case, send, recv, variant):
    with C.group():
        for r, c in enumerate(comms):
            if case.func == "rs":
                C.reduce_scatter(c, send[r], recv[r], case.count, case.code, K.SUM)
            elif case.func == "rd":
                C.reduce(c, send[r], recv[r], case.count, case.code, K.SUM, case.root)
            else:
                C.broadcast(c, send[r] or None, recv[r], case.count, case.root)
    algos = [c.last_algo() for c in comms]
    assert algos == [variant] * case.n, (case.tag(), algos)
    for c in comms:
        c.sync()


def sweep(orc, cases, variant):
    """Every case, on one set of communicators per configuration; the failures."""
    bad = {}
    for key in dict.fromkeys(c.comm_key() for c in cases):
        group = [c for c in cases if c.comm_key() == key]
        comms = make_comms(group[0], variant)
        try:
            for case in group:
                assert case.func in ("rs", "rd", "bc") and case.count * K.ESIZE[case.code] <= D.LL_BYTES
                b = K.Buffers(case, K.inputs(case), K.expected(orc, case), DEV)
                launch(comms, case, b.send, b.recv, variant)
                for r, msg in b.check().items():
                    bad[case.tag() + (r,)] = msg
        finally:
            vnode.destroy(comms)
    return bad


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("n", [2, 3, 8])
def test_reduce_scatter_direct_footprint(orc, n, variant):
    """Counts {1, n-1, pack+1, 4097} and the alternation block, fp16, fp32,
    int8 (int64 at n = 2), every offset assignment, out of place and in place
    (recv = send + r * count: only the rank's own block may change)."""
    cases = K.rs_cases(n)
    assert {c.inplace for c in cases} == {False, True}
    bad = sweep(orc, cases, variant)
    assert not bad, F.brief(bad)


ROOTED = [(n, root) for n in (2, 3, 8) for root in K.roots(n)]


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("func", ["bc", "rd"])
@pytest.mark.parametrize("n,root", ROOTED, ids=[f"n{n}-root{root}" for n, root in ROOTED])
def test_rooted_direct_footprint(orc, func, n, root, variant):
    """Reduce: every non-root's guarded recvbuff stays unchanged, in place at
    the root.  Broadcast: null sendbuff off the root, in place at the root.
    Only the root, only the chain's last rank and all but the root misaligned."""
    cases = K.rooted_cases(func, n, root)
    assert {c.inplace for c in cases} == {False, True}
    bad = sweep(orc, cases, variant)
    assert not bad, F.brief(bad)
