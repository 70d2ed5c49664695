"""GPU, virtual node: ReduceScatter, Reduce, Broadcast, AllToAll and the
AllGather alternation case on guarded buffers at every mix of alignments.

What tests/test_gpu_footprint.py does for AllReduce and AllGather, for the
schedules whose operand base moves by one block per call: when a block's byte
size is no multiple of 16 the slices of one work element alternate between
the 16-byte pack path and the typed loop of ring_stream.h
reduce_copy_rows_dyn, and the unit counter of each parity has to stay
consistent across that.  The cases, the model of the path every slice takes
and the buffers are tests/footprint_cases.py's; tests/test_footprint_cases.py
asserts on the CPU what the cases cover and runs them on the host-thread ring.

Every buffer is a footprint.Guarded one, every destination prefilled with the
NOT of its expectation.  After each call the result equals the reference bit
for bit, every pad is intact and every buffer that is no destination is
unchanged.  Every test asserts from the model that the paths it is meant to
reach were reached, that the ring ran and, for AllToAll, the route.  Ring
only; every communicator has an 8 s watchdog.  The last section calls the
unmodified kernels with one element too many on buffers guarded for `count`.
"""
import numpy as np
import pytest

import a2a_ref
import footprint as F
import footprint_cases as K
import vnode
from footprint import Guarded
from footprint_cases import F16, F32, I8, ROOTED_PATHS, SUM, SWEEP_PATHS
from mccs_amd import comm as C

pytestmark = pytest.mark.gpu
DIRECT_DEFAULTS = True  # conftest: thresholds are set per communicator below

RING_ONLY = dict(direct_bytes=-1, oneshot_bytes=-1, ll_bytes=-1)
TIMEOUT_MS = 8000
DEV = "cuda"
NO_ALT = SWEEP_PATHS - {"alternation", "alternation by block base"}


def make_comms(case, monkeypatch):
    if case.relay:
        monkeypatch.setenv("MCCS_ALLTOALL_HOPS", "relay")
    else:
        monkeypatch.delenv("MCCS_ALLTOALL_HOPS", raising=False)
    comms = C.init_all([0] * case.n, C.CommConfig(timeout_ms=TIMEOUT_MS, **RING_ONLY, **case.config()))
    try:  # the model's geometry is the communicators'
        assert comms[0].rings() == K.rings_of(case) and comms[0].lanes == case.lanes
        if case.func == "a2a":
            route = a2a_ref.route(case.n, comms[0].rings(), case.relay)
            assert all(c.all_to_all_route() == {"hops": route["hops"], "m": route["m"]} for c in comms)
    except BaseException:
        vnode.destroy(comms)
        raise
    return comms


def issue(comm, case, send, recv, count=None):
    count = case.count if count is None else count
    if case.func == "rs":
        C.reduce_scatter(comm, send, recv, count, case.code, SUM)
    elif case.func == "rd":
        C.reduce(comm, send, recv, count, case.code, SUM, case.root)
    elif case.func == "bc":
        C.broadcast(comm, send or None, recv, count, case.root)
    elif case.func == "ag":
        C.all_gather(comm, send, recv, count)
    else:
        C.all_to_all(comm, send, recv, count)


def launch(comms, case, send, recv, count=None):
    with C.group():
        for r, c in enumerate(comms):
            issue(c, case, send[r], recv[r], count)
    for c in comms:
        c.sync()
    algos = {c.last_algo() for c in comms}
    assert algos == {"ring"}, algos


def sweep(orc, monkeypatch, cases):
    """Every case, on one set of communicators per configuration.  Returns
    (failures, paths reached)."""
    bad = {}
    keys = list(dict.fromkeys(c.comm_key() for c in cases))
    for key in keys:
        group = [c for c in cases if c.comm_key() == key]
        comms = make_comms(group[0], monkeypatch)
        try:
            for case in group:
                b = K.Buffers(case, K.inputs(case), K.expected(orc, case), DEV)
                launch(comms, case, b.send, b.recv)
                for r, msg in b.check().items():
                    bad[case.tag() + (r,)] = msg
        finally:
            vnode.destroy(comms)
    return bad, K.reached(cases)


# =====================================================================================
# the sweeps
# =====================================================================================
@pytest.mark.parametrize("n", [2, 3, 8])
def test_reduce_scatter_footprint(orc, monkeypatch, n):
    """Counts {1, n-1, pack+1, 4097} and the alternation block, fp16, fp32,
    int8 (int64 at n = 2), every offset assignment, out of place and in place
    (recv = send + r * count: only the rank's own block may change)."""
    bad, reached = sweep(orc, monkeypatch, K.rs_cases(n))
    assert not bad, F.brief(bad)
    assert reached >= (NO_ALT if n == 2 else SWEEP_PATHS), reached  # n = 2: two slices per loop, one base each


ROOTED = [(n, root) for n in (2, 3, 8) for root in K.roots(n)]


@pytest.mark.parametrize("func", ["bc", "rd"])
@pytest.mark.parametrize("n,root", ROOTED, ids=[f"n{n}-root{root}" for n, root in ROOTED])
def test_rooted_footprint(orc, monkeypatch, func, n, root):
    """Reduce: every non-root's guarded recvbuff stays unchanged, in place at
    the root.  Broadcast: null sendbuff off the root, in place at the root.
    Only the root, only the chain's last rank and all but the root misaligned:
    ranks of one chain on different paths."""
    bad, reached = sweep(orc, monkeypatch, K.rooted_cases(func, n, root))
    assert not bad, F.brief(bad)
    assert reached >= ROOTED_PATHS, reached


A2A_PATHS = {"n2": NO_ALT - {"tail"}, "n4": NO_ALT, "n8": NO_ALT, "n6": SWEEP_PATHS, "n3-relay": SWEEP_PATHS}


@pytest.mark.parametrize("shape", list(K.A2A_SHAPES))
def test_all_to_all_footprint(orc, monkeypatch, shape):
    """B in {1, 15, 4099, the alternation size}, independent per-rank send
    and receive offsets; the self block (a2a_self_copy) is checked like the
    rest.  A one-hop element reads one block and writes one: no alternation."""
    bad, reached = sweep(orc, monkeypatch, K.a2a_cases(shape))
    assert not bad, F.brief(bad)
    assert reached >= A2A_PATHS[shape], reached


def test_allgather_alternation_footprint(orc, monkeypatch):
    bad, reached = sweep(orc, monkeypatch, K.ag_alternation_cases())
    assert not bad, F.brief(bad)
    assert reached >= {"alternation", "alternation by block base", "units", "typed", "tail"}, reached


@pytest.mark.parametrize("half", ["same on all ranks", "differing per rank"])
@pytest.mark.parametrize("func", ["rs", "a2a"])
@pytest.mark.parametrize("n", [2, 3, 8])
def test_several_loops_footprint(orc, monkeypatch, func, n, half):
    """A 1 MiB buffer on one channel of 4 lanes, two whole loops and a
    partial third: the alternation goes on across loops.  Two offset
    assignments per case (aligned buffers and per-rank offsets; one
    misaligned receive buffer and, for ReduceScatter, in place)."""
    cases = K.loops_cases(func, n)
    cases = cases[:2] if half == "same on all ranks" else cases[2:]
    bad, reached = sweep(orc, monkeypatch, cases)
    assert not bad, F.brief(bad)
    alternation = "alternation by block base" if half == "same on all ranks" else "alternation"
    assert reached >= {"units", "typed", "tail"} | ({alternation} if n > 2 else set()), reached


@pytest.mark.parametrize("func", ["rs", "a2a"])
@pytest.mark.parametrize("shape", list(K.LAUNCH_SHAPES))
def test_launch_shapes_footprint(orc, monkeypatch, func, shape):
    bad, reached = sweep(orc, monkeypatch, K.launch_shape_cases(func, shape))
    assert not bad, F.brief(bad)
    assert reached >= {"typed", "packs", "tail"}, reached


@pytest.mark.parametrize("order", ["typed first", "units first"])
def test_two_elements_in_one_launch(orc, monkeypatch, order):
    """Two ReduceScatters per communicator in one group: the unit counters
    and every wave's bases restart per element."""
    pair = K.two_element_cases()
    assert K.reached([pair[0]]) == {"typed"} and K.reached([pair[1]]) >= {"units", "tail"}
    assert K.elements(pair[0])[0] == K.elements(pair[1])[0]  # equal thread counts: one work
    if order == "units first":
        pair = pair[::-1]
    comms = make_comms(pair[0], monkeypatch)
    try:
        bufs = [K.Buffers(case, K.inputs(case), K.expected(orc, case), DEV) for case in pair]
        with C.group():
            for r, c in enumerate(comms):
                for case, b in zip(pair, bufs):
                    issue(c, case, b.send[r], b.recv[r])
        for c in comms:
            c.sync()
        assert {c.last_algo() for c in comms} == {"ring"}
        bad = {(case.name, r): msg for case, b in zip(pair, bufs) for r, msg in b.check().items()}
        assert not bad, F.brief(bad)
    finally:
        vnode.destroy(comms)


# =====================================================================================
# positive controls: the unmodified kernels asked for one element more
# =====================================================================================
def planted(exp_plus, lo, hi):
    """The NOT of bytes [lo, hi) of the larger call's result (what the pad
    holds there before the call)."""
    return ~np.ascontiguousarray(exp_plus).view(np.uint8).reshape(-1)[lo:hi]


CONTROL_OFFS = [0, "es"]


@pytest.mark.parametrize("off", CONTROL_OFFS, ids=["aligned", "misaligned"])
@pytest.mark.parametrize("code,count", [(F16, 4097), (F32, 4 * 1025 - 1)], ids=["typed tail", "pack"])
def test_control_reduce_scatter_one_element_too_many(orc, monkeypatch, code, count, off):
    n, es = 3, K.ESIZE[code]
    off = es if off == "es" else 0
    more = K.Case("rs", n, code, count + 1, ((off, off),) * n, **K.ONE_CH)
    comms = make_comms(more, monkeypatch)
    try:
        xs = K.inputs(more)
        exp = K.expected(orc, more)
        send = [Guarded(xs[r].nbytes, off, DEV) for r in range(n)]
        recv = [Guarded(count * es, off, DEV) for _ in range(n)]
        for r in range(n):
            send[r].write(xs[r])
            recv[r].prefill_not(exp[r][:count])
            recv[r].poke(count * es, planted(exp[r], count * es, (count + 1) * es))
        launch(comms, more, [g.ptr for g in send], [g.ptr for g in recv])
        for r in range(n):
            assert recv[r].check().tolist() == list(range(count * es, (count + 1) * es)), r
            assert "wrote outside" in recv[r].pads_message()
            assert not F.diff_message(recv[r].read(), exp[r][:count]), r
            assert send[r].unchanged(), r
    finally:
        vnode.destroy(comms)


@pytest.mark.parametrize("off", CONTROL_OFFS, ids=["aligned", "misaligned"])
def test_control_reduce_one_element_too_many(orc, monkeypatch, off):
    n, code, count, root = 3, F16, 4097, 1
    es = K.ESIZE[code]
    off = es if off == "es" else 0
    more = K.Case("rd", n, code, count + 1, ((off, off),) * n, root=root, **K.ONE_CH)
    comms = make_comms(more, monkeypatch)
    try:
        xs = K.inputs(more)
        exp = K.expected(orc, more)[root]
        send = [Guarded(xs[r].nbytes, off, DEV) for r in range(n)]
        recv = [Guarded(count * es, off, DEV) for _ in range(n)]
        for r in range(n):
            send[r].write(xs[r])
        recv[root].prefill_not(exp[:count])
        recv[root].poke(count * es, planted(exp, count * es, (count + 1) * es))
        launch(comms, more, [g.ptr for g in send], [g.ptr for g in recv])
        assert recv[root].check().tolist() == list(range(count * es, (count + 1) * es))
        assert not F.diff_message(recv[root].read(), exp[:count])
        for r in range(n):
            assert send[r].unchanged(), r
            assert r == root or recv[r].unchanged(), r  # root only
    finally:
        vnode.destroy(comms)


@pytest.mark.parametrize("off", CONTROL_OFFS, ids=["aligned", "misaligned"])
def test_control_broadcast_one_byte_too_many(monkeypatch, off):
    n, nbytes, root = 3, 4099, 2
    off = 1 if off == "es" else 0
    more = K.Case("bc", n, I8, nbytes + 1, ((off, off),) * n, root=root, **K.ONE_CH)
    comms = make_comms(more, monkeypatch)
    try:
        data = K.inputs(more)[root]
        send = Guarded(nbytes + 1, off, DEV)
        send.write(data)
        recv = [Guarded(nbytes, off, DEV) for _ in range(n)]
        for g in recv:
            g.prefill_not(data[:nbytes])
            g.poke(nbytes, planted(data, nbytes, nbytes + 1))
        launch(comms, more, [send.ptr if r == root else 0 for r in range(n)], [g.ptr for g in recv])
        for r in range(n):  # every rank
            assert recv[r].check().tolist() == [nbytes], r
            assert not F.diff_message(recv[r].read(), data[:nbytes]), r
        assert send.unchanged()
    finally:
        vnode.destroy(comms)


@pytest.mark.parametrize("off", CONTROL_OFFS, ids=["aligned", "misaligned"])
def test_control_all_to_all_one_byte_too_many(orc, monkeypatch, off):
    """B + 1 bytes per peer into a buffer guarded for n * B: exactly the n
    bytes past it."""
    n, B = 2, 4099
    off = 1 if off == "es" else 0
    more = K.Case("a2a", n, I8, B + 1, ((off, off),) * n)
    comms = make_comms(more, monkeypatch)
    try:
        xs = K.inputs(more)
        exp = K.expected(orc, more)
        send = [Guarded(n * (B + 1), off, DEV) for _ in range(n)]
        recv = [Guarded(n * B, off, DEV) for _ in range(n)]
        for r in range(n):
            send[r].write(xs[r])
            recv[r].prefill_not(exp[r][:n * B])
            recv[r].poke(n * B, planted(exp[r], n * B, n * (B + 1)))
        launch(comms, more, [g.ptr for g in send], [g.ptr for g in recv])
        for r in range(n):
            assert recv[r].check().tolist() == list(range(n * B, n * B + n)), r
            assert not F.diff_message(recv[r].read(), exp[r][:n * B]), r
            assert send[r].unchanged(), r
    finally:
        vnode.destroy(comms)
