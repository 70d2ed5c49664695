"""CPU: the host-thread ring's Send/Recv (mccs_host_ring_send_recv: the
planner's pairing of a group's calls, walked over the FIFO protocol as the
kernel walks it) against tests/sr_ref.py.  Every buffer sits inside a 0xA5
frame that must survive; send buffers must come back unchanged.
"""
import numpy as np
import pytest

import a2a_ref
import a2av_ref as V
import sr_ref as SR
from mccs_amd import comm as C
from mccs_amd._lib import MccsError

INVALID_ARGUMENT, INVALID_USAGE = 4, 5
NS = [2, 3, 4, 5, 7, 8]


def rings_m(n, channels=0):
    rings = C.default_rings(n, channels)
    return rings, a2a_ref.route(n, rings)["m"]


def host_ops(ops, bufs):
    return [(o.rank, o.kind, o.peer, a.ctypes.data + sl.start, o.nbytes) for o, (a, sl) in zip(ops, bufs)]


def run(n, ops, rings, nthreads=544):
    bufs = SR.frames(ops)
    C.host_ring_send_recv(n, host_ops(ops, bufs), len(rings), nthreads, SR.BUFF, rings)
    SR.check(ops, bufs)


@pytest.mark.parametrize("n", NS)
def test_every_pattern_byte_for_byte(n):
    rings, m = rings_m(n)
    for name, ops in SR.patterns(n, m, rings).items():
        run(n, ops, rings)


@pytest.mark.parametrize("n", NS)
def test_a_ring_shift_equals_all_to_all_v(n):
    rings, m = rings_m(n)
    B = 2 * V.loop_bytes(m) + 999
    ops = [op for r in range(n) for op in (SR.S(r, (r + 1) % n, B), SR.R(r, (r - 1) % n, B))]
    bufs = SR.frames(ops)
    C.host_ring_send_recv(n, host_ops(ops, bufs), len(rings), 544, SR.BUFF, rings)
    SR.check(ops, bufs)
    cnt = SR.shift_matrix(n, B)
    zero = [[0] * n for _ in range(n)]
    sends = [bufs[2 * r][0][bufs[2 * r][1]].copy() for r in range(n)]
    outs = [np.full(B, SR.SENTINEL, np.uint8) for _ in range(n)]
    C.host_ring_all_to_all_v(sends, outs, cnt, zero, zero, len(rings), 544, SR.BUFF, rings)
    for r in range(n):
        a, sl = bufs[2 * r + 1]
        assert a[sl].tobytes() == outs[r].tobytes(), r


def test_other_thread_counts_change_the_granule_not_the_result():
    rings, m = rings_m(4)
    for nthr in (96, 288):
        run(4, SR.patterns(4, m, rings)["a_all_pairs"], rings, nthreads=nthr)


def test_twelve_messages_on_one_pair():
    rings, m = rings_m(2)
    v = [x for x in V.values(m) if x] + [0, 17, 4099, 1, 33]
    ops = [SR.S(0, 1, b) for b in v] + [SR.R(1, 0, b) for b in v] + [SR.S(1, 0, 4099), SR.R(0, 1, 4099)]
    assert len(v) == 12
    run(2, ops, rings)


def test_user_rings_with_complete_arcs():
    rings = [[(i * k) % 5 for i in range(5)] for k in (1, 2, 3, 4)]
    for rs in (rings, rings + rings):  # m = 1, m = 2
        m = a2a_ref.route(5, rs)["m"]
        for ops in SR.patterns(5, m, rs).values():
            run(5, ops, rs)


@pytest.mark.parametrize("how", ["six ranks", "one channel", "incomplete user rings"])
def test_refuses_a_route_that_is_not_one_hop(how):
    n = 6 if how == "six ranks" else 5 if how == "incomplete user rings" else 4
    rings = {"six ranks": C.default_rings(6), "one channel": C.default_rings(4, 1),
             "incomplete user rings": [[(i * 2) % 5 for i in range(5)]] * 3}[how]
    ops = [SR.S(0, 1, 16), SR.R(1, 0, 16)]
    bufs = SR.frames(ops)
    with pytest.raises(MccsError) as ei:
        C.host_ring_send_recv(n, host_ops(ops, bufs), len(rings), 544, SR.BUFF, rings)
    assert ei.value.code == INVALID_USAGE
    assert (bufs[1][0] == SR.SENTINEL).all()


def test_argument_refusals():
    rings = C.default_rings(2)
    a = np.zeros(64, np.uint8)
    p = a.ctypes.data

    def refused(n, ops, rs=rings):
        with pytest.raises(MccsError) as ei:
            C.host_ring_send_recv(n, ops, len(rs), 544, SR.BUFF, rs)
        assert ei.value.code == INVALID_ARGUMENT, ei.value.code

    refused(1, [], [[0]])  # one rank has no peer
    refused(2, [(0, "send", 2, p, 8), (1, "recv", 0, p + 32, 8)])  # peer out of range
    refused(2, [(2, "send", 1, p, 8)])  # rank out of range
    refused(2, [(0, "send", 0, p, 8), (0, "recv", 0, p + 32, 8)])  # self send
    refused(2, [(0, "send", 1, None, 8), (1, "recv", 0, p, 8)])  # NULL buffer with bytes
    refused(2, [(0, "send", 1, p, 8)])  # no receive
    refused(2, [(0, "send", 1, p, 8), (1, "recv", 0, p + 32, 9)])  # sizes differ
    refused(2, [(0, "send", 1, p, 8), (1, "recv", 0, p + 32, 8)], [[0, 0]])  # not a permutation
    with pytest.raises(ValueError):
        C.host_ring_send_recv(2, [(0, "put", 1, p, 8)], len(rings), 544, SR.BUFF, rings)
    # allowed: nothing at all, and zero bytes without buffers
    C.host_ring_send_recv(2, [], len(rings), 544, SR.BUFF, rings)
    C.host_ring_send_recv(2, [(0, "send", 1, None, 0), (1, "recv", 0, None, 0)], len(rings), 544, SR.BUFF, rings)
    assert not a.any()
