"""CPU: the AllToAll schedule and FIFO protocol on host threads
(mccs_host_ring_all_to_all: the walk of ring_walk.h a2a_call and the route of
mccs_alltoall_route, as the kernels take them), against the block transpose of
tests/a2a_ref.py.  Receive buffers sit between 0xA5 sentinels, send buffers
must come back unchanged.
"""
import numpy as np
import pytest

import a2a_ref
from mccs_amd import comm as C

BUFF = 1 << 16  # 8 KiB steps: a chunk is 32 KiB


def run(n, B, rings, force_relay=False, send_off=0, recv_off=0, buff_size=BUFF, nthreads=96):
    inputs = a2a_ref.make_inputs(n, B)
    sends, recvs, views = [], [], []
    for r in range(n):
        s, ssl = a2a_ref.sentinel_frame(n * B, 16 + (send_off + r) % 16)
        s[ssl] = inputs[r]
        d, dsl = a2a_ref.sentinel_frame(n * B, 16 + (recv_off + 3 * r) % 16)
        sends.append((s, ssl))
        recvs.append((d, dsl))
        views.append((s[ssl].ctypes.data, d[dsl].ctypes.data))
    C.host_ring_all_to_all([v[0] for v in views], [v[1] for v in views], B, len(rings), nthreads, buff_size, rings,
                           force_relay)
    want = a2a_ref.expected(inputs, B)
    for r in range(n):
        d, dsl = recvs[r]
        bad = np.flatnonzero(d[dsl] != want[r])
        assert bad.size == 0, f"rank {r}: {bad.size} wrong bytes, first at {bad[0]} (block {bad[0] // max(B, 1)})"
        assert (d[:dsl.start] == a2a_ref.SENTINEL).all() and (d[dsl.stop:] == a2a_ref.SENTINEL).all(), r
        s, ssl = sends[r]
        assert (s[ssl] == inputs[r]).all() and (s[:ssl.start] == a2a_ref.SENTINEL).all() and \
            (s[ssl.stop:] == a2a_ref.SENTINEL).all(), r


@pytest.mark.parametrize("B", [1, 15, 4099, 65537])
@pytest.mark.parametrize("n", [2, 3, 4, 5, 6, 7, 8])
def test_default_rings(n, B):
    run(n, B, C.default_rings(n))


@pytest.mark.parametrize("B", [1, 15, 4099, 65537])
@pytest.mark.parametrize("n", [3, 4, 8])
def test_forced_relay(n, B):
    run(n, B, C.default_rings(n), force_relay=True)


@pytest.mark.parametrize("B", [1, 15, 4099, 65537])
def test_one_channel(B):
    run(4, B, C.default_rings(4, 1))


@pytest.mark.parametrize("n,ch,relay", [(2, 0, False), (4, 0, False), (8, 14, False), (6, 0, False), (8, 0, True)])
def test_fewer_bytes_than_channels(n, ch, relay):
    """B below the channel count: channels past the end of the block make empty
    calls that still take and post their steps."""
    rings = C.default_rings(n, ch)
    m = C.alltoall_route(n, len(rings), rings, relay)["m"] or len(rings)
    assert m >= 2
    run(n, m - 1, rings, force_relay=relay)
    run(n, 1, rings, force_relay=relay)


@pytest.mark.parametrize("send_off,recv_off", [(1, 15), (7, 2), (15, 8), (3, 3)])
def test_misaligned_buffers(send_off, recv_off):
    for n, relay in ((4, False), (3, True), (8, False)):
        run(n, 4099, C.default_rings(n), force_relay=relay, send_off=send_off, recv_off=recv_off)


@pytest.mark.parametrize("n,ch,relay", [(2, 0, False), (8, 0, False), (4, 0, False), (4, 0, True), (3, 0, True)])
def test_three_loops(n, ch, relay):
    """buff_size = 1 << 16 gives 32 KiB chunks: B = 2*m*32768 + 999 is two full
    loops of the m channels and a short third."""
    rings = C.default_rings(n, ch)
    m = C.alltoall_route(n, len(rings), rings, relay)["m"] or len(rings)
    B = 2 * m * 32768 + 999
    walk = C.ring_walk(C.FUNC_ALLGATHER, n, m, 1, 96, BUFF, B)
    assert len({g for g, _, _, _ in walk}) == 3
    run(n, B, rings, force_relay=relay)


def test_more_threads_change_the_granule_not_the_result():
    run(4, 70001, C.default_rings(4), nthreads=544)
    run(5, 70001, C.default_rings(5), nthreads=288, force_relay=True)


def test_one_rank_and_zero_bytes():
    run(1, 4099, C.default_rings(1))
    run(4, 0, C.default_rings(4))


def test_user_rings_with_complete_arcs():
    rings = [[(i * k) % 5 for i in range(5)] for k in (1, 2, 3, 4)]
    run(5, 4099, rings)
    run(5, 4099, rings + rings)  # m = 2
    run(5, 4099, [rings[1]] * 3)  # incomplete: relay over three copies of one ring
