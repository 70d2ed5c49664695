"""GPU, virtual node: mccsAllToAll against the block transpose of
tests/a2a_ref.py, byte for byte, on the default rings (one hop where they allow
it, the relay at n = 6), with the relay forced, on one channel, over several
loops, at odd sizes and alignments between 0xA5 sentinels, and for one rank.
Every communicator has an 8 s watchdog.
"""
import numpy as np
import pytest

import a2a_ref
from mccs_amd import comm as C
import vnode

pytestmark = pytest.mark.gpu
DIRECT_DEFAULTS = True  # every threshold below is explicit

TIMEOUT_MS = 8000
RING_ONLY = dict(oneshot_bytes=-1, direct_bytes=-1, ll_bytes=-1)
ROUTES = {2: (1, 4), 3: (1, 1), 4: (1, 2), 5: (1, 1), 6: (5, 0), 8: (1, 1)}  # default rings: (hops, m)


def _comms(n, monkeypatch, relay=False, **cfg):
    if relay:
        monkeypatch.setenv("MCCS_ALLTOALL_HOPS", "relay")
    else:
        monkeypatch.delenv("MCCS_ALLTOALL_HOPS", raising=False)
    return C.init_all([0] * n, C.CommConfig(timeout_ms=TIMEOUT_MS, **{**RING_ONLY, **cfg}))


def exchange(comms, B, send_off=0, recv_off=0, salt=0, tag=None):
    """One AllToAll of B bytes per peer; rank r's buffers start send_off + r /
    recv_off + 3r bytes (mod 16) past a 16-byte boundary, inside sentinels."""
    import torch

    n = len(comms)
    inputs = a2a_ref.make_inputs(n, B, salt)
    want = a2a_ref.expected(inputs, B)
    sends, recvs = [], []
    for r in range(n):
        s, ssl = a2a_ref.sentinel_frame(n * B, 16 + (send_off + r) % 16)
        s[ssl] = inputs[r]
        d, dsl = a2a_ref.sentinel_frame(n * B, 16 + (recv_off + 3 * r) % 16)
        sends.append((torch.from_numpy(s).cuda(), ssl, s))
        recvs.append((torch.from_numpy(d).cuda(), dsl))
    torch.cuda.synchronize()
    with C.group():
        for r in range(n):
            C.all_to_all(comms[r], sends[r][0][sends[r][1]], recvs[r][0][recvs[r][1]], B)
    torch.cuda.synchronize()
    for c in comms:
        c.sync()
    for r in range(n):
        d, dsl = recvs[r][0].cpu().numpy(), recvs[r][1]
        bad = np.flatnonzero(d[dsl] != want[r])
        assert bad.size == 0, (tag, f"rank {r}: {bad.size} wrong bytes, first at {bad[0]} (block {bad[0] // B})")
        assert (d[:dsl.start] == a2a_ref.SENTINEL).all() and (d[dsl.stop:] == a2a_ref.SENTINEL).all(), (tag, r)
        assert (sends[r][0].cpu().numpy() == sends[r][2]).all(), (tag, r, "send buffer written")


@pytest.mark.parametrize("n", [2, 3, 4, 5, 6, 8])
def test_default_rings(monkeypatch, n):
    comms = _comms(n, monkeypatch)
    try:
        hops, m = ROUTES[n]
        assert all(c.all_to_all_route() == {"hops": hops, "m": m} for c in comms)
        assert comms[0].all_to_all_route() == {k: a2a_ref.route(n, comms[0].rings())[k] for k in ("hops", "m")}
        exchange(comms, 70001, tag=n)
        exchange(comms, 1 << 20, salt=3, tag=n)  # every channel of a relay too
        assert all(c.last_algo() == "ring" for c in comms)
    finally:
        vnode.destroy(comms)


@pytest.mark.parametrize("n", [3, 8])
def test_forced_relay(monkeypatch, n):
    comms = _comms(n, monkeypatch, relay=True)
    try:
        assert all(c.all_to_all_route() == {"hops": n - 1, "m": 0} for c in comms)
        exchange(comms, 70001, tag=n)
        exchange(comms, 9, salt=5, tag=n)
    finally:
        vnode.destroy(comms)


def test_one_channel(monkeypatch):
    comms = _comms(4, monkeypatch, channel_count=1)
    try:
        assert comms[0].all_to_all_route() == {"hops": 3, "m": 0}
        exchange(comms, 70001)
    finally:
        vnode.destroy(comms)


@pytest.mark.parametrize("n,relay", [(2, False), (8, False), (4, True)])
def test_three_loops(monkeypatch, n, relay):
    """buffer_size = 1 << 16: 32 KiB chunks, B = 2*m*32768 + 999 is two full
    loops of a block's m channels and a short third."""
    buff = 1 << 16
    comms = _comms(n, monkeypatch, relay=relay, buffer_size=buff)
    try:
        nch = comms[0].nchannels
        m = comms[0].all_to_all_route()["m"] or nch
        B = 2 * m * 32768 + 999
        assert relay == (comms[0].all_to_all_route()["hops"] != 1)
        if relay:  # the call takes every channel: the m the size was made for
            assert C.task_schema(n * B, nch)[0] == m
        nthr = C.task_schema(n * B, nch)[1]
        assert len({g for g, _, _, _ in C.ring_walk(C.FUNC_ALLGATHER, n, m, 1, nthr, buff, B)}) == 3
        exchange(comms, B, tag=(n, relay))
    finally:
        vnode.destroy(comms)


@pytest.mark.parametrize("n,relay", [(4, False), (3, True)])
def test_odd_sizes_misaligned_buffers(monkeypatch, n, relay):
    comms = _comms(n, monkeypatch, relay=relay)
    try:
        for i, B in enumerate((1, 15, 4099)):
            for send_off, recv_off in ((1, 15), (7, 2), (13, 8)):
                exchange(comms, B, send_off, recv_off, salt=i, tag=(B, send_off, recv_off))
    finally:
        vnode.destroy(comms)


def test_fewer_bytes_than_channels(monkeypatch):
    """Channels past the end of a short block make empty calls."""
    comms = _comms(2, monkeypatch)  # m = 4
    try:
        for B in (1, 3):
            exchange(comms, B, tag=B)
    finally:
        vnode.destroy(comms)


def test_one_rank(monkeypatch):
    comms = _comms(1, monkeypatch)
    try:
        assert comms[0].all_to_all_route() == {"hops": 0, "m": 0}
        exchange(comms, 4099, send_off=5, recv_off=9)
        exchange(comms, 1 << 20)
    finally:
        vnode.destroy(comms)


def test_ring_with_the_ll_threshold_live(monkeypatch):
    import torch

    n = 4
    comms = _comms(n, monkeypatch, oneshot_bytes=256 << 10, ll_bytes=32 << 10)
    try:
        assert comms[0].fifo_memory != C.FIFO_DEVICE  # LL needs the uncached arena
        x = [torch.ones(1000, dtype=torch.float32, device="cuda") for _ in range(n)]
        y = [torch.zeros(1000, dtype=torch.float32, device="cuda") for _ in range(n)]
        with C.group():
            for r in range(n):
                C.all_reduce(comms[r], x[r], y[r], 1000, 7, 0)
        assert [c.last_algo() for c in comms] == ["ll"] * n
        exchange(comms, 1000)  # 1000 bytes per peer: LL-sized, still the ring
        assert [c.last_algo() for c in comms] == ["ring"] * n
        torch.cuda.synchronize()
        assert all(float(t[0]) == n for t in y)
    finally:
        vnode.destroy(comms)


def test_overlap_and_null_are_refused_on_the_device_path(monkeypatch):
    import torch

    comms = _comms(2, monkeypatch)
    try:
        buf = torch.zeros(8192, dtype=torch.uint8, device="cuda")
        for send, recv in ((buf, buf), (buf, buf[2047:]), (None, buf), (buf, None)):
            with pytest.raises(C._lib.MccsError) as ei:
                C.all_to_all(comms[0], send, recv, 1024)
            assert ei.value.code == 4
        C.all_to_all(comms[0], buf, buf, 0)  # nothing to do, nothing launched
        exchange(comms, 4099)  # the comms stay usable
    finally:
        vnode.destroy(comms)
