"""GPU, virtual node: mccsSend / mccsRecv against tests/sr_ref.py, byte for
byte.  Every buffer, send or receive, sits inside its own 0xA5 frame; the
frames must survive and the send buffers come back untouched.  The pattern
lists (a)-(h) at n = 2 (m = 4), 3, 4 (m = 2) and 8 (seven channels), (f) at
n = 3; typed counts; a ring shift against mccsAllToAllv with the same sparse
matrix; the refusals.  buffer_size = 1 << 16, ring only, an 8 s watchdog.

A send and its receive are always issued in the same group() across the ranks'
communicators, so they land in one fused launch: on one GPU a send launched
ahead of its receive would sit in front of it until the watchdog.
"""
import numpy as np
import pytest

import a2a_ref
import a2av_ref as V
import sr_ref as SR
from mccs_amd import comm as C
import test_gpu_all_to_all_v as G
import vnode

pytestmark = pytest.mark.gpu
DIRECT_DEFAULTS = True  # every threshold is explicit (G._comms)

_comms = G._comms  # ring-only thresholds, buffer_size = V.BUFF, the 8 s watchdog
U8 = C.AllReduceDataType.Uint8


class SRStaged:
    """Device frames of one group of sends and receives on the virtual node
    (the interface of test_gpu_rooted_sequences.Staged): issue, refill, check."""

    def __init__(self, n, ops, salt=0, call=None):
        import torch

        self.n, self.ops, self.salt = n, ops, salt
        self.call = call or dict(kind="sr", root=None, count=max(o.nbytes for o in ops))
        self.host = SR.frames(ops, salt)
        self.dev = [torch.from_numpy(a).cuda() for a, _ in self.host]
        for t, (_, sl), o in zip(self.dev, self.host, ops):
            assert (t.data_ptr() + sl.start) % 16 == o.off  # the misalignment the case names

    def refill(self, salt):
        import torch

        self.salt = salt
        self.host = SR.frames(self.ops, salt)
        for t, (a, _) in zip(self.dev, self.host):
            t.copy_(torch.from_numpy(a))

    def issue_rank(self, comm, r, stream=None):
        for i, o in enumerate(self.ops):
            if o.rank == r:
                assert o.nbytes % SR.ESIZE[o.code] == 0  # the call counts elements of the op's type (uint8 by default)
                (C.send if o.kind == "send" else C.recv)(comm, self.dev[i].data_ptr() + self.host[i][1].start,
                                                         o.nbytes // SR.ESIZE[o.code], o.code, o.peer, stream=stream)

    def issue(self, comms, stream=None):
        with C.group():
            for r in range(self.n):
                self.issue_rank(comms[r], r, stream)

    def check_rank(self, r, tag):
        mine = [i for i, o in enumerate(self.ops) if o.rank == r]
        got = {i: (self.dev[i].cpu().numpy(), self.host[i][1]) for i in mine}
        try:
            SR.check(self.ops, got, self.salt, only=mine)
        except AssertionError as e:
            raise AssertionError((tag, r, str(e))) from None

    def check(self, orc, comm0, tag):
        for r in SR.ranks_of(self.ops):
            self.check_rank(r, tag)


def run(comms, ops, salt=0, tag=None):
    import torch

    st = SRStaged(len(comms), ops, salt)
    torch.cuda.synchronize()
    st.issue(comms)
    torch.cuda.synchronize()
    for c in comms:
        c.sync()
    st.check(None, comms[0], tag)


@pytest.mark.parametrize("n", [2, 3, 4, 8])
def test_patterns(monkeypatch, n):
    """Every pattern list of the set: all pairs (n <= 4), the 3C ring shift,
    pairwise exchange, fan-out and fan-in, two messages on a pair, the send
    issued after two receives (n = 3), a one-way message, misaligned buffers."""
    comms = _comms(n, monkeypatch)
    try:
        route = comms[0].all_to_all_route()
        assert route == {k: a2a_ref.route(n, comms[0].rings())[k] for k in ("hops", "m")} and route["hops"] == 1
        pats = SR.patterns(n, route["m"], comms[0].rings())
        assert ("f_send_after_recvs" in pats) == (n == 3)
        for i, (name, ops) in enumerate(pats.items()):
            run(comms, ops, salt=i, tag=(n, name))
            assert all(comms[r].last_algo() == "ring" for r in SR.ranks_of(ops)), name
    finally:
        vnode.destroy(comms)


@pytest.mark.parametrize("n", [2, 4])
def test_typed_counts(monkeypatch, n):
    import torch

    comms = _comms(n, monkeypatch)
    try:
        cnt = 4099
        xs = [torch.from_numpy(np.random.default_rng(r).standard_normal(cnt).astype(np.float16)).cuda()
              for r in range(n)]
        ws = [torch.from_numpy(np.random.default_rng(9 + r).integers(-1 << 40, 1 << 40, cnt)).cuda() for r in range(n)]
        ys = [torch.zeros(cnt, dtype=torch.float16, device="cuda") for _ in range(n)]
        zs = [torch.zeros(cnt, dtype=torch.int64, device="cuda") for _ in range(n)]
        torch.cuda.synchronize()
        with C.group():
            for r in range(n):
                comms[r].send(xs[r], cnt, C.AllReduceDataType.Float16, (r + 1) % n)
                comms[r].recv(ys[r], cnt, C.AllReduceDataType.Float16, (r - 1) % n)
                C.batch_send_recv(comms[r], [("send", ws[r], cnt, C.AllReduceDataType.Int64, (r - 1) % n),
                                             ("recv", zs[r], cnt * 8, None, (r + 1) % n)])
        torch.cuda.synchronize()
        for c in comms:
            c.sync()
        for r in range(n):
            assert torch.equal(ys[r], xs[(r - 1) % n]) and torch.equal(zs[r], ws[(r + 1) % n]), r
    finally:
        vnode.destroy(comms)


@pytest.mark.parametrize("n", [2, 4, 8])
def test_a_ring_shift_equals_all_to_all_v(monkeypatch, n):
    import torch

    comms = _comms(n, monkeypatch)
    try:
        m = comms[0].all_to_all_route()["m"]
        for B in (4099, 2 * V.loop_bytes(m) + 999):
            send = [vnode.to_dev(V.make_send(r, B, salt=n)) for r in range(n)]
            out_p = [torch.zeros(B, dtype=torch.uint8, device="cuda") for _ in range(n)]
            out_v = [torch.zeros(B, dtype=torch.uint8, device="cuda") for _ in range(n)]
            cnt = SR.shift_matrix(n, B)
            torch.cuda.synchronize()
            with C.group():
                for r in range(n):
                    C.send(comms[r], send[r], B, U8, (r + 1) % n)
                    C.recv(comms[r], out_p[r], B, U8, (r - 1) % n)
            with C.group():
                for r in range(n):
                    C.all_to_all_v(comms[r], send[r], cnt[r], [0] * n, out_v[r], [cnt[s][r] for s in range(n)], [0] * n)
            torch.cuda.synchronize()
            for c in comms:
                c.sync()
            for r in range(n):
                want = V.make_send((r - 1) % n, B, salt=n)
                assert out_p[r].cpu().numpy().tobytes() == out_v[r].cpu().numpy().tobytes() == want.tobytes(), (B, r)
    finally:
        vnode.destroy(comms)


def _refused(code, start, call):
    with pytest.raises(C._lib.MccsError) as ei:
        call()
    assert ei.value.code == code and C._lib.last_error().startswith(start), (ei.value.code, C._lib.last_error())


def test_refusals_on_the_device_path(monkeypatch):
    import torch

    comms = _comms(2, monkeypatch)
    one = _comms(1)
    try:
        buf = torch.zeros(8192, dtype=torch.uint8, device="cuda")
        c = comms[0]
        for fn, name in ((C.send, "mccsSend"), (C.recv, "mccsRecv")):
            _refused(4, f"{name}: peer 2 outside 0..1", lambda: fn(c, buf, 8, U8, 2))
            _refused(4, f"{name}: peer is the calling rank", lambda: fn(c, buf, 8, U8, 0))
            _refused(4, f"{name}: null buffer with a non-zero count", lambda: fn(c, None, 8, U8, 1))
            _refused(4, f"{name}: a communicator of one rank has no peer", lambda: fn(one[0], buf, 8, U8, 0))
        with pytest.raises(C._lib.MccsError) as ei:  # mixing with another function in one group
            with C.group():
                C.send(c, buf, 8, U8, 1)
                C.all_to_all(c, buf, buf[4096:], 64)
        assert ei.value.code == 5 and "mixes collectives" in C._lib.last_error()
        C.send(c, None, 0, U8, 1)  # nothing to do, nothing launched
        assert c.last_algo() is None
        run(comms, SR.patterns(2, 4, comms[0].rings())["e_two_on_a_pair"])  # the comms stay usable
    finally:
        vnode.destroy(comms + one)


@pytest.mark.parametrize("how", ["six ranks", "env", "one channel"])
def test_a_relay_route_is_refused_on_the_device_path(monkeypatch, how):
    import torch

    n = 6 if how == "six ranks" else 4
    monkeypatch.delenv("MCCS_ALLTOALL_HOPS", raising=False)
    if how == "env":
        monkeypatch.setenv("MCCS_ALLTOALL_HOPS", "relay")
    comms = _comms(n, **({"channel_count": 1} if how == "one channel" else {}))
    try:
        assert comms[0].all_to_all_route()["hops"] == n - 1
        buf = torch.zeros(4096, dtype=torch.uint8, device="cuda")
        for fn, name in ((C.send, "mccsSend"), (C.recv, "mccsRecv")):
            _refused(5, f"{name}: the AllToAll route is not one hop", lambda: fn(comms[0], buf, 8, U8, 1))
            assert ("MCCS_ALLTOALL_HOPS=relay" in C._lib.last_error()) == (how == "env")
        # the comms stay usable: the uniform call relays
        inputs = a2a_ref.make_inputs(n, 4099)
        send = [vnode.to_dev(x) for x in inputs]
        recv = [torch.zeros(n * 4099, dtype=torch.uint8, device="cuda") for _ in range(n)]
        torch.cuda.synchronize()
        with C.group():
            for r in range(n):
                C.all_to_all(comms[r], send[r], recv[r], 4099)
        torch.cuda.synchronize()
        for c in comms:
            c.sync()
        for r, w in enumerate(a2a_ref.expected(inputs, 4099)):
            assert recv[r].cpu().numpy().tobytes() == w.tobytes(), r
    finally:
        vnode.destroy(comms)
