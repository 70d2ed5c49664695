"""GPU, virtual node: mccsAllToAllv against tests/a2av_ref.py, byte for byte,
inside 0xA5 frames (the gaps between receive segments included) with the send
buffers untouched.  n = 2 (m = 4), 3, 4 (m = 2) and 8 (seven channels) on the
matrices of a2av_ref.matrices, whose elements reach Ls = 3 / Lr = 0, Ls = 0 /
Lr = 3, Ls = 1 / Lr = 3 and Ls = Lr (tests/test_all_to_all_v_host.py asserts
that on the CPU); n = 1; uniform counts against mccsAllToAll; the torch-shaped
all_to_all_single; the refusals.  buffer_size = 1 << 16 and an 8 s watchdog.
"""
import numpy as np
import pytest

import a2a_ref
import a2av_ref as V
from mccs_amd import comm as C
import vnode

pytestmark = pytest.mark.gpu
DIRECT_DEFAULTS = True  # every threshold below is explicit

TIMEOUT_MS = 8000
RING_ONLY = dict(oneshot_bytes=-1, direct_bytes=-1, ll_bytes=-1)


def _comms(n, monkeypatch=None, **cfg):
    if monkeypatch is not None:
        monkeypatch.delenv("MCCS_ALLTOALL_HOPS", raising=False)
    return C.init_all([0] * n, C.CommConfig(timeout_ms=TIMEOUT_MS, **{"buffer_size": V.BUFF, **RING_ONLY, **cfg}))


class VStaged:
    """Device frames of one AllToAllv on the virtual node (the interface of
    test_gpu_rooted_sequences.Staged): issue, refill, check."""

    def __init__(self, n, cnt, kind, salt=0, call=None):
        import torch

        self.n, self.cnt, self.lay = n, cnt, V.layout(cnt, kind)
        self.call = call or dict(kind="a2av", root=None, count=max(max(r) for r in cnt))
        self.sf = [V.frame(self.lay["send_len"][r]) for r in range(n)]
        self.rf = [V.frame(self.lay["recv_len"][r]) for r in range(n)]
        self.send = [torch.from_numpy(a).cuda() for a, _ in self.sf]
        self.recv = [torch.from_numpy(a).cuda() for a, _ in self.rf]
        self.refill(salt)

    def refill(self, salt):
        import torch

        self.xs = [V.make_send(s, self.lay["send_len"][s], salt) for s in range(self.n)]
        for r in range(self.n):
            a, sl = self.sf[r]
            a[sl] = self.xs[r]
            self.send[r].copy_(torch.from_numpy(a))
            self.recv[r].fill_(V.SENTINEL)

    def issue_rank(self, comm, r, stream=None):
        C.all_to_all_v(comm, self.send[r].data_ptr() + self.sf[r][1].start, self.cnt[r], self.lay["sdispls"][r],
                       self.recv[r].data_ptr() + self.rf[r][1].start, [self.cnt[s][r] for s in range(self.n)],
                       self.lay["rdispls"][r], stream=stream)

    def issue(self, comms, stream=None):
        with C.group():
            for r in range(self.n):
                self.issue_rank(comms[r], r, stream)

    def check_rank(self, r, tag):
        want = V.expected(self.xs, self.cnt, self.lay)[r]
        a, sl = self.rf[r]
        frame = np.full_like(a, V.SENTINEL)
        frame[sl] = want
        got = self.recv[r].cpu().numpy()
        bad = np.flatnonzero(got != frame)
        assert bad.size == 0, (tag, f"rank {r}: {bad.size} wrong bytes, first at {bad[0] - sl.start} of the payload")
        assert self.send[r].cpu().numpy().tobytes() == self.sf[r][0].tobytes(), (tag, r, "send buffer written")

    def check(self, orc, comm0, tag):
        for r in range(self.n):
            self.check_rank(r, tag)


def run(comms, cnt, kind, salt=0, tag=None):
    import torch

    st = VStaged(len(comms), cnt, kind, salt)
    torch.cuda.synchronize()
    st.issue(comms)
    torch.cuda.synchronize()
    for c in comms:
        c.sync()
    st.check(None, comms[0], tag)


@pytest.mark.parametrize("n", [2, 3, 4, 8])
def test_matrices(monkeypatch, n):
    """Every matrix of the set (zero row, zero column, zero self, all zero and
    uniform among them), the layouts in turn: packed, descending, gaps, misaligned."""
    comms = _comms(n, monkeypatch)
    try:
        route = comms[0].all_to_all_route()
        assert route == {k: a2a_ref.route(n, comms[0].rings())[k] for k in ("hops", "m")} and route["hops"] == 1
        for i, (name, cnt) in enumerate(V.matrices(n, route["m"], comms[0].rings()).items()):
            run(comms, cnt, V.LAYOUTS[i % 4], salt=i, tag=(n, name))
        assert all(c.last_algo() == "ring" for c in comms)
    finally:
        vnode.destroy(comms)


@pytest.mark.parametrize("kind", V.LAYOUTS)
def test_layouts(monkeypatch, kind):
    """Each layout on the matrices with the unequal walks, at n = 4 (m = 2):
    descending displacements, gaps that must survive, displacements 1-15 bytes
    off 16-byte alignment, two peers reading one overlapping send segment."""
    comms = _comms(4, monkeypatch)
    try:
        mats = V.matrices(4, 2, comms[0].rings())
        for name in ("s3r0", "s0r3", "s1r3", "cyc5"):
            run(comms, mats[name], kind, tag=(kind, name))
    finally:
        vnode.destroy(comms)


def test_one_rank(monkeypatch):
    comms = _comms(1, monkeypatch)
    try:
        run(comms, [[4099]], "gaps")
        run(comms, [[300001]], "misaligned", salt=1)
        run(comms, [[0]], "packed")
    finally:
        vnode.destroy(comms)


@pytest.mark.parametrize("n", [2, 4, 8])
def test_uniform_counts_equal_all_to_all(monkeypatch, n):
    import torch

    comms = _comms(n, monkeypatch)
    try:
        for B in (4099, 70001):
            inputs = a2a_ref.make_inputs(n, B, salt=n)
            send = [vnode.to_dev(x) for x in inputs]
            out_u = [torch.zeros(n * B, dtype=torch.uint8, device="cuda") for _ in range(n)]
            out_v = [torch.zeros(n * B, dtype=torch.uint8, device="cuda") for _ in range(n)]
            disp = [t * B for t in range(n)]
            torch.cuda.synchronize()
            with C.group():
                for r in range(n):
                    C.all_to_all(comms[r], send[r], out_u[r], B)
            with C.group():
                for r in range(n):
                    C.all_to_all_v(comms[r], send[r], [B] * n, disp, out_v[r], [B] * n, disp)
            torch.cuda.synchronize()
            for c in comms:
                c.sync()
            want = a2a_ref.expected(inputs, B)
            for r in range(n):
                assert out_v[r].cpu().numpy().tobytes() == out_u[r].cpu().numpy().tobytes() == want[r].tobytes(), (B, r)
    finally:
        vnode.destroy(comms)


def test_all_to_all_single_with_and_without_splits(monkeypatch):
    import torch

    n = 4
    comms = _comms(n, monkeypatch)
    try:
        rng = np.random.default_rng(5)
        split = [[int(v) for v in rng.integers(0, 40, n)] for _ in range(n)]  # split[s][t]: rows s sends to t
        split[2] = [0] * n  # a rank that sends nothing
        xs = [torch.from_numpy(rng.standard_normal((sum(split[s]), 33)).astype(np.float32)).cuda() for s in range(n)]
        ys = [torch.full((sum(split[s][r] for s in range(n)), 33), -1.0, device="cuda") for r in range(n)]
        torch.cuda.synchronize()
        with C.group():
            for r in range(n):
                C.all_to_all_single(comms[r], ys[r], xs[r], [split[s][r] for s in range(n)], split[r])
        torch.cuda.synchronize()
        for c in comms:
            c.sync()
        for r in range(n):
            want = torch.cat([xs[s][sum(split[s][:r]):sum(split[s][:r + 1])] for s in range(n)])
            assert torch.equal(ys[r], want), r
        # no splits: dim 0 cut evenly, the uniform call
        xs = [torch.from_numpy(rng.integers(0, 1 << 30, (n * 7, 5)).astype(np.int32)).cuda() for _ in range(n)]
        ys = [torch.zeros_like(x) for x in xs]
        torch.cuda.synchronize()
        with C.group():
            for r in range(n):
                C.all_to_all_single(comms[r], ys[r], xs[r])
        torch.cuda.synchronize()
        for c in comms:
            c.sync()
        for r in range(n):
            assert torch.equal(ys[r], torch.cat([xs[s][7 * r:7 * r + 7] for s in range(n)])), r
        with pytest.raises(ValueError):
            C.all_to_all_single(comms[0], ys[0], xs[0], [1, 2, 3], None)
    finally:
        vnode.destroy(comms)


def _refused(code, start, call):
    with pytest.raises(C._lib.MccsError) as ei:
        call()
    assert ei.value.code == code and C._lib.last_error().startswith(start), (ei.value.code, C._lib.last_error())


def test_refusals_on_the_device_path(monkeypatch):
    import torch

    comms = _comms(2, monkeypatch)
    try:
        buf = torch.zeros(8192, dtype=torch.uint8, device="cuda")
        out = torch.zeros(8192, dtype=torch.uint8, device="cuda")
        c = comms[0]
        v = lambda **kw: lambda: C.all_to_all_v(c, kw.get("send", buf), kw.get("sc", [16, 32]), kw.get("sd", [0, 16]),
                                                kw.get("recv", out), kw.get("rc", [16, 64]), kw.get("rd", [0, 16]))
        for name in ("sc", "sd", "rc", "rd"):
            _refused(4, "mccsAllToAllv: null count or displacement array", v(**{name: None}))
        _refused(4, "mccsAllToAllv: null buffer", v(send=None))
        _refused(4, "mccsAllToAllv: null buffer", v(recv=None))
        _refused(4, "mccsAllToAllv: sendcounts[rank] != recvcounts[rank]", v(rc=[17, 64]))
        _refused(4, "mccsAllToAllv: two receive segments overlap", v(rd=[0, 15]))
        _refused(4, "mccsAllToAllv: a receive segment overlaps a send segment", v(recv=buf[40:]))
        C.all_to_all_v(c, None, [0, 0], [0, 0], None, [0, 0], [0, 0])  # nothing to do, nothing launched
        assert c.last_algo() is None
        mats = V.matrices(2, 4, comms[0].rings())
        run(comms, mats["s1r3"], "gaps")  # the comms stay usable
    finally:
        vnode.destroy(comms)


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
        out = torch.zeros(4096, dtype=torch.uint8, device="cuda")
        disp = [8 * t for t in range(n)]
        _refused(5, "mccsAllToAllv: the AllToAll route is not one hop",
                 lambda: C.all_to_all_v(comms[0], buf, [8] * n, disp, out, [8] * n, disp))
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
