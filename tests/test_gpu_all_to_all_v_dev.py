"""GPU, virtual node: mccsAllToAllvDev, whose size table lives in device memory
and is read by the kernel when it runs.  Every comparison is byte-exact, inside
0xA5 frames, against tests/a2av_ref.py, with the send buffers untouched.

1. the matrices of a2av_ref.matrices at n = 2, 3, 4, 8 and one rank, the
   layouts in turn ("misaligned" and "overlap_send" among them); the all-zero
   matrix still launches and writes nothing;
2. the same receive frames as mccsAllToAllv on the same inputs;
3. one graph, captured once, holding exchange_counts and all_to_all_v_dev,
   replayed for five matrices of which only row 0 of the tables and the
   payloads are rewritten (stream-ordered copies); a captured mccsAllToAllv as
   the control repeats its first sizes;
4. Dev calls beside host-count calls between the other collectives
   (test_gpu_all_to_all_v_sequences.sequence): one stream, two streams, a
   batched group of two, one rank per process (tests/a2avd_worker.py);
5. the refusals reach Python and leave the communicator usable.
buffer_size = 1 << 16 and an 8 s watchdog.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import a2a_ref
import a2avd_ref as D
import a2av_ref as V
from mccs_amd import comm as C
import test_gpu_all_to_all_v as G
import test_gpu_all_to_all_v_sequences as Q
import test_gpu_rooted_sequences as S
import vnode

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
DIRECT_DEFAULTS = True  # every threshold below is explicit

_comms = G._comms  # ring-only thresholds, buffer_size = V.BUFF, the 8 s watchdog


class DStaged(G.VStaged):
    """G.VStaged issued through all_to_all_v_dev: the sizes go to the device once, as each rank's table."""

    def __init__(self, n, cnt, kind, salt=0, call=None, lay=None):
        import torch

        super().__init__(n, cnt, kind, salt, call)
        if lay is not None:
            assert lay == self.lay
        self.tab = [torch.from_numpy(D.table(cnt, self.lay, r).view(np.int64)).cuda() for r in range(n)]

    def issue_rank(self, comm, r, stream=None):
        C.all_to_all_v_dev(comm, self.send[r].data_ptr() + self.sf[r][1].start,
                           self.recv[r].data_ptr() + self.rf[r][1].start, self.tab[r], stream=stream)


def run(comms, cnt, kind, salt=0, tag=None):
    import torch

    st = DStaged(len(comms), cnt, kind, salt)
    torch.cuda.synchronize()
    st.issue(comms)
    torch.cuda.synchronize()
    for c in comms:
        c.sync()
    st.check(None, comms[0], tag)
    return st


# ---- 1. the matrices ---------------------------------------------------------
@pytest.mark.parametrize("n", [2, 3, 4, 8])
def test_matrices(monkeypatch, n):
    comms = _comms(n, monkeypatch)
    try:
        route = comms[0].all_to_all_route()
        assert route == {k: a2a_ref.route(n, comms[0].rings())[k] for k in ("hops", "m")} and route["hops"] == 1
        mats = V.matrices(n, route["m"], comms[0].rings())
        # nothing has run on these comms: the all-zero call launches all the same, and writes nothing
        assert all(c.last_algo() is None for c in comms)
        run(comms, mats["all_zero"], "gaps", tag=(n, "all_zero first"))
        assert all(c.last_algo() == "ring" for c in comms)
        for i, (name, cnt) in enumerate(mats.items()):
            run(comms, cnt, V.LAYOUTS[i % len(V.LAYOUTS)], salt=i, tag=(n, name))
    finally:
        vnode.destroy(comms)


@pytest.mark.parametrize("kind", ["misaligned", "overlap_send"])
def test_layouts_on_the_unequal_walks(monkeypatch, kind):
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
        assert comms[0].last_algo() == "ring"
    finally:
        vnode.destroy(comms)


# ---- 2. the host-count call's bytes -----------------------------------------------
@pytest.mark.parametrize("n", [2, 4, 8])
def test_same_bytes_as_the_host_count_call(monkeypatch, n):
    import torch

    comms = _comms(n, monkeypatch)
    try:
        mats = V.matrices(n, comms[0].all_to_all_route()["m"], comms[0].rings())
        for i, (name, kind) in enumerate((("s1r3", "misaligned"), ("cyc5", "gaps"))):
            host, dev = G.VStaged(n, mats[name], kind, salt=i), DStaged(n, mats[name], kind, salt=i)
            torch.cuda.synchronize()
            host.issue(comms)
            dev.issue(comms)
            torch.cuda.synchronize()
            for c in comms:
                c.sync()
            dev.check(None, comms[0], (n, name))
            for r in range(n):
                assert dev.recv[r].cpu().numpy().tobytes() == host.recv[r].cpu().numpy().tobytes(), (n, name, r)
    finally:
        vnode.destroy(comms)


# ---- 3. one graph, fresh sizes at every replay -------------------------------------
def replay_matrices(n, m, rings):
    """Five matrices for one captured graph.  The pair (0 -> its successor on
    channel 0) goes 0 -> 3C -> 1 -> C+1 -> 0, so that connection's steps per
    replay are 0, 12, 4, 8, 0 while its neighbours take their own; the first
    matrix is all zero."""
    Cb = V.loop_bytes(m)
    nxt, _ = V.ring_next_prev(rings, n)
    t = nxt[0][0]
    out = [[[0] * n for _ in range(n)]]
    for k, v in enumerate((3 * Cb, 1, Cb + 1, 0)):
        cnt = V.cyclic(n, m, start=k + 1, stride=1 + k % 3, self_start=k)
        cnt[0][t] = v
        out.append(cnt)
    assert [c[0][t] for c in out] == [0, 3 * Cb, 1, Cb + 1, 0]
    assert [V.loops(c[0][t], m) for c in out] == [0, 3, 1, 2, 0]
    return out


@pytest.mark.parametrize("n", [4, 8])
def test_one_graph_takes_each_replays_sizes(monkeypatch, n):
    import torch

    comms = _comms(n, monkeypatch)
    try:
        rings, m = comms[0].rings(), comms[0].all_to_all_route()["m"]
        mats = replay_matrices(n, m, rings)
        lay = D.sequence_layout(mats)
        sf = [V.frame(lay["send_len"][r]) for r in range(n)]
        rf = [V.frame(lay["recv_len"][r]) for r in range(n)]
        send = [torch.from_numpy(a).cuda() for a, _ in sf]
        recv = [torch.from_numpy(a).cuda() for a, _ in rf]
        # the displacement rows are fixed; row 0 is written before every replay; the host only ever
        # writes zeros to row 2
        tab = []
        for r in range(n):
            t = D.table(mats[0], lay, r)
            t[2 * n:3 * n] = 0
            tab.append(torch.from_numpy(t.view(np.int64)).cuda())
        sptr = [send[r].data_ptr() + sf[r][1].start for r in range(n)]
        rptr = [recv[r].data_ptr() + rf[r][1].start for r in range(n)]
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            with C.group():
                for r in range(n):
                    C.exchange_counts(comms[r], tab[r])
            with C.group():
                for r in range(n):
                    C.all_to_all_v_dev(comms[r], sptr[r], rptr[r], tab[r])
        for k, cnt in enumerate(mats):
            xs = [V.make_send(s, lay["send_len"][s], salt=40 + k) for s in range(n)]
            for r in range(n):  # stream-ordered: row 0, the payload, the sentinels
                tab[r][0:n].copy_(torch.tensor(cnt[r], dtype=torch.int64))
                tab[r][2 * n:3 * n].zero_()
                a, sl = sf[r]
                a[sl] = xs[r]
                send[r].copy_(torch.from_numpy(a))
                recv[r].fill_(V.SENTINEL)
            g.replay()
            torch.cuda.synchronize()
            for c in comms:
                c.sync()
            want = V.expected(xs, cnt, lay)
            for r in range(n):
                got_tab = tab[r].cpu().numpy()
                assert got_tab[2 * n:3 * n].tolist() == [cnt[s][r] for s in range(n)], (k, r, "row 2")
                assert got_tab.tolist() == D.table(cnt, lay, r).astype(np.int64).tolist(), (k, r, "table")
                a, sl = rf[r]
                frame = np.full_like(a, V.SENTINEL)
                frame[sl] = want[r]
                bad = np.flatnonzero(recv[r].cpu().numpy() != frame)
                assert bad.size == 0, (k, f"rank {r}: {bad.size} wrong bytes, first at {bad[0] - sl.start}")
                assert send[r].cpu().numpy().tobytes() == sf[r][0].tobytes(), (k, r, "send buffer written")
        del g
        # the control: the host-count call, captured with the second matrix's sizes, repeats them
        first, other = mats[1], mats[2]
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            with C.group():
                for r in range(n):
                    C.all_to_all_v(comms[r], sptr[r], first[r], lay["sdispls"][r], rptr[r],
                                   [first[s][r] for s in range(n)], lay["rdispls"][r])
        xs = [V.make_send(s, lay["send_len"][s], salt=90) for s in range(n)]
        for r in range(n):
            a, sl = sf[r]
            a[sl] = xs[r]
            send[r].copy_(torch.from_numpy(a))
            recv[r].fill_(V.SENTINEL)
        g.replay()  # "the sizes are now `other`" cannot reach it
        torch.cuda.synchronize()
        for c in comms:
            c.sync()
        repeated, fresh = V.expected(xs, first, lay), V.expected(xs, other, lay)
        assert any((a != b).any() for a, b in zip(repeated, fresh))
        for r in range(n):
            sl = rf[r][1]
            assert recv[r].cpu().numpy()[sl].tobytes() == repeated[r].tobytes(), r
        del g
    finally:
        vnode.destroy(comms)


# ---- 4. between other collectives ---------------------------------------------------
def stage_call(call, n, rings, m, rng):
    """Q.stage_call with every second v call of the sequence issued as a Dev call."""
    if call["kind"] == "a2av" and call["salt"] % 2 == 0:
        return DStaged(n, V.matrices(n, m, rings)[call["mat"]], call["layout"], call["salt"], call=call)
    return Q.stage_call(call, n, rings, m, rng)


def _stage(n, rng, comms):
    rings, m = comms[0].rings(), comms[0].all_to_all_route()["m"]
    items = [stage_call(call, n, rings, m, rng) for call in Q.sequence(n)]
    assert sum(isinstance(s, DStaged) for s in items) == 4 and sum(type(s) is G.VStaged for s in items) == 3
    return items


@pytest.mark.parametrize("n", [4, 8])
def test_sequence(orc, monkeypatch, n):
    import torch

    comms = Q._comms(n, monkeypatch)
    try:
        items = _stage(n, np.random.default_rng(n), comms)
        torch.cuda.synchronize()
        took = []
        for s in items:
            s.issue(comms)
            took.append((s.call["kind"], comms[0].last_algo(), Q._algo(s.call)))
        S._finish(orc, comms, items, ("a2avd sequence", n))
        assert not [t for t in took if t[1] != t[2]], took
    finally:
        vnode.destroy(comms)


@pytest.mark.parametrize("n", [4, 8])
def test_sequence_across_two_streams(orc, monkeypatch, n):
    import torch

    comms = Q._comms(n, monkeypatch)
    streams = [torch.cuda.current_stream(), torch.cuda.Stream()]
    try:
        rng = np.random.default_rng(10 + n)
        items = _stage(n, rng, comms)
        torch.cuda.synchronize()
        for s in items:
            s.issue(comms, streams[int(rng.integers(0, 2))])
        S._finish(orc, comms, items, ("a2avd streams", n))
    finally:
        vnode.destroy(comms)


@pytest.mark.parametrize("n", [4, 8])
def test_batched_group_of_two_dev_calls(orc, monkeypatch, n):
    """Two Dev calls with tables of their own in one group are one launch; an
    AllReduce before and after leaves and finds the connections in step."""
    import torch

    comms = Q._comms(n, monkeypatch)
    try:
        rng = np.random.default_rng(60 + n)
        mats = V.matrices(n, comms[0].all_to_all_route()["m"], comms[0].rings())
        ar = dict(kind="ar", code=7, op=0, root=None, inplace=False, count=100000)
        before = S.Staged(ar, n, [S.call_input(ar, n, rng) for _ in range(n)])
        after = S.Staged(ar, n, [S.call_input(ar, n, rng) for _ in range(n)])
        batch = [DStaged(n, mats["s1r3"], "gaps", 1), DStaged(n, mats["cyc5"], "descending", 2)]
        torch.cuda.synchronize()
        before.issue(comms)
        with C.group():
            for s in batch:
                for r in range(n):
                    s.issue_rank(comms[r], r)
        after.issue(comms)
        S._finish(orc, comms, [before] + batch + [after], ("batched dev", n))
    finally:
        vnode.destroy(comms)


def test_sequence_one_rank_per_process():
    """n = 2 (m = 4), one rank per process: each process's table is in its own
    device memory, its works go through the work FIFO."""
    world = 2
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}",
           "--master-addr", "127.0.0.1", "--master-port", str(Q._free_port()), os.path.join(HERE, "a2avd_worker.py")]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("MCCS_ONESHOT_BYTES", "MCCS_DIRECT_BYTES", "MCCS_LL_BYTES", "MCCS_ALLTOALL_HOPS"):
        env.pop(k, None)
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=240, env=env, cwd=os.path.dirname(HERE))
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    lib_lines = "\n".join(l for l in (r.stdout + r.stderr).splitlines() if "mccs" in l.lower() or "hip" in l)[-3000:]
    assert r.returncode == 0 and lines, lib_lines + "\n----\n" + r.stdout[-2000:] + r.stderr[-2000:]
    res = json.loads(lines[-1])
    bad = [k for k, v in res["checks"].items() if not v]
    assert res["all_ok"] and not bad, bad
    kinds = [k.split("/")[1] for k in res["checks"]]
    assert kinds.count("a2avd") == 4 and kinds.count("a2av") == 3 and kinds.count("a2a") == 1
    assert res["route"] == {"hops": 1, "m": 4}


# ---- 5. refusals ----------------------------------------------------------------------
def _refused(code, start, call):
    with pytest.raises(C._lib.MccsError) as ei:
        call()
    assert ei.value.code == code and C._lib.last_error().startswith(start), (ei.value.code, C._lib.last_error())


def test_refusals_reach_python_and_leave_the_comm_usable(monkeypatch):
    import torch

    comms = _comms(2, monkeypatch)
    try:
        buf = torch.zeros(8192, dtype=torch.uint8, device="cuda")
        out = torch.zeros(8192, dtype=torch.uint8, device="cuda")
        tab = torch.zeros(8, dtype=torch.int64, device="cuda")
        c = comms[0]
        v = lambda **kw: lambda: C.all_to_all_v_dev(c, kw.get("send", buf), kw.get("recv", out), kw.get("table", tab))
        _refused(4, "mccsAllToAllvDev: null size table", v(table=None))
        _refused(4, "mccsAllToAllvDev: the size table is not 8-byte aligned", v(table=tab.data_ptr() + 4))
        _refused(4, "mccsAllToAllvDev: null buffer", v(send=None))
        _refused(4, "mccsAllToAllvDev: null buffer", v(recv=None))
        for bad in (tab[:7], tab.to(torch.int32), tab.cpu()):
            with pytest.raises(ValueError):
                v(table=bad)()
        assert c.last_algo() is None  # nothing was launched
        run(comms, V.matrices(2, 4, comms[0].rings())["s1r3"], "gaps")  # the comms stay usable
    finally:
        vnode.destroy(comms)


def test_a_relay_route_is_refused_on_the_device_path(monkeypatch):
    import torch

    n = 4
    monkeypatch.setenv("MCCS_ALLTOALL_HOPS", "relay")
    comms = _comms(n)
    try:
        assert comms[0].all_to_all_route()["hops"] == n - 1
        buf = torch.zeros(4096, dtype=torch.uint8, device="cuda")
        out = torch.zeros(4096, dtype=torch.uint8, device="cuda")
        tab = torch.zeros(4 * n, dtype=torch.int64, device="cuda")
        _refused(5, "mccsAllToAllvDev: the AllToAll route is not one hop",
                 lambda: C.all_to_all_v_dev(comms[0], buf, out, tab))
        assert "MCCS_ALLTOALL_HOPS=relay" in C._lib.last_error()
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
