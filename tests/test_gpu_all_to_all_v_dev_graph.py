"""GPU, virtual node: the flow mccsAllToAllvDev exists for, and chained works.

1. One captured graph builds the whole size table on the device: per rank
   row 0 <- router counts, row 1 <- their exclusive cumsum, a group of
   exchange_counts (row 2), row 3 <- the exclusive cumsum of row 2, a group
   of all_to_all_v_dev.  Seven replays: an all-zero matrix, four seeded random
   matrices over a2av_ref.values(m) and boundary_values(m), the first of them
   again, all zero again.  Before each replay the host writes the router
   counts, the payloads, the 0xA5 frames and the value 7 into rows 1 to 3 of
   every table (stream-ordered copies): the graph has to rebuild each of those
   rows.  The displacements are packed, so they move with the counts and a
   displacement captured or kept from the replay before shows.
2. A group of six Dev calls at n = 4, each with its own table, matrix and
   layout, between two ring AllReduces; then six host-count calls whose self
   counts are all non-zero.  Either way every channel gets 6 * 2 = 12
   elements, more than the 10 a work holds: two chained works per channel.
buffer_size = 1 << 16, the ring-only thresholds and an 8 s watchdog.
"""
import numpy as np
import pytest

import a2av_ref as V
import a2avd_ref as D
from mccs_amd import abi
from mccs_amd import comm as C
import test_gpu_all_to_all_v as G
import test_gpu_rooted_sequences as S
from test_gpu_all_to_all_v_dev import DStaged
import vnode

pytestmark = pytest.mark.gpu
DIRECT_DEFAULTS = True  # RING_ONLY is passed explicitly

M = {4: 2, 8: 1}
STALE = 7  # what the host leaves in rows 1 to 3 before a replay


def replay_matrices(n, m):
    """Seven matrices: zero, four random ones, the first random one again, zero."""
    rng = np.random.default_rng([9100, n])
    pool = sorted(set(V.values(m)) | set(V.boundary_values(m)))
    rand = []
    for _ in range(4):
        cnt = [[int(pool[int(rng.integers(0, len(pool)))]) for _ in range(n)] for _ in range(n)]
        for r in range(n):
            cnt[r][r] = int(V.SELF_VALUES[int(rng.integers(0, len(V.SELF_VALUES)))])
        rand.append(cnt)
    zero = [[0] * n for _ in range(n)]
    return [zero] + rand + [[row[:] for row in rand[0]]] + [[row[:] for row in zero]]


def check_replays_differ(n, mats):
    """On the host: each replay's expected frames, and at least one word of each of rows 1 and 3
    of some table, differ from the replay before, on one fixed payload."""
    lays = [V.layout(cnt, "packed") for cnt in mats]
    top = max(max(lay["send_len"]) for lay in lays)
    xs = [V.make_send(s, top, 0) for s in range(n)]
    room = [max(lay["recv_len"][r] for lay in lays) for r in range(n)]

    def frames(cnt, lay):
        out = []
        for r, w in enumerate(V.expected(xs, cnt, lay)):
            a = np.full(room[r], V.SENTINEL, np.uint8)
            a[:w.size] = w
            out.append(a)
        return out

    for k in range(1, len(mats)):
        a, b = frames(mats[k - 1], lays[k - 1]), frames(mats[k], lays[k])
        assert any((x != y).any() for x, y in zip(a, b)), k
        ta, tb = D.tables(mats[k - 1], lays[k - 1]), D.tables(mats[k], lays[k])
        for row in (1, 3):
            assert any((x[row * n:(row + 1) * n] != y[row * n:(row + 1) * n]).any() for x, y in zip(ta, tb)), (k, row)


@pytest.mark.parametrize("config", ["default", "lanes2_slots8_slice2"])
@pytest.mark.parametrize("n", [4, 8])
def test_a_table_built_on_the_device_inside_the_graph(monkeypatch, n, config):
    import torch

    monkeypatch.delenv("MCCS_SLICE_STEPS", raising=False)
    cfg = {}
    if config != "default":
        monkeypatch.setenv("MCCS_SLICE_STEPS", "2")
        cfg = dict(lanes=2, fifo_slots=8)
    m = M[n]
    mats = replay_matrices(n, m)
    assert len(mats) == 7 and mats[5] == mats[1] and mats[1] != mats[2]
    assert not any(v for row in mats[0] + mats[6] for v in row)
    check_replays_differ(n, mats)
    lays = [V.layout(cnt, "packed") for cnt in mats]
    send_len = [max(lay["send_len"][r] for lay in lays) for r in range(n)]
    recv_len = [max(lay["recv_len"][r] for lay in lays) for r in range(n)]
    assert max(send_len + recv_len) < 1 << 20
    comms = G._comms(n, monkeypatch, **cfg)
    try:
        assert comms[0].all_to_all_route() == {"hops": 1, "m": m}
        assert all(c.lanes == cfg.get("lanes", c.lanes) for c in comms)
        sf = [V.frame(send_len[r]) for r in range(n)]
        rf = [V.frame(recv_len[r]) for r in range(n)]
        send = [torch.from_numpy(a).cuda() for a, _ in sf]
        recv = [torch.from_numpy(a).cuda() for a, _ in rf]
        router = [torch.zeros(n, dtype=torch.int64, device="cuda") for _ in range(n)]
        tab = [torch.full((4 * n,), STALE, dtype=torch.int64, device="cuda") for _ in range(n)]
        stale = torch.full((3 * n,), STALE, dtype=torch.int64, device="cuda")
        sptr = [send[r].data_ptr() + sf[r][1].start for r in range(n)]
        rptr = [recv[r].data_ptr() + rf[r][1].start for r in range(n)]
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for r in range(n):
                tab[r][0:n].copy_(router[r])
            for r in range(n):
                x = tab[r][0:n]
                tab[r][n:2 * n].copy_(torch.cumsum(x, 0) - x)
            with C.group():
                for r in range(n):
                    C.exchange_counts(comms[r], tab[r])
            for r in range(n):
                x = tab[r][2 * n:3 * n]
                tab[r][3 * n:4 * n].copy_(torch.cumsum(x, 0) - x)
            with C.group():
                for r in range(n):
                    C.all_to_all_v_dev(comms[r], sptr[r], rptr[r], tab[r])
        for k, (cnt, lay) in enumerate(zip(mats, lays)):
            xs = [V.make_send(s, send_len[s], salt=40 + k) for s in range(n)]
            for r in range(n):  # stream-ordered: the router counts, the payload, the sentinels, the stale rows
                router[r].copy_(torch.tensor(cnt[r], dtype=torch.int64))
                a, sl = sf[r]
                a[sl] = xs[r]
                send[r].copy_(torch.from_numpy(a))
                recv[r].fill_(V.SENTINEL)
                tab[r][n:4 * n].copy_(stale)
            g.replay()
            torch.cuda.synchronize()
            for c in comms:
                c.sync()
            want = V.expected(xs, cnt, lay)
            for r in range(n):
                assert tab[r].cpu().tolist() == D.table(cnt, lay, r).astype(np.int64).tolist(), (k, r, "table")
                a, sl = rf[r]
                frame = np.full_like(a, V.SENTINEL)
                frame[sl.start:sl.start + want[r].size] = want[r]
                bad = np.flatnonzero(recv[r].cpu().numpy() != frame)
                assert bad.size == 0, (n, config, "replay", k,
                                       f"rank {r}: {bad.size} wrong bytes, first at {bad[0] - sl.start}")
                assert send[r].cpu().numpy().tobytes() == sf[r][0].tobytes(), (k, r, "send buffer written")
            assert all(c.last_algo() == "ring" for c in comms)
        del g
    finally:
        vnode.destroy(comms)


# ---- 2. more elements than one work holds --------------------------------------------
NCALLS = 6


def six_matrices(n, m, rings, self_nonzero):
    named = V.matrices(n, m, rings)
    mats = [named["s1r3"], named["cyc5"], named["s3r0"], named["zero_row"]] + V.boundary_matrices(n, m, rings)[:2]
    mats = [[row[:] for row in cnt] for cnt in mats]
    if self_nonzero:
        for cnt in mats:
            for r in range(n):
                cnt[r][r] = cnt[r][r] or 17
    assert len(mats) == NCALLS
    return mats


def test_a_group_of_six_calls_chains_two_works(orc, monkeypatch):
    """A Dev call queues its FIFO element and its self element on every channel
    (plan.cpp plan_enqueue_a2av_dev), a host-count call with a non-zero self
    count too (plan_enqueue_a2av): six calls in one group are 6 * 2 = 12
    elements per channel, a work holds MCCS_MAX_WORK_ELEMENTS = 10, so every
    channel runs a full work and a second one of two elements chained to it.
    The Dev kernel rewrites its LDS copy of the work in place before the next
    work is loaded over it.  First six Dev calls, then six host-count calls,
    each group between two ring AllReduces on the same communicators."""
    import torch

    n, per_call = 4, 2
    assert abi.MCCS_MAX_WORK_ELEMENTS == 10
    assert abi.MCCS_MAX_WORK_ELEMENTS < NCALLS * per_call <= 2 * abi.MCCS_MAX_WORK_ELEMENTS
    comms = G._comms(n, monkeypatch)
    try:
        rings, m = comms[0].rings(), comms[0].all_to_all_route()["m"]
        rng = np.random.default_rng(70)
        ar = dict(kind="ar", code=7, op=0, root=None, inplace=False, count=100000)
        for call in ("dev", "host_counts"):
            mats = six_matrices(n, m, rings, self_nonzero=call == "host_counts")
            if call == "host_counts":
                assert all(cnt[r][r] > 0 for cnt in mats for r in range(n))
            before = S.Staged(ar, n, [S.call_input(ar, n, rng) for _ in range(n)])
            after = S.Staged(ar, n, [S.call_input(ar, n, rng) for _ in range(n)])
            cls = DStaged if call == "dev" else G.VStaged
            batch = [cls(n, cnt, V.LAYOUTS[i % len(V.LAYOUTS)], salt=i + 1) for i, cnt in enumerate(mats)]
            torch.cuda.synchronize()
            before.issue(comms)
            assert all(c.last_algo() == "ring" for c in comms)
            with C.group():
                for s in batch:
                    for r in range(n):
                        s.issue_rank(comms[r], r)
            after.issue(comms)
            S._finish(orc, comms, [before] + batch + [after], ("six " + call, n))
    finally:
        vnode.destroy(comms)
