"""GPU: Send/Recv groups that put more than MCCS_MAX_WORK_ELEMENTS elements on
a channel, so the planner chains works and the kernel walks them (workNext).

The two groups of tests/sr_ref.chained: at n = 2, 23 messages one way and 12
the other on every channel (three works and two), sizes through the cut edges
up to one loop, one of 2C + 999 in the middle, zero bytes at queue positions
0, 9, 10 and last; at n = 4, 12 messages 0 -> 1 beside the idle channels of
rank 0, rank 1's send issued after its 12 receives, and one message of 3C on
another pair.  Under the default engine and under MCCS_SLICE_STEPS=2 with 8
FIFO slots (the smallest send window).  The n = 4 group also inside a HIP
graph replayed three times with refilled payloads (the captured chained works
carry their own pointers), followed by an AllToAllv on the same communicators.
Every byte of every frame compared; ring only, buffer_size = 1 << 16, an 8 s
watchdog.  tests/test_send_recv_fuzz_cases.py runs the same groups on the
host-thread ring and the fake runtime.
"""
import pytest

import a2av_ref as V
import sr_ref as SR
import test_gpu_all_to_all_v as G
import test_gpu_send_recv as P
import test_gpu_send_recv_fuzz as F
import vnode

pytestmark = pytest.mark.gpu
DIRECT_DEFAULTS = True  # G._comms sets every threshold

CONFIGS = {"default": ({}, False), "slice2_8slots": ({"fifo_slots": 8}, True)}  # name -> (CommConfig keywords, slice2)


def _comms(monkeypatch, n, name):
    cfg, slice2 = CONFIGS[name]
    F.set_env(monkeypatch, slice2, False)
    comms = G._comms(n, **cfg)
    assert comms[0].all_to_all_route()["hops"] == 1
    return comms, SR.chained(n, comms[0].all_to_all_route()["m"])


@pytest.mark.parametrize("name", list(CONFIGS))
@pytest.mark.parametrize("n", [2, 4])
def test_chained_works(monkeypatch, n, name):
    comms, ops = _comms(monkeypatch, n, name)
    try:
        assert max(SR.works(ops, 0, comms[0].rings())) == (3 if n == 2 else 2)
        st = P.SRStaged(n, ops, salt=n)
        F.run_staged(comms, st, (n, name, "first run"))
        st.refill(50 + n)
        F.run_staged(comms, st, (n, name, "second run"))
        F.step_check(comms, (n, name))
    finally:
        vnode.destroy(comms)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_chained_works_in_a_graph_replayed_three_times(monkeypatch, name):
    import torch

    n = 4
    comms, ops = _comms(monkeypatch, n, name)
    try:
        st = P.SRStaged(n, ops, salt=1)
        F.run_staged(comms, st, (name, "eager"))
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            st.issue(comms)
        for rep in range(3):
            st.refill(10 + rep)
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            for c in comms:
                c.sync()
            st.check(None, comms[0], (name, "replay", rep))
        del g
        m = comms[0].all_to_all_route()["m"]
        G.run(comms, V.matrices(n, m, comms[0].rings())["cyc5"], "gaps", salt=3, tag=(name, "cyc5 after the graph"))
        assert all(c.last_algo() == "ring" for c in comms)
    finally:
        vnode.destroy(comms)
