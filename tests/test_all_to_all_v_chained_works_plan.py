"""CPU: a group of six AllToAllvDev calls, and of six AllToAllv calls with
non-empty self blocks, on the recording fake device runtime.  Each call queues
two elements per channel, so a channel gets 12: more than the 10 a work holds.
The launch record walks a channel's works along workNext and lists every used
element, so all 12 show, in issue order, only if the planner chained a second
work to the full one.  tests/test_gpu_all_to_all_v_dev_graph.py runs the same
groups on the GPU.
"""
from mccs_amd import abi
from mccs_amd import comm as C
import a2av_ref as V
import test_all_to_all_v_dev_plan as PD
import test_all_to_all_v_plan as PV
from test_all_to_all_v_dev_plan import fake  # noqa: F401  (the fixture)

NCALLS = 6
OFF = 0x400000


def test_six_dev_calls_in_one_group_chain_a_second_work(fake):  # noqa: F811
    fake(1)
    n = 4
    comms = C.init_all([0] * n, C.CommConfig(buffer_size=V.BUFF))
    try:
        PD._log()
        rings = comms[0].rings()
        assert abi.MCCS_MAX_WORK_ELEMENTS < NCALLS * 2 <= 2 * abi.MCCS_MAX_WORK_ELEMENTS
        with C.group():
            for k in range(NCALLS):
                for r, c in enumerate(comms):
                    C.all_to_all_v_dev(c, PD._send(r) + k * OFF, PD._recv(r) + k * OFF, PD._table(r, k), stream=0)
        launches = [kv for kind, kv in PD._log() if kind == "launch"]
        assert len(launches) == 1 and launches[0]["inline_works"] == "0", launches
        got = PD._elems(launches[0])
        for r in range(n):
            per_call = [PD._want(n, rings, r, k * OFF, k) for k in range(NCALLS)]
            want = []
            for c in range(len(rings)):
                for w in per_call:
                    want += w[2 * c:2 * c + 2]
            assert len(want) == 12 * len(rings) and got[r] == want, r
    finally:
        for c in comms:
            c.destroy()


def test_six_host_count_calls_with_self_blocks_chain_a_second_work(fake):  # noqa: F811
    fake(1)
    n = 4
    comms = C.init_all([0] * n, C.CommConfig(buffer_size=V.BUFF))
    try:
        PV._log()
        rings = comms[0].rings()
        m = comms[0].all_to_all_route()["m"]
        mats = V.boundary_matrices(n, m, rings)[:3] + [V.cyclic(n, m, k) for k in range(3)]
        mats = [[[v or 17 if s == t else v for t, v in enumerate(row)] for s, row in enumerate(cnt)] for cnt in mats]
        assert len(mats) == NCALLS and all(cnt[r][r] > 0 for cnt in mats for r in range(n))
        lays = [V.layout(cnt, V.LAYOUTS[k % 4]) for k, cnt in enumerate(mats)]
        with C.group():
            for k, (cnt, lay) in enumerate(zip(mats, lays)):
                for r, c in enumerate(comms):
                    C.all_to_all_v(c, PV._send(r) + k * OFF, cnt[r], lay["sdispls"][r], PV._recv(r) + k * OFF,
                                   [cnt[s][r] for s in range(n)], lay["rdispls"][r], stream=0)
        launches = [kv for kind, kv in PV._log() if kind == "launch"]
        assert len(launches) == 1 and launches[0]["inline_works"] == "0", launches
        got = PV._elems(launches[0])
        for r in range(n):
            per_call = [PV._want(n, rings, cnt, lay, r, k * OFF) for k, (cnt, lay) in enumerate(zip(mats, lays))]
            want = []
            for c in range(len(rings)):
                for w in per_call:
                    want += w[2 * c:2 * c + 2]
            assert len(want) == 12 * len(rings) and got[r] == want, r
    finally:
        for c in comms:
            c.destroy()
