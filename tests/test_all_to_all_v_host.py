"""CPU: the AllToAllv call list and the host-thread ring
(mccs_host_ring_all_to_all_v: the walk of ring_walk.h a2av_next over the FIFO
protocol, as the kernel takes it) against tests/a2av_ref.py.  Receive buffers
sit inside 0xA5 frames whose gaps must survive; send buffers must come back
unchanged.
"""
import numpy as np
import pytest

import a2a_ref
import a2av_ref as V
from mccs_amd import comm as C
from mccs_amd._lib import MccsError

INVALID_USAGE = 5
NS = [2, 3, 4, 5, 7, 8]


def rings_m(n, channels=0):
    rings = C.default_rings(n, channels)
    return rings, a2a_ref.route(n, rings)["m"]


def run(n, cnt, kind, rings, nthreads=544, salt=0):
    lay = V.layout(cnt, kind)
    sends = [V.make_send(s, lay["send_len"][s], salt) for s in range(n)]
    sf, rf = [], []
    for r in range(n):
        a, sl = V.frame(lay["send_len"][r])
        a[sl] = sends[r]
        sf.append((a, sl))
        rf.append(V.frame(lay["recv_len"][r]))
    C.host_ring_all_to_all_v([a[sl].ctypes.data if sl.stop > sl.start else a.ctypes.data + sl.start for a, sl in sf],
                             [a.ctypes.data + sl.start for a, sl in rf], cnt, lay["sdispls"], lay["rdispls"],
                             len(rings), nthreads, V.BUFF, rings)
    want = V.expected(sends, cnt, lay)
    for r in range(n):
        a, sl = rf[r]
        bad = np.flatnonzero(a[sl] != want[r])
        assert bad.size == 0, f"rank {r}: {bad.size} wrong bytes, first at {bad[0]}"
        assert (a[:sl.start] == V.SENTINEL).all() and (a[sl.stop:] == V.SENTINEL).all(), r
        a, sl = sf[r]
        assert (a[sl] == sends[r]).all() and (a[:sl.start] == V.SENTINEL).all() and (a[sl.stop:] == V.SENTINEL).all(), r


def test_the_call_list_model():
    m = 2
    Cb = V.loop_bytes(m)
    assert V.call_list(0, 0, m) == []
    assert V.call_list(2 * Cb + 999, 0, m) == [("send", 0), ("send", 1), ("send", 2)]
    assert V.call_list(0, 3 * Cb, m) == [("recv", 0), ("recv", 1), ("recv", 2)]
    assert V.call_list(Cb, 3 * Cb, m) == [("send", 0), ("recv", 0), ("recv", 1), ("recv", 2)]
    assert V.call_list(Cb + 1, 1, m) == [("send", 0), ("recv", 0), ("send", 1)]
    assert [V.loops(v, m) for v in V.values(m)] == [0, 1, 1, 1, 1, 2, 3, 3]


@pytest.mark.parametrize("n", NS)
def test_the_matrices_reach_every_cursor_case_and_can_fail(n):
    """Over the matrices of one test some channel sees Ls = 3 / Lr = 0, Ls = 0 /
    Lr = 3, Ls = 1 / Lr = 3 and Ls = Lr > 0 on one element, every value of the
    set occurs, and every non-trivial case differs from a wrong candidate."""
    rings, m = rings_m(n)
    mats = V.matrices(n, m, rings)
    seen, vals = set(), set()
    for cnt in mats.values():
        seen |= V.loop_cases(cnt, rings, m)
        vals |= {cnt[s][t] for s in range(n) for t in range(n) if s != t}
    assert {(3, 0), (0, 3), (1, 3)} <= seen and any(a == b and a > 0 for a, b in seen), seen
    assert set(V.values(m)) <= vals
    if n == 2:
        Cb = V.loop_bytes(m)
        pairs = {(cnt[0][1], cnt[1][0]) for cnt in mats.values()}
        assert {(0, 2 * Cb + 999), (2 * Cb + 999, 0), (Cb, 3 * Cb), (1, 15)} <= pairs
    for name, cnt in mats.items():
        if name == "all_zero":
            continue
        for kind in ("gaps", "descending"):
            lay = V.layout(cnt, kind)
            sends = [V.make_send(s, lay["send_len"][s]) for s in range(n)]
            want = V.expected(sends, cnt, lay)
            wrong = V.wrong_candidates(sends, cnt, lay)
            differs = {k for k, w in wrong.items() if any((a != b).any() for a, b in zip(w, want))}
            assert differs, (name, kind)
            if name != "uniform" and kind == "gaps":  # gaps move every segment off its packed place
                assert "uniform_transpose" in differs and "displs_ignored" in differs, (name, kind, differs)
    # swapped counts show wherever the matrix is not symmetric
    lay = V.layout(mats["s1r3"], "packed")
    sends = [V.make_send(s, lay["send_len"][s]) for s in range(n)]
    want, wrong = V.expected(sends, mats["s1r3"], lay), V.wrong_candidates(sends, mats["s1r3"], lay)
    assert any((a != b).any() for a, b in zip(wrong["swapped_counts"], want))


@pytest.mark.parametrize("n", NS)
def test_steps_follow_each_pair_alone(n):
    """The model's invariant: both ends of a connection derive the same number
    of steps, from that pair's count alone."""
    rings, m = rings_m(n)
    nxt, prv = V.ring_next_prev(rings, n)
    for cnt in V.matrices(n, m, rings).values():
        el = V.elements(cnt, rings)
        for (r, c), (S, R) in el.items():
            sends = sum(1 for k, _ in V.call_list(S, R, m) if k == "send")
            t = nxt[c][r]
            recvs = sum(1 for k, _ in V.call_list(*el[(t, c)], m) if k == "recv")
            assert sends == recvs == V.loops(cnt[r][t], m)
            assert V.steps_per_connection(cnt, rings, m)[(c, r)] == 4 * sends


@pytest.mark.parametrize("n", NS)
def test_matrices_on_default_rings(n):
    rings, m = rings_m(n)
    for i, (name, cnt) in enumerate(V.matrices(n, m, rings).items()):
        run(n, cnt, V.LAYOUTS[i % 4], rings, salt=i)


@pytest.mark.parametrize("kind", V.LAYOUTS)
@pytest.mark.parametrize("n", [2, 4, 8])
def test_layouts(n, kind):
    """Descending displacements, sentinel gaps, displacements 1-15 bytes off
    16-byte alignment, and two peers reading one overlapping send segment."""
    rings, m = rings_m(n)
    mats = V.matrices(n, m, rings)
    run(n, mats["cyc5"], kind, rings)
    run(n, mats["s1r3"], kind, rings)


@pytest.mark.parametrize("off", range(1, 16))
def test_every_misalignment(off):
    n = 4
    rings, m = rings_m(n)
    cnt = V.cyclic(n, m, off)
    lay = V.layout(cnt, "packed")
    lay["sdispls"] = [[d + off for d in row] for row in lay["sdispls"]]
    lay["rdispls"] = [[d + 16 - off for d in row] for row in lay["rdispls"]]
    lay["send_len"] = [v + off for v in lay["send_len"]]
    lay["recv_len"] = [v + 16 - off for v in lay["recv_len"]]
    sends = [V.make_send(s, lay["send_len"][s]) for s in range(n)]
    rf = [V.frame(lay["recv_len"][r]) for r in range(n)]
    C.host_ring_all_to_all_v([s.ctypes.data for s in sends], [a.ctypes.data + sl.start for a, sl in rf], cnt,
                             lay["sdispls"], lay["rdispls"], len(rings), 544, V.BUFF, rings)
    for r, w in enumerate(V.expected(sends, cnt, lay)):
        a, sl = rf[r]
        assert (a[sl] == w).all() and (a[:sl.start] == V.SENTINEL).all() and (a[sl.stop:] == V.SENTINEL).all(), r


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 7, 8])
def test_uniform_counts_equal_all_to_all(n):
    B = 70001
    rings = C.default_rings(n)
    inputs = a2a_ref.make_inputs(n, B)
    out_u = [np.zeros(n * B, np.uint8) for _ in range(n)]
    out_v = [np.zeros(n * B, np.uint8) for _ in range(n)]
    C.host_ring_all_to_all(inputs, out_u, B, len(rings), 544, V.BUFF, rings)
    cnt = [[B] * n for _ in range(n)]
    disp = [[t * B for t in range(n)] for _ in range(n)]
    C.host_ring_all_to_all_v(inputs, out_v, cnt, disp, disp, len(rings), 544, V.BUFF, rings)
    for r in range(n):
        assert out_u[r].tobytes() == out_v[r].tobytes(), r
        assert (out_v[r] == a2a_ref.expected(inputs, B)[r]).all()


def test_other_thread_counts_change_the_granule_not_the_result():
    rings, m = rings_m(4)
    for nthr in (96, 288):
        run(4, V.matrices(4, m, rings)["cyc5"], "gaps", rings, nthreads=nthr)


def test_user_rings_with_complete_arcs():
    rings = [[(i * k) % 5 for i in range(5)] for k in (1, 2, 3, 4)]
    for rs in (rings, rings + rings):  # m = 1, m = 2
        m = a2a_ref.route(5, rs)["m"]
        run(5, V.matrices(5, m, rs)["cyc5"], "gaps", rs)


@pytest.mark.parametrize("how", ["six ranks", "forced relay", "one channel", "incomplete user rings"])
def test_refuses_a_route_that_is_not_one_hop(how):
    n = 6 if how == "six ranks" else 5 if how == "incomplete user rings" else 4
    rings = {"six ranks": C.default_rings(6), "forced relay": C.default_rings(4), "one channel": C.default_rings(4, 1),
             "incomplete user rings": [[(i * 2) % 5 for i in range(5)]] * 3}[how]
    cnt = [[16] * n for _ in range(n)]
    disp = [[16 * t for t in range(n)] for _ in range(n)]
    sends = [np.full(16 * n, r, np.uint8) for r in range(n)]
    recvs = [np.full(16 * n, V.SENTINEL, np.uint8) for _ in range(n)]
    with pytest.raises(MccsError) as ei:
        C.host_ring_all_to_all_v(sends, recvs, cnt, disp, disp, len(rings), 544, V.BUFF, rings,
                                 force_relay=how == "forced relay")
    assert ei.value.code == INVALID_USAGE
    assert all((x == V.SENTINEL).all() for x in recvs)
