"""CPU: the AllToAll route (mccs_alltoall_route) of the default rings and of
user ring sets, against the Python model in tests/a2a_ref.py.
"""
import ctypes

import pytest

import a2a_ref
from mccs_amd import _lib
from mccs_amd import comm as C

# (nranks, channel count asked for (0 = default), hops, m): the issue's table
TABLE = [(2, 0, 1, 4), (3, 0, 1, 1), (4, 0, 1, 2), (5, 0, 1, 1), (6, 0, 5, 0), (7, 0, 1, 1), (8, 0, 1, 1),
         (8, 14, 1, 2), (4, 14, 3, 0)]
DEFAULT_CHANNELS = {2: 4, 3: 2, 4: 6, 5: 4, 6: 4, 7: 6, 8: 7}


@pytest.mark.parametrize("n,ch,hops,m", TABLE)
def test_route_table(n, ch, hops, m):
    rings = C.default_rings(n, ch)
    if ch == 0:
        assert len(rings) == DEFAULT_CHANNELS[n]
    got = C.alltoall_route(n, len(rings), rings)
    assert (got["hops"], got["m"]) == (hops, m), got
    assert got == a2a_ref.route(n, rings)


# (3 ranks, 2 channels is the default ring set of 3 ranks: one hop, test_route_table)
@pytest.mark.parametrize("n,ch", [(n, ch) for n in (3, 4, 5, 6, 7, 8) for ch in (1, 2, 3) if (n, ch) != (3, 2)])
def test_few_channels_relay(n, ch):
    rings = C.default_rings(n, ch)
    got = C.alltoall_route(n, ch, rings)
    assert (got["hops"], got["m"]) == (n - 1, 0), got
    assert got == a2a_ref.route(n, rings)
    assert got["send_bid"] == got["recv_bid"] == [list(range(ch))] * n


def test_six_ranks_cover_24_of_30_arcs():
    rings = C.default_rings(6)
    arcs = {(r[i], r[(i + 1) % 6]) for r in rings for i in range(6)}
    assert len(rings) == 4 and len(arcs) == 24


def test_four_ranks_14_channels_arc_counts():
    rings = C.default_rings(4, 14)
    counts = {}
    for r in rings:
        for i in range(4):
            counts[(r[i], r[(i + 1) % 4])] = counts.get((r[i], r[(i + 1) % 4]), 0) + 1
    assert sorted(set(counts.values())) == [4, 5]


@pytest.mark.parametrize("n,ch", [(2, 0), (3, 0), (4, 0), (5, 0), (7, 0), (8, 0), (8, 14)])
def test_sender_and_receiver_name_the_same_part(n, ch):
    rings = C.default_rings(n, ch)
    got = C.alltoall_route(n, len(rings), rings)
    assert got["hops"] == 1
    for c, ring in enumerate(rings):
        for i in range(n):
            s, t = ring[i], ring[(i + 1) % n]
            assert got["send_bid"][s][c] == got["recv_bid"][t][c], (c, s, t)
            assert 0 <= got["send_bid"][s][c] < got["m"]
    # the m channels of a pair carry parts 0 .. m-1, each once
    for s in range(n):
        for t in range(n):
            if s != t:
                parts = sorted(got["send_bid"][s][c] for c, ring in enumerate(rings)
                               if ring[(ring.index(s) + 1) % n] == t)
                assert parts == list(range(got["m"])), (s, t, parts)


@pytest.mark.parametrize("n", [2, 3, 4, 8])
def test_forced_relay(n):
    rings = C.default_rings(n)
    got = C.alltoall_route(n, len(rings), rings, force_relay=True)
    assert (got["hops"], got["m"]) == (n - 1, 0)
    assert got == a2a_ref.route(n, rings, force_relay=True)


def test_user_rings_with_complete_arcs():
    # 5 ranks: the four rotations by k = 1..4 steps are Hamiltonian cycles (5 is
    # prime) whose arcs r -> r+k cover every ordered pair once
    rings = [[(i * k) % 5 for i in range(5)] for k in (1, 2, 3, 4)]
    got = C.alltoall_route(5, 4, rings)
    assert (got["hops"], got["m"]) == (1, 1)
    assert got == a2a_ref.route(5, rings)
    assert got["send_bid"] == got["recv_bid"] == [[0] * 4] * 5
    # twice the set: m = 2, the second copy of an arc carries part 1
    got = C.alltoall_route(5, 8, rings + rings)
    assert (got["hops"], got["m"]) == (1, 2)
    assert got["send_bid"] == [[0] * 4 + [1] * 4] * 5 == got["recv_bid"]
    # one ring repeated is no complete set
    got = C.alltoall_route(5, 4, [rings[0]] * 4)
    assert (got["hops"], got["m"]) == (4, 0)


def test_identity_rings_and_one_rank():
    assert C.alltoall_route(2, 3)["m"] == 3  # rings = None: the identity on every channel
    got = C.alltoall_route(1, 2)
    assert (got["hops"], got["m"]) == (0, 0)


def test_bad_arguments():
    lib = _lib.load()
    h, m = ctypes.c_int(), ctypes.c_int()
    bad = (ctypes.c_int * 3)(0, 1, 1)  # not a permutation
    assert lib.mccs_alltoall_route(3, 1, bad, 0, ctypes.byref(h), ctypes.byref(m), None, None) == 4
    assert lib.mccs_alltoall_route(0, 1, None, 0, ctypes.byref(h), ctypes.byref(m), None, None) == 4
    assert lib.mccs_alltoall_route(2, 33, None, 0, ctypes.byref(h), ctypes.byref(m), None, None) == 4
    assert lib.mccs_alltoall_route(2, 1, None, 0, None, ctypes.byref(m), None, None) == 4


def test_call_list_model():
    for n in range(2, 9):
        assert len(a2a_ref.calls(n - 1)) == (n - 1) * (n + 2) // 2
    assert a2a_ref.calls(1) == [("send", 1), ("recv", 1)]
    assert a2a_ref.calls(3) == [("send", 1), ("recv", 1), ("send", 2), ("recvSend", 2), ("recv", 2), ("send", 3),
                                ("recvSend", 3), ("recvSend", 3), ("recv", 3)]
