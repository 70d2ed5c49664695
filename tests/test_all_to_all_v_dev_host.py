"""CPU: the AllToAllvDev table indexing on the host-thread ring
(mccs_host_ring_all_to_all_v_tables resolves each channel's element from the
rank's size table through ring_walk.h a2avd_resolve, the arithmetic the kernel
uses, then walks as mccs_host_ring_all_to_all_v does) against
tests/a2av_ref.py, byte for byte inside 0xA5 frames, and against the
host-count model on the same inputs.  Tables with two rows exchanged must make
the comparison fail: the cases can tell a wrong row index.
"""
import numpy as np
import pytest

import a2a_ref
import a2avd_ref as D
import a2av_ref as V
from mccs_amd import comm as C
from mccs_amd._lib import MccsError

NS = [2, 3, 4, 5, 7, 8]


def rings_m(n):
    rings = C.default_rings(n, 0)
    return rings, a2a_ref.route(n, rings)["m"]


def frames(n, lay, sends, room=None):
    """Send and receive frames; `room` widens the payloads (a wrong table may
    reach past the layout's lengths, never past the room)."""
    sf, rf = [], []
    for r in range(n):
        a, sl = V.frame(max(lay["send_len"][r], room or 0))
        a[sl.start:sl.start + sends[r].size] = sends[r]
        sf.append((a, sl))
        rf.append(V.frame(max(lay["recv_len"][r], room or 0)))
    return sf, rf


def run_tables(n, rings, sf, rf, tabs):
    C.host_ring_all_to_all_v_tables([a.ctypes.data + sl.start for a, sl in sf],
                                    [a.ctypes.data + sl.start for a, sl in rf], tabs, len(rings), 544, V.BUFF, rings)


def matches(n, lay, rf, want):
    for r in range(n):
        a, sl = rf[r]
        pay = a[sl.start:sl.start + lay["recv_len"][r]]
        if (pay != want[r]).any() or (a[:sl.start] != V.SENTINEL).any() or \
                (a[sl.start + lay["recv_len"][r]:] != V.SENTINEL).any():
            return False
    return True


@pytest.mark.parametrize("n", NS)
def test_matrices_from_tables(n):
    rings, m = rings_m(n)
    for i, (name, cnt) in enumerate(V.matrices(n, m, rings).items()):
        lay = V.layout(cnt, V.LAYOUTS[i % len(V.LAYOUTS)])
        sends = [V.make_send(s, lay["send_len"][s], i) for s in range(n)]
        sf, rf = frames(n, lay, sends)
        run_tables(n, rings, sf, rf, D.tables(cnt, lay))
        assert matches(n, lay, rf, V.expected(sends, cnt, lay)), (n, name)
        for (a, sl), x in zip(sf, sends):  # send buffers untouched
            assert (a[sl] == x).all() and (a[:sl.start] == V.SENTINEL).all() and (a[sl.stop:] == V.SENTINEL).all()
        # identical to the host-count model on the same inputs
        sf2, rf2 = frames(n, lay, sends)
        C.host_ring_all_to_all_v([a.ctypes.data + sl.start for a, sl in sf2],
                                 [a.ctypes.data + sl.start for a, sl in rf2], cnt, lay["sdispls"], lay["rdispls"],
                                 len(rings), 544, V.BUFF, rings)
        for (a, _), (b, _) in zip(rf, rf2):
            assert a.tobytes() == b.tobytes(), (n, name)


def test_one_rank_reads_its_size_and_offsets_from_the_table():
    for size, kind in ((4099, "gaps"), (300001, "misaligned"), (0, "packed")):
        cnt = [[size]]
        lay = V.layout(cnt, kind)
        sends = [V.make_send(0, lay["send_len"][0])]
        sf, rf = frames(1, lay, sends)
        run_tables(1, [[0]], sf, rf, D.tables(cnt, lay))
        assert matches(1, lay, rf, V.expected(sends, cnt, lay)), size


@pytest.mark.parametrize("rows", [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)])
def test_a_table_with_two_rows_swapped_fails_the_comparison(rows):
    """Negative controls, every row in at least one: small counts and
    displacements that differ in every row, so that reading any row for
    another moves or resizes a segment; the frames have room for whatever a
    swapped table addresses.  Rows 0 and 2 swapped still describe a matched
    exchange (cnt transposed), the others are cut to a consistent count below."""
    n = 4
    rings, m = rings_m(n)
    cnt = [[16 + 8 * ((3 * s + t) % 5) + (s == t) for t in range(n)] for s in range(n)]
    assert all(cnt[s][t] != cnt[t][s] for s in range(n) for t in range(s))
    lay = V.layout(cnt, "gaps")
    room = 4096
    sends = [V.make_send(s, room, 1) for s in range(n)]
    want = V.expected([x[:lay["send_len"][s]] for s, x in enumerate(sends)], cnt, lay)
    good = D.tables(cnt, lay)
    assert all(len({tuple(t[k * n:(k + 1) * n]) for k in range(4)}) == 4 for t in good)  # the four rows differ
    sf, rf = frames(n, lay, sends, room)
    run_tables(n, rings, sf, rf, good)
    assert matches(n, lay, rf, want)
    bad = [D.swap_rows(t, *rows) for t in good]
    # both ends of a pair must move the same bytes or the model would stall: take the
    # sender's (swapped) count on both sides, the displacements stay the swapped ones
    for s in range(n):
        for t in range(n):
            bad[t][D.index(2, n, s)] = bad[s][D.index(0, n, t)]
    assert all(int(v) < room // 2 for t in bad for v in t)
    sf, rf = frames(n, lay, sends, room)
    run_tables(n, rings, sf, rf, bad)
    assert not matches(n, lay, rf, want), rows


def test_refusals():
    n = 4
    rings, m = rings_m(n)
    cnt = [[16] * n for _ in range(n)]
    lay = V.layout(cnt, "packed")
    sends = [np.full(16 * n, r, np.uint8) for r in range(n)]
    recvs = [np.full(16 * n, V.SENTINEL, np.uint8) for _ in range(n)]
    tabs = D.tables(cnt, lay)
    with pytest.raises(MccsError) as ei:  # a relay route
        C.host_ring_all_to_all_v_tables(sends, recvs, tabs, len(rings), 544, V.BUFF, rings, force_relay=True)
    assert ei.value.code == 5
    with pytest.raises(MccsError) as ei:
        C.host_ring_all_to_all_v_tables(sends, recvs, [tabs[0], None, tabs[2], tabs[3]], len(rings), 544, V.BUFF, rings)
    assert ei.value.code == 4
    with pytest.raises(ValueError):
        C.host_ring_all_to_all_v_tables(sends, recvs, [t[:-1].copy() for t in tabs], len(rings), 544, V.BUFF, rings)
    with pytest.raises(ValueError):
        C.host_ring_all_to_all_v_tables(sends, recvs, [t.astype(np.uint32) for t in tabs], len(rings), 544, V.BUFF,
                                        rings)
    assert all((x == V.SENTINEL).all() for x in recvs)
