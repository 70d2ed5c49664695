"""CPU: the byte cut of AllToAllv / AllToAllvDev on counts that sit on its
edges (tests/a2av_ref.py boundary_values, boundary_matrices).

1. channel_cut, written from the description of the cut, equals the library's
   walk (ring_walk.h through mccs_ring_walk) on every boundary value and every
   value of the older set, at m = 1, 2 and 4;
2. the boundary matrices reach the situations a streaming kernel usually breaks
   on (a2av_ref.SITUATIONS), the matrices of the older value set miss them;
3. both host-thread rings give the expected bytes on every boundary matrix
   (packed, misaligned, overlap_send), inside intact 0xA5 frames, with the send
   buffers untouched and identical receive frames;
4. the wrong results a broken implementation would give differ from the
   expected ones on every matrix.

A call has two slices only under MCCS_SLICE_STEPS=2 (sps = 2, spc = 2, floor
512 bytes: ring_kernel.h kStepPerSlice).  The default is one 4-step slice per
call (sps = 4, spc = 1, floor 1024 bytes), which has no second slice; for it
the situations are the one slice holding 1 byte, its floor and its floor + 1.
"""
import numpy as np
import pytest

import a2a_ref
import a2av_ref as V
import a2avd_ref as D
from mccs_amd import comm as C

NM = ((2, 4), (4, 2), (8, 1))  # the one-hop default ring sets: n ranks, m channels per pair
KINDS = ("packed", "misaligned", "overlap_send")


def rings_m(n):
    rings = C.default_rings(n, 0)
    return rings, a2a_ref.route(n, rings)["m"]


def element_counts(mats, rings):
    """Every S and every R of every element of the matrices."""
    S, R = set(), set()
    for cnt in mats:
        for s, r in V.elements(cnt, rings).values():
            S.add(s)
            R.add(r)
    return S, R


def test_the_slicings_are_the_kernels():
    # default: one slice of 4 steps; MCCS_SLICE_STEPS=2: two slices of 2 steps (8 KiB steps at V.BUFF)
    assert V.STEP == 8192 and V.SLICINGS == {"default": 1, "slice2": 2}
    assert V.slice_size(0, 1) == 1024 and V.slice_size(0, 2) == 512
    assert V.slice_cut(1025, 1) == [1025] and V.slice_size(1025, 1) == 1040
    assert V.slice_cut(512, 2) == [512, 0] and V.slice_cut(513, 2) == [512, 1]
    assert V.slice_cut(1024, 2) == [512, 512] and V.slice_cut(1025, 2) == [528, 497]
    assert V.slice_cut(V.CHUNK, 2) == [V.CHUNK // 2] * 2 and V.slice_cut(V.CHUNK, 1) == [V.CHUNK]
    for nelem in (0, 1, 17, 4095, 32767):
        for spc in (1, 2):
            assert sum(V.slice_cut(nelem, spc)) == nelem and V.slice_size(nelem, spc) % 16 == 0


@pytest.mark.parametrize("m", [1, 2, 4])
def test_channel_cut_is_the_librarys_walk(m):
    n = {1: 8, 2: 4, 4: 2}[m]
    assert len(V.boundary_values(m)) >= {1: 19, 2: 22, 4: 24}[m]
    for count in sorted(set(V.boundary_values(m)) | set(V.values(m))):
        lib = C.ring_walk(C.FUNC_ALLGATHER, n, m, 1, 544, V.BUFF, count)
        assert V.channel_cut(count, m) == [tuple(int(v) for v in row) for row in lib], (m, count)
        assert sum(row[3] for row in V.channel_cut(count, m)) == count
        assert len(V.channel_cut(count, m)) == m * V.loops(count, m)


@pytest.mark.parametrize("n,m", NM)
def test_boundary_matrices_put_every_value_on_both_sides(n, m):
    rings, m_ = rings_m(n)
    assert m_ == m
    mats = V.boundary_matrices(n, m, rings)
    assert 1 <= len(mats) <= {2: 20, 4: 6, 8: 2}[n]
    S, R = element_counts(mats, rings)
    want = set(V.boundary_values(m)) | {0}
    assert want <= S and want <= R, (want - S, want - R)
    rel = set()
    for cnt in mats:
        assert all(cnt[s][s] in V.SELF_VALUES for s in range(n))
        assert all(cnt[s][t] in want for s in range(n) for t in range(n) if s != t)
        for s, r in V.elements(cnt, rings).values():
            if s != r:
                ls, lr = V.loops(s, m), V.loops(r, m)
                rel.add("<" if ls < lr else "=" if ls == lr else ">")
        for kind in KINDS + ("gaps", "descending"):
            lay = V.layout(cnt, kind)
            assert max(lay["send_len"] + lay["recv_len"]) < 1 << 20
    assert rel == {"<", "=", ">"}
    assert {cnt[s][s] for cnt in mats for s in range(n)} == set(V.SELF_VALUES)


# what one m cannot reach: with one channel per pair no channel is past the end or starts on it
UNREACHABLE = {1: {"last 0", "past"}, 2: set(), 4: set()}


@pytest.mark.parametrize("n,m", NM)
def test_boundary_matrices_reach_the_situations_the_older_values_miss(n, m):
    rings, _ = rings_m(n)
    S, R = element_counts(V.boundary_matrices(n, m, rings), rings)
    for side in (S, R):
        assert V.cut_situations(side, m) == V.SITUATIONS - UNREACHABLE[m], (n, V.SITUATIONS - V.cut_situations(side, m))
    old = list(V.matrices(n, m, rings).values()) + [V.cyclic(n, m, k, stride) for k in range(8) for stride in (1, 3)]
    So, Ro = element_counts(old, rings)
    assert So | Ro == set(V.values(m)) | {V.loop_bytes(m) + 1}
    reached = V.cut_situations(So | Ro, m)
    # the older set has C (full chunks, so a full second slice too) and C + 1 (a second loop of 1 byte,
    # which is also a 1-byte slice); with more than one channel per pair its 1 and 15 leave channels
    # past the end
    assert reached == {"last chunk", "second loop 1", "last 1", "default slice 1", "slice2 second full"} | \
        ({"past"} if m > 1 else set())
    missed = V.SITUATIONS - UNREACHABLE[m] - reached
    assert missed == {"last G-1", "last G", "slice2 second 0", "slice2 second 1", "default slice floor",
                      "default slice floor + 1"} | ({"last 0"} if m > 1 else set())
    # and no full second slice on the 512-byte floor: 1024 bytes cut into 512 + 512
    assert 1024 in S and 1024 in R and not any(row[3] == 1024 for c in So | Ro for row in V.channel_cut(c, m))


def test_every_situation_is_reached_at_some_rank_count():
    got = set()
    for n, m in NM:
        rings, _ = rings_m(n)
        S, R = element_counts(V.boundary_matrices(n, m, rings), rings)
        got |= V.cut_situations(S, m) & V.cut_situations(R, m)
    assert got == V.SITUATIONS


def _frames(n, lay, sends):
    sf = []
    for r in range(n):
        a, sl = V.frame(lay["send_len"][r])
        a[sl] = sends[r]
        sf.append((a, sl))
    return sf, [V.frame(lay["recv_len"][r]) for r in range(n)]


@pytest.mark.parametrize("n,m", NM)
def test_both_host_rings_on_the_boundary_matrices(n, m):
    rings, _ = rings_m(n)
    for i, cnt in enumerate(V.boundary_matrices(n, m, rings)):
        for kind in KINDS:
            lay = V.layout(cnt, kind)
            sends = [V.make_send(s, lay["send_len"][s], i) for s in range(n)]
            want = V.expected(sends, cnt, lay)
            sf, rf = _frames(n, lay, sends)
            C.host_ring_all_to_all_v([a.ctypes.data + sl.start for a, sl in sf],
                                     [a.ctypes.data + sl.start for a, sl in rf], cnt, lay["sdispls"], lay["rdispls"],
                                     len(rings), 544, V.BUFF, rings)
            sf2, rf2 = _frames(n, lay, sends)
            C.host_ring_all_to_all_v_tables([a.ctypes.data + sl.start for a, sl in sf2],
                                            [a.ctypes.data + sl.start for a, sl in rf2], D.tables(cnt, lay),
                                            len(rings), 544, V.BUFF, rings)
            for r in range(n):
                for frames_s, frames_r in ((sf, rf), (sf2, rf2)):
                    a, sl = frames_r[r]
                    bad = np.flatnonzero(a[sl] != want[r])
                    assert bad.size == 0, (n, i, kind, r, f"first wrong byte at {bad[0]}")
                    assert (a[:sl.start] == V.SENTINEL).all() and (a[sl.stop:] == V.SENTINEL).all(), (n, i, kind, r)
                    a, sl = frames_s[r]
                    assert (a[sl] == sends[r]).all() and (a[:sl.start] == V.SENTINEL).all() and \
                        (a[sl.stop:] == V.SENTINEL).all(), (n, i, kind, r, "send frame")
                assert rf[r][0].tobytes() == rf2[r][0].tobytes(), (n, i, kind, r)


@pytest.mark.parametrize("n,m", NM)
def test_wrong_candidates_differ_on_every_boundary_matrix(n, m):
    rings, _ = rings_m(n)
    for i, cnt in enumerate(V.boundary_matrices(n, m, rings)):
        told = {}
        for kind in KINDS:
            lay = V.layout(cnt, kind)
            sends = [V.make_send(s, lay["send_len"][s], i) for s in range(n)]
            want = V.expected(sends, cnt, lay)
            for name, cand in V.wrong_candidates(sends, cnt, lay).items():
                if any((a != b).any() for a, b in zip(cand, want)):
                    told.setdefault(name, set()).add(kind)
        # packed displacements are the ones a call that ignores them would use, and a near-uniform
        # packed matrix is its own uniform transpose: the misaligned layout tells every candidate
        assert all("misaligned" in told.get(name, ()) for name in ("uniform_transpose", "swapped_counts",
                                                                   "displs_ignored")), (n, i, told)
        assert told["swapped_counts"] == set(KINDS), (n, i, told)
