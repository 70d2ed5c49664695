"""CPU: the Send/Recv pattern lists of tests/sr_ref.py cover what they claim,
and every case can fail.  The last test holds the library's own pairing of a
group's calls (the host-thread ring runs on it, byte for byte) to the same
lists, so the file needs the library's Send/Recv entry points.
"""
import numpy as np
import pytest

import a2a_ref
import a2av_ref as V
import sr_ref as SR
from mccs_amd import _lib
from mccs_amd import comm as C

NS = [2, 3, 4, 5, 7, 8]


def rings_m(n):
    rings = C.default_rings(n)
    return rings, a2a_ref.route(n, rings)["m"]


def test_the_library_has_send_and_recv():
    lib = _lib.load()
    assert all(hasattr(lib, name) for name in ("mccsSend", "mccsRecv", "mccs_host_ring_send_recv"))
    assert callable(C.send) and callable(C.recv) and callable(C.batch_send_recv) and callable(C.host_ring_send_recv)


@pytest.mark.parametrize("n", NS)
def test_pattern_lists_cover_what_they_claim(n):
    rings, m = rings_m(n)
    Cb = V.loop_bytes(m)
    pats = SR.patterns(n, m, rings)
    want = {"b_shift_3C", "c_pairwise", "d_fan", "e_two_on_a_pair", "e_zero_first", "g_one_way", "h_misaligned"}
    want |= {"a_all_pairs"} if n <= 4 else set()
    want |= {"f_send_after_recvs"} if n == 3 else set()
    assert set(pats) == want
    for ops in pats.values():
        SR.matches(ops)  # every send has its receive, of its size
        assert all(o.peer != o.rank and 0 <= o.peer < n and 0 <= o.rank < n for o in ops)
    nch = len(rings)
    el = lambda name, r: SR.elements(pats[name], r, rings)
    if n <= 4:  # (a) every ordered pair once, every size of the set, one element per channel
        ops = pats["a_all_pairs"]
        assert sorted((o.rank, o.peer) for o in ops if o.kind == "send") == [(s, t) for s in range(n) for t in range(n)
                                                                              if s != t]
        assert all(len(es) == 1 for r in range(n) for es in el("a_all_pairs", r))
    sizes = {o.nbytes for ops in pats.values() for o in ops}
    assert set(V.values(m)) <= sizes, sorted(set(V.values(m)) - sizes)
    # (b) both walks of every channel in use have three loops: each send must wait for the FIFO to drain
    assert SR.loop_cases(pats["b_shift_3C"], rings, m) <= {(3, 3), (0, 0), (3, 0), (0, 3)}
    assert 3 * Cb > SR.BUFF
    if n == 2:
        assert SR.loop_cases(pats["b_shift_3C"], rings, m) == {(3, 3)}
    # (c) odd n leaves the last rank out of the group; its peers' idle channels carry the zero element
    assert (n - 1 in SR.ranks_of(pats["c_pairwise"])) == (n % 2 == 0)
    if n > 3:
        assert any(e["S"] == 0 and e["R"] == 0 for es in el("c_pairwise", 0) for e in es)
    assert Cb + 1 in {e["S"] for es in el("c_pairwise", 0) for e in es}
    assert 4099 in {e["R"] for es in el("c_pairwise", 0) for e in es}
    # (d) rank 0 uses every channel, in both directions; the others one pair's
    assert all(e["S"] > 0 and e["R"] > 0 for es in el("d_fan", 0) for e in es)
    assert sum(e["S"] > 0 for es in el("d_fan", 1) for e in es) == m
    # (e) two elements on the pair's channels, in issue order; the zero-byte call keeps its place
    on_pair = [es for es in el("e_two_on_a_pair", 0) if len(es) > 1]
    assert len(on_pair) == m and all([e["S"] for e in es] == [2 * Cb + 999, 15] for es in on_pair)
    assert all([e["R"] for e in es] == [2 * Cb + 999, 15] for es in el("e_two_on_a_pair", 1) if len(es) > 1)
    on_pair = [es for es in el("e_zero_first", 0) if len(es) > 1]
    assert len(on_pair) == m and all([e["S"] for e in es] == [0, Cb, 4099] for es in on_pair)
    # (f) b's send, issued after its two receives, sits in element 0 beside the first receive
    if n == 3:
        ops = pats["f_send_after_recvs"]
        a, b, c = rings[0][0], rings[0][1], rings[0][2]
        kinds = [o.kind for o in ops if o.rank == b]
        assert kinds == ["recv", "recv", "send"]
        es = SR.elements(ops, b, rings)[0]
        assert [(e["S"], e["R"]) for e in es] == [(Cb + 1, 3 * Cb), (0, 2 * Cb + 999)]
        assert all(V.loops(o.nbytes, m) >= 3 for o in ops if o.rank == a and o.kind == "send")
        assert all(V.loops(o.nbytes, m) >= 2 for o in ops if o.rank == c and o.kind == "send")
        assert all(len(ch) == 1 and ch[0]["S"] == ch[0]["R"] == 0 for r in (a, b, c)
                   for ch in SR.elements(ops, r, rings)[1:])  # the other channel idles
    # (g) Ls = 3 / Lr = 0 on the sender, the reverse on the receiver
    assert (3, 0) in {(V.loops(e["S"], m), V.loops(e["R"], m)) for es in el("g_one_way", 0) for e in es}
    assert (0, 3) in {(V.loops(e["S"], m), V.loops(e["R"], m)) for es in el("g_one_way", 1) for e in es}
    # (h) every buffer off alignment, many different offsets
    offs = {o.off for o in pats["h_misaligned"]}
    assert all(1 <= o <= 15 for o in offs) and len(offs) >= min(4, n)
    for (a, sl), o in zip(SR.frames(pats["h_misaligned"]), pats["h_misaligned"]):
        assert (a.ctypes.data + sl.start) % 16 == (a.ctypes.data + o.off) % 16
    # multi-element channels and idle channels both occur
    counts = {len(es) for ops in pats.values() for r in range(n) for es in SR.elements(ops, r, rings)}
    assert {1, 2, 3} <= counts
    assert all(len(SR.elements(ops, r, rings)) == nch for ops in pats.values() for r in range(n))


@pytest.mark.parametrize("n", [2, 3, 4, 8])
def test_every_case_can_fail(n):
    """Swapping two messages or shifting one by a byte changes the expected bytes."""
    rings, m = rings_m(n)
    for name, ops in SR.patterns(n, m, rings).items():
        sent = SR.payloads(ops)
        live = [i for i in sent if ops[i].nbytes > 0]
        assert live, name
        want = SR.expected(ops, sent)
        for i in live:
            shifted = dict(sent)
            shifted[i] = V.make_send(0, ops[i].nbytes + 1, salt=1 + i)[1:]
            got = SR.expected(ops, shifted)
            assert any((got[k] != want[k]).any() for k in want), (name, i)
        for x, i in enumerate(live):
            for j in live[x + 1:]:
                k = min(ops[i].nbytes, ops[j].nbytes)
                assert (sent[i][:k] != sent[j][:k]).all(), (name, i, j)  # any two messages differ at every byte


def test_the_matching_rule():
    ops = [SR.S(0, 1, 5), SR.S(0, 1, 9), SR.R(1, 0, 5), SR.R(1, 0, 9), SR.S(1, 0, 3), SR.R(0, 1, 3)]
    assert SR.matches(ops) == [(0, 2), (1, 3), (4, 5)]
    with pytest.raises(AssertionError):
        SR.matches([SR.S(0, 1, 5), SR.R(1, 0, 6)])
    with pytest.raises(AssertionError):
        SR.matches([SR.S(0, 1, 5)])


@pytest.mark.parametrize("n", [2, 3, 4, 8])
def test_frames_catch_a_wrong_result(n):
    rings, m = rings_m(n)
    ops = SR.patterns(n, m, rings)["c_pairwise"]
    bufs = SR.frames(ops)
    want = SR.expected(ops)
    for i, w in want.items():
        bufs[i][0][bufs[i][1]] = w
    SR.check(ops, bufs)
    i = next(iter(want))
    a, sl = bufs[i]
    a[sl.stop] = 0  # one byte past a receive buffer
    with pytest.raises(AssertionError):
        SR.check(ops, bufs)
    a[sl.stop] = SR.SENTINEL
    a[sl.start] ^= 1
    with pytest.raises(AssertionError):
        SR.check(ops, bufs)
