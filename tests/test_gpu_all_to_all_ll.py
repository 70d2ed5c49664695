"""GPU, virtual node: the LL all-to-all (mccsCommSetAllToAllLL) under the three
calls, byte for byte against tests/a2a_ref.py, tests/a2av_ref.py and
tests/a2avd_ref.py: segment copies inside 0xA5 frames, send buffers untouched.

ll_bytes = 16 KiB, so one pair moves at most CAP = 16376 bytes per launch and
the capacity edge is cheap to reach.
1. uniform calls at n = 2, 3, 4, 6, 8 with B in {1, 7, 8, 9, 4099, CAP - 1,
   CAP}, either buffer 0 to 15 bytes off alignment; B = CAP + 1 on the same
   communicators takes the ring and gives the same bytes;
2. v matrices over {0, 1, 7, 8, 9, 15, 4099, CAP - 1, CAP} with a zero row, a
   zero column and zero self blocks, on the five layouts of a2av_ref at n = 2,
   4, 6, 8 (6 ranks have no one-hop route: the ring refuses these calls);
3. one case under MCCS_DIRECT_BLOCKS=1: one workgroup per rank, so every thread
   loops over several words and a pass straddles two peers' blocks;
4. the same matrices through Dev tables;
5. a Dev table with one count of CAP + 64: the first CAP bytes of it arrive and
   every frame stays intact.
"""
import numpy as np
import pytest

import a2a_ref
import a2av_ref as V
from mccs_amd import comm as C
import test_gpu_all_to_all_v as G
import test_gpu_all_to_all_v_dev as GD
import vnode

pytestmark = pytest.mark.gpu
DIRECT_DEFAULTS = True  # every threshold below is explicit

LL_BYTES = 16 << 10
CAP = LL_BYTES - 8
SIZES = [1, 7, 8, 9, 4099, CAP - 1, CAP]
OFFS = [(0, 0), (1, 15), (8, 3), (15, 8), (5, 0), (0, 9), (7, 7)]  # (send, recv) bytes off 16-byte alignment
VALS = [0, 1, 7, 8, 9, 15, 4099, CAP - 1, CAP]


def _comms(n, monkeypatch, uniform=0, v=0):
    comms = G._comms(n, monkeypatch, ll_bytes=LL_BYTES)
    assert all(c.all_to_all_ll_max() == CAP for c in comms)
    for c in comms:
        c.set_all_to_all_ll(bytes_per_peer=uniform, v_bytes_per_peer=v)
    return comms


class UStaged:
    """One uniform AllToAll whose payloads sit `soff` / `roff` bytes past a 16-byte boundary, in 0xA5 frames."""

    def __init__(self, n, B, soff, roff, salt=0):
        import torch

        self.n, self.B = n, B
        self.xs = a2a_ref.make_inputs(n, B, salt)
        self.ss, self.rs = slice(16 + soff, 16 + soff + n * B), slice(16 + roff, 16 + roff + n * B)
        self.sframe = [np.full(16 + soff + n * B + 64, a2a_ref.SENTINEL, np.uint8) for _ in range(n)]
        for r in range(n):
            self.sframe[r][self.ss] = self.xs[r]
        self.send = [torch.from_numpy(a).cuda() for a in self.sframe]
        self.recv = [torch.full((16 + roff + n * B + 64,), a2a_ref.SENTINEL, dtype=torch.uint8, device="cuda")
                     for _ in range(n)]
        assert all(t.data_ptr() % 16 == 0 for t in self.send + self.recv)

    def issue(self, comms, stream=None):
        with C.group():
            for r in range(self.n):
                C.all_to_all(comms[r], self.send[r].data_ptr() + self.ss.start, self.recv[r].data_ptr() + self.rs.start,
                             self.B, stream=stream)

    def check(self, tag):
        want = a2a_ref.expected(self.xs, self.B)
        for r in range(self.n):
            frame = np.full(self.recv[r].numel(), a2a_ref.SENTINEL, np.uint8)
            frame[self.rs] = want[r]
            got = self.recv[r].cpu().numpy()
            bad = np.flatnonzero(got != frame)
            assert bad.size == 0, (tag, f"rank {r}: {bad.size} wrong bytes, first at {bad[0] - self.rs.start}")
            assert self.send[r].cpu().numpy().tobytes() == self.sframe[r].tobytes(), (tag, r, "send buffer written")


def _run(st, comms, tag, algo):
    import torch

    torch.cuda.synchronize()
    st.issue(comms)
    assert all(c.last_algo() == algo for c in comms), (tag, comms[0].last_algo())
    torch.cuda.synchronize()
    for c in comms:
        c.sync()
    if isinstance(st, UStaged):
        st.check(tag)
    else:
        st.check(None, comms[0], tag)


# ---- 1. uniform calls -----------------------------------------------------------
@pytest.mark.parametrize("n", [2, 3, 4, 6, 8])
def test_uniform_sizes_and_alignments(monkeypatch, n):
    comms = _comms(n, monkeypatch, uniform=CAP)
    try:
        for i, (B, (soff, roff)) in enumerate(zip(SIZES, OFFS)):
            _run(UStaged(n, B, soff, roff, salt=i), comms, (n, B, soff, roff), "ll")
        # one byte past the limit: the ring, and the same bytes
        _run(UStaged(n, CAP + 1, 3, 5, salt=9), comms, (n, CAP + 1), "ring")
        _run(UStaged(n, CAP, 0, 0, salt=10), comms, (n, CAP, "after the ring"), "ll")
    finally:
        vnode.destroy(comms)


# ---- 2. v matrices ----------------------------------------------------------------
def matrices(n):
    """Five matrices (nine at n = 2) whose entries walk through VALS (every value lands off the
    diagonal at every n): plain, a zero row, a zero column, zero self blocks,
    and one whose first row is all CAP."""
    out, k = {}, 0
    names = ("plain", "zero_row", "zero_col", "zero_self", "cap_row")
    if n == 2:  # two entries off the diagonal: more matrices to get through VALS
        names += ("plain2", "plain3", "plain4", "plain5")
    for name in names:
        cnt = [[0] * n for _ in range(n)]
        for s in range(n):
            for t in range(n):
                if s == t:
                    cnt[s][t] = VALS[(k + 3 * s) % len(VALS)]
                else:
                    cnt[s][t] = VALS[k % len(VALS)]
                    k += 1
        if name == "zero_row":
            cnt[n - 1] = [0] * n
        if name == "zero_col":
            for s in range(n):
                cnt[s][0] = 0
        if name == "zero_self":
            for s in range(n):
                cnt[s][s] = 0
        if name == "cap_row":
            cnt[0] = [CAP] * n
        out[name] = cnt
        k += 2
    return out


def test_the_matrices_reach_every_value_off_the_diagonal():
    for n in (2, 4, 6, 8):
        mats = matrices(n)
        off = {c[s][t] for c in mats.values() for s in range(n) for t in range(n) if s != t}
        assert off == set(VALS), (n, sorted(set(VALS) - off))
        assert any(not any(c[n - 1]) for c in mats.values()) and any(not any(r[0] for r in c) for c in mats.values())


@pytest.mark.parametrize("n", [2, 4, 6, 8])
def test_v_matrices_on_every_layout(monkeypatch, n):
    comms = _comms(n, monkeypatch, v=CAP)
    try:
        assert (comms[0].all_to_all_route()["hops"] == 1) == (n != 6)
        for i, (name, cnt) in enumerate(matrices(n).items()):
            _run(G.VStaged(n, cnt, V.LAYOUTS[i % len(V.LAYOUTS)], salt=i), comms, (n, name), "ll")
        zero = [[0] * n for _ in range(n)]
        _run(G.VStaged(n, zero, "gaps"), comms, (n, "all zero"), "ll")  # still launches, writes nothing
    finally:
        vnode.destroy(comms)


# ---- 3. one workgroup per rank ----------------------------------------------------
def test_one_workgroup_loops_over_words_and_straddles_blocks(monkeypatch):
    monkeypatch.setenv("MCCS_DIRECT_BLOCKS", "1")
    n = 4
    comms = _comms(n, monkeypatch, uniform=CAP, v=CAP)
    try:
        # 4099 bytes are 513 words: the second pass of 512 threads starts on the last word of a
        # block and runs into the next peer's
        cnt = [[4099, 9, CAP, 4099], [4099, 0, 4099, 1], [CAP - 1, 4099, 7, 4099], [15, 4099, 4099, 4099]]
        for i, kind in enumerate(("misaligned", "gaps", "overlap_send")):
            _run(G.VStaged(n, cnt, kind, salt=i), comms, ("blocks=1", kind), "ll")
        _run(GD.DStaged(n, cnt, "misaligned", salt=5), comms, ("blocks=1", "dev"), "ll")
        _run(UStaged(n, 4099, 1, 2), comms, ("blocks=1", "uniform"), "ll")
    finally:
        vnode.destroy(comms)


# ---- 4. Dev tables ------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 4, 6, 8])
def test_dev_tables_on_every_layout(monkeypatch, n):
    comms = _comms(n, monkeypatch, v=CAP)
    try:
        for i, (name, cnt) in enumerate(matrices(n).items()):
            _run(GD.DStaged(n, cnt, V.LAYOUTS[(i + 2) % len(V.LAYOUTS)], salt=20 + i), comms, (n, name), "ll")
    finally:
        vnode.destroy(comms)


# ---- 5. a table that breaks the promise ------------------------------------------------
def test_a_dev_count_above_the_capacity_is_clamped(monkeypatch):
    n = 4
    comms = _comms(n, monkeypatch, v=CAP)
    try:
        cnt = matrices(n)["plain"]
        big = [list(row) for row in cnt]
        big[1][2] = CAP + 64  # in rank 1's sendcounts and in rank 2's recvcounts
        for kind in ("gaps", "misaligned"):
            st = GD.DStaged(n, big, kind, salt=3)  # the layout leaves CAP + 64 bytes of room
            clamped = [list(row) for row in big]
            clamped[1][2] = CAP
            st.cnt = clamped  # what must arrive: the first CAP bytes; the 64 after them stay 0xA5
            _run(st, comms, ("clamp", kind), "ll")
    finally:
        vnode.destroy(comms)
