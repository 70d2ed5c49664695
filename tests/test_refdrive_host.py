"""CPU: host logic of the reference-driven harness (mccs_amd/refdrive.py) --
plan.rs's work-ring reservation and rolling acknowledgements (plan.rs:380-541)
against a simulated kernel, and the configuration-only variants the bench
times.  No GPU."""
import pytest

from mccs_amd import comm as C
from mccs_amd import refdrive


class _SimKernel:
    """Launches run in order, one per host poll of workFifoDone (the kernel
    writes doneAcks to each of its channels' done words, common.h:153-155)."""

    def __init__(self, nch, stuck=False):
        self.done = [0] * nch
        self.pending = []
        self.stuck = stuck

    def read(self):
        if self.pending and not self.stuck:
            chans, acks, _ = self.pending.pop(0)
            for c in chans:
                self.done[c] = acks
        return list(self.done)

    def write(self, c, v):
        self.done[c] = v


@pytest.mark.parametrize("depth,nch,ks", [(16, 3, [3]), (16, 4, [1, 2, 3, 4]), (64, 7, [7, 5, 1])])
def test_work_ring_never_splits_a_launch_and_never_reuses_unacked_slots(depth, nch, ks):
    ring = refdrive.WorkRing(nch, depth)
    sim = _SimKernel(nch)
    held = {}  # slot -> launch id still pending
    wraps = 0
    for i in range(40 * depth):
        k = ks[i % len(ks)]
        chans = list(range(k))
        before = ring.next_available
        start, acks = ring.reserve(chans, sim.read, sim.write, timeout_s=5)
        if start != before:
            wraps += 1
            assert start % depth == 0  # wrapped to the ring start
        assert (start % depth) + k <= depth  # one launch's works are contiguous
        done_ids = {lid for lid in held.values() if all(lid != p[2] for p in sim.pending)}
        for s in range(start, start + k):
            lid = held.get(s % depth)
            assert lid is None or lid in done_ids, f"slot {s % depth} reused before launch {lid} was acknowledged"
        for s in range(start, start + k):
            held[s % depth] = i
        assert acks == (start + k) & 0xFFFFFFFF
        sim.pending.append((chans, acks, i))
    assert wraps > 0 or depth % k == 0


def test_reference_ack_arithmetic_lets_the_host_overwrite_an_unread_work():
    """The reference quirk the default avoids (plan.rs:461-470): with
    DoneAcks = first + k + 1, one acknowledged launch also releases the
    first entry of the launch after it.  A host that runs a full ring ahead
    then reuses that entry while its launch is still pending."""
    depth, nch = 16, 4
    ks = [1, 2, 3, 4]
    ring = refdrive.WorkRing(nch, depth, reference_acks=True)
    sim = _SimKernel(nch)
    held, hit = {}, False
    for i in range(40 * depth):
        k = ks[i % len(ks)]
        start, acks = ring.reserve(list(range(k)), sim.read, sim.write, timeout_s=5)
        pending = {p[2] for p in sim.pending}
        hit = hit or any(held.get(s % depth) in pending for s in range(start, start + k))
        for s in range(start, start + k):
            held[s % depth] = i
        sim.pending.append((list(range(k)), acks, i))
    assert hit


def test_work_ring_flow_control_stops_at_depth_without_acknowledgements():
    depth, nch = 16, 2
    ring = refdrive.WorkRing(nch, depth)
    sim = _SimKernel(nch, stuck=True)
    n = 0
    with pytest.raises(RuntimeError, match="no acknowledgement"):
        for _ in range(depth):
            ring.reserve([0, 1], sim.read, sim.write, timeout_s=0.05)
            n += 1
    assert n * 2 <= depth + 2


def test_idle_channel_does_not_stop_the_ring():
    """Channel 1 works once and then idles while channel 0 takes four ring
    depths of launches: the host must keep moving the idle channel's expected
    value along with its done word (NCCL waitWorkFifoAvailable), or the idle
    channel looks busy at a stale value from the second wait on."""
    depth = 16
    ring = refdrive.WorkRing(2, depth)
    sim = _SimKernel(2)
    start, acks = ring.reserve([0, 1], sim.read, sim.write, timeout_s=2)
    sim.pending.append(([0, 1], acks, 0))
    for i in range(4 * depth):
        start, acks = ring.reserve([0], sim.read, sim.write, timeout_s=2)
        sim.pending.append(([0], acks, i + 1))
    assert ring.next_available == 2 + 4 * depth
    assert sim.read()[1] == ring.chan_next[1]  # idle: done word and expectation agree


def test_work_ring_counters_wrap_u32():
    ring = refdrive.WorkRing(2, 16)
    ring.next_available = ring.acked_min = 0xFFFFFFF0
    ring.chan_next = [0xFFFFFFF0, 0xFFFFFFF0]
    sim = _SimKernel(2)
    sim.done = [0xFFFFFFF0, 0xFFFFFFF0]
    for _ in range(40):
        start, acks = ring.reserve([0, 1], sim.read, sim.write, timeout_s=5)
        sim.pending.append(([0, 1], acks, 0))
        assert 0 <= start <= 0xFFFFFFFF and (start % 16) + 2 <= 16


# ---- batched plans: pre_launch_schedule + upload_work, host only --------------------------
F32, MB = 7, 1 << 18  # 1 MiB of fp32: two channels, 544 threads


def _tasks(counts, dtype=F32):
    """One task per count; the send pointer names the task."""
    return [(0x10000 * (t + 1), 0x10000 * (t + 1) + 8, c, dtype) for t, c in enumerate(counts)]


def _ring_of(p, depth):
    """The work ring after the upload: slot -> work.  No two works of one
    launch share a slot."""
    ring = {}
    for at, w in p.works:
        assert (at & (depth - 1)) not in ring
        ring[at & (depth - 1)] = w
    return ring


def _walk(p, depth):
    """ring_kernel_body's walk (common.h:92-179): block chIdx starts at
    workHead + chIdx and follows workHead + workNext until isLast; the pointer
    arithmetic does not wrap, so every slot it computes must lie inside the
    ring.  Returns per channel id the works visited, each a list of elements
    (sendbuff, count, nWarps, bid, nChannels), and the doneAcks seen."""
    ring, head = _ring_of(p, depth), p.start & (depth - 1)
    out, acks, seen = {}, {}, set()
    assert p.grid == len(p.chans) == bin(p.mask).count("1")
    for ch_idx, c in enumerate(p.chans):
        assert p.mask >> c & 1 and bin(p.mask & ((1 << c) - 1)).count("1") == ch_idx
        slot, works = head + ch_idx, []
        while True:
            assert 0 <= slot < depth and slot not in seen, (slot, c)
            seen.add(slot)
            w = ring[slot]
            assert w.header.type == 1
            elems = []
            for i in range(10):
                e = w.elems[i]
                if not e.isUsed:
                    assert all(not w.elems[j].isUsed for j in range(i, 10))
                    break
                elems.append((e.sendbuff, e.count, e.nWarps, e.bid, e.nChannels))
            works.append(elems)
            if w.header.isLast:
                assert w.header.inFifo
                acks[c] = w.header.doneAcks
                break
            slot = head + w.header.workNext
        out[c] = works
    assert seen == set(ring)  # every uploaded work is visited, by exactly one channel
    return out, acks


def _check_plan(p, tasks, nch, depth):
    """Every channel visits exactly the elements the plan gave it, in task
    order; at most 10 per work; a new work exactly where nWarps changes or
    the work before is full."""
    visited, acks = _walk(p, depth)
    want = {c: [] for c in range(nch)}
    for t, (k, nthr, sel) in enumerate(p.tasks):
        assert (k, nthr) == C.task_schema(tasks[t][2] * refdrive.ESIZE[tasks[t][3]], nch) and len(sel) == k
        for bid, c in enumerate(sel):
            want[c].append((tasks[t][0], tasks[t][2], nthr // 32, bid, k))
    assert sorted(visited) == [c for c in range(nch) if want[c]] == p.chans
    for c, works in visited.items():
        assert [e for w in works for e in w] == want[c]
        for i, w in enumerate(works):
            assert 1 <= len(w) <= 10 and len({e[2] for e in w}) == 1
            if i:
                assert len(works[i - 1]) == 10 or works[i - 1][0][2] != w[0][2]
    assert p.block == max(nthr for _, nthr, _ in p.tasks)
    assert [acks[c] for c in p.chans] == p.acks
    assert p.nworks == [len(visited[c]) for c in p.chans] and p.end == p.start + sum(p.nworks)
    return visited


@pytest.mark.parametrize("ntasks,nworks", [(1, 1), (10, 1), (11, 2), (21, 3)])
@pytest.mark.parametrize("position", [0, 5, 1024 + 3])
def test_batched_plan_walk_two_channels(ntasks, nworks, position):
    tasks = _tasks([MB + t for t in range(ntasks)])
    p = refdrive.build_plan(tasks, 2, position)
    assert p.start == position and p.chans == [0, 1] and p.nworks == [nworks, nworks]
    visited = _check_plan(p, tasks, 2, refdrive.WORK_DEPTH)
    assert [len(w) for w in visited[0]] == [10] * (nworks - 1) + [ntasks - 10 * (nworks - 1)]
    # first works at head + chIdx, later works behind all first works, channel by channel
    assert sorted(at for at, _ in p.works) == list(range(position, position + 2 * nworks))
    assert [at for at, _ in p.works] == [position] + list(range(position + 2, position + 1 + nworks)) + \
        [position + 1] + list(range(position + 1 + nworks, position + 2 * nworks))


MIXED = [1000 + 7919 * i for i in range(12)]  # fp32: 96- to 544-thread elements, one to five channels


def test_batched_plan_mixed_sizes_five_channels_follow_the_load():
    import vnode

    nch = 5
    tasks = _tasks(MIXED)
    p = refdrive.build_plan(tasks, nch, 7)
    _check_plan(p, tasks, nch, refdrive.WORK_DEPTH)
    planner = vnode.Planner(nch, list(range(nch)))
    for t, (k, nthr, sel) in enumerate(p.tasks):
        assert (k, nthr, sel) == planner.select(4 * MIXED[t], 4 * MIXED[t]), t
    # block id b is not channel b, and a channel's elements differ in nWarps
    assert any(sel != list(range(k)) for k, _, sel in p.tasks)
    assert len({nthr for _, nthr, _ in p.tasks}) > 1 and max(p.nworks) > 1
    assert p.block == 544 and p.grid == 5


@pytest.mark.parametrize("depth", [16, 1024])
def test_later_works_cross_the_ring_end_with_negative_work_next(depth):
    """The wrap test looks at the first works only (plan.rs:436), so with the
    head two first works before the ring's end the later works continue at
    slot 0: their workNext, relative to the head, is negative."""
    tasks = _tasks([MB + t for t in range(21)])  # 2 first + 4 later works
    for laps in (0, 3):
        position = laps * depth + depth - 4
        p = refdrive.build_plan(tasks, 2, position, depth=depth)
        assert p.start == position and p.end == position + 6  # not moved to the ring start
        nexts = [w.header.workNext for _, w in p.works if not w.header.isLast]
        assert min(nexts) == -(depth - 4) and max(nexts) > 0
        _check_plan(p, tasks, 2, depth)
    # one slot further the FIRST works would cross: the launch moves to the ring start
    p = refdrive.build_plan(tasks, 2, depth - 1, depth=depth)
    assert p.start == depth and all(w.header.workNext > 0 for _, w in p.works if not w.header.isLast)
    _check_plan(p, tasks, 2, depth)


def test_reference_acks_of_a_multi_work_launch():
    """plan.rs:461-470: DoneAcks = new_subsequent_start + 1 when the channel's
    last work is written.  Channels 0 and 2 have one work, channel 1 three."""
    nworks = [1, 3, 1]
    assert refdrive.WorkRing.acks_for(100, nworks, True) == [104, 105, 106]
    assert refdrive.WorkRing.acks_for(100, nworks, False) == [105, 105, 105]
    assert refdrive.WorkRing.acks_for(100, [3, 1, 2], True) == [105, 106, 106]
    assert refdrive.WorkRing.acks_for(100, [3, 1, 2], False) == [105, 106, 106]
    assert refdrive.WorkRing.acks_for(100, [1, 3], True) == [103, 104]
    assert refdrive.WorkRing.acks_for(100, [1, 3], False) == [104, 104]
    assert refdrive.WorkRing.acks_for(100, [1, 1], True) == [103, 103]
    assert refdrive.WorkRing.acks_for(0xFFFFFFFE, [1, 1], False) == [0, 0]


def test_reserve_without_later_works_is_unchanged():
    for ref in (False, True):
        a, b = refdrive.WorkRing(4, 16, reference_acks=ref), refdrive.WorkRing(4, 16, reference_acks=ref)
        sa, sb = _SimKernel(4), _SimKernel(4)
        for i in range(100):
            chans = list(range(1 + i % 4))
            start, acks = a.reserve(chans, sa.read, sa.write, timeout_s=5)
            start2, acks2 = b.reserve_works(chans, [1] * len(chans), sb.read, sb.write, timeout_s=5)
            assert (start, [acks] * len(chans)) == (start2, acks2)
            assert acks == (start + len(chans) + ref) & 0xFFFFFFFF
            assert (a.next_available, a.chan_next, a.acked_min) == (b.next_available, b.chan_next, b.acked_min)
            sa.pending.append((chans, acks, i))
            sb.pending.append((chans, acks, i))


class _SimChannels:
    """Launches run in stream order; within the oldest one, one channel per
    host poll loads its next work (walking workNext as the kernel does) and
    acknowledges only when that work is its last.  `mem` is the ring: slot ->
    id of the launch whose work the host wrote there last."""

    def __init__(self, nch, depth, rng):
        self.done, self.depth, self.rng = [0] * nch, depth, rng
        self.mem, self.pending, self.overwritten = {}, [], []

    def launch(self, lid, start, works, chans):
        ring = {}
        for at, w in works:
            self.mem[at % self.depth] = lid
            ring[at % self.depth] = w
        head = start % self.depth
        self.pending.append({"id": lid, "head": head, "ring": ring, "at": {c: head + i for i, c in enumerate(chans)}})

    def read(self):
        if self.pending:
            la = self.pending[0]
            c = sorted(la["at"])[self.rng.integers(len(la["at"]))]
            slot = la["at"][c]
            if self.mem[slot] != la["id"]:  # the host reused the slot before this channel read it
                self.overwritten.append((la["id"], slot, slot == la["head"]))
            w = la["ring"][slot]
            if w.header.isLast:
                self.done[c] = w.header.doneAcks
                del la["at"][c]
                if not la["at"]:
                    self.pending.pop(0)
            else:
                la["at"][c] = la["head"] + w.header.workNext
        return list(self.done)

    def write(self, c, v):
        self.done[c] = v


def _random_launches(depth, nch, reference_acks, seed, launches):
    import numpy as np

    rng = np.random.default_rng(seed)
    ring = refdrive.WorkRing(nch, depth, reference_acks=reference_acks)
    sim = _SimChannels(nch, depth, rng)
    task = [(0x1000, 0x2000, 1, F32)]
    crossed = multi = 0
    for lid in range(launches):
        k = int(rng.integers(1, nch + 1))
        chans = sorted(rng.choice(nch, k, replace=False).tolist())
        nworks = [int(rng.integers(1, 4)) if rng.random() < 0.5 else 1 for _ in chans]
        queues = [[] for _ in range(nch)]
        for c, w in zip(chans, nworks):
            queues[c] = [[(0, 3, 0, 1)] for _ in range(w)]
        start, acks = ring.reserve_works(chans, nworks, sim.read, sim.write, timeout_s=5)
        assert start % depth + k <= depth  # the first works are contiguous
        works, chans2, nworks2, acks2 = refdrive.layout_works(task, queues, start, depth, reference_acks)
        assert (chans2, nworks2, acks2) == (chans, nworks, acks)
        crossed += any(w.header.workNext < 0 for _, w in works if not w.header.isLast)
        multi += sum(nworks) > k
        sim.launch(lid, start, works, chans)
    return sim.overwritten, crossed, multi


@pytest.mark.parametrize("depth,nch", [(16, 3), (16, 5), (64, 6)])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_multi_work_launches_never_reuse_an_unread_slot(depth, nch, seed):
    """With the exact acknowledgement (the slot after a chained channel's last
    work, the launch's end for a single work; written when the channel loads
    its LAST work) the host, always as far ahead as the
    flow control lets it, never rewrites a slot before its channel read it."""
    overwritten, crossed, multi = _random_launches(depth, nch, False, seed, 60 * depth)
    assert not overwritten
    assert crossed > 0 and multi > 10  # later works crossed the ring's end on the way


def test_reference_acks_with_multi_work_launches_free_only_the_next_head_early():
    """The reference arithmetic is one past the launch only for a single-work
    channel behind which no later works follow; the slot it frees early is
    the head of the next launch, and no other."""
    hits = []
    for seed in (1, 2, 3):
        overwritten, crossed, multi = _random_launches(16, 4, True, seed, 60 * 16)
        assert crossed > 0 and multi > 10
        hits += overwritten
    assert hits and all(is_head for _, _, is_head in hits)


def test_all_gather_plan_uses_total_bytes_of_every_rank():
    """task.rs:95-102: the schema of an AllGather comes from nbytes * n; the
    element count is the rank's own nbytes (all_gather.h:16)."""
    n, nbytes = 3, 30000
    assert C.task_schema(nbytes, 2)[0] == 1 and C.task_schema(nbytes * n, 2) == (2, 544)
    p = refdrive.build_plan([(0x7000, 0x9000, nbytes, 0)], 2, 11, func=refdrive.FUNC_ALLGATHER, nranks=n)
    assert p.tasks == [(2, 544, [0, 1])] and (p.grid, p.block, p.mask, p.start, p.end) == (2, 544, 3, 11, 13)
    visited, _ = _walk(p, refdrive.WORK_DEPTH)
    assert visited == {0: [[(0x7000, nbytes, 17, 0, 2)]], 1: [[(0x7000, nbytes, 17, 1, 2)]]}
    assert [w.elems[0].recvbuff for _, w in p.works] == [0x9000, 0x9000]
    # a small one: one channel, the thread count of the total
    p = refdrive.build_plan([(0x7000, 0x9000, 4000, 0)], 2, 0, func=refdrive.FUNC_ALLGATHER, nranks=n)
    assert p.tasks == [(1, C.task_schema(12000, 2)[1], [0])] and p.tasks[0][1] != C.task_schema(4000, 2)[1]
    assert p.works[0][1].elems[0].count == 4000 and p.works[0][1].elems[0].nChannels == 1


@pytest.mark.parametrize("n", [2, 4, 8])
def test_configuration_only_variants(n):
    vs = refdrive.default_variants(n, C.default_rings)
    names = [v["name"] for v in vs]
    assert names[:5] == ["ch2_reference_ring_sender", "ch2_reference_ring_receiver",
                         "ch2_reference_ring_sender_hostfifo", "ch32_reference_ring_sender",
                         "ch32_reference_ring_sender_hostfifo"]
    # the shipped 2-channel shape under each config-only choice: locality and
    # the reference's own host-memory FIFOs
    assert [(v["locality"], v["fifo"]) for v in vs[:3]] == [("sender", "device"), ("receiver", "device"),
                                                           ("sender", "host")]
    for v in vs:
        assert 1 <= v["nch"] <= 32 and v["locality"] in ("sender", "receiver") and v["fifo"] in ("device", "host")
        if v["rings"] is not None:
            assert len(v["rings"]) == v["nch"]
            for r in v["rings"]:
                assert sorted(r) == list(range(n))
    spread = vs[5]["rings"]
    # the spread variants cycle over every distinct default ring equally often
    uniq = {tuple(r) for r in spread}
    assert all(sum(1 for r in spread if tuple(r) == u) == len(spread) // len(uniq) for u in uniq)
    if n == 8:
        assert len(uniq) == 7 and vs[5]["nch"] == 28


def test_variants_capped_when_ranks_share_a_gpu():
    vs = refdrive.default_variants(8, C.default_rings, 16)
    assert [v["nch"] for v in vs] == [2, 2, 2, 16, 16, 14, 14]
    assert all(v["nch"] * 8 <= 128 for v in vs)


def test_reference_rings_are_the_engine_default():
    assert refdrive.reference_rings(4, 2) == [[0, 1, 2, 3], [0, 1, 2, 3]]


def test_host_segment_roundtrip_without_gpu(monkeypatch):
    """The host connector's segment: shm_open + ftruncate (zeroed) + mmap +
    mlock, registered through hipHostRegister (faked here: no GPU); a peer
    opening the name sees the creator's bytes; the name is unlinked once
    every rank mapped it."""
    import ctypes
    import uuid

    calls = []

    class FakeHip:
        def hipHostRegister(self, p, n, flags):
            calls.append(("reg", n, flags))
            return 0

        def hipHostGetDevicePointer(self, out, p, flags):
            out._obj.value = p.value
            return 0

        def hipHostUnregister(self, p):
            calls.append(("unreg",))
            return 0

    monkeypatch.setattr(refdrive, "hip", lambda: FakeHip())
    name = f"/mccs_test_{uuid.uuid4().hex[:12]}"
    a = refdrive.HostSegment(name, 3 * 4096 + 5, create=True)
    try:
        assert a.nbytes == 4 * 4096 and a.dev == a.host
        assert bytes((ctypes.c_char * 64).from_address(a.host)) == bytes(64)
        ctypes.memset(a.host + 4096, 0x5A, 16)
        b = refdrive.HostSegment(name, 3 * 4096 + 5, create=False)
        assert bytes((ctypes.c_char * 16).from_address(b.host + 4096)) == b"\x5a" * 16
        a.unlink()
        with pytest.raises(OSError):
            refdrive.HostSegment(name, 4096, create=False)
        b.close()
    finally:
        a.close()
    assert calls.count(("reg", 4 * 4096, refdrive.hipHostRegisterMapped)) == 2 and calls.count(("unreg",)) == 2


# ---- redOpArg: PreMulSum's scalar / SumPostDiv's divisor, per work element ------------------
def _golden():
    import json
    import os

    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "abi_layout.json")) as f:
        return json.load(f)


def _raw_work(word0, last, elems):
    """One mccsDevWork byte by byte from the golden layout alone: word0 is
    workNext or doneAcks; elems = [(nWarps, send, recv, count, bid, nChannels, redOpArg)]."""
    import struct

    g = _golden()
    b = bytearray(g["sizeof(mccsDevWork)"])
    struct.pack_into("<I", b, 0, word0 & 0xFFFFFFFF)
    b[6] = 3 if last else 0  # isLast | inFifo
    b[g["mccsDevWorkHeader.type"]] = 1
    for i, (nwarps, send, recv, count, bid, nch, arg) in enumerate(elems):
        at = g["sizeof(mccsDevWorkHeader)"] + i * g["sizeof(mccsDevWorkElem)"]
        b[at] = 1  # isUsed
        b[at + g["mccsDevWorkElem.nWarps"]] = nwarps
        struct.pack_into("<Q", b, at + g["mccsDevWorkElem.sendbuff"], send)
        struct.pack_into("<Q", b, at + g["mccsDevWorkElem.recvbuff"], recv)
        struct.pack_into("<Q", b, at + g["mccsDevWorkElem.count"], count)
        b[at + g["mccsDevWorkElem.bid"]] = bid
        b[at + g["mccsDevWorkElem.nChannels"]] = nch
        struct.pack_into("<Q", b, at + g["mccsDevWorkElem.redOpArg"], arg)
    return bytes(b)


def _arg_at(work, i):
    """redOpArg of element i, read from the raw work bytes at the golden offset."""
    g = _golden()
    assert g["mccsDevWorkElem.redOpArg"] == 40
    at = g["sizeof(mccsDevWorkHeader)"] + i * g["sizeof(mccsDevWorkElem)"] + g["mccsDevWorkElem.redOpArg"]
    return int.from_bytes(bytes(work)[at:at + 8], "little")


# fp32 counts: 40 000 bytes (544 threads) load channel 0; the two 5 000-byte
# tasks (96 threads) then share channel 1's first work; the 10 000-byte task
# (160 threads) opens a chained second work there
SCALAR_COUNTS = [10000, 1250, 1250, 2500]
SCALARS = [0x3F400000, 0x3EAAAAAB, 0xFFFFFFFF00000007, None]  # the last task leaves op_arg out


def _scalar_tasks(with_args):
    return [t + ((a,) if with_args and a is not None else ()) for t, a in zip(_tasks(SCALAR_COUNTS), SCALARS)]


@pytest.mark.parametrize("position", [0, 1024 + 9])
def test_four_field_tasks_lay_out_the_same_bytes_as_before(position):
    """The works of tasks without op_arg, against bytes written by hand from
    tests/golden/abi_layout.json: what the bench's reference-driven leg uploads."""
    tasks = _scalar_tasks(False)
    assert all(len(t) == 4 for t in tasks)
    p = refdrive.build_plan(tasks, 2, position)
    (s0, r0, c0, _), (s1, r1, c1, _), (s2, r2, c2, _), (s3, r3, c3, _) = tasks
    want = [(position, _raw_work(position + 3, True, [(17, s0, r0, c0, 0, 1, 0)])),
            (position + 1, _raw_work(2, False, [(3, s1, r1, c1, 0, 1, 0), (3, s2, r2, c2, 0, 1, 0)])),
            (position + 2, _raw_work(position + 3, True, [(5, s3, r3, c3, 0, 1, 0)]))]
    assert [(at, bytes(w)) for at, w in p.works] == want
    _check_plan(p, tasks, 2, refdrive.WORK_DEPTH)


def test_build_plan_gives_every_element_its_own_red_op_arg():
    tasks = _scalar_tasks(True)
    assert [len(t) for t in tasks] == [5, 5, 5, 4]
    p = refdrive.build_plan(tasks, 2, 7)
    _check_plan(p, tasks, 2, refdrive.WORK_DEPTH)
    (_, w0), (_, first), (_, chained) = p.works
    assert p.nworks == [1, 2] and first.header.workNext == 2 and chained.header.isLast and p.block == 544
    # two elements of one work, each with its own scalar, all 64 bits of it
    assert [first.elems[i].isUsed for i in range(3)] == [1, 1, 0]
    assert (_arg_at(first, 0), _arg_at(first, 1), _arg_at(first, 2)) == (SCALARS[1], SCALARS[2], 0)
    assert (first.elems[0].redOpArg, first.elems[1].redOpArg) == (SCALARS[1], SCALARS[2])
    assert _arg_at(w0, 0) == SCALARS[0]
    # the chained work's task left op_arg out: 0
    assert chained.elems[0].nWarps == 5 and _arg_at(chained, 0) == 0
    # with a scalar, the chained work keeps it; nothing but the scalars differs from the plain layout
    tasks[3] = tasks[3] + (0x40400000,)
    q = refdrive.build_plan(tasks, 2, 7)
    assert _arg_at(q.works[2][1], 0) == 0x40400000 and _arg_at(q.works[1][1], 1) == SCALARS[2]
    plain = refdrive.build_plan(_scalar_tasks(False), 2, 7)
    g = _golden()
    for (at, w), (at0, w0) in zip(q.works, plain.works):
        a, b = bytearray(bytes(w)), bytearray(bytes(w0))
        for i in range(10):
            lo = g["sizeof(mccsDevWorkHeader)"] + i * g["sizeof(mccsDevWorkElem)"] + g["mccsDevWorkElem.redOpArg"]
            a[lo:lo + 8] = bytes(8)
        assert at == at0 and a == b


class _HostOnlyRank(refdrive.RefDrivenRank):
    """RefDrivenRank's planner state without a GPU: the work ring in host
    memory, launches recorded instead of made."""

    def __init__(self, nch=2, depth=16):
        import ctypes
        import types

        from mccs_amd import _lib, abi

        real = _lib.load()
        self.launched = []
        self.lib = types.SimpleNamespace(
            mccs_task_schema=real.mccs_task_schema,
            mccs_hip_launch_coll=lambda *a: self.launched.append(a) or 0)
        self.nch, self.n, self.work_depth = nch, 2, depth
        self.rings = refdrive.reference_rings(2, nch)
        self._work_mem = ctypes.create_string_buffer(abi.MCCS_WORK_SIZE * depth)
        self._done_mem = (ctypes.c_uint32 * abi.MCCS_MAX_NCHANNELS)()
        self.h_work = self.d_work = ctypes.addressof(self._work_mem)
        self.h_done = ctypes.addressof(self._done_mem)
        self.d_comm = 0
        self.ring = refdrive.WorkRing(nch, depth)
        self.launches, self._works = 0, {}

    def work_at(self, slot):
        from mccs_amd import abi

        return self._work_mem.raw[slot * abi.MCCS_WORK_SIZE:(slot + 1) * abi.MCCS_WORK_SIZE]


def test_all_reduce_uploads_the_scalar_of_this_call_not_of_an_earlier_one():
    """Same buffers, count and schema, call after call: the works cache is
    keyed by dtype, op and op_arg too, so each upload carries its own scalar."""
    rr = _HostOnlyRank()
    calls = [(2, 0, 0), (2, 4, 3), (2, 2, 0), (2, 5, 7), (2, 4, 0xFFFFFFFF), (2, 0, 0), (3, 4, 3), (2, 4, 3)]
    for i, (dtype, op, arg) in enumerate(calls):
        if arg:
            rr.all_reduce(0x7000, 0x9000, 2503, dtype, op, 0, op_arg=arg)
        else:
            rr.all_reduce(0x7000, 0x9000, 2503, dtype, op, 0)
        assert rr.launched[-1][:3] == (refdrive.FUNC_ALLREDUCE, dtype, op) and rr.launched[-1][6:8] == (1, 160)
        w = rr.work_at(i % 16)
        assert _arg_at(w, 0) == arg, (i, hex(_arg_at(w, 0)))
        assert w == _raw_work(i + 1, True, [(5, 0x7000, 0x9000, 2503, 0, 1, arg)])
        rr._write_done(0, i + 1)  # the kernel's acknowledgement
    keys = list(rr._works)
    assert len(keys) == len(set(calls)) == 6 and all(k[-3:] in set(calls) for k in keys)  # two calls came back


def test_plan_refuses_mixed_ops_and_accepts_mixed_scalars():
    rr = _HostOnlyRank()
    a, b = (0x7000, 0x9000, 1250, 7, 4, 0x3EAAAAAB), (0x17000, 0x19000, 1250, 7, 4, 0x40400000)
    with pytest.raises(ValueError, match="one dtype and op"):
        rr.plan([a, (0x17000, 0x19000, 1250, 7, 5, 2)], 0)
    with pytest.raises(ValueError, match="one dtype and op"):
        rr.plan([a, (0x17000, 0x19000, 1250, 2, 4, 3)], 0)
    assert not rr.launched
    p = rr.plan([a, b, (0x27000, 0x29000, 1250, 7, 4)], 0)  # the third task without op_arg
    assert rr.launched[-1][:3] == (refdrive.FUNC_ALLREDUCE, 7, 4) and len(rr.launched) == 1
    # least-loaded channel first: tasks 0 and 2 on channel 0, task 1 on channel 1
    assert [sel for _, _, sel in p.tasks] == [[0], [1], [0]] and p.nworks == [1, 1]
    assert [_arg_at(rr.work_at(0), i) for i in range(3)] == [0x3EAAAAAB, 0, 0]
    assert [_arg_at(rr.work_at(1), i) for i in range(2)] == [0x40400000, 0]
    assert rr.work_at(0) == _raw_work(2, True, [(3, 0x7000, 0x9000, 1250, 0, 1, 0x3EAAAAAB),
                                                (3, 0x27000, 0x29000, 1250, 0, 1, 0)])
