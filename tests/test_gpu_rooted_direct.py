"""GPU: the opt-in direct and LL Broadcast and Reduce (csrc/direct_rooted.h) on
the virtual node, bit for bit against their definitions.

Expected values come from tests/rooted_ref.py alone -- reduce_expected_planned
with the C oracle's element functor and, for the dtype x op sweep, again with
the independent rs_ref.ELEM_REF; broadcast_expected -- never from the library's
own ring; the first test then also holds the direct result to the same call on
a communicator that never opted in.  Every test asserts last_algo(): "oneshot"
for the count-based variant, "ll" for the LL one.  One-shot slots of 256 KiB
and LL slots for 128 KiB buffers, so the caps are 65536 and 32768 fp32
elements.
Edge values, guarded footprints and seeded configurations and sequences:
tests/test_gpu_rooted_direct_values.py, tests/test_gpu_footprint_direct.py,
tests/test_gpu_direct_collectives_fuzz.py.
"""
import numpy as np
import pytest

from mccs_amd import comm as C
import rooted_ref
import rs_ref
import vnode

pytestmark = pytest.mark.gpu
DIRECT_DEFAULTS = True  # CFG sets every threshold

I8, F16, F32, BF16 = 0, 6, 7, 9
SUM = 0
ONESHOT, LL_BYTES = 256 << 10, 128 << 10
CFG = dict(oneshot_bytes=ONESHOT, ll_bytes=LL_BYTES, direct_bytes=-1)
ESIZE = vnode.ESIZE
VARIANTS = ["oneshot", "ll"]
FUNCS = ["bc", "rd"]
SENTINEL = 0xA5


def _comms(n, func, variant, **kw):
    """n ranks on one GPU; `func` opted in to `variant` at its cap (None: never opted in)."""
    cfg = dict(CFG, timeout_ms=8000)
    cfg.update(kw)
    comms = C.init_all([0] * n, C.CommConfig(**cfg))
    cap, ll_cap = comms[0].rooted_direct_max()
    assert cap == (cfg["oneshot_bytes"] + 65535) // 65536 * 65536 and ll_cap == cfg["ll_bytes"]
    for c in comms:
        lim = dict(bytes=cap) if variant == "oneshot" else dict(ll_bytes=ll_cap) if variant == "ll" else {}
        c.set_rooted_direct(**{("bcast_" if func == "bc" else "reduce_") + k: v for k, v in lim.items()})
    return comms


def _reduce(comms, inputs, code, op, root, algo, inplace=False):
    """One grouped reduce; the root's numpy output.  Non-roots pass no recvbuff."""
    n = len(comms)
    cnt = inputs[0].size
    send = [vnode.to_dev(x) for x in inputs]
    recv = send[root] if inplace else vnode.to_dev(np.zeros(cnt, vnode.NPDT[code]))
    with C.group():
        for r in range(n):
            C.reduce(comms[r], send[r], recv if r == root else None, cnt, code, op, root)
    assert [c.last_algo() for c in comms] == [algo] * n
    for c in comms:
        c.sync()
    for r in range(n):
        if not (inplace and r == root):
            assert vnode.from_dev(send[r], code).tobytes() == inputs[r].tobytes(), ("send buffer written", r)
    return vnode.from_dev(recv, code).copy()


def _broadcast(comms, x, root, algo, inplace=False):
    """One grouped broadcast of the root's bytes x; every rank's numpy output.
    Non-roots pass no sendbuff."""
    n = len(comms)
    send = vnode.to_dev(x)
    recv = [send if inplace and r == root else vnode.to_dev(np.zeros(x.size, np.uint8)) for r in range(n)]
    with C.group():
        for r in range(n):
            C.broadcast(comms[r], send if r == root else None, recv[r], x.size, root)
    assert [c.last_algo() for c in comms] == [algo] * n
    for c in comms:
        c.sync()
    assert vnode.from_dev(send, I8).tobytes() == x.tobytes(), "send buffer written"
    return [vnode.from_dev(recv[r], 1).copy() for r in range(n)]


def _same(got, want, tag):
    bad = np.flatnonzero(np.ascontiguousarray(got).view(np.uint8) != np.ascontiguousarray(want).view(np.uint8))
    assert bad.size == 0, (tag, f"{bad.size} wrong bytes, first at byte {bad[0]} of {got.nbytes}")


_REDUCE_CASES = {}


def _reduce_case(orc, n, code, comm0):
    """Inputs of 30011 elements and, per root, the expected result: computed once, shared by both variants."""
    if (n, code) not in _REDUCE_CASES:
        rng = np.random.default_rng([n, code])
        xs = [vnode.gen(code, 30011, rng) for _ in range(n)]
        want = [rooted_ref.reduce_expected_planned(orc, xs, code, SUM, root, comm0) for root in range(n)]
        for w in want:
            w.setflags(write=False)
        _REDUCE_CASES[n, code] = (xs, want)
    return _REDUCE_CASES[n, code]


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("n", [2, 3, 4, 5, 8])
def test_reduce_every_root_matches_the_ring_order_and_a_ring_only_communicator(orc, n, variant):
    comms = _comms(n, "rd", variant)
    plain = _comms(n, "rd", None)  # never opted in
    try:
        for code in (F32, F16, BF16):
            xs, want = _reduce_case(orc, n, code, comms[0])
            for root in range(n):
                for inplace in (False, True):
                    _same(_reduce(comms, xs, code, SUM, root, variant, inplace), want[root],
                          (n, code, root, variant, inplace))
                _same(_reduce(plain, xs, code, SUM, root, "ring"), want[root], (n, code, root, "ring"))
            if code == F32 and n >= 4:
                # the control: a schedule-blind fold differs, so the order check above is live.  (From four
                # ranks on: vnode.gen's fp32 are multiples of 2^-23 below 1, so a sum of two is exact and a
                # sum of three rounds once, the same in any order.  The root is every ring's last operand,
                # so at n = 4 the root 3 folds the other three in some order and adds x[3] last: the
                # rank-order value by that same argument, and the one root the control leaves out.)
                blind = rooted_ref.rank_order(orc, xs, code, SUM)
                assert all(blind.tobytes() != want[root].tobytes() for root in range(n) if (n, root) != (4, 3))
    finally:
        vnode.destroy(comms)
        vnode.destroy(plain)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("n", [2, 3, 4, 5, 8])
def test_broadcast_every_root_and_a_ring_only_communicator(n, variant):
    comms = _comms(n, "bc", variant)
    plain = _comms(n, "bc", None)
    try:
        rng = np.random.default_rng(100 + n)
        for root in range(n):
            x = rng.integers(0, 256, 30011, dtype=np.uint8)
            want = rooted_ref.broadcast_expected([x if r == root else None for r in range(n)], root)
            for inplace in (False, True):
                for r, got in enumerate(_broadcast(comms, x, root, variant, inplace)):
                    _same(got, want, (n, root, r, variant, inplace))
            for r, got in enumerate(_broadcast(plain, x, root, "ring")):
                _same(got, want, (n, root, r, "ring"))
    finally:
        vnode.destroy(comms)
        vnode.destroy(plain)


@pytest.mark.parametrize("variant", VARIANTS)
def test_reduce_all_ten_dtypes_and_four_ops(orc, variant):
    n, cnt = 4, 4001
    comms = _comms(n, "rd", variant)
    try:
        rng = np.random.default_rng(7)
        for code in range(10):
            for op in range(4):
                root = (code + op) % n
                xs = [vnode.gen(code, cnt, rng) for _ in range(n)]
                got = _reduce(comms, xs, code, op, root, variant)
                _same(got, rooted_ref.reduce_expected_planned(orc, xs, code, op, root, comms[0]), (code, op, "oracle"))
                _same(got, rooted_ref.reduce_expected_planned(rs_ref.ELEM_REF, xs, code, op, root, comms[0]),
                      (code, op, "elem_ref"))
    finally:
        vnode.destroy(comms)


def _boundary(cap, ll_cap, variant, esize, extra=()):
    top = (cap if variant == "oneshot" else ll_cap) // esize
    return sorted({1, 7, 255, 1023, 1024, 1025, 4097, min(top, ll_cap // esize), top, *extra}), top


@pytest.mark.parametrize("variant", VARIANTS)
def test_reduce_boundary_counts(orc, variant):
    """1, 7, 255, 4097 elements, one granule +- 1 (the per-channel piece is
    rounded up to it: 512 reference threads x 8 bytes = 1024 fp32), the LL cap
    in elements and the cap of the variant in elements; one more: the ring."""
    n, code = 4, F32
    comms = _comms(n, "rd", variant)
    try:
        counts, top = _boundary(*comms[0].rooted_direct_max(), variant, ESIZE[code])
        rng = np.random.default_rng(11)
        for i, cnt in enumerate(counts):
            root = i % n
            xs = [vnode.gen(code, cnt, rng) for _ in range(n)]
            want = rooted_ref.reduce_expected_planned(orc, xs, code, SUM, root, comms[0])
            for inplace in (False, True):
                _same(_reduce(comms, xs, code, SUM, root, variant, inplace), want, (cnt, variant, inplace))
        xs = [vnode.gen(code, top + 1, rng) for _ in range(n)]
        _same(_reduce(comms, xs, code, SUM, 1, "ring"), rooted_ref.reduce_expected_planned(orc, xs, code, SUM, 1, comms[0]),
              "above")
    finally:
        vnode.destroy(comms)


@pytest.mark.parametrize("variant", VARIANTS)
def test_broadcast_boundary_sizes(variant):
    """The Reduce test's set in bytes, and 8k +- 1 bytes (a last word of 7 bytes, of 1 byte)."""
    n = 4
    comms = _comms(n, "bc", variant)
    try:
        sizes, top = _boundary(*comms[0].rooted_direct_max(), variant, 1, extra=(8191, 8192, 8193))
        rng = np.random.default_rng(12)
        for i, nbytes in enumerate(sizes + [top + 1]):
            root = i % n
            x = rng.integers(0, 256, nbytes, dtype=np.uint8)
            for inplace in (False, True):
                for r, got in enumerate(_broadcast(comms, x, root, variant if nbytes <= top else "ring", inplace)):
                    _same(got, rooted_ref.broadcast_expected({root: x}, root), (nbytes, r, variant, inplace))
    finally:
        vnode.destroy(comms)


@pytest.mark.parametrize("variant", VARIANTS)
def test_reduce_three_loops_and_a_partial_last_chunk(orc, variant):
    """A 64 KiB FIFO buffer: chunks of 8192 fp32, so the buffer takes three
    whole loops of all the channels the planner selects and 1235 elements of a
    fourth."""
    n, code, buff = 4, F32, 1 << 16
    comms = _comms(n, "rd", variant, buffer_size=buff, oneshot_bytes=1 << 20, ll_bytes=1 << 20)
    try:
        chunk = buff // 8 // 4 * 4
        nch = comms[0].nchannels
        cnt = 3 * nch * chunk + 1235
        sel, nthr, _ = vnode.Planner(nch, comms[0].rings()).select(cnt * 4, cnt * 4)
        assert sel == nch and cnt // (sel * chunk) == 3 and len(rs_ref.pieces(cnt, code, sel, nthr, buff)) > 3 * sel
        rng = np.random.default_rng(13)
        xs = [vnode.gen(code, cnt, rng) for _ in range(n)]
        for root in (0, 3):
            want = rooted_ref.reduce_expected_planned(orc, xs, code, SUM, root, comms[0], buff_size=buff)
            for inplace in (False, True):
                _same(_reduce(comms, xs, code, SUM, root, variant, inplace), want, (variant, root, inplace))
    finally:
        vnode.destroy(comms)


@pytest.mark.parametrize("variant", VARIANTS)
def test_fourteen_channels_doubled_and_reversed_rings_roots_at_both_ends(orc, variant):
    n = 8
    rings = C.default_rings(8, 0)
    rings = rings + [list(reversed(r)) for r in rings]
    ends = (rings[0][0], rings[0][-1])  # the first ring's two ends: the last ring's, swapped
    # a rooted call counts the buffer's bytes, not n blocks: all 14 channels take 14 x 32 KiB, above the
    # small configuration's caps, so this test has 1 MiB slots
    comms = _comms(n, "rd", variant, rings=rings, oneshot_bytes=1 << 20, ll_bytes=1 << 20)
    for c in comms:  # and the Broadcast of the same variant
        cap, ll_cap = c.rooted_direct_max()
        c.set_rooted_direct(**(dict(bcast_bytes=cap, reduce_bytes=cap) if variant == "oneshot"
                               else dict(bcast_ll_bytes=ll_cap, reduce_ll_bytes=ll_cap)))
    try:
        assert comms[0].nchannels == 14 and ends[0] != ends[1]
        rng = np.random.default_rng(17)
        for code, cnt, want_nch in ((F32, 14 * 8192 + 77, 14), (BF16, 4 * 16384 + 77, 4), (F16, 5, 1)):
            xs = [vnode.gen(code, cnt, rng) for _ in range(n)]
            nch, _, _ = vnode.Planner(14, rings).select(cnt * ESIZE[code], cnt * ESIZE[code])
            assert nch == want_nch
            for root in ends:
                want = rooted_ref.reduce_expected_planned(orc, xs, code, SUM, root, comms[0])
                for inplace in (False, True):
                    _same(_reduce(comms, xs, code, SUM, root, variant, inplace), want, (code, cnt, root, inplace))
        for root in ends:
            x = rng.integers(0, 256, 30011, dtype=np.uint8)
            for r, got in enumerate(_broadcast(comms, x, root, variant)):
                _same(got, x, (root, r))
    finally:
        vnode.destroy(comms)


def _frames(n, nbytes, band):
    import torch

    f = [torch.empty(band + 16 + nbytes + band, dtype=torch.uint8, device="cuda") for _ in range(n)]
    assert all(t.data_ptr() % 16 == 0 for t in f)
    return f


def _bands_intact(frame, lo, hi):
    return bool((frame[:lo] == SENTINEL).all()) and bool((frame[hi:] == SENTINEL).all())


def _reduce_misaligned(orc, variant, code, cnt, offsets):
    """Every (send, recv) byte misalignment of `offsets`, out of place, inside
    0xA5 bands, the root rotating: the root's bands intact and payload exact,
    send untouched on every rank; a non-root's recvbuff -- a sentinel-filled
    frame for even send offsets, NULL for odd ones -- untouched."""
    import torch

    n, es, band = 4, ESIZE[code], 32
    comms = _comms(n, "rd", variant)
    try:
        rng = np.random.default_rng(19)
        xs = [vnode.gen(code, cnt, rng) for _ in range(n)]
        want = [vnode.to_dev(rooted_ref.reduce_expected_planned(orc, xs, code, SUM, root, comms[0])) for root in range(n)]
        data = [vnode.to_dev(x) for x in xs]
        sframe, rframe = _frames(n, cnt * es, band), _frames(n, cnt * es, band)
        for a in offsets:
            keep = []
            for r in range(n):
                sframe[r].fill_(SENTINEL)
                sframe[r][band + a:band + a + cnt * es] = data[r]
                keep.append(sframe[r].clone())
            for b in offsets:
                root = (a + b) % n
                for r in range(n):
                    rframe[r].fill_(SENTINEL)
                with C.group():
                    for r in range(n):
                        recv = rframe[r].data_ptr() + band + b if r == root or a % 2 == 0 else None
                        C.reduce(comms[r], sframe[r].data_ptr() + band + a, recv, cnt, code, SUM, root)
                assert comms[0].last_algo() == variant
                for c in comms:
                    c.sync()
                lo, hi = band + b, band + b + cnt * es
                assert torch.equal(rframe[root][lo:hi], want[root]), (a, b, root, "payload")
                assert _bands_intact(rframe[root], lo, hi), (a, b, root, "a band was written")
                for r in range(n):
                    assert r == root or bool((rframe[r] == SENTINEL).all()), (a, b, r, "a non-root's recvbuff written")
                    assert torch.equal(sframe[r], keep[r]), (a, b, r, "send buffer written")
    finally:
        vnode.destroy(comms)


@pytest.mark.parametrize("variant", VARIANTS)
def test_reduce_int8_every_misalignment_of_send_and_recv(orc, variant):
    _reduce_misaligned(orc, variant, I8, 1021, range(16))


@pytest.mark.parametrize("variant", VARIANTS)
def test_reduce_fp16_every_even_misalignment_of_send_and_recv(orc, variant):
    _reduce_misaligned(orc, variant, F16, 1021, range(2, 16, 2))


@pytest.mark.parametrize("nbytes", [1021, 2042])  # the int8 and the fp16 payload of the Reduce tests
@pytest.mark.parametrize("variant", VARIANTS)
def test_broadcast_every_misalignment_of_send_and_recv(variant, nbytes):
    """Every (send, recv) byte misalignment, out of place, inside 0xA5 bands,
    the root rotating: every rank's bands intact and payload exact, the root's
    send untouched.  A non-root's sendbuff is NULL for odd send offsets, as the
    ring allows, and a sentinel-filled frame otherwise, which stays untouched
    (and unread: the payload is the root's)."""
    import torch

    n, band = 4, 32
    comms = _comms(n, "bc", variant)
    try:
        rng = np.random.default_rng(23)
        x = rng.integers(0, 256, nbytes, dtype=np.uint8)
        x[x == SENTINEL] = 0  # the payload never looks like a band
        data = vnode.to_dev(x)
        sframe, rframe = _frames(n, nbytes, band), _frames(n, nbytes, band)
        for a in range(16):
            for b in range(16):
                root = (a + b) % n
                for r in range(n):
                    sframe[r].fill_(SENTINEL)
                    rframe[r].fill_(SENTINEL)
                sframe[root][band + a:band + a + nbytes] = data
                keep = sframe[root].clone()
                with C.group():
                    for r in range(n):
                        send = sframe[r].data_ptr() + band + a if r == root or a % 2 == 0 else None
                        C.broadcast(comms[r], send, rframe[r].data_ptr() + band + b, nbytes, root)
                assert comms[0].last_algo() == variant
                for c in comms:
                    c.sync()
                lo, hi = band + b, band + b + nbytes
                for r in range(n):
                    assert torch.equal(rframe[r][lo:hi], data), (a, b, root, r, "payload")
                    assert _bands_intact(rframe[r], lo, hi), (a, b, root, r, "a band was written")
                    if r == root:
                        assert torch.equal(sframe[r], keep), (a, b, r, "send buffer written")
                    else:
                        assert bool((sframe[r] == SENTINEL).all()), (a, b, r, "a non-root's sendbuff written")
    finally:
        vnode.destroy(comms)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("func", FUNCS)
def test_one_workgroup_per_rank_sends_and_makes_the_count_only_hand_offs(orc, monkeypatch, func, variant):
    """MCCS_DIRECT_BLOCKS=1: the single workgroup of a rank moves the data,
    makes the hand-offs of the pairs without data and waits for every peer's,
    over consecutive launches with every root."""
    monkeypatch.setenv("MCCS_DIRECT_BLOCKS", "1")
    n, code = 4, F32
    comms = _comms(n, func, variant)
    try:
        rng = np.random.default_rng(29)
        for cnt in (30011, 5):
            for root in range(n):
                if func == "rd":
                    xs = [vnode.gen(code, cnt, rng) for _ in range(n)]
                    want = rooted_ref.reduce_expected_planned(orc, xs, code, SUM, root, comms[0])
                    for inplace in (False, True):
                        _same(_reduce(comms, xs, code, SUM, root, variant, inplace), want, (cnt, root, inplace))
                else:
                    x = rng.integers(0, 256, cnt, dtype=np.uint8)
                    for inplace in (False, True):
                        for r, got in enumerate(_broadcast(comms, x, root, variant, inplace)):
                            _same(got, x, (cnt, root, r, inplace))
    finally:
        vnode.destroy(comms)
