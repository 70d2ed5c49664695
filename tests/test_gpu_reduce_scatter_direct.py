"""GPU: the opt-in direct and LL ReduceScatter (csrc/direct_rs.h) on the virtual
node, bit for bit against the ring's definition.

Expected values come from tests/rs_ref.py alone -- expected_planned with the C
oracle's element functor and, for the dtype x op sweep, again with the
independent ELEM_REF -- never from the library's own ring; one test then also
holds the direct result to the same call on a communicator that never opted in.
Every test asserts last_algo(): "oneshot" for the count-based variant, "ll" for
the LL one.  One-shot slots of 256 KiB and LL slots for 128 KiB blocks, so the
caps are 65536 and 32768 fp32 elements.
Edge values, guarded footprints and seeded configurations and sequences:
tests/test_gpu_reduce_scatter_direct_values.py, tests/test_gpu_footprint_direct.py,
tests/test_gpu_direct_collectives_fuzz.py.
"""
import numpy as np
import pytest

from mccs_amd import comm as C
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
SENTINEL = 0xA5


def _comms(n, variant, **kw):
    cfg = dict(CFG, timeout_ms=8000)
    cfg.update(kw)
    comms = C.init_all([0] * n, C.CommConfig(**cfg))
    cap, ll_cap = comms[0].reduce_scatter_direct_max()
    assert cap == (cfg["oneshot_bytes"] + 65535) // 65536 * 65536 and ll_cap == cfg["ll_bytes"]
    for c in comms:
        if variant == "oneshot":
            c.set_reduce_scatter_direct(block_bytes=cap)
        elif variant == "ll":
            c.set_reduce_scatter_direct(ll_block_bytes=ll_cap)
    return comms


def _run(comms, inputs, code, op, variant, inplace=False):
    """One grouped reduce_scatter; per-rank numpy outputs and the device send buffers."""
    n = len(comms)
    cnt = inputs[0].size // n
    es = ESIZE[code]
    send = [vnode.to_dev(x) for x in inputs]
    recv = [send[r][r * cnt * es:(r + 1) * cnt * es] if inplace else vnode.to_dev(np.zeros(cnt, vnode.NPDT[code]))
            for r in range(n)]
    with C.group():
        for r in range(n):
            C.reduce_scatter(comms[r], send[r], recv[r], cnt, code, op)
    assert [c.last_algo() for c in comms] == [variant] * n
    for c in comms:
        c.sync()
    out = [vnode.from_dev(recv[r], code).copy() for r in range(n)]
    if not inplace:
        for r in range(n):
            assert vnode.from_dev(send[r], code).tobytes() == inputs[r].tobytes(), ("send buffer written", r)
    return out


def _same(got, want, tag):
    for r, (g, w) in enumerate(zip(got, want)):
        bad = np.flatnonzero(g.view(np.uint8) != np.ascontiguousarray(w).view(np.uint8))
        assert bad.size == 0, (tag, f"rank {r}: {bad.size} wrong bytes, first at byte {bad[0]} of {g.nbytes}")


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("n", [2, 3, 4, 5, 8])
def test_every_rank_count_matches_the_ring_order_and_a_ring_only_communicator(orc, n, variant):
    cnt = 30011
    comms = _comms(n, variant)
    plain = _comms(n, None)  # never opted in
    try:
        rng = np.random.default_rng(n)
        for code in (F32, F16, BF16):
            xs = [vnode.gen(code, n * cnt, rng) for _ in range(n)]
            want = rs_ref.expected_planned(orc, xs, code, SUM, comms[0])
            for inplace in (False, True):
                _same(_run(comms, xs, code, SUM, variant, inplace), want, (n, code, variant, inplace))
            _same(_run(plain, xs, code, SUM, "ring"), want, (n, code, "ring"))
            if code == F32 and n >= 4:
                # the control: a schedule-blind fold differs, so the order check above is live.  (From four
                # ranks on: vnode.gen's fp32 are multiples of 2^-23 below 1, so a sum of two is exact and a
                # sum of three rounds once, the same in any order.)
                blind = rs_ref.rank_order(orc, xs, code, SUM)
                assert any(b.tobytes() != w.tobytes() for b, w in zip(blind, want))
    finally:
        vnode.destroy(comms)
        vnode.destroy(plain)


@pytest.mark.parametrize("variant", VARIANTS)
def test_all_ten_dtypes_and_four_ops(orc, variant):
    n, cnt = 4, 4001
    comms = _comms(n, variant)
    try:
        rng = np.random.default_rng(7)
        for code in range(10):
            for op in range(4):
                xs = [vnode.gen(code, n * cnt, rng) for _ in range(n)]
                got = _run(comms, xs, code, op, variant)
                _same(got, rs_ref.expected_planned(orc, xs, code, op, comms[0]), (code, op, "oracle"))
                _same(got, rs_ref.expected_planned(rs_ref.ELEM_REF, xs, code, op, comms[0]), (code, op, "elem_ref"))
    finally:
        vnode.destroy(comms)


@pytest.mark.parametrize("variant", VARIANTS)
def test_boundary_counts(orc, variant):
    """1, 7, 255, 4097 elements, one granule +- 1 (the per-channel piece is
    rounded up to it: 512 reference threads x 8 bytes = 1024 fp32), the LL cap
    in elements and the cap of the variant in elements."""
    n, code = 4, F32
    comms = _comms(n, variant)
    try:
        cap, ll_cap = comms[0].reduce_scatter_direct_max()
        top = (cap if variant == "oneshot" else ll_cap) // ESIZE[code]
        rng = np.random.default_rng(11)
        for cnt in sorted({1, 7, 255, 4097, 1023, 1024, 1025, min(top, ll_cap // ESIZE[code]), top}):
            xs = [vnode.gen(code, n * cnt, rng) for _ in range(n)]
            want = rs_ref.expected_planned(orc, xs, code, SUM, comms[0])
            for inplace in (False, True):
                _same(_run(comms, xs, code, SUM, variant, inplace), want, (cnt, variant, inplace))
        # one element above the cap: the ring again
        xs = [vnode.gen(code, n * (top + 1), rng) for _ in range(n)]
        _same(_run(comms, xs, code, SUM, "ring"), rs_ref.expected_planned(orc, xs, code, SUM, comms[0]), "above")
    finally:
        vnode.destroy(comms)


@pytest.mark.parametrize("variant", VARIANTS)
def test_three_loops_and_a_partial_last_chunk(orc, variant):
    """A 64 KiB FIFO buffer: chunks of 8192 fp32, so the block takes three
    whole loops of all the channels the planner selects and 1235 elements of a
    fourth."""
    n, code, buff = 4, F32, 1 << 16
    comms = _comms(n, variant, buffer_size=buff, oneshot_bytes=1 << 20, ll_bytes=1 << 20)
    try:
        chunk = buff // 8 // 4 * 4
        nch = comms[0].nchannels
        cnt = 3 * nch * chunk + 1235
        sel, nthr, _ = vnode.Planner(nch, comms[0].rings()).select(n * cnt * 4, cnt * 4)
        assert sel == nch and cnt // (sel * chunk) == 3 and len(rs_ref.pieces(cnt, code, sel, nthr, buff)) > 3 * sel
        rng = np.random.default_rng(13)
        xs = [vnode.gen(code, n * cnt, rng) for _ in range(n)]
        want = rs_ref.expected_planned(orc, xs, code, SUM, comms[0], buff_size=buff)
        for inplace in (False, True):
            _same(_run(comms, xs, code, SUM, variant, inplace), want, (variant, inplace))
    finally:
        vnode.destroy(comms)


@pytest.mark.parametrize("variant", VARIANTS)
def test_fourteen_channels_doubled_and_reversed_rings(orc, variant):
    n = 8
    rings = C.default_rings(8, 0)
    rings = rings + [list(reversed(r)) for r in rings]
    comms = _comms(n, variant, rings=rings)
    try:
        assert comms[0].nchannels == 14
        rng = np.random.default_rng(17)
        for code, cnt in ((F32, 30011), (BF16, 14 * 2048 + 77), (F16, 5)):
            xs = [vnode.gen(code, n * cnt, rng) for _ in range(n)]
            nch, _, _ = vnode.Planner(14, rings).select(n * cnt * ESIZE[code], cnt * ESIZE[code])
            assert nch == 14 or cnt == 5
            want = rs_ref.expected_planned(orc, xs, code, SUM, comms[0])
            for inplace in (False, True):
                _same(_run(comms, xs, code, SUM, variant, inplace), want, (code, cnt, variant, inplace))
    finally:
        vnode.destroy(comms)


def _misaligned(orc, variant, code, cnt, offsets):
    """Every (send, recv) byte misalignment of `offsets`, out of place, inside
    0xA5 bands: bands intact, send untouched, payload exact."""
    import torch

    n, es = 4, ESIZE[code]
    comms = _comms(n, variant)
    try:
        rng = np.random.default_rng(19)
        xs = [vnode.gen(code, n * cnt, rng) for _ in range(n)]
        want = [vnode.to_dev(w) for w in rs_ref.expected_planned(orc, xs, code, SUM, comms[0])]
        data = [vnode.to_dev(x) for x in xs]
        band = 32
        sframe = [torch.empty(band + 16 + n * cnt * es + band, dtype=torch.uint8, device="cuda") for _ in range(n)]
        rframe = [torch.empty(band + 16 + cnt * es + band, dtype=torch.uint8, device="cuda") for _ in range(n)]
        assert all(t.data_ptr() % 16 == 0 for t in sframe + rframe)
        for a in offsets:
            keep = []
            for r in range(n):
                sframe[r].fill_(SENTINEL)
                sframe[r][band + a:band + a + n * cnt * es] = data[r]
                keep.append(sframe[r].clone())
            for b in offsets:
                for r in range(n):
                    rframe[r].fill_(SENTINEL)
                with C.group():
                    for r in range(n):
                        C.reduce_scatter(comms[r], sframe[r].data_ptr() + band + a, rframe[r].data_ptr() + band + b, cnt,
                                         code, SUM)
                assert comms[0].last_algo() == variant
                for c in comms:
                    c.sync()
                for r in range(n):
                    lo, hi = band + b, band + b + cnt * es
                    assert torch.equal(rframe[r][lo:hi], want[r]), (a, b, r, "payload")
                    assert bool((rframe[r][:lo] == SENTINEL).all()) and bool((rframe[r][hi:] == SENTINEL).all()), \
                        (a, b, r, "a band was written")
                    assert torch.equal(sframe[r], keep[r]), (a, b, r, "send buffer written")
    finally:
        vnode.destroy(comms)


@pytest.mark.parametrize("variant", VARIANTS)
def test_int8_every_misalignment_of_send_and_recv(orc, variant):
    _misaligned(orc, variant, I8, 1021, range(16))


@pytest.mark.parametrize("variant", VARIANTS)
def test_fp16_every_even_misalignment_of_send_and_recv(orc, variant):
    _misaligned(orc, variant, F16, 1021, range(2, 16, 2))
