"""GPU: ring Broadcast and Reduce on the one-GPU virtual node, bit for bit
against tests/rooted_ref.py (the definitions in include/mccs_hip.h restated
with numpy, tests/rs_ref.py and the oracle's element functor).

Every communicator gets a watchdog of a few seconds, so a schedule mistake
ends as mccsTimeout from sync() instead of a long wait.
"""
import numpy as np
import pytest

from mccs_amd import comm as C
import rooted_ref
import rs_ref
import vnode

pytestmark = pytest.mark.gpu

I32, F16, F32, BF16 = 2, 6, 7, 9
SUM, PROD, MAX, MIN = range(4)
TIMEOUT_MS = 8000
SENTINEL = 0xA5


def _cfg(**kw):
    return C.CommConfig(timeout_ms=TIMEOUT_MS, **kw)


def _roots(n):
    return list(range(n)) if n <= 4 else sorted({0, 3, n - 1})


def _sync(comms):
    for c in comms:
        c.sync()
    assert all(c.last_algo() == "ring" for c in comms)


def _broadcast(comms, data, root):
    """One grouped out-of-place Broadcast of `data` (uint8) from `root`;
    per-rank received bytes.  Ranks other than the root pass no sendbuff."""
    n = len(comms)
    send = vnode.to_dev(data)
    recv = [vnode.to_dev(np.zeros(data.size, np.uint8)) for _ in range(n)]
    with C.group():
        for r, c in enumerate(comms):
            C.broadcast(c, send if r == root else None, recv[r], data.size, root)
    _sync(comms)
    assert send.cpu().numpy().tobytes() == data.tobytes(), "the root's sendbuff was written"
    return [recv[r].cpu().numpy() for r in range(n)]


def _reduce(comms, inputs, code, op, root):
    """One grouped out-of-place Reduce to `root`; the root's numpy result.
    Ranks other than the root pass no recvbuff."""
    n = len(comms)
    cnt = inputs[0].size
    send = [vnode.to_dev(x) for x in inputs]
    recv = vnode.to_dev(np.zeros(cnt, vnode.NPDT[code]))
    with C.group():
        for r, c in enumerate(comms):
            C.reduce(c, send[r], recv if r == root else None, cnt, code, op, root)
    _sync(comms)
    for r in range(n):
        assert send[r].cpu().numpy().tobytes() == inputs[r].tobytes(), ("sendbuff written", r)
    return vnode.from_dev(recv, code)


def _same(got, exp, tag):
    if got.tobytes() != exp.tobytes():
        bad = np.flatnonzero(got.view(np.uint8) != exp.view(np.uint8))
        raise AssertionError(f"{tag}: {bad.size} bytes differ, first at byte {bad[0]}")


@pytest.mark.parametrize("n", [2, 3, 4, 5, 8])
def test_parity(orc, n):
    """Default buffer, one loop, ragged across the channels; every root at
    n <= 4, roots 0, 3 and n-1 above."""
    comms = C.init_all([0] * n, _cfg())
    try:
        cnt = 30011
        for root in _roots(n):
            for code in (F16, BF16, F32):
                rng = np.random.default_rng(1000 * n + 10 * root + code)
                inputs = [vnode.gen(code, cnt, rng) for _ in range(n)]
                exp = rooted_ref.reduce_expected_planned(orc, inputs, code, SUM, root, comms[0])
                _same(_reduce(comms, inputs, code, SUM, root), exp, ("reduce", n, root, code))
            data = np.random.default_rng(n + root).integers(0, 256, cnt * 2 + 1, dtype=np.uint8)
            for r, got in enumerate(_broadcast(comms, data, root)):
                _same(got, rooted_ref.broadcast_expected([data] * n, root), ("broadcast", n, root, r))
    finally:
        vnode.destroy(comms)


def test_single_rank_is_a_local_copy():
    comms = C.init_all([0], _cfg())
    try:
        x = vnode.gen(F32, 4099, np.random.default_rng(3))
        assert _reduce(comms, [x], F32, SUM, 0).tobytes() == x.tobytes()
        data = x.view(np.uint8)[:16393]
        assert _broadcast(comms, data, 0)[0].tobytes() == data.tobytes()
    finally:
        vnode.destroy(comms)


@pytest.mark.parametrize("n", [2, 4, 8])
def test_more_than_one_loop(orc, n):
    """A 64 KiB FIFO buffer makes a chunk 8192 int32 elements, so
    2 * channels * chunk + 999 elements take three loops.  With
    x_r[i] = (r + 1) * 1000003 + i the root must hold
    1000003 * n (n + 1) / 2 + n * i: the sum names every rank and the index, so
    a wrong offset or a dropped hop changes it.  The Broadcast of the same
    bytes (32-bit words naming root and index) takes 4x as many loops."""
    buff = 1 << 16
    comms = C.init_all([0] * n, _cfg(buffer_size=buff))
    try:
        chunk = buff // 2 // 4
        cnt = 2 * comms[0].nchannels * chunk + 999
        i = np.arange(cnt, dtype=np.int64)
        inputs = [((r + 1) * 1000003 + i).astype(np.int32) for r in range(n)]
        want = (1000003 * n * (n + 1) // 2 + n * i).astype(np.int32)
        for root in (0, n - 1):
            got = _reduce(comms, inputs, I32, SUM, root)
            assert got.tobytes() == want.tobytes(), (n, root, np.flatnonzero(got != want)[:4])
            exp = rooted_ref.reduce_expected_planned(orc, inputs, I32, SUM, root, comms[0], buff_size=buff)
            _same(got, exp, (n, root, "helper"))
            data = ((root + 1) * 16777259 + i).astype(np.int32).view(np.uint8)
            for r, b in enumerate(_broadcast(comms, data, root)):
                _same(b, data, ("broadcast", n, root, r))
    finally:
        vnode.destroy(comms)


def test_ops(orc):
    n, cnt = 4, 65537
    comms = C.init_all([0] * n, _cfg())
    try:
        for op in (PROD, MAX, MIN):
            for code in (F32, F16, I32):
                rng = np.random.default_rng(10 * op + code)
                inputs = [vnode.gen(code, cnt, rng) for _ in range(n)]
                root = (op + code) % n
                exp = rooted_ref.reduce_expected_planned(orc, inputs, code, op, root, comms[0])
                _same(_reduce(comms, inputs, code, op, root), exp, (op, code, root))
    finally:
        vnode.destroy(comms)


def test_tiny_counts(orc):
    """A few elements: one channel holds them all and, where the plan keeps
    more channels, the later ones run empty calls that still take and post
    their steps."""
    n = 4
    comms = C.init_all([0] * n, _cfg())
    try:
        for cnt in (1, 7, 63, 64, 65):
            root = cnt % n
            rng = np.random.default_rng(cnt)
            inputs = [vnode.gen(F16, cnt, rng) for _ in range(n)]
            exp = rooted_ref.reduce_expected_planned(orc, inputs, F16, SUM, root, comms[0])
            _same(_reduce(comms, inputs, F16, SUM, root), exp, ("reduce", cnt))
            data = rng.integers(0, 256, cnt, dtype=np.uint8)
            for r, b in enumerate(_broadcast(comms, data, root)):
                _same(b, data, ("broadcast", cnt, r))
    finally:
        vnode.destroy(comms)


def test_empty_trailing_channels(orc):
    """The ReduceScatter suite's case adapted.  A rooted call counts its own
    bytes, so the schema keeps a channel only while the buffer has 32 KiB for
    it; a piece is the buffer over the channels rounded up to a granule of
    4096 bytes, so the last channel goes empty only when
    (channels - 1) * 4096 >= 32768: ten channels here.  330000 bytes keep ten
    channels of 544 threads, pieces of 36864 bytes, nine of which cover the
    buffer: channel 9 runs empty calls that still take and post their steps."""
    n, code, nch_cfg = 4, F16, 10
    comms = C.init_all([0] * n, _cfg(channel_count=nch_cfg, rings=[list(range(n)), list(range(n))[::-1]] * 5))
    try:
        cnt = 165000
        nch, nthr = C.task_schema(cnt * 2, nch_cfg)
        assert (nch, nthr) == (10, 544)
        assert {bid for bid, _, _ in rs_ref.pieces(cnt, code, nch, nthr, 1 << 22)} == set(range(9))
        assert {bid for bid, _, _ in rs_ref.pieces(cnt * 2, 0, nch, nthr, 1 << 22)} == set(range(9))  # as bytes
        for root in (0, 2):
            rng = np.random.default_rng(8 + root)
            inputs = [vnode.gen(code, cnt, rng) for _ in range(n)]
            exp = rooted_ref.reduce_expected_planned(orc, inputs, code, SUM, root, comms[0])
            _same(_reduce(comms, inputs, code, SUM, root), exp, ("reduce", root))
            data = inputs[root].view(np.uint8)
            for r, b in enumerate(_broadcast(comms, data, root)):
                _same(b, data, ("broadcast", root, r))
    finally:
        vnode.destroy(comms)


@pytest.mark.parametrize("odd", [3, 0])
@pytest.mark.parametrize("inplace", [False, True])
def test_footprint(orc, inplace, odd):
    """Every written buffer at an odd element offset inside a sentinel-filled
    allocation (the typed loops), and at an aligned one (16-byte packs): the
    bands stay intact.  Out of place the root's sendbuff is unchanged byte for
    byte; a Reduce leaves every other rank's recvbuff (passed, though unused)
    untouched; a Broadcast never reads the other ranks' sendbuff (null)."""
    import torch

    n, code, cnt, es, root = 4, F16, 30011, 2, 2
    guard = 4096 + es * odd  # bytes before the buffer: `odd` elements past a 4 KiB band
    inner = cnt * es
    comms = C.init_all([0] * n, _cfg())
    try:
        rng = np.random.default_rng(5 + inplace)
        inputs = [vnode.gen(code, cnt, rng) for _ in range(n)]
        exp = rooted_ref.reduce_expected_planned(orc, inputs, code, SUM, root, comms[0])

        def banded():
            return [torch.full((guard + inner + 4096,), SENTINEL, dtype=torch.uint8, device="cuda") for _ in range(n)]

        def bands_intact(t):
            host = t.cpu().numpy()
            return bool(np.all(host[:guard] == SENTINEL) and np.all(host[guard + inner:] == SENTINEL))

        # Reduce: every rank passes a sentinel-filled recvbuff, only the root's may change
        alloc = banded()
        keep = [vnode.to_dev(x) for x in inputs]
        send = [t.data_ptr() for t in keep]
        recv = [t.data_ptr() + guard for t in alloc]
        if inplace:
            alloc[root][guard:guard + inner].copy_(keep[root])
            send[root] = recv[root]
        torch.cuda.synchronize()
        with C.group():
            for r, c in enumerate(comms):
                C.reduce(c, send[r], recv[r], cnt, code, SUM, root)
        _sync(comms)
        for r in range(n):
            host = alloc[r].cpu().numpy()
            if r == root:
                assert bands_intact(alloc[r]), ("reduce bands", r)
                assert host[guard:guard + inner].tobytes() == exp.tobytes(), "reduce result"
            else:
                assert np.all(host == SENTINEL), ("a non-root recvbuff was written", r)
            if r != root or not inplace:
                assert keep[r].cpu().numpy().tobytes() == inputs[r].tobytes(), ("sendbuff written", r)

        # Broadcast: every rank's recvbuff banded; the root's sendbuff kept out of place
        alloc = banded()
        data = inputs[root].view(np.uint8)
        src = vnode.to_dev(data)
        recv = [t.data_ptr() + guard for t in alloc]
        send = [None] * n
        send[root] = src.data_ptr()
        if inplace:
            alloc[root][guard:guard + inner].copy_(src)
            send[root] = recv[root]
        torch.cuda.synchronize()
        with C.group():
            for r, c in enumerate(comms):
                C.broadcast(c, send[r], recv[r], inner, root)
        _sync(comms)
        for r in range(n):
            assert bands_intact(alloc[r]), ("broadcast bands", r)
            assert alloc[r].cpu().numpy()[guard:guard + inner].tobytes() == data.tobytes(), ("broadcast", r)
        assert src.cpu().numpy().tobytes() == data.tobytes(), "the root's sendbuff was written"
    finally:
        vnode.destroy(comms)


def test_batched_roots_in_one_group(orc):
    """Three Broadcasts, then three Reduces, of every comm in one group with
    three different roots: one launch each, works of three elements, every
    element resolving its own role."""
    n = 4
    comms = C.init_all([0] * n, _cfg())
    try:
        rng = np.random.default_rng(21)
        roots, sizes = (1, 3, 0), (30011, 5000, 77)
        datas = [rng.integers(0, 256, s, dtype=np.uint8) for s in sizes]
        srcs = [vnode.to_dev(d) for d in datas]
        recv = [[vnode.to_dev(np.zeros(s, np.uint8)) for _ in range(n)] for s in sizes]
        with C.group():
            for k, root in enumerate(roots):
                for r, c in enumerate(comms):
                    C.broadcast(c, srcs[k] if r == root else None, recv[k][r], sizes[k], root)
        _sync(comms)
        for k in range(3):
            for r in range(n):
                _same(recv[k][r].cpu().numpy(), datas[k], ("broadcast", k, r))
        inputs = [[vnode.gen(F32, s, rng) for _ in range(n)] for s in sizes]
        planner = vnode.Planner(comms[0].nchannels, comms[0].rings())
        exp = [rooted_ref.reduce_expected_planned(orc, inputs[k], F32, SUM, roots[k], comms[0], planner=planner)
               for k in range(3)]
        send = [[vnode.to_dev(x) for x in inputs[k]] for k in range(3)]
        out = [vnode.to_dev(np.zeros(s, np.float32)) for s in sizes]
        with C.group():
            for k, root in enumerate(roots):
                for r, c in enumerate(comms):
                    C.reduce(c, send[k][r], out[k] if r == root else None, sizes[k], F32, SUM, root)
        _sync(comms)
        for k in range(3):
            _same(vnode.from_dev(out[k], F32), exp[k], ("reduce", k))
    finally:
        vnode.destroy(comms)
