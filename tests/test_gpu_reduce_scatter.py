"""GPU: ring ReduceScatter on the one-GPU virtual node, bit for bit against
tests/rs_ref.py (the definition in include/mccs_hip.h restated with numpy and
the oracle's element functor).

Every communicator gets a watchdog of a few seconds, so a schedule mistake
ends as mccsTimeout from sync() instead of a long wait.
"""
import numpy as np
import pytest

from mccs_amd import comm as C
import rs_ref
import vnode

pytestmark = pytest.mark.gpu

I32, F16, F32, BF16 = 2, 6, 7, 9
SUM, PROD, MAX, MIN = range(4)
TIMEOUT_MS = 8000
SENTINEL = 0xA5


def _cfg(**kw):
    return C.CommConfig(timeout_ms=TIMEOUT_MS, **kw)


def _reduce_scatter(comms, send, recv, cnt, code, op):
    with C.group():
        for r, c in enumerate(comms):
            C.reduce_scatter(c, send[r], recv[r], cnt, code, op)
    for c in comms:
        c.sync()


def _run(comms, inputs, code, op):
    """One grouped out-of-place ReduceScatter; per-rank numpy results."""
    n = len(comms)
    cnt = inputs[0].size // n
    send = [vnode.to_dev(x) for x in inputs]
    recv = [vnode.to_dev(np.zeros(cnt, vnode.NPDT[code])) for _ in range(n)]
    _reduce_scatter(comms, send, recv, cnt, code, op)
    assert all(c.last_algo() == "ring" for c in comms)
    return [vnode.from_dev(recv[r], code) for r in range(n)]


def _check(got, exp, tag):
    for r, (g, e) in enumerate(zip(got, exp)):
        if g.tobytes() != e.tobytes():
            bad = np.flatnonzero(g.view(np.uint8) != e.view(np.uint8))
            raise AssertionError(f"{tag} rank {r}: {bad.size} bytes differ, first at byte {bad[0]}")


@pytest.mark.parametrize("n", [2, 3, 4, 5, 8])
def test_parity(orc, n):
    """Default buffer, one loop, ragged across the channels."""
    comms = C.init_all([0] * n, _cfg())
    try:
        cnt = 30011
        for code in (F16, BF16, F32):
            rng = np.random.default_rng(1000 * n + code)
            inputs = [vnode.gen(code, n * cnt, rng) for _ in range(n)]
            exp = rs_ref.expected_planned(orc, inputs, code, SUM, comms[0])
            _check(_run(comms, inputs, code, SUM), exp, (n, code))
    finally:
        vnode.destroy(comms)


def test_single_rank_is_a_local_copy():
    comms = C.init_all([0], _cfg())
    try:
        x = vnode.gen(F32, 4099, np.random.default_rng(3))
        got = _run(comms, [x], F32, SUM)
        assert got[0].tobytes() == x.tobytes()
    finally:
        vnode.destroy(comms)


@pytest.mark.parametrize("n", [2, 4, 8])
def test_more_than_one_loop(orc, n):
    """A 64 KiB FIFO buffer makes a chunk 8192 int32 elements, so
    2 * channels * chunk + 999 elements per block take three loops.  With
    x_r[D * cnt + i] = (r + 1) * (D + 1) + i % 7, rank D must hold
    (D + 1) * n (n + 1) / 2 + n * (i % 7): a wrong block, a wrong offset or a
    dropped hop changes the value."""
    buff = 1 << 16
    comms = C.init_all([0] * n, _cfg(buffer_size=buff))
    try:
        chunk = buff // 2 // 4
        cnt = 2 * comms[0].nchannels * chunk + 999
        i = np.arange(cnt, dtype=np.int64)
        inputs = [np.concatenate([(r + 1) * (d + 1) + i % 7 for d in range(n)]).astype(np.int32) for r in range(n)]
        got = _run(comms, inputs, I32, SUM)
        for d in range(n):
            want = ((d + 1) * n * (n + 1) // 2 + n * (i % 7)).astype(np.int32)
            assert got[d].tobytes() == want.tobytes(), (n, d, np.flatnonzero(got[d] != want)[:4])
        exp = rs_ref.expected_planned(orc, inputs, I32, SUM, comms[0], buff_size=buff)
        _check(got, exp, (n, "helper"))
    finally:
        vnode.destroy(comms)


def test_ops(orc):
    n, cnt = 4, 65537
    comms = C.init_all([0] * n, _cfg())
    try:
        for op in (PROD, MAX, MIN):
            for code in (F32, F16, I32):
                rng = np.random.default_rng(10 * op + code)
                inputs = [vnode.gen(code, n * cnt, rng) for _ in range(n)]
                exp = rs_ref.expected_planned(orc, inputs, code, op, comms[0])
                _check(_run(comms, inputs, code, op), exp, (op, code))
    finally:
        vnode.destroy(comms)


def test_tiny_counts(orc):
    """A few elements per block: one channel holds them all and, where the
    plan keeps more channels, the later ones run empty calls that still take
    and post their steps."""
    n = 4
    comms = C.init_all([0] * n, _cfg())
    try:
        for cnt in (1, 7, 63, 64, 65):
            rng = np.random.default_rng(cnt)
            inputs = [vnode.gen(F16, n * cnt, rng) for _ in range(n)]
            exp = rs_ref.expected_planned(orc, inputs, F16, SUM, comms[0])
            _check(_run(comms, inputs, F16, SUM), exp, cnt)
    finally:
        vnode.destroy(comms)


def test_empty_trailing_channels(orc):
    """Four channels kept by the schema (block_bytes * n >= 4 * 32 KiB) but a
    block shorter than three granules of 4096 bytes: the per-channel piece is
    rounded up to a granule, so the last channels get nothing."""
    n, code = 8, F16
    comms = C.init_all([0] * n, _cfg(channel_count=4, rings=[list(range(n)), list(range(n))[::-1]] * 2))
    try:
        cnt = 8200  # 16400 B per block: 131 KiB enter the ring -> 4 channels of 544 threads; pieces of 4096 B
        nch, nthr = C.task_schema(cnt * 2 * n, 4)
        assert (nch, nthr) == (4, 544)
        assert {bid for bid, _, _ in rs_ref.pieces(cnt, code, nch, nthr, 1 << 22)} == {0, 1, 2}
        rng = np.random.default_rng(8)
        inputs = [vnode.gen(code, n * cnt, rng) for _ in range(n)]
        exp = rs_ref.expected_planned(orc, inputs, code, SUM, comms[0])
        _check(_run(comms, inputs, code, SUM), exp, "empty channels")
    finally:
        vnode.destroy(comms)


def test_batched_in_one_group(orc):
    """Two ReduceScatters of every comm in one group: one launch, works of two
    elements, the second call planned on the channels the first left lighter."""
    n = 4
    comms = C.init_all([0] * n, _cfg())
    try:
        rng = np.random.default_rng(21)
        counts = (30011, 5000)
        inputs = [[vnode.gen(F32, n * cnt, rng) for _ in range(n)] for cnt in counts]
        planner = vnode.Planner(comms[0].nchannels, comms[0].rings())
        exp = [rs_ref.expected_planned(orc, inputs[k], F32, SUM, comms[0], planner=planner) for k in range(2)]
        send = [[vnode.to_dev(x) for x in inputs[k]] for k in range(2)]
        recv = [[vnode.to_dev(np.zeros(cnt, np.float32)) for _ in range(n)] for cnt in counts]
        with C.group():
            for k in range(2):
                for r, c in enumerate(comms):
                    C.reduce_scatter(c, send[k][r], recv[k][r], counts[k], F32, SUM)
        for c in comms:
            c.sync()
        for k in range(2):
            _check([vnode.from_dev(recv[k][r], F32) for r in range(n)], exp[k], ("batched", k))
    finally:
        vnode.destroy(comms)


@pytest.mark.parametrize("odd", [3, 0])
@pytest.mark.parametrize("inplace", [False, True])
def test_footprint(orc, inplace, odd):
    """recvbuff at an odd element offset inside a sentinel-filled allocation
    (the typed loops), and at an aligned one (16-byte packs): the bands stay
    intact; out of place sendbuff is unchanged byte for byte; in place only
    the rank's own block changes."""
    import torch

    n, code, cnt, es = 4, F16, 30011, 2
    guard = 4096 + es * odd  # bytes before the buffer: `odd` elements past a 4 KiB band
    comms = C.init_all([0] * n, _cfg())
    try:
        rng = np.random.default_rng(5 + inplace)
        inputs = [vnode.gen(code, n * cnt, rng) for _ in range(n)]
        exp = rs_ref.expected_planned(orc, inputs, code, SUM, comms[0])
        inner = (n * cnt if inplace else cnt) * es
        alloc = [torch.full((guard + inner + 4096,), SENTINEL, dtype=torch.uint8, device="cuda") for _ in range(n)]
        if inplace:
            for r in range(n):
                alloc[r][guard:guard + inner].copy_(vnode.to_dev(inputs[r]))
            send = [alloc[r].data_ptr() + guard for r in range(n)]
            recv = [send[r] + r * cnt * es for r in range(n)]
            keep = None
        else:
            keep = [vnode.to_dev(x) for x in inputs]
            send = [t.data_ptr() for t in keep]
            recv = [alloc[r].data_ptr() + guard for r in range(n)]
        torch.cuda.synchronize()
        _reduce_scatter(comms, send, recv, cnt, code, SUM)
        for r in range(n):
            host = alloc[r].cpu().numpy()
            assert np.all(host[:guard] == SENTINEL) and np.all(host[guard + inner:] == SENTINEL), ("bands", r)
            body = host[guard:guard + inner]
            if inplace:
                want = inputs[r].copy()
                want[r * cnt:(r + 1) * cnt] = exp[r]
                assert body.tobytes() == want.tobytes(), ("in place", r)
            else:
                assert body.tobytes() == exp[r].tobytes(), ("out of place", r)
                assert keep[r].cpu().numpy().tobytes() == inputs[r].tobytes(), ("sendbuff written", r)
    finally:
        vnode.destroy(comms)


@pytest.mark.parametrize("n", [4, 8])
@pytest.mark.parametrize("code", [F16, F32])
def test_reduce_scatter_then_allgather_equals_allreduce(n, code):
    """The FSDP step on exact inputs (k/64, |k| <= 255: every partial sum is
    exact in fp16, so any order gives the same bits): ReduceScatter, in-place
    AllGather of the shards, and AllReduce of the same inputs, in three groups
    on the same communicators.  Also carries the FIFO step counters from one
    collective to the next."""
    cnt, es = 20011, vnode.ESIZE[code]
    comms = C.init_all([0] * n, _cfg())
    try:
        rng = np.random.default_rng(n + code)
        inputs = [vnode.gen(code, n * cnt, rng, "exact") for _ in range(n)]
        want = np.sum([x.astype(np.float64) for x in inputs], axis=0).astype(vnode.NPDT[code])
        send = [vnode.to_dev(x) for x in inputs]
        full = [vnode.to_dev(np.zeros(n * cnt, vnode.NPDT[code])) for _ in range(n)]
        red = [vnode.to_dev(np.zeros(n * cnt, vnode.NPDT[code])) for _ in range(n)]
        shard = [full[r].data_ptr() + r * cnt * es for r in range(n)]
        _reduce_scatter(comms, send, shard, cnt, code, SUM)
        for r in range(n):
            got = vnode.from_dev(full[r], code)[r * cnt:(r + 1) * cnt]
            assert got.tobytes() == want[r * cnt:(r + 1) * cnt].tobytes(), ("shard", r)
        with C.group():
            for r, c in enumerate(comms):
                C.all_gather(c, shard[r], full[r], cnt * es)
        for c in comms:
            c.sync()
        with C.group():
            for r, c in enumerate(comms):
                C.all_reduce(c, send[r], red[r], n * cnt, code, SUM)
        for c in comms:
            c.sync()
        for r in range(n):
            assert vnode.from_dev(full[r], code).tobytes() == want.tobytes(), ("gathered", r)
            assert vnode.from_dev(red[r], code).tobytes() == want.tobytes(), ("allreduce", r)
    finally:
        vnode.destroy(comms)


def test_captured_in_hip_graph(orc):
    """One grouped ReduceScatter captured with torch.cuda.graph and replayed
    twice with new inputs: the replays run the captured work list and pick up
    the FIFO steps where the previous launch left them."""
    import torch

    n, cnt = 2, 77777
    comms = C.init_all([0] * n, _cfg())
    try:
        rng = np.random.default_rng(9)
        send = [torch.zeros(n * cnt, dtype=torch.float16, device="cuda") for _ in range(n)]
        recv = [torch.zeros(cnt, dtype=torch.float16, device="cuda") for _ in range(n)]
        s = torch.cuda.Stream()
        with C.group():  # warm-up outside capture (the first launch loads the code object)
            for r in range(n):
                C.reduce_scatter(comms[r], send[r], recv[r], cnt, F16, SUM, stream=s)
        s.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            with C.group():
                for r in range(n):
                    C.reduce_scatter(comms[r], send[r], recv[r], cnt, F16, SUM, stream=s)
        for it in range(2):
            inputs = [vnode.gen(F16, n * cnt, rng) for _ in range(n)]
            for r in range(n):
                send[r].copy_(torch.from_numpy(inputs[r]).cuda())
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            for c in comms:
                c.sync()
            exp = rs_ref.expected_planned(orc, inputs, F16, SUM, comms[0])
            _check([recv[r].cpu().numpy() for r in range(n)], exp, ("replay", it))
    finally:
        torch.cuda.synchronize()
        vnode.destroy(comms)
