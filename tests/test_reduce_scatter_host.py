"""CPU: the ring ReduceScatter schedule on host threads
(mccs_host_ring_reduce_scatter), bit for bit against tests/rs_ref.py.

The host ring runs the walk of the gfx950 kernels (ring_kernel.h) through the
same FIFO protocol, so these cases check the schedule itself without a GPU:
block addressing, the per-channel split with empty trailing channels, ragged
tails, more than one loop, in place and out of place, and the footprint.
buff_size = 16384 makes a chunk 8192 bytes (2048 fp32 elements), so a
two-channel loop is 4096 fp32 elements and a few thousand elements already
take several loops.
"""
import numpy as np
import pytest

from mccs_amd import comm as C
import rs_ref
import vnode

I8, U8, I32, U32, I64, U64, F16, F32, F64, BF16 = range(10)
SUM, PROD, MAX, MIN = range(4)
BUFF = 16384
NTHR = 96
GUARD = 64  # elements of sentinel on each side
SENTINEL = 0xA5


def _rings(n, nch):
    ident = list(range(n))
    return [ident, ident[::-1]][:nch]


def _counts(code, nch):
    es = vnode.ESIZE[code]
    gran = (NTHR - 32) * 8 // es
    loop = nch * (BUFF // 2 // es)
    return [1, 7, gran - 1, gran, gran + 1, 2 * loop + 999]


def _banded(npdt, count):
    """(whole array of sentinel bytes, view of `count` elements inside it)."""
    whole = np.full((count + 2 * GUARD) * np.dtype(npdt).itemsize, SENTINEL, np.uint8)
    return whole, whole.view(npdt)[GUARD:GUARD + count]


def _bands_intact(whole, npdt, count):
    es = np.dtype(npdt).itemsize
    return bool(np.all(whole[:GUARD * es] == SENTINEL) and np.all(whole[(GUARD + count) * es:] == SENTINEL))


def _run_case(orc, n, code, op, nch, cnt, inplace, rng):
    npdt = vnode.NPDT[code]
    rings = _rings(n, nch)
    inputs = [vnode.gen(code, n * cnt, rng) for _ in range(n)]
    exp = rs_ref.expected(orc, inputs, code, op, nch, NTHR, rings, BUFF)
    if inplace:
        wholes, sends = zip(*[_banded(npdt, n * cnt) for _ in range(n)])
        for r in range(n):
            sends[r][:] = inputs[r]
        recvs = [sends[r][r * cnt:(r + 1) * cnt] for r in range(n)]
    else:
        sends = [x.copy() for x in inputs]
        wholes, recvs = zip(*[_banded(npdt, cnt) for _ in range(n)])
    C.host_ring_reduce_scatter(list(sends), list(recvs), cnt, code, op, channels=nch, nthreads=NTHR, buffer_size=BUFF,
                               rings=rings)
    tag = (n, code, op, nch, cnt, inplace)
    for r in range(n):
        assert recvs[r].tobytes() == exp[r].tobytes(), (tag, r)
        if inplace:
            assert _bands_intact(wholes[r], npdt, n * cnt), (tag, r)
            keep = np.ones(n * cnt, bool)
            keep[r * cnt:(r + 1) * cnt] = False  # only the rank's own block may change
            assert sends[r].view(np.uint8).reshape(-1, vnode.ESIZE[code])[keep].tobytes() == \
                inputs[r].view(np.uint8).reshape(-1, vnode.ESIZE[code])[keep].tobytes(), (tag, r)
        else:
            assert _bands_intact(wholes[r], npdt, cnt), (tag, r)
            assert sends[r].tobytes() == inputs[r].tobytes(), (tag, r)


@pytest.mark.parametrize("code", [F16, BF16, F32, I32, U8, F64])
@pytest.mark.parametrize("n", [1, 2, 3, 4, 8])
def test_host_ring_reduce_scatter_matches_the_definition(orc, n, code):
    rng = np.random.default_rng(100 * n + code)
    for nch in (1, 2):
        for cnt in _counts(code, nch):
            for inplace in (False, True):
                _run_case(orc, n, code, SUM, nch, cnt, inplace, rng)


@pytest.mark.parametrize("code", [F16, BF16, F32, I32, U8, F64])
@pytest.mark.parametrize("op", [PROD, MAX, MIN])
def test_host_ring_reduce_scatter_ops(orc, op, code):
    rng = np.random.default_rng(1000 + 10 * op + code)
    for nch in (1, 2):
        for cnt in _counts(code, nch):
            for inplace in (False, True):
                _run_case(orc, 4, code, op, nch, cnt, inplace, rng)


def test_host_ring_reduce_scatter_other_thread_granule(orc):
    """nthreads_ref = 544 (the schema's value for large calls): a granule of
    4096 bytes, half a chunk here, so the per-channel split rounds differently."""
    rng = np.random.default_rng(77)
    n, code, nch = 4, F32, 2
    rings = _rings(n, nch)
    for cnt in (1023, 1024, 1025, 2 * 4096 + 999):
        inputs = [vnode.gen(code, n * cnt, rng) for _ in range(n)]
        exp = rs_ref.expected(orc, inputs, code, SUM, nch, 544, rings, BUFF)
        recvs = [np.zeros(cnt, np.float32) for _ in range(n)]
        C.host_ring_reduce_scatter(inputs, recvs, cnt, code, SUM, channels=nch, nthreads=544, buffer_size=BUFF,
                                   rings=rings)
        for r in range(n):
            assert recvs[r].tobytes() == exp[r].tobytes(), (cnt, r)


@pytest.mark.parametrize("n", [3, 4, 8])
def test_expected_values_depend_on_the_ring_order(orc, n):
    """The comparison above can tell the summation order: in fp16, over the
    blocks other than n-1 (which the identity ring folds in rank order), the
    ring-order result differs from a plain rank-order fold in at least 10 %
    of the elements (numpy: 33 % at n = 3, 42-44 % at n = 4, 57-61 % at
    n = 8), and the host ring produces the ring-order one."""
    rng = np.random.default_rng(n)
    cnt = 2 * (BUFF // 2 // 2) + 999
    inputs = [vnode.gen(F16, n * cnt, rng) for _ in range(n)]
    rings = _rings(n, 1)
    exp = rs_ref.expected(orc, inputs, F16, SUM, 1, NTHR, rings, BUFF)
    plain = rs_ref.rank_order(orc, inputs, F16, SUM)
    assert exp[n - 1].tobytes() == plain[n - 1].tobytes()
    differ = sum(int(np.count_nonzero(exp[d].view(np.uint16) != plain[d].view(np.uint16))) for d in range(n - 1))
    frac = differ / ((n - 1) * cnt)
    print(f"n={n}: ring order differs from rank order in {frac:.1%} of the elements")
    assert frac >= 0.10, frac
    recvs = [np.zeros(cnt, np.float16) for _ in range(n)]
    C.host_ring_reduce_scatter(inputs, recvs, cnt, F16, SUM, channels=1, nthreads=NTHR, buffer_size=BUFF, rings=rings)
    for r in range(n):
        assert recvs[r].tobytes() == exp[r].tobytes(), r


def test_host_ring_reduce_scatter_refuses_bad_arguments():
    from mccs_amd._lib import MccsError

    x = [np.zeros(8, np.float32) for _ in range(2)]
    y = [np.zeros(4, np.float32) for _ in range(2)]
    for kw in (dict(data_type=10), dict(op_type=4), dict(channels=0), dict(nthreads=32), dict(buffer_size=1000)):
        args = dict(data_type=F32, op_type=SUM, channels=1, nthreads=96, buffer_size=BUFF)
        args.update(kw)
        with pytest.raises(MccsError) as ei:
            C.host_ring_reduce_scatter(x, y, 4, args["data_type"], args["op_type"], channels=args["channels"],
                                       nthreads=args["nthreads"], buffer_size=args["buffer_size"])
        assert ei.value.code == 4, kw
