"""CPU: the ring Broadcast and Reduce schedules on host threads
(mccs_host_ring_broadcast / mccs_host_ring_reduce), bit for bit against
tests/rooted_ref.py.

The host ring runs the walk of the gfx950 kernels (ring_kernel.h) through the
same FIFO protocol, so these cases check the rooted schedules without a GPU:
the role of every rank on the chain for every root, the per-channel split with
empty trailing channels, ragged tails, more than one loop, in place and out of
place, the footprint, and the buffers a role must leave alone.
buff_size = 16384 makes a chunk 8192 bytes, so a two-channel loop is 16 KiB and
a few thousand elements already take several loops.
"""
import numpy as np
import pytest

from mccs_amd import comm as C
import rooted_ref
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


def _roots(n):
    return list(range(n)) if n <= 4 else [0, n // 2, n - 1]


def _counts(code, nch):
    es = vnode.ESIZE[code]
    gran = (NTHR - 32) * 8 // es
    loop = nch * (BUFF // 2 // es)
    return [1, 7, gran - 1, gran, gran + 1, 2 * loop + 999]


def _banded(npdt, count):
    """(whole array of sentinel bytes, view of `count` elements inside it)."""
    whole = np.full((count + 2 * GUARD) * np.dtype(npdt).itemsize, SENTINEL, np.uint8)
    return whole, whole.view(npdt)[GUARD:GUARD + count]


def _untouched(whole):
    return bool(np.all(whole == SENTINEL))


def _bands_intact(whole, npdt, count):
    es = np.dtype(npdt).itemsize
    return bool(np.all(whole[:GUARD * es] == SENTINEL) and np.all(whole[(GUARD + count) * es:] == SENTINEL))


def _broadcast_case(n, root, nch, nbytes, inplace, rng):
    rings = _rings(n, nch)
    data = rng.integers(0, 256, nbytes).astype(np.uint8)
    wholes, recvs = zip(*[_banded(np.uint8, nbytes) for _ in range(n)])
    sends = [None] * n  # never dereferenced off the root
    if inplace:
        recvs[root][:] = data
        sends[root] = recvs[root]
    else:
        sends[root] = data.copy()
    C.host_ring_broadcast(sends, list(recvs), nbytes, root, channels=nch, nthreads=NTHR, buffer_size=BUFF, rings=rings)
    tag = ("broadcast", n, root, nch, nbytes, inplace)
    for r in range(n):
        assert recvs[r].tobytes() == data.tobytes(), (tag, r)
        assert _bands_intact(wholes[r], np.uint8, nbytes), (tag, r)
    if not inplace:
        assert sends[root].tobytes() == data.tobytes(), (tag, "the root's sendbuff was written")


def _reduce_case(orc, n, root, code, op, nch, cnt, inplace, rng):
    npdt = vnode.NPDT[code]
    rings = _rings(n, nch)
    inputs = [vnode.gen(code, cnt, rng) for _ in range(n)]
    exp = rooted_ref.reduce_expected(orc, inputs, code, op, root, nch, NTHR, rings, BUFF)
    sends = [x.copy() for x in inputs]
    # every rank passes a sentinel-filled recvbuff; only the root's may change
    wholes, recvs = (list(t) for t in zip(*[_banded(npdt, cnt) for _ in range(n)]))
    if inplace:
        recvs[root][:] = inputs[root]
        sends[root] = recvs[root]
    C.host_ring_reduce(sends, recvs, cnt, code, op, root, channels=nch, nthreads=NTHR, buffer_size=BUFF, rings=rings)
    tag = ("reduce", n, root, code, op, nch, cnt, inplace)
    assert recvs[root].tobytes() == exp.tobytes(), tag
    assert _bands_intact(wholes[root], npdt, cnt), tag
    for r in range(n):
        if r != root:
            assert _untouched(wholes[r]), (tag, r, "a non-root recvbuff was written")
        if r != root or not inplace:
            assert sends[r].tobytes() == inputs[r].tobytes(), (tag, r, "sendbuff was written")


@pytest.mark.parametrize("n", [2, 3, 4, 8])
def test_host_ring_broadcast_matches_the_definition(n):
    rng = np.random.default_rng(n)
    for root in _roots(n):
        for nch in (1, 2):
            for nbytes in _counts(I8, nch):
                for inplace in (False, True):
                    _broadcast_case(n, root, nch, nbytes, inplace, rng)


@pytest.mark.parametrize("op", [SUM, PROD, MAX, MIN])
@pytest.mark.parametrize("code", [I32, F16, F32, BF16])
@pytest.mark.parametrize("n", [2, 3, 4, 8])
def test_host_ring_reduce_matches_the_definition(orc, n, code, op):
    rng = np.random.default_rng(1000 * n + 10 * code + op)
    for root in _roots(n):
        for nch in (1, 2):
            for cnt in _counts(code, nch):
                for inplace in (False, True):
                    _reduce_case(orc, n, root, code, op, nch, cnt, inplace, rng)


def test_host_ring_reduce_against_the_independent_element_reference():
    """The same schedule evaluated under tests/elem_ref.py instead of the oracle's functor."""
    rng = np.random.default_rng(5)
    for code in (F16, BF16, F32):
        _reduce_case(rs_ref.ELEM_REF, 4, 2, code, SUM, 2, 2 * 2 * (BUFF // 2 // vnode.ESIZE[code]) + 999, False, rng)


def test_non_root_buffers_may_be_null(orc):
    """Reduce with no recvbuff off the root (Broadcast passes no sendbuff there in every case above)."""
    rng = np.random.default_rng(6)
    n, root, cnt = 4, 1, 5000
    inputs = [vnode.gen(F32, cnt, rng) for _ in range(n)]
    rings = _rings(n, 2)
    exp = rooted_ref.reduce_expected(orc, inputs, F32, SUM, root, 2, NTHR, rings, BUFF)
    recvs = [None] * n
    recvs[root] = np.zeros(cnt, np.float32)
    C.host_ring_reduce(inputs, recvs, cnt, F32, SUM, root, channels=2, nthreads=NTHR, buffer_size=BUFF, rings=rings)
    assert recvs[root].tobytes() == exp.tobytes()


def test_single_rank_is_a_local_copy():
    x = np.arange(1000, dtype=np.float32)
    y = np.zeros_like(x)
    C.host_ring_reduce([x], [y], x.size, F32, SUM, 0)
    assert y.tobytes() == x.tobytes()
    z = np.zeros(x.nbytes, np.uint8)
    C.host_ring_broadcast([x], [z], x.nbytes, 0)
    assert z.tobytes() == x.tobytes()


def test_expected_values_depend_on_the_ring_order(orc):
    """fp32 Sum at n = 4, root 1 on the identity ring: the chain folds ranks
    2, 3, 0, 1, which rounds differently from the rank-order fold 0, 1, 2, 3
    in some elements (with this seed the two results are not the same bytes,
    which is all the control has to show), and the host ring produces the
    ring-order one."""
    n, root, cnt = 4, 1, 4099
    rng = np.random.default_rng(4)
    inputs = [vnode.gen(F32, cnt, rng) for _ in range(n)]
    rings = _rings(n, 1)
    exp = rooted_ref.reduce_expected(orc, inputs, F32, SUM, root, 1, NTHR, rings, BUFF)
    plain = rooted_ref.rank_order(orc, inputs, F32, SUM)
    differ = int(np.count_nonzero(exp.view(np.uint32) != plain.view(np.uint32)))
    print(f"ring order differs from rank order in {differ} of {cnt} elements")
    assert differ > 0
    recv = np.zeros(cnt, np.float32)
    recvs = [recv if r == root else None for r in range(n)]
    C.host_ring_reduce(inputs, recvs, cnt, F32, SUM, root, channels=1, nthreads=NTHR, buffer_size=BUFF, rings=rings)
    assert recv.tobytes() == exp.tobytes()
    assert recv.tobytes() != plain.tobytes()


def test_refuses_bad_arguments():
    from mccs_amd._lib import MccsError

    x = [np.zeros(8, np.float32) for _ in range(2)]
    y = [np.zeros(8, np.float32) for _ in range(2)]
    for kw in (dict(root=-1), dict(root=2), dict(data_type=10), dict(op_type=4), dict(channels=0), dict(nthreads=32),
               dict(buffer_size=1000)):
        args = dict(data_type=F32, op_type=SUM, root=0, channels=1, nthreads=96, buffer_size=BUFF)
        args.update(kw)
        with pytest.raises(MccsError) as ei:
            C.host_ring_reduce(x, y, 8, args["data_type"], args["op_type"], args["root"], channels=args["channels"],
                               nthreads=args["nthreads"], buffer_size=args["buffer_size"])
        assert ei.value.code == 4, kw
    for root in (-1, 2):
        with pytest.raises(MccsError) as ei:
            C.host_ring_broadcast(x, y, 32, root)
        assert ei.value.code == 4, root
