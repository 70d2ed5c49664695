"""CPU: the host-thread ring's three _oparg functions (PreMulSum, SumPostDiv,
and the plain ops with op_arg = 0), bit for bit against tests/avg_ref.py.

n = 2, 3, 4 with every root for Reduce; all sixteen (dtype, op) pairs on
rs_ref.edge_inputs under SUM and on random inputs; 1 and 2 channels; a count
that spans several loops of an 8 KiB FIFO; in place; one rank.
"""
import numpy as np
import pytest

import avg_ref as A
import elem_ref as E
import vnode
from mccs_amd import comm as C
from mccs_amd._lib import MccsError

NTHR = 96
INVALID_ARGUMENT = 4


def _same(code, got, ref, what):
    ok, _ = E.same_bits(code, got, ref)
    bad = E.mismatches(code, got, ref) if not ok and got.shape == ref.shape else []
    assert ok, (what, len(bad), [(int(i), hex(int(E.bits_of(code, got)[i])), hex(int(E.bits_of(code, ref)[i])))
                                  for i in bad[:4]])


def _random(n, code, count, seed):
    rng = np.random.default_rng(seed)
    if E.is_fp(code):
        return [E.random_bits(code, count, rng, exp_span=6) for _ in range(n)]
    return [E.random_bits(code, count, rng) for _ in range(n)]


def _check_all(inputs, code, op, arg, nch, buff=1 << 22, inplace=False):
    n = len(inputs)
    cnt = inputs[0].size // n
    rings = [list(range(n))] * nch
    tag = (n, code, op, hex(arg), nch, buff, inplace)
    # AllReduce
    send = [x.copy() for x in inputs]
    recv = send if inplace else [np.zeros_like(x) for x in inputs]
    C.host_ring_allreduce(send, recv, inputs[0].size, code, op, channels=nch, nthreads=NTHR, buffer_size=buff,
                          op_arg=arg)
    exp = A.allreduce_expected(inputs, code, op, arg, nch, NTHR, rings, buff)
    for r in range(n):
        _same(code, recv[r], exp[r], ("allreduce", r) + tag)
        if not inplace:
            assert np.array_equal(E.bits_of(code, send[r]), E.bits_of(code, inputs[r]))
    # ReduceScatter
    send = [x.copy() for x in inputs]
    recv = [send[r][r * cnt:(r + 1) * cnt] for r in range(n)] if inplace else [np.zeros(cnt, x.dtype) for x in inputs]
    C.host_ring_reduce_scatter(send, recv, cnt, code, op, channels=nch, nthreads=NTHR, buffer_size=buff, op_arg=arg)
    exp = A.reduce_scatter_expected(inputs, code, op, arg, nch, NTHR, rings, buff)
    for r in range(n):
        _same(code, recv[r], exp[r], ("reduce_scatter", r) + tag)
    # Reduce, every root
    for root in range(n):
        send = [x.copy() for x in inputs]
        out = send[root] if inplace else np.zeros_like(inputs[0])
        recv = [out if r == root else None for r in range(n)]
        C.host_ring_reduce(send, recv, inputs[0].size, code, op, root, channels=nch, nthreads=NTHR, buffer_size=buff,
                           op_arg=arg)
        _same(code, out, A.reduce_expected(inputs, code, op, arg, root, nch, NTHR, rings, buff),
              ("reduce", root) + tag)


@pytest.mark.parametrize("n", [2, 3, 4])
@pytest.mark.parametrize("code,op", A.PAIRS, ids=[f"dt{c}-op{o}" for c, o in A.PAIRS])
def test_edge_values(n, code, op):
    import rs_ref

    inputs = rs_ref.edge_inputs(n, code, E.SUM)
    for i, arg in enumerate(A.case_args(code, op, n)):
        _check_all(inputs, code, op, arg, nch=1 + i)  # first argument on 1 channel, second on 2


@pytest.mark.parametrize("n", [2, 3, 4])
@pytest.mark.parametrize("code,op", A.PAIRS, ids=[f"dt{c}-op{o}" for c, o in A.PAIRS])
def test_random_values_in_place_and_several_loops(n, code, op):
    arg = A.case_args(code, op, n)[0]
    _check_all(_random(n, code, n * 331, 10 * n + code), code, op, arg, nch=2, inplace=True)
    # 8 KiB FIFO: a chunk is 4 KiB, so a few thousand elements walk several loops
    # (AllReduce: n chunks per loop; ReduceScatter: one chunk of each block)
    count = n * (2 * 4096 // vnode.ESIZE[code] + 237)
    loops = -(-count * vnode.ESIZE[code] // (n * 4096))
    assert loops >= 3, loops
    _check_all(_random(n, code, count, 20 * n + code), code, op, arg, nch=1, buff=8192)


@pytest.mark.parametrize("code,op", A.PAIRS, ids=[f"dt{c}-op{o}" for c, o in A.PAIRS])
def test_one_rank(code, op):
    """nranks == 1: post(pre(x)), out of place and in place."""
    for arg in A.case_args(code, op, 3):
        x = _random(1, code, 777, code)[0]
        want = A.apply_one(code, op, arg, x)
        for name, call in (("allreduce", lambda s, r: C.host_ring_allreduce(s, r, 777, code, op, op_arg=arg)),
                           ("reduce_scatter",
                            lambda s, r: C.host_ring_reduce_scatter(s, r, 777, code, op, op_arg=arg)),
                           ("reduce", lambda s, r: C.host_ring_reduce(s, r, 777, code, op, 0, op_arg=arg))):
            send, out = [x.copy()], [np.zeros_like(x)]
            call(send, out)
            _same(code, out[0], want, (name, code, op, hex(arg)))
            assert np.array_equal(E.bits_of(code, send[0]), E.bits_of(code, x))
            call(send, send)
            _same(code, send[0], want, (name, "in place", code, op, hex(arg)))


def test_plain_ops_through_oparg_and_refusals():
    x = _random(2, 7, 500, 1)
    a, b = [np.zeros_like(v) for v in x], [np.zeros_like(v) for v in x]
    C.host_ring_allreduce(x, a, 500, 7, E.SUM)
    C.host_ring_allreduce(x, b, 500, 7, E.SUM, op_arg=0)
    assert all(np.array_equal(p.view(np.uint32), q.view(np.uint32)) for p, q in zip(a, b))
    out = [np.zeros_like(v) for v in x]
    bad = [(7, E.SUM, 1), (7, A.SUMPOSTDIV, 2), (2, A.SUMPOSTDIV, 0), (2, A.SUMPOSTDIV, 1 << 31),
           (6, A.PREMULSUM, 0x13C00), (0, A.PREMULSUM, 0x100), (2, 6, 0)]
    for code, op, arg in bad:
        xs = [np.zeros(8, E.NPDT[code]) for _ in range(2)]
        with pytest.raises(MccsError) as ei:
            C.host_ring_allreduce(xs, [v.copy() for v in xs], 8, code, op, op_arg=arg)
        assert ei.value.code == INVALID_ARGUMENT, (code, op, arg)
    # today's three functions keep refusing ops 4 and 5
    for op in (A.PREMULSUM, A.SUMPOSTDIV):
        for call in (lambda: C.host_ring_allreduce(x, out, 500, 2, op),
                     lambda: C.host_ring_reduce_scatter(x, out, 250, 2, op),
                     lambda: C.host_ring_reduce(x, out, 500, 2, op, 0)):
            with pytest.raises(MccsError) as ei:
                call()
            assert ei.value.code == INVALID_ARGUMENT
