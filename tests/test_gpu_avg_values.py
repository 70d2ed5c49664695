"""GPU: all 48 PreMulSum / SumPostDiv ring kernels (three collectives x sixteen
(dtype, op) pairs) on edge values, bit for bit against tests/avg_ref.py.

n = 2 and 3 ranks on one GPU, identity rings, AllReduce, ReduceScatter and
Reduce at roots 0 and n-1.  Inputs are rs_ref.edge_inputs(n, code, SUM): block
d of a rank's buffer holds elem_ref's edge values and random bits (at n = 2 no
block is a multiple of a 16-byte pack).  Each pair runs with the two arguments of
avg_ref.case_args: fp the Avg scalar and 3.0, signed integers 3 and -1,
unsigned 3 and the type's maximum, SumPostDiv n and 7.

Before any launch the expected arrays are checked on the CPU so the test can
fail: at least 75 % of each is non-NaN, and each differs from the plain Sum's
expected array in at least half its elements.
"""
import numpy as np
import pytest

import avg_ref as A
import elem_ref as E
import rooted_ref
import rs_ref
import vnode
from mccs_amd import comm as C

pytestmark = pytest.mark.gpu
DIRECT_DEFAULTS = True  # the library's default routing: the new ops must take the ring whatever the size

TIMEOUT_MS = 8000
FUNCS = ("all_reduce", "reduce_scatter", "reduce")
_comms = {}
_launched = set()


@pytest.fixture(scope="module")
def nodes():
    """comms(n): one identity-ring communicator set per n, shared by the module."""
    def get(n):
        if n not in _comms:
            nch = len(C.default_rings(n))
            _comms[n] = C.init_all([0] * n, C.CommConfig(timeout_ms=TIMEOUT_MS, rings=[list(range(n))] * nch))
            assert _comms[n][0].rings() == [list(range(n))] * nch
        return _comms[n]

    yield get
    for comms in _comms.values():
        vnode.destroy(comms)
    _comms.clear()


def _plan(comm0, nbytes_total, nbytes_load):
    return vnode.Planner(comm0.nchannels, comm0.rings()).select(nbytes_total, nbytes_load)


def expected(comm0, inputs, code, op, arg, func, root=0):
    """(expected per rank, the plain Sum's expected per rank) for one call."""
    n, es = len(inputs), vnode.ESIZE[code]
    total = inputs[0].size
    if func == "all_reduce":
        nch, nthr, rings = _plan(comm0, total * es, total * es)
        return (A.allreduce_expected(inputs, code, op, arg, nch, nthr, rings),
                A.sum_allreduce_expected(inputs, code, nch, nthr, rings))
    if func == "reduce_scatter":
        cnt = total // n
        nch, nthr, rings = _plan(comm0, cnt * es * n, cnt * es)
        return (A.reduce_scatter_expected(inputs, code, op, arg, nch, nthr, rings),
                A.reduce_scatter_expected(inputs, code, E.SUM, 0, nch, nthr, rings))
    nch, nthr, rings = rooted_ref.select(total * es, comm0)
    return ([A.reduce_expected(inputs, code, op, arg, root, nch, nthr, rings)],
            [A.reduce_expected(inputs, code, E.SUM, 0, root, nch, nthr, rings)])


def can_fail(code, exp, plain, what):
    for e, p in zip(exp, plain):
        _, live = E.same_bits(code, e, e)
        assert live >= 0.75, (what, live)
        differ = E.mismatches(code, e, p).size / e.size
        assert differ >= 0.5, (what, differ)


def diff(code, got, ref):
    ok, _ = E.same_bits(code, got, ref)
    if ok:
        return ""
    bad = E.mismatches(code, got, ref) if got.shape == ref.shape else np.arange(0)
    return (f"{bad.size} of {ref.size} differ, first at {bad[:5].tolist()}: got "
            f"{[hex(v) for v in E.bits_of(code, got)[bad[:5]].tolist()]} want "
            f"{[hex(v) for v in E.bits_of(code, ref)[bad[:5]].tolist()]}")


def run(comms, inputs, code, op, arg, func, root=0):
    """One grouped call out of place; returns the per-rank outputs that the call defines."""
    n = len(comms)
    total = inputs[0].size
    send = [vnode.to_dev(x) for x in inputs]
    if func == "reduce_scatter":
        recv = [vnode.to_dev(np.zeros(total // n, vnode.NPDT[code])) for _ in range(n)]
    else:
        recv = [vnode.to_dev(np.zeros(total, vnode.NPDT[code])) for _ in range(n)]
    with C.group():
        for r, c in enumerate(comms):
            if func == "all_reduce":
                C.all_reduce(c, send[r], recv[r], total, code, op, op_arg=arg)
            elif func == "reduce_scatter":
                C.reduce_scatter(c, send[r], recv[r], total // n, code, op, op_arg=arg)
            else:
                C.reduce(c, send[r], recv[r] if r == root else None, total, code, op, root, op_arg=arg)
    for c in comms:
        c.sync()
    assert {c.last_algo() for c in comms} == {"ring"}
    for r in range(n):  # out of place: the send buffer is unchanged
        assert np.array_equal(E.bits_of(code, vnode.from_dev(send[r], code)), E.bits_of(code, inputs[r]))
    if func == "reduce":
        return [vnode.from_dev(recv[root], code)]
    return [vnode.from_dev(recv[r], code) for r in range(n)]


@pytest.mark.parametrize("n", [2, 3])
@pytest.mark.parametrize("code,op", A.PAIRS, ids=[f"dt{c}-op{o}" for c, o in A.PAIRS])
def test_edge_values(nodes, n, code, op):
    comms = nodes(n)
    inputs = rs_ref.edge_inputs(n, code, E.SUM)  # vacuity of the Sum fold asserted inside
    if n == 2:  # edge_pairs: no block is a multiple of a pack (typed tails carry data)
        assert (inputs[0].size // n) % (16 // vnode.ESIZE[code]) != 0
    cases = []
    for arg in A.case_args(code, op, n):
        for func, root in (("all_reduce", 0), ("reduce_scatter", 0), ("reduce", 0), ("reduce", n - 1)):
            exp, plain = expected(comms[0], inputs, code, op, arg, func, root)
            can_fail(code, exp, plain, (n, code, op, hex(arg), func, root))
            cases.append((arg, func, root, exp))
    bad = {}
    for arg, func, root, exp in cases:
        got = run(comms, inputs, code, op, arg, func, root)
        _launched.add((func, code, op))
        for k, (g, e) in enumerate(zip(got, exp)):
            d = diff(code, g, e)
            if d:
                bad[(hex(arg), func, root, k)] = d
    assert not bad, bad


def test_all_48_kernels_were_launched():
    """Runs after the sweep above (file order): three collectives x sixteen pairs."""
    want = {(f, c, o) for f in FUNCS for c, o in A.PAIRS}
    assert len(want) == 48
    assert _launched == want, sorted(want - _launched)


def test_signed_sumpostdiv_truncates_and_wraps(nodes):
    """Small integers of both signs: at least 10 % of the sums are negative and
    no multiple of the divisor, where flooring and truncating differ; and one
    case whose sums wrap before the division."""
    n = 3
    comms = nodes(n)
    rng = np.random.default_rng(77)
    for code in A.SIGNED:
        npdt = vnode.NPDT[code]
        w = E.width(code)
        lo, hi = (-40, 40) if code == 0 else (-100, 100)
        small = [rng.integers(lo, hi, n * 1501).astype(npdt) for _ in range(n)]
        tot = sum(x.astype(np.int64) for x in small)
        assert np.mean((tot < 0) & (tot % 3 != 0)) >= 0.10
        big = [rng.integers(-(1 << (w - 1)), (1 << (w - 1)) - 1, n * 1501, dtype=np.int64, endpoint=True).astype(npdt)
               for _ in range(n)]
        exact = sum(x.astype(object) for x in big)
        assert np.mean([abs(int(v)) >= (1 << (w - 1)) for v in exact]) >= 0.10  # the sums wrap
        for inputs in (small, big):
            for func, root in (("all_reduce", 0), ("reduce_scatter", 0), ("reduce", 1)):
                exp, _ = expected(comms[0], inputs, code, A.SUMPOSTDIV, 3, func, root)
                if inputs is small and func == "all_reduce":
                    floor = (tot // 3).astype(npdt)
                    assert np.mean(floor != exp[0]) >= 0.10  # a flooring kernel would fail here
                got = run(comms, inputs, code, A.SUMPOSTDIV, 3, func, root)
                for g, e in zip(got, exp):
                    assert not diff(code, g, e), (code, func, diff(code, g, e))
