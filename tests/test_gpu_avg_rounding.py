"""GPU: PreMulSum rounds the product and the sum separately (no fused multiply-add).

At -O3 the compiler contracts x * s + y into one fused instruction (one
rounding) unless the pre-multiply is compiled with contraction off; the
contract is round(round(x * s) + acc).  For fp16, bf16, fp32 and fp64, the
three collectives, n = 3 and the Avg scalar 1/3 (at n = 2 the scalar is 0.5,
every product is exact and the fault invisible), on standard-normal inputs,
the CPU computes both the contract's result and the single-rounding
alternative, round(x * s + acc) in exact arithmetic at the first reducing hop,
requires that at least 10 % of the elements tell the two apart, and then
requires the GPU result to equal the contract's bit for bit.

Which ranks an output element folds, and in which order, is read off the Sum
schedules themselves (avg_ref's: ring_sim / rs_ref / rooted_ref) by running
them on rank numbers with fn(x, acc) = 4 * acc + x.
"""
import numpy as np
import pytest

import avg_ref as A
import elem_ref as E
import ring_sim
import rooted_ref
import rs_ref
import vnode
from mccs_amd import comm as C
from test_gpu_avg_values import diff, run

pytestmark = pytest.mark.gpu
DIRECT_DEFAULTS = True

N = 3
CNT = 1003  # elements per block: 3009 per rank
TIMEOUT_MS = 8000
SEED = {6: 1, 7: 1, 8: 1, 9: 1}


class _Order:
    """Element functor that records the fold: acc * 4 + (rank + 1)."""

    @staticmethod
    def apply(code, op, x, acc):
        return acc * 4 + x


def normal(code, count, rng):
    x = rng.standard_normal(count)
    if code == 9:
        u = x.astype(np.float32).view(np.uint32)
        return ((u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype(np.uint16)
    return x.astype(vnode.NPDT[code])


def orders(func, code, root, nch, nthr, rings):
    """Per output rank, per element: the fold order encoded base 4 (s1, s2, s3 as rank + 1)."""
    tags = [np.full(N * CNT, r + 1, np.int64) for r in range(N)]
    if func == "all_reduce":
        return ring_sim.simulate(tags, E.SUM, nch, nthr, ring=rings, fn=lambda op, x, acc: acc * 4 + x)
    if func == "reduce_scatter":
        return rs_ref.expected(_Order, tags, code, E.SUM, nch, nthr, rings)
    return [rooted_ref.reduce_expected(_Order, tags, code, E.SUM, root, nch, nthr, rings)]


def both(inputs, code, arg, func, order, base):
    """(contract, single-rounding alternative) of one output array whose element
    i folds the inputs' element base + i in the recorded order."""
    out_c = np.empty(order.size, vnode.NPDT[code])
    out_f = np.empty(order.size, vnode.NPDT[code])
    for o in np.unique(order):
        s1, s2, s3 = (int(o) // 16) % 4 - 1, (int(o) // 4) % 4 - 1, int(o) % 4 - 1
        assert sorted((s1, s2, s3)) == [0, 1, 2], o
        idx = np.flatnonzero(order == o)
        x1, x2, x3 = (np.ascontiguousarray(inputs[s][base + idx]) for s in (s1, s2, s3))
        acc = A.pre(code, x1, arg)
        last = A.pre(code, x3, arg)
        out_c[idx] = E.ref_op(code, E.SUM, last, E.ref_op(code, E.SUM, A.pre(code, x2, arg), acc))
        out_f[idx] = E.ref_op(code, E.SUM, last, A.fused_first_hop(code, x2, arg, acc))
    return out_c, out_f


@pytest.fixture(scope="module")
def comms():
    nch = len(C.default_rings(N))
    cs = C.init_all([0] * N, C.CommConfig(timeout_ms=TIMEOUT_MS, rings=[list(range(N))] * nch))
    yield cs
    vnode.destroy(cs)


@pytest.mark.parametrize("func", ["all_reduce", "reduce_scatter", "reduce"])
@pytest.mark.parametrize("code", [6, 9, 7, 8], ids=["fp16", "bf16", "fp32", "fp64"])
def test_product_and_sum_round_separately(comms, code, func):
    rng = np.random.default_rng(SEED[code])
    inputs = [normal(code, N * CNT, rng) for _ in range(N)]
    op, arg = A.avg_op(code, N)
    assert op == A.PREMULSUM
    es, root = vnode.ESIZE[code], 1
    plan = vnode.Planner(comms[0].nchannels, comms[0].rings())
    if func == "reduce_scatter":
        nch, nthr, rings = plan.select(CNT * es * N, CNT * es)
        exp = A.reduce_scatter_expected(inputs, code, op, arg, nch, nthr, rings)
    elif func == "all_reduce":
        nch, nthr, rings = plan.select(N * CNT * es, N * CNT * es)
        exp = A.allreduce_expected(inputs, code, op, arg, nch, nthr, rings)
    else:
        nch, nthr, rings = plan.select(N * CNT * es, N * CNT * es)
        exp = [A.reduce_expected(inputs, code, op, arg, root, nch, nthr, rings)]
    order = orders(func, code, root, nch, nthr, rings)
    told_apart = []
    for k, (e, o) in enumerate(zip(exp, order)):
        contract, fused = both(inputs, code, arg, func, o, k * CNT if func == "reduce_scatter" else 0)
        assert not diff(code, contract, e), "the fold order read off the schedule disagrees with avg_ref"
        told_apart.append(E.mismatches(code, fused, contract).size / contract.size)
    print(f"dtype {code} {func}: a fused multiply-add changes {[round(t, 3) for t in told_apart]} of the elements")
    assert min(told_apart) >= 0.10, told_apart
    got = run(comms, inputs, code, op, arg, func, root)
    for g, e in zip(got, exp):
        assert not diff(code, g, e), (code, func, diff(code, g, e))
