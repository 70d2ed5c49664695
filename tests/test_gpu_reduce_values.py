"""GPU: every Reduce kernel (ten dtypes x four ops) on edge values, against
the independent element reference.

tests/test_gpu_rooted.py checks the schedule on numbers from the middle of the
number line and against the oracle's own functor.  Here the inputs are
tests/elem_ref.py's edge values as tests/rs_ref.py's edge_inputs arranges them
for a ReduceScatter, with block `root` of each rank's ReduceScatter input as
that rank's Reduce buffer: on identity rings the Reduce to `root` folds exactly
what the ReduceScatter folds for block `root`, so the vacuity checks made in
edge_inputs (at least 75 % of every expected block non-NaN, every targeted
class met in some step of the fold) hold for these cases too.  Expected values
are tests/rooted_ref.py's restatement of the schedule evaluated with
elem_ref.ref_op in the ring's operand order fn(x[s_k], acc).
"""
import numpy as np
import pytest

import elem_ref as E
import rooted_ref
import rs_ref
import vnode
from mccs_amd import comm as C

pytestmark = pytest.mark.gpu

CODES = list(range(10))
OPS = [E.SUM, E.PROD, E.MAX, E.MIN]
TIMEOUT_MS = 8000

_expected = {}


def buffers(n, code, op, root):
    """Per-rank Reduce inputs: block `root` of rs_ref.edge_inputs."""
    inputs = rs_ref.edge_inputs(n, code, op)  # vacuity asserted inside, before any launch
    cnt = inputs[0].size // n
    return [np.ascontiguousarray(x[root * cnt:(root + 1) * cnt]) for x in inputs]


def expected(comm0, n, code, op, root):
    """The root's expected result under elem_ref for the channels, threads and
    rings the planner gives this call; computed once per plan."""
    bufs = buffers(n, code, op, root)
    nbytes = bufs[0].size * vnode.ESIZE[code]
    nch, nthr, rings = rooted_ref.select(nbytes, comm0)
    key = (n, code, op, root, nch, nthr, str(rings))
    if key not in _expected:
        exp = rooted_ref.reduce_expected(rs_ref.ELEM_REF, bufs, code, op, root, nch, nthr, rings)
        _, live = E.same_bits(code, exp, exp)
        assert live >= 0.75, (n, code, op, root, live)
        exp.setflags(write=False)
        _expected[key] = exp
    return _expected[key]


def _diff(code, got, ref):
    ok, _ = E.same_bits(code, got, ref)
    if ok:
        return ""
    bad = E.mismatches(code, got, ref)
    return (f"{bad.size} of {ref.size} differ, first at {bad[:5].tolist()}: got "
            f"{[hex(v) for v in E.bits_of(code, got)[bad[:5]].tolist()]} want "
            f"{[hex(v) for v in E.bits_of(code, ref)[bad[:5]].tolist()]}")


@pytest.mark.parametrize("n", [2, 3])
def test_all_forty_reduce_kernels_on_edge_values(n):
    """Identity rings on every channel: the Reduce to `root` visits ranks
    root+1, .., root, which hold the operands edge_inputs laid out for block
    `root`.  Roots 0 and n-1, out of place, every dtype x op."""
    nch = len(C.default_rings(n))
    comms = C.init_all([0] * n, C.CommConfig(timeout_ms=TIMEOUT_MS, rings=[list(range(n))] * nch))
    try:
        assert comms[0].rings() == [list(range(n))] * nch
        bad, launched = {}, set()
        for code in CODES:
            for op in OPS:
                for root in (0, n - 1):
                    bufs = buffers(n, code, op, root)
                    exp = expected(comms[0], n, code, op, root)
                    cnt = bufs[0].size
                    send = [vnode.to_dev(x) for x in bufs]
                    recv = vnode.to_dev(np.zeros(cnt, vnode.NPDT[code]))
                    with C.group():
                        for r, c in enumerate(comms):
                            C.reduce(c, send[r], recv if r == root else None, cnt, code, op, root)
                    for c in comms:
                        c.sync()
                    assert {c.last_algo() for c in comms} == {"ring"}, (code, op, root)
                    launched.add((code, op))
                    d = _diff(code, vnode.from_dev(recv, code), exp)
                    if d:
                        bad[(code, op, root)] = d
        print(f"n={n}: launched {len(launched)} Reduce kernels (dtype, op)")
        assert len(launched) == 40
        assert not bad, bad
    finally:
        vnode.destroy(comms)
