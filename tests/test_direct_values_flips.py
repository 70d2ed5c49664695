"""CPU: the comparison of the direct kernels' edge-value tests sees the
failures those tests are for.

tests/test_gpu_reduce_scatter_direct_values.py and
tests/test_gpu_rooted_direct_values.py compare with the `_diff` of the two
ring values modules (elem_ref.same_bits).  An LL body that lost or swapped the
high half of a 64-bit word, or a fold that returned the other zero, changes
single bits: planted here into an expected block, each must be reported.
"""
import numpy as np

import elem_ref as E
import rooted_ref
import rs_ref
import test_gpu_reduce_scatter_values as V
import test_gpu_reduce_values as R
import vnode
from mccs_amd import comm as C

I64, F16 = 4, 6


def _rs_block(n, code, op, d):
    """Block d of the ReduceScatter expectation, as V.expected builds it for the default rings."""
    rings = C.default_rings(n)
    xs = rs_ref.edge_inputs(n, code, op)
    nbytes = xs[0].size // n * vnode.ESIZE[code]
    nch, nthr, sel = vnode.Planner(len(rings), rings).select(nbytes * n, nbytes)
    return rs_ref.expected(rs_ref.ELEM_REF, xs, code, op, nch, nthr, sel)[d]


def test_one_bit_in_the_high_word_of_one_int64_is_reported():
    exp = _rs_block(2, I64, E.SUM, 1)
    assert not V._diff(I64, exp.copy(), exp)
    busy = np.flatnonzero((E.bits_of(I64, exp) >> np.uint64(32)) % np.uint64(0xFFFFFFFF) != 0)
    assert busy.size > exp.size // 4  # high words that are neither all zeros nor all ones
    for k, bit in ((int(busy[0]), 32), (int(busy[-1]), 47), (exp.size - 1, 63)):
        got = exp.copy()
        E.bits_of(I64, got)[k] ^= np.uint64(1) << np.uint64(bit)
        msg = V._diff(I64, got, exp)
        assert msg.startswith(f"1 of {exp.size} differ, first at [{k}]"), msg
        assert R._diff(I64, got, exp) == msg


def test_the_sign_of_one_fp16_zero_is_reported():
    n, root = 3, 2
    rings = [list(range(n))]
    bufs = R.buffers(n, F16, E.MAX, root)
    exp = rooted_ref.reduce_expected(rs_ref.ELEM_REF, bufs, F16, E.MAX, root, 1, 512, rings)
    bits = E.bits_of(F16, exp)
    zeros = np.flatnonzero((bits & np.uint16(0x7FFF)) == 0)
    assert {int(b) for b in bits[zeros]} == {0x0000, 0x8000}  # both zeros occur: Max of +0 and -0 is decided
    for k in (int(zeros[0]), int(zeros[-1])):
        got = exp.copy()
        E.bits_of(F16, got)[k] ^= np.uint16(0x8000)
        assert float(got.view(np.float16)[k]) == float(exp.view(np.float16)[k])  # equal as numbers
        msg = R._diff(F16, got, exp)
        assert msg.startswith(f"1 of {exp.size} differ, first at [{k}]"), msg
        assert V._diff(F16, got, exp) == msg
