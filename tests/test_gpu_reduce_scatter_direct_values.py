"""GPU: every direct ReduceScatter kernel (ten dtypes x four ops), both bodies,
on edge values, against the independent element reference.

tests/test_gpu_reduce_scatter_direct.py draws its inputs from vnode.gen (floats
in (-1, 1), integers in -5..5), and tests/test_gpu_reduce_scatter_values.py
asserts that the ring ran: no NaN, Inf, signed zero, subnormal, round-to-even
tie, integer wrap or 64-bit value with a busy high word reaches
direct_rs_kernel<DT, OP> there.  The LL body (csrc/direct_rs.h
direct_rs_ll_body) cuts each 8-byte word into two 32-bit halves around a flag,
puts it together again from h0 / h1, folds it through ll_pack and
pack_op<DT, OP> with two dead lanes and stores a partial last word through
ll_store_word; with int64 in -5..5 the high half is all zeros or all ones.

Here the inputs are rs_ref.edge_inputs, unchanged, and the expected values the
other values module's (`expected`: rs_ref.expected_planned under
rs_ref.ELEM_REF, cached per plan, so the slow bf16 reference is computed once
per process whichever module runs first); nothing comes from the library's
ring.  Communicators as tests/test_gpu_reduce_scatter_direct.py's: one-shot
slots of 256 KiB, LL slots for 128 KiB blocks, opted in at the cap of the
variant under test.  The largest block is 54 760 bytes (fp64, n = 2): every
case fits both caps.  At n = 2 no count of a 1-, 2- or 4-byte type fills its
last 8-byte word (at n = 4 none of an 8- or 32-bit integer), so the LL tail
word is partial, and with int8 the foreign blocks start off an 8-byte boundary.

n = 2 on the default rings and n = 4 on identity rings, each aligned, with
both buffers one element past a 16-byte boundary, and in place; every test
launches all 40 (dtype, op) pairs and compares with elem_ref.same_bits (bit
for bit, NaN as "is NaN").  tests/test_direct_values_flips.py shows on the CPU
that the comparison sees one flipped bit in an int64's high word and a zero's
flipped sign.
"""
import pytest

import elem_ref as E
import rs_ref
import test_gpu_reduce_scatter_direct as D
import test_gpu_reduce_scatter_values as V
import vnode
from mccs_amd import comm as C

pytestmark = pytest.mark.gpu
DIRECT_DEFAULTS = True  # D.CFG sets every threshold

LAYOUTS = V.VARIANTS  # aligned, misaligned, inplace


def _fits(n):
    """Counts as the suite keeps them, every block within both caps, and the
    LL tail word partial: at n = 2 for every 1-, 2- and 4-byte type, at n = 4
    (edge_sources' 3508 fp16 / fp32 and 1508 bf16 elements are whole words)
    for the 8- and 32-bit integers."""
    for code in V.CODES:
        cnt = rs_ref.edge_inputs(n, code, E.SUM)[0].size // n
        es = vnode.ESIZE[code]
        assert (3577 <= cnt <= 6845) if n == 2 else (1508 <= cnt <= 3508), (n, code, cnt)
        assert cnt * es <= 54760 <= min(D.ONESHOT, D.LL_BYTES)
        if es < 8 and (n == 2 or code < 4):
            assert cnt * es % 8 != 0, (n, code, cnt)


def _sweep(comms, n, layout, variant):
    for code in V.CODES:
        for op in V.OPS:
            for d, block in enumerate(V.expected(comms[0], n, code, op)):
                _, live = E.same_bits(code, block, block)
                assert live >= 0.75, (n, code, op, d, live)
    bad = V.sweep(comms, n, layout, algo=variant)  # asserts last_algo() on every rank and 40 launched pairs
    assert not bad, bad


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("variant", D.VARIANTS)
def test_edge_pairs_two_ranks(variant, layout):
    _fits(2)
    comms = D._comms(2, variant)
    try:
        _sweep(comms, 2, layout, variant)
    finally:
        vnode.destroy(comms)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("variant", D.VARIANTS)
def test_edge_sources_four_ranks(variant, layout):
    """Identity rings on every channel: block d's fold visits ranks d+1, ..,
    d, which hold the sources 0, 1, 2, 3 of edge_sources(seed=d)."""
    n = 4
    _fits(n)
    nch = len(C.default_rings(n))
    comms = D._comms(n, variant, rings=[list(range(n))] * nch)
    try:
        assert comms[0].rings() == [list(range(n))] * nch
        _sweep(comms, n, layout, variant)
    finally:
        vnode.destroy(comms)
