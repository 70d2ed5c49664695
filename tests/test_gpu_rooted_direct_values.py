"""GPU: every direct Reduce kernel (ten dtypes x four ops), both bodies, on
edge values, against the independent element reference.

What tests/test_gpu_reduce_scatter_direct_values.py does for
direct_rs_kernel<DT, OP>, for direct_rd_kernel<DT, OP> (csrc/direct_rooted.h):
tests/test_gpu_rooted_direct.py draws its inputs from vnode.gen, and
tests/test_gpu_reduce_values.py asserts that the ring ran.  The inputs are
that module's `buffers` (block `root` of rs_ref.edge_inputs, unchanged) and the
expected values its `expected` (rooted_ref.reduce_expected under
rs_ref.ELEM_REF, cached per plan: the bf16 reference is computed once per
process); nothing comes from the library's ring.  Communicators as
tests/test_gpu_rooted_direct.py's, opted in at the cap of the variant under
test; the largest buffer is 54 760 bytes, within both caps.  At n = 2 no
count of a 1-, 2- or 4-byte type fills its last 8-byte word, at n = 3 none of
an 8- or 32-bit integer (the 3508 fp16 / fp32 and 1508 bf16 elements there are
whole words), so the LL tail word is partial; the test asserts it.

n = 2 and n = 3 on identity rings, roots 0 and n - 1, out of place and in
place on the root; every test launches all 40 (dtype, op) pairs and compares
with elem_ref.same_bits.
"""
import numpy as np
import pytest

import elem_ref as E
import test_gpu_reduce_values as R
import test_gpu_rooted_direct as D
import vnode
from mccs_amd import comm as C

pytestmark = pytest.mark.gpu
DIRECT_DEFAULTS = True  # D.CFG sets every threshold


@pytest.mark.parametrize("inplace", [False, True], ids=["out of place", "in place"])
@pytest.mark.parametrize("variant", D.VARIANTS)
@pytest.mark.parametrize("n", [2, 3])
def test_all_forty_reduce_kernels_on_edge_values(n, variant, inplace):
    """Identity rings on every channel: the Reduce to `root` visits ranks
    root+1, .., root, which hold the operands edge_inputs laid out for block
    `root`.  Non-roots pass no recvbuff."""
    nch = len(C.default_rings(n))
    comms = D._comms(n, "rd", variant, rings=[list(range(n))] * nch)
    try:
        assert comms[0].rings() == [list(range(n))] * nch
        bad, launched = {}, set()
        for code in R.CODES:
            for op in R.OPS:
                for root in (0, n - 1):
                    bufs = R.buffers(n, code, op, root)
                    exp = R.expected(comms[0], n, code, op, root)
                    _, live = E.same_bits(code, exp, exp)
                    assert live >= 0.75, (n, code, op, root, live)
                    cnt = bufs[0].size
                    es = vnode.ESIZE[code]
                    assert cnt * es <= 54760 <= min(D.ONESHOT, D.LL_BYTES)
                    if es < 8 and (n == 2 or code < 4):  # the last 8-byte word is partial: ll_store_word's tail path
                        assert cnt * es % 8 != 0, (n, code, cnt)
                    send = [vnode.to_dev(x) for x in bufs]
                    recv = send[root] if inplace else vnode.to_dev(np.zeros(cnt, vnode.NPDT[code]))
                    with C.group():
                        for r, c in enumerate(comms):
                            C.reduce(c, send[r], recv if r == root else None, cnt, code, op, root)
                    algos = [c.last_algo() for c in comms]
                    assert algos == [variant] * n, (code, op, root, algos)
                    for c in comms:
                        c.sync()
                    launched.add((code, op))
                    d = R._diff(code, vnode.from_dev(recv, code), exp)
                    if d:
                        bad[(code, op, root)] = d
                    for r in range(n):  # a source is read only
                        if not (inplace and r == root) and vnode.from_dev(send[r], code).tobytes() != bufs[r].tobytes():
                            bad[(code, op, root, "send", r)] = "send buffer written"
        print(f"n={n} {variant} inplace={inplace}: launched {len(launched)} direct Reduce kernels (dtype, op)")
        assert len(launched) == 40
        assert not bad, bad
    finally:
        vnode.destroy(comms)
