"""GPU: every ReduceScatter kernel (ten dtypes x four ops) on edge values,
against the independent element reference.

tests/test_gpu_reduce_scatter.py checks the schedule on numbers from the
middle of the number line and against the oracle's own functor.  Here the
inputs are tests/elem_ref.py's edge values (signed zeros, subnormals,
round-to-even ties, sums and products that just reach Inf or just do not,
NaNs on either side, integer wrap, busy high words) and the expected values
are tests/rs_ref.py's restatement of the schedule evaluated with
elem_ref.ref_op in the ring's operand order fn(x[s_k], acc), which decides
Max / Min of +0 and -0.

n = 2: ranks 0 / 1 hold x / y of edge_pairs (3577-6845 elements per block, no
multiple of a pack); n = 4 on identity rings: block d folds the sources of
edge_sources(seed=d) in the order 0, 1, 2, 3.  Each communicator set runs all
forty (dtype, op) pairs aligned and out of place, with both buffers one
element past a 16-byte boundary (the typed loops), or in place
(recv = send + rank * cnt * esize).

rs_ref.edge_inputs refuses vacuous inputs before the GPU is touched: every
expected block is at least 75 % non-NaN (those compare bit for bit, NaNs as
"is NaN") and every targeted class occurs in some step of the fold.
"""
import numpy as np
import pytest

import elem_ref as E
import rs_ref
import vnode
from mccs_amd import comm as C

pytestmark = pytest.mark.gpu
DIRECT_DEFAULTS = True  # the library's default routing: a ReduceScatter must take the ring whatever its size

CODES = list(range(10))
OPS = [E.SUM, E.PROD, E.MAX, E.MIN]
TIMEOUT_MS = 8000
VARIANTS = ["aligned", "misaligned", "inplace"]

_expected = {}


def expected(comm0, n, code, op):
    """Per-rank expected blocks under elem_ref for the channels, threads and
    rings the planner gives this call; computed once per plan."""
    inputs = rs_ref.edge_inputs(n, code, op)
    cnt = inputs[0].size // n
    nch, nthr, rings = vnode.Planner(comm0.nchannels, comm0.rings()).select(cnt * vnode.ESIZE[code] * n,
                                                                             cnt * vnode.ESIZE[code])
    key = (n, code, op, nch, nthr, str(rings))
    if key not in _expected:
        exp = rs_ref.expected_planned(rs_ref.ELEM_REF, inputs, code, op, comm0)
        for d in range(n):
            _, live = E.same_bits(code, exp[d], exp[d])
            assert live >= 0.75, (n, code, op, d, live)
            exp[d].setflags(write=False)
        _expected[key] = exp
    return _expected[key]


def run(comms, inputs, code, variant):
    """Stages `inputs` for one grouped ReduceScatter.  Returns launch(op),
    fetch(rank) -> that rank's received block, and the device buffers."""
    import torch

    n, es = len(comms), vnode.ESIZE[code]
    cnt = inputs[0].size // n
    if variant == "misaligned":  # both buffers one element past a 16-byte boundary
        sbuf = [torch.zeros(n * cnt * es + 64, dtype=torch.uint8, device="cuda") for _ in range(n)]
        rbuf = [torch.zeros(cnt * es + 64, dtype=torch.uint8, device="cuda") for _ in range(n)]
        for r in range(n):
            assert sbuf[r].data_ptr() % 16 == 0 and rbuf[r].data_ptr() % 16 == 0
            sbuf[r][es:es + n * cnt * es].copy_(vnode.to_dev(inputs[r]))
        send = [t.data_ptr() + es for t in sbuf]
        recv = [t.data_ptr() + es for t in rbuf]
        fetch = lambda r: rbuf[r][es:es + cnt * es].cpu().numpy().view(vnode.NPDT[code])  # noqa: E731
    elif variant == "inplace":
        sbuf = [vnode.to_dev(x) for x in inputs]
        rbuf = None
        send = [t.data_ptr() for t in sbuf]
        recv = [send[r] + r * cnt * es for r in range(n)]
        fetch = lambda r: vnode.from_dev(sbuf[r], code)[r * cnt:(r + 1) * cnt]  # noqa: E731
    else:
        sbuf = [vnode.to_dev(x) for x in inputs]
        rbuf = [vnode.to_dev(np.zeros(cnt, vnode.NPDT[code])) for _ in range(n)]
        send = [t.data_ptr() for t in sbuf]
        recv = [t.data_ptr() for t in rbuf]
        fetch = lambda r: vnode.from_dev(rbuf[r], code)  # noqa: E731
    torch.cuda.synchronize()

    def launch(op):
        with C.group():
            for r, c in enumerate(comms):
                C.reduce_scatter(c, send[r], recv[r], cnt, code, op)
        for c in comms:
            c.sync()

    return launch, fetch, (sbuf, rbuf)


def _diff(code, got, ref):
    ok, _ = E.same_bits(code, got, ref)
    if ok:
        return ""
    bad = E.mismatches(code, got, ref)
    return (f"{bad.size} of {ref.size} differ, first at {bad[:5].tolist()}: got "
            f"{[hex(v) for v in E.bits_of(code, got)[bad[:5]].tolist()]} want "
            f"{[hex(v) for v in E.bits_of(code, ref)[bad[:5]].tolist()]}")


def sweep(comms, n, variant, algo="ring"):
    """Every dtype x op on one communicator set; returns the failures.  `algo`
    is the kernel every rank must have taken (the direct bodies:
    tests/test_gpu_reduce_scatter_direct_values.py)."""
    bad, launched = {}, []
    for code in CODES:
        for op in OPS:
            inputs = rs_ref.edge_inputs(n, code, op)  # vacuity asserted inside, before the launch
            exp = expected(comms[0], n, code, op)
            launch, fetch, keep = run(comms, inputs, code, variant)
            launch(op)
            algos = [c.last_algo() for c in comms]
            assert algos == [algo] * n, (code, op, algos)
            launched.append((code, op))
            for r in range(n):
                d = _diff(code, fetch(r), exp[r])
                if d:
                    bad[(code, op, r)] = d
            del keep
    print(f"n={n} {variant}: launched {len(launched)} ReduceScatter kernels (dtype, op): {launched}")
    assert len(set(launched)) == 40
    return bad


@pytest.mark.parametrize("variant", VARIANTS)
def test_edge_pairs_two_ranks(variant):
    comms = C.init_all([0] * 2, C.CommConfig(timeout_ms=TIMEOUT_MS))
    try:
        for code in CODES:  # no count is a multiple of a 16-byte pack
            cnt = rs_ref.edge_inputs(2, code, E.SUM)[0].size // 2
            assert 3577 <= cnt <= 6845 and cnt % (16 // vnode.ESIZE[code]) != 0, (code, cnt)
        assert not sweep(comms, 2, variant)
    finally:
        vnode.destroy(comms)


@pytest.mark.parametrize("variant", VARIANTS)
def test_edge_sources_four_ranks(variant):
    """Identity rings on every channel: block d's fold visits ranks d+1, ..,
    d, which hold the sources 0, 1, 2, 3 of edge_sources(seed=d)."""
    n = 4
    nch = len(C.default_rings(n))
    comms = C.init_all([0] * n, C.CommConfig(timeout_ms=TIMEOUT_MS, rings=[list(range(n))] * nch))
    try:
        assert comms[0].rings() == [list(range(n))] * nch
        assert not sweep(comms, n, variant)
    finally:
        vnode.destroy(comms)
