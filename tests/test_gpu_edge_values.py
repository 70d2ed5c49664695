"""GPU: every element op on edge values against the independent reference.

The other GPU suites compare the kernels with oracle/mccs_oracle.c, our own
restatement of the reference's functors, on inputs from the middle of the
number line.  Here the expected values come from tests/elem_ref.py (written
from the functor table, no binary32 detour for the half types, explicit
fmaxf/fminf rules) and the inputs are the cross product of each type's edge
values plus random bit patterns: signed zeros, subnormals, round-to-even
ties, sums and products that just reach Inf or just do not, NaNs on either
side, integer wrap, 64-bit operands with busy high words.

Covered routes: the chunk reduce's pack path with its scalar tail, its
scalar kernel (misaligned buffers), its four main-loop variants, 3- and
8-source folds; the ring on the virtual node at n = 2 and n = 4, aligned and
misaligned; the direct, one-shot and LL kernels.  The ring's expected output
is tests/ring_sim.py driven by the reference functor.

Every case first checks that it is not vacuous: at least 75 % of the expected
elements are non-NaN (those are compared bit for bit, NaNs as "is NaN"), and
each targeted class -- subnormal result, tie, overflow to Inf, -0, wrap --
occurs in the reference output (tests/test_elem_ref.py checks the same on the
CPU).
"""
from functools import lru_cache

import numpy as np
import pytest

import elem_ref as E
import ring_sim
import vnode
from mccs_amd import comm as C

pytestmark = pytest.mark.gpu
DIRECT_DEFAULTS = True  # conftest: thresholds are set per communicator below

CODES = list(range(10))
OPS = [E.SUM, E.PROD, E.MAX, E.MIN]
RING4_CODES = [6, 9, 7, 8, 2, 4, 5]
RING_ONLY = dict(direct_bytes=-1, oneshot_bytes=-1, ll_bytes=-1)
DIRECT, LL_MAX = 8 << 20, 1 << 20


@lru_cache(maxsize=None)
def pair_case(code, op):
    """(x, y, fn(x, y)) on edge_pairs, checked once for vacuity."""
    x, y = E.edge_pairs(code)
    ref = E.ref_op(code, op, x, y)
    _, live = E.same_bits(code, ref, ref)
    assert live >= 0.75, (code, op, live)
    assert E.result_classes(code, op, x, y, ref) >= E.required_classes(code, op), (code, op)
    for a in (x, y, ref):
        a.setflags(write=False)
    return x, y, ref


@lru_cache(maxsize=None)
def fold_case(code, op, nsrcs):
    """(sources, left fold) on edge_sources, checked once for vacuity."""
    srcs = E.edge_sources(code, nsrcs, op)
    ref, classes = E.fold_classes(code, op, srcs)
    _, live = E.same_bits(code, ref, ref)
    assert live >= 0.75, (code, op, nsrcs, live)
    assert classes >= E.required_classes(code, op), (code, op, nsrcs, classes)
    for a in srcs + [ref]:
        a.setflags(write=False)
    return srcs, ref


def _diff(code, got, ref):
    """'' when got equals ref (NaNs as "is NaN"), else a short description."""
    ok, _ = E.same_bits(code, got, ref)
    if ok:
        return ""
    bad = E.mismatches(code, got, ref)
    return (f"{bad.size} of {ref.size} differ, first at {bad[:5].tolist()}: got "
            f"{[hex(v) for v in E.bits_of(code, got)[bad[:5]].tolist()]} want "
            f"{[hex(v) for v in E.bits_of(code, ref)[bad[:5]].tolist()]}")


def run_reduce(srcs, code, op, misalign=0):
    """mccs_amd.reduce_copy of the sources into one destination; misalign
    offsets every buffer by that many elements from a 16-byte boundary."""
    import mccs_amd
    import torch

    n, es = srcs[0].size, srcs[0].itemsize
    off = misalign * es

    def dev(x):
        buf = torch.zeros(n * es + 64, dtype=torch.uint8, device="cuda")  # 64 spare bytes cover the offset
        if x is not None:
            buf[off:off + n * es].copy_(torch.from_numpy(x.view(np.uint8).copy()))
        return buf

    s_dev, d_dev = [dev(s) for s in srcs], dev(None)
    mccs_amd.reduce_copy([d_dev.data_ptr() + off], [b.data_ptr() + off for b in s_dev], count=n, dtype=code, op=op)
    torch.cuda.synchronize()
    return d_dev[off:off + n * es].cpu().numpy().view(E.NPDT[code])


# ---- 1. chunk reduce, two sources ----------------------------------------------------
@pytest.mark.parametrize("misalign", [0, 1], ids=["pack+tail", "scalar"])
@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("code", CODES)
def test_reduce_edge_pairs(code, op, misalign):
    """Aligned: 16-byte packs (pack_op) and a scalar tail, the count being no
    multiple of the pack.  Offset by one element: the whole array goes through
    reduce_scalar_kernel (scalar_op)."""
    x, y, ref = pair_case(code, op)
    assert x.size % (16 // x.itemsize) != 0
    got = run_reduce([x, y], code, op, misalign=misalign)
    assert not _diff(code, got, ref)


@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("code", [6, 7, 9])
def test_reduce_edge_pairs_every_main_loop(code, op):
    import mccs_amd

    x, y, ref = pair_case(code, op)
    bad = {}
    try:
        for variant in (1, 2, 3, 4):
            mccs_amd.tune(variant)
            got = run_reduce([x, y], code, op)
            if _diff(code, got, ref):
                bad[variant] = _diff(code, got, ref)
    finally:
        mccs_amd.tune()
    assert not bad


# ---- 2. chunk reduce, 3 and 8 sources ---------------------------------------------------
@pytest.mark.parametrize("misalign", [0, 1], ids=["pack+tail", "scalar"])
@pytest.mark.parametrize("nsrcs", [3, 8])
@pytest.mark.parametrize("code", CODES)
def test_reduce_fold_of_edge_sources(code, nsrcs, misalign):
    """fn(fn(s0, s1), s2)... in ReduceOrCopyMulti's order, every op."""
    bad = {}
    for op in OPS:
        srcs, ref = fold_case(code, op, nsrcs)
        got = run_reduce(srcs, code, op, misalign=misalign)
        if _diff(code, got, ref):
            bad[op] = _diff(code, got, ref)
    assert not bad


# ---- 3. / 4. ring and direct kernels on the virtual node ---------------------------------
_expected = {}


def expected_ring(comm0, inputs, code, op, key):
    """Per-rank outputs of the FIFO simulation under ref_op, for the channels,
    thread count and rings the planner gives this bucket."""
    count = inputs[0].size
    nbytes = count * vnode.ESIZE[code]
    nch, nthr, rings = vnode.Planner(comm0.nchannels, comm0.rings()).select(nbytes, nbytes)
    key = (key, code, op, nch, nthr, str(rings))
    if key not in _expected:
        outs = ring_sim.simulate(list(inputs), op, nch, nthr, ring=rings, fn=lambda o, a, b: E.ref_op(code, o, a, b))
        for o in outs:
            _, live = E.same_bits(code, o, o)
            assert live >= 0.75, (code, op, live)
        _expected[key] = outs
    return _expected[key]


def ring_inputs(n, code, op):
    if n == 2:  # rank 0 holds x, rank 1 holds y
        x, y, _ = pair_case(code, op)
        return [x, y]
    return list(fold_case(code, op, n)[0])


def run_misaligned(comms, inputs, code, op, off):
    """As test_gpu_ring.test_allreduce_misaligned_buffers: send and receive
    buffers `off` bytes past a 16-byte boundary."""
    import torch

    n, count, nbytes = len(comms), inputs[0].size, inputs[0].nbytes
    sbuf = [torch.zeros(nbytes + 64, dtype=torch.uint8, device="cuda") for _ in range(n)]
    rbuf = [torch.zeros(nbytes + 64, dtype=torch.uint8, device="cuda") for _ in range(n)]
    for r in range(n):
        sbuf[r][off:off + nbytes].copy_(torch.from_numpy(inputs[r].view(np.uint8).copy()).cuda())
    with C.group():
        for r in range(n):
            C.all_reduce(comms[r], sbuf[r].data_ptr() + off, rbuf[r].data_ptr() + off, count, code, op)
    for c in comms:
        c.sync()
    return [rbuf[r][off:off + nbytes].cpu().numpy().view(inputs[0].dtype) for r in range(n)]


def sweep(comms, n, codes, want_algo, misaligned=False):
    """Every dtype x op of `codes` on one communicator set; returns the failures."""
    bad = {}
    for code in codes:
        for op in OPS:
            inputs = ring_inputs(n, code, op)
            if misaligned:
                outs = run_misaligned(comms, inputs, code, op, vnode.ESIZE[code])
            else:
                outs = vnode.run_allreduce(comms, inputs, code, op)
            algos = {c.last_algo() for c in comms}
            assert algos == {want_algo}, (code, op, algos)
            exp = expected_ring(comms[0], inputs, code, op, n)
            for r in range(n):
                d = _diff(code, outs[r], exp[r])
                if d:
                    bad[(code, op, r)] = d
    return bad


@pytest.mark.parametrize("misaligned", [False, True], ids=["aligned", "misaligned"])
def test_ring_edge_pairs_two_ranks(misaligned):
    comms = C.init_all([0] * 2, C.CommConfig(**RING_ONLY))
    try:
        assert not sweep(comms, 2, CODES, "ring", misaligned)
    finally:
        vnode.destroy(comms)


def test_ring_edge_sources_four_ranks():
    comms = C.init_all([0] * 4, C.CommConfig(**RING_ONLY))
    try:
        assert not sweep(comms, 4, RING4_CODES, "ring")
    finally:
        vnode.destroy(comms)


def _cfg(variant):
    """One direct kernel per communicator set, as test_gpu_direct._cfg."""
    return C.CommConfig(direct_bytes=DIRECT if variant == "direct" else -1,
                        oneshot_bytes=DIRECT if variant in ("oneshot", "ll") else -1,
                        ll_bytes=LL_MAX if variant == "ll" else -1)


@pytest.mark.parametrize("n", [2, 4])
@pytest.mark.parametrize("variant", ["direct", "oneshot", "ll"])
def test_direct_kernels_edge_values(variant, n):
    """The direct kernels reduce in the ring's order, so the ring simulation
    is their expected output too.  Every bucket here is below 1 MiB: the LL
    communicator really runs LL (last_algo is asserted for every call)."""
    comms = C.init_all([0] * n, _cfg(variant))
    try:
        assert not sweep(comms, n, CODES if n == 2 else RING4_CODES, variant)
    finally:
        vnode.destroy(comms)
