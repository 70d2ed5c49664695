"""CPU: the independent element reference (tests/elem_ref.py) checked against
itself, then the C oracle and the host ring checked against it on edge values.

elem_ref.ref_op is written from the reference's functor table and shares no
code and no binary32 detour with oracle/mccs_oracle.c, csrc/dtypes.h or
host_ring.cpp, so a misreading common to those three shows up here: float and
double Max/Min are fmaxf/fminf/fmax/fmin (reduce_kernel.h:435-463: a NaN
operand is dropped whichever side it is on, +0 > -0 in either order), not the
generic (x < y) ? y : x.
"""
from fractions import Fraction

import numpy as np
import pytest

import elem_ref as E
import ring_sim
from mccs_amd import comm as C

CODES = list(range(10))
OPS = [E.SUM, E.PROD, E.MAX, E.MIN]


# ---- self-checks of the reference ---------------------------------------------------
def test_round_rne_round_trips_every_fp16_pattern():
    p, emin, emax, _, sign, inf = E.fp_fields(6)
    for b in range(1 << 16):
        s, v = E.decode(6, b)
        if isinstance(v, str):
            continue
        assert (sign if s else 0) | E.round_rne(v, p, emin, emax) == b, hex(b)
        assert float(v) == abs(float(np.array([b], np.uint16).view(np.float16)[0])), hex(b)


def test_round_rne_matches_numpy_fp16_and_torch_bfloat16():
    import torch

    rng = np.random.default_rng(1)
    f32 = np.concatenate([E.random_bits(7, 20000, rng), E.edge_values(7),
                          # every bf16 tie and near-tie around a few exponents
                          (np.arange(0x3F7F0000, 0x3F7F0000 + 0x30000, 0x4000, dtype=np.uint32)).view(np.float32),
                          np.array([0x7F7F8000, 0x7F7F7FFF, 0x00008000, 0x00008001, 0x00004000], np.uint32).view(np.float32)])
    f32 = f32[~np.isnan(f32) & ~np.isinf(f32)]
    want_bf = torch.from_numpy(f32.copy()).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    with np.errstate(over="ignore"):
        want_h = f32.astype(np.float16).view(np.uint16)
    for x, wb, wh in zip(f32.tolist(), want_bf.tolist(), want_h.tolist()):
        v = Fraction(x)
        neg = np.signbit(x)
        assert (0x8000 if neg else 0) | E.round_rne(v, 8, -126, 127) == wb, (x, hex(wb))
        assert (0x8000 if neg else 0) | E.round_rne(v, 11, -14, 15) == wh, (x, hex(wh))


def _enc(code, values):
    """Exactly representable Python floats -> storage of the dtype."""
    a = np.array(values, np.float64)
    if code == 9:
        return (a.astype(np.float32).view(np.uint32) >> 16).astype(np.uint16)
    return a.astype(E.NPDT[code])


NAN, INF = float("nan"), float("inf")
# (op, x, y, fn(x, y)) written out by hand: CUDA fmaxf/fminf and IEEE +, *
TABLE = [
    (E.MAX, NAN, 1.0, 1.0), (E.MAX, 1.0, NAN, 1.0), (E.MIN, NAN, 1.0, 1.0), (E.MIN, 1.0, NAN, 1.0),
    (E.MAX, NAN, NAN, NAN), (E.MIN, NAN, NAN, NAN), (E.MAX, NAN, -0.0, -0.0), (E.MIN, -INF, NAN, -INF),
    (E.MAX, 0.0, -0.0, 0.0), (E.MAX, -0.0, 0.0, 0.0), (E.MIN, 0.0, -0.0, -0.0), (E.MIN, -0.0, 0.0, -0.0),
    (E.MAX, -0.0, -0.0, -0.0), (E.MIN, 0.0, 0.0, 0.0), (E.MAX, -INF, INF, INF), (E.MIN, 2.0, -3.0, -3.0),
    (E.SUM, -0.0, -0.0, -0.0), (E.SUM, 0.0, -0.0, 0.0), (E.SUM, 1.0, -1.0, 0.0), (E.SUM, INF, -INF, NAN),
    (E.PROD, -0.0, 1.0, -0.0), (E.PROD, -0.0, -1.0, 0.0), (E.PROD, INF, 0.0, NAN), (E.PROD, -2.0, INF, -INF),
]


@pytest.mark.parametrize("code", E.FP_CODES)
def test_zero_and_nan_table(code):
    for op, x, y, want in TABLE:
        got = E.ref_op(code, op, _enc(code, [x]), _enc(code, [y]))
        ok, _ = E.same_bits(code, got, _enc(code, [want]))
        assert ok, (code, op, x, y, want, E.bits_of(code, got))


def test_fp16_targeted_pairs_by_hand():
    """The issue's fp16 examples: 2048 + 1 ties down, 2048 + 3 ties up,
    65504 + 16 ties into Inf, 65504 + 15 does not; 2^-24 * 1.5 ties up to
    2 * 2^-24, 2^-24 * 0.5 ties down to 0."""
    h = lambda *v: np.array(v, np.float16)  # noqa: E731
    assert E.ref_op(6, E.SUM, h(2048, 2048, 65504, 65504), h(1, 3, 16, 15)).tolist() == [2048, 2052, INF, 65504]
    s = 2.0 ** -24
    assert E.ref_op(6, E.PROD, h(s, s, s, -s), h(1.5, 0.5, 2.5, 0.5)).view(np.uint16).tolist() == [2, 0, 2, 0x8000]


@pytest.mark.parametrize("code", [6, 7, 8])
@pytest.mark.parametrize("op", [E.SUM, E.PROD])
def test_exact_rational_route_agrees_with_native_route(code, op):
    """Sum/Prod through Fractions and round_rne (bf16's route) equals the
    native route of the other three types on the whole edge cross product."""
    x, y = E.edge_pairs(code)
    x, y = x[:-E.N_RANDOM + 500], y[:-E.N_RANDOM + 500]
    ok, _ = E.same_bits(code, E.exact_op(code, op, x, y), E.ref_op(code, op, x, y))
    assert ok


def test_integers_wrap_and_keep_signedness():
    i32 = lambda *v: np.array(v, np.int64).astype(np.int32)  # noqa: E731
    assert E.ref_op(2, E.SUM, i32(2**31 - 1), i32(1)).tolist() == [-2**31]
    assert E.ref_op(2, E.PROD, i32(46341), i32(46341)).tolist() == [46341 * 46341 - 2**32]
    assert E.ref_op(2, E.MAX, i32(-1), i32(1)).tolist() == [1]
    u = np.array([0xFFFFFFFF], np.uint32)
    assert E.ref_op(3, E.MAX, u, np.array([1], np.uint32)).tolist() == [0xFFFFFFFF]
    a = np.array([0xFFFFFFFF00000000], np.uint64)
    assert E.ref_op(5, E.SUM, a, np.array([1 << 32], np.uint64)).tolist() == [0]
    assert E.ref_op(4, E.MIN, a.view(np.int64), np.array([1], np.int64)).tolist() == [-(1 << 32)]
    assert E.ref_op(5, E.MIN, a, np.array([1], np.uint64)).tolist() == [1]
    assert E.ref_op(4, E.PROD, np.array([1 << 32], np.int64), np.array([1 << 31], np.int64)).tolist() == [-2**63]


# ---- the inputs of the GPU edge tests are not vacuous -------------------------------
@pytest.mark.parametrize("code", CODES)
def test_edge_inputs_reach_every_targeted_class(code):
    """For every op: at least 75 % of the reference output is non-NaN, and
    every targeted class (subnormal result, tie, overflow to Inf, -0, integer
    wrap) occurs -- for the pairs and for the 3-, 4- and 8-source folds."""
    v = E.edge_values(code)
    assert v.size <= 128
    x, y = E.edge_pairs(code)
    assert x.size == y.size == v.size ** 2 + E.N_RANDOM and v.size ** 2 <= 16384
    for op in OPS:
        r = E.ref_op(code, op, x, y)
        _, live = E.same_bits(code, r, r)
        assert live >= 0.75, (op, live)
        assert E.result_classes(code, op, x, y, r) >= E.required_classes(code, op), op
        for nsrcs in (3, 4, 8):
            srcs = E.edge_sources(code, nsrcs, op)
            r, classes = E.fold_classes(code, op, srcs)
            _, live = E.same_bits(code, r, r)
            assert live >= 0.75, (op, nsrcs, live)
            assert classes >= E.required_classes(code, op), (op, nsrcs, classes)


# ---- the oracle and the host ring against the reference ------------------------------
def _assert_same(code, got, ref, what):
    ok, live = E.same_bits(code, got, ref)
    if not ok:
        bad = E.mismatches(code, got, ref)
        raise AssertionError(f"{what}: {bad.size} of {ref.size} differ, first at {bad[:6].tolist()}: got "
                             f"{E.bits_of(code, got)[bad[:6]].tolist()} want {E.bits_of(code, ref)[bad[:6]].tolist()}")
    assert live >= 0.75


@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("code", CODES)
def test_oracle_apply_matches_reference_on_edge_pairs(orc, code, op):
    x, y = E.edge_pairs(code)
    _assert_same(code, orc.apply(code, op, x, y), E.ref_op(code, op, x, y), f"oracle dtype {code} op {op}")


@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("code", CODES)
def test_host_ring_matches_reference_at_two_ranks(code, op):
    """Rank 0 holds x, rank 1 holds y; two channels, so both operand orders
    fn(x, y) and fn(y, x) occur.  Expected: the per-rank FIFO simulation with
    ref_op as its functor."""
    x, y = E.edge_pairs(code)
    nch, nthr = 2, 160
    outs = [np.zeros_like(x), np.zeros_like(x)]
    C.host_ring_allreduce([x.copy(), y.copy()], outs, x.size, code, op, channels=nch, nthreads=nthr)
    exp = ring_sim.simulate([x, y], op, nch, nthr, fn=lambda o, a, b: E.ref_op(code, o, a, b))
    for r in range(2):
        _assert_same(code, outs[r], exp[r], f"host ring rank {r} dtype {code} op {op}")
