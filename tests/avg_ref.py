"""Test helper: expected values of PreMulSum, SumPostDiv and Avg (test-only, CPU).

Built on tests/elem_ref.py alone (not on oracle/ and not on the library):

  pre    PreMulSum's step on a rank's own input, x * s rounded once in the
         type.  fp: elem_ref.ref_op(code, PROD, x, s), an exact-rational or
         host-IEEE product rounded once; integers: the product modulo 2^w.
         s is the low sizeof(T) bytes of the 64-bit op argument.
  post   SumPostDiv's step on the finished sum, T(x / n) with n = (int)op_arg:
         C division, truncating toward zero (numpy's // floors), computed in
         Python integers; n converts to unsigned for uint32 / uint64.
  Avg    floating types: PreMulSum with s = 1/n (fp64: RNE(1/n); fp32: RNE to
         binary32; fp16 / bf16: that binary32 value rounded once more to the
         type); integer types: SumPostDiv with n = nranks.

Expected results come from two identities (include/mccs_hip.h): a PreMulSum
collective is the Sum collective over elementwise pre-scaled inputs, and a
SumPostDiv collective is post applied elementwise to the Sum collective's
output.  The Sum schedules are rs_ref.expected, rooted_ref.reduce_expected
(both under rs_ref.ELEM_REF) and ring_sim.simulate with elem_ref.ref_op.
"""
from __future__ import annotations

from fractions import Fraction

import numpy as np

import elem_ref as E
import ring_sim
import rooted_ref
import rs_ref

PREMULSUM, SUMPOSTDIV = 4, 5
INT32_MAX = (1 << 31) - 1
SIGNED = (0, 2, 4)


# ---- the op argument -----------------------------------------------------------------
def scalar_bits(code, op_arg):
    """The PreMulSum scalar's bit pattern: the low sizeof(T) bytes of op_arg."""
    return int(op_arg) & ((1 << E.width(code)) - 1)


def scalar(code, op_arg, size=1):
    """The scalar as a storage array of `size` equal elements."""
    return E.from_bits(code, [scalar_bits(code, op_arg)] * size)


def divisor(op_arg):
    """SumPostDiv's n = (int)op_arg."""
    v = int(op_arg) & 0xFFFFFFFF
    return v - (1 << 32) if v >> 31 else v


def encode(code, value):
    """op_arg of an exactly representable PreMulSum scalar: a Fraction / int for
    fp types (asserted exact), an int taken modulo 2^w for integer types."""
    if not E.is_fp(code):
        return int(value) & ((1 << E.width(code)) - 1)
    p, emin, emax, _, sign, _ = E.fp_fields(code)
    v = Fraction(value)
    b = E.round_rne(v, p, emin, emax)
    assert E.decode(code, b)[1] == abs(v), (code, value)
    return b | (sign if v < 0 else 0)


def _rne_value(code, v):
    """The positive rational v rounded to nearest even in format `code`: (bits, value)."""
    p, emin, emax, _, _, _ = E.fp_fields(code)
    b = E.round_rne(v, p, emin, emax)
    return b, E.decode(code, b)[1]


def avg_scalar_bits(code, n):
    """Bits of the Avg scalar 1/n: rounded to the type directly for fp64 and
    fp32, through binary32 for fp16 and bf16 (1.0f / (float)n, then once more)."""
    v = Fraction(1, n)
    if code in (7, 8):
        return _rne_value(code, v)[0]
    return _rne_value(code, _rne_value(7, v)[1])[0]


def avg_op(code, n):
    """(op, op_arg) of the average over n ranks."""
    if E.is_fp(code):
        return PREMULSUM, avg_scalar_bits(code, n)
    return SUMPOSTDIV, n


PAIRS = [(code, PREMULSUM) for code in range(10)] + [(code, SUMPOSTDIV) for code in E.INT_CODES]  # the sixteen


def case_args(code, op, n):
    """The two op arguments the value tests run each (dtype, op) pair with.
    PreMulSum: fp the Avg scalar and 3.0 (no power of two), signed integers 3
    and -1, unsigned 3 and the type's maximum; SumPostDiv: n and 7."""
    if op == SUMPOSTDIV:
        return [n, 7]
    if E.is_fp(code):
        return [avg_scalar_bits(code, n), encode(code, 3)]
    return [encode(code, 3), encode(code, -1)]  # -1 is the unsigned types' maximum


# ---- pre and post ---------------------------------------------------------------------
def pre(code, x, op_arg):
    x = np.ascontiguousarray(x).view(E.NPDT[code])
    return E.ref_op(code, E.PROD, x, scalar(code, op_arg, x.size))


def _trunc_div(a, n):
    q = abs(a) // abs(n)
    return q if (a < 0) == (n < 0) else -q


def post(code, x, op_arg):
    assert not E.is_fp(code), "SumPostDiv is defined for the integer types only"
    n = divisor(op_arg)
    w = E.width(code)
    if code in (3, 5):  # uint32 / uint64: n converts to unsigned
        n &= (1 << w) - 1
    vals = np.ascontiguousarray(x).view(E.NPDT[code]).tolist()
    return E.from_bits(code, [_trunc_div(a, n) & ((1 << w) - 1) for a in vals])


def apply_one(code, op, op_arg, x):
    """post(pre(x)): the result at nranks == 1."""
    if op == PREMULSUM:
        return pre(code, x, op_arg)
    if op == SUMPOSTDIV:
        return post(code, x, op_arg)
    return np.ascontiguousarray(x).view(E.NPDT[code]).copy()


def _inputs(code, op, op_arg, inputs):
    return [pre(code, x, op_arg) for x in inputs] if op == PREMULSUM else [np.ascontiguousarray(x) for x in inputs]


def _outputs(code, op, op_arg, out):
    return post(code, out, op_arg) if op == SUMPOSTDIV else out


def _sum_fn(code):
    return lambda op, x, y: E.ref_op(code, op, x, y)


# ---- the three collectives --------------------------------------------------------------
def allreduce_expected(inputs, code, op, op_arg, nch, nthr, rings, buff_size=1 << 22):
    """Per-rank outputs.  rings: one order per selected channel."""
    if len(inputs) == 1:
        return [apply_one(code, op, op_arg, inputs[0])]
    outs = ring_sim.simulate(_inputs(code, op, op_arg, inputs), E.SUM, nch, nthr, buff_size, ring=rings,
                             fn=_sum_fn(code))
    return [_outputs(code, op, op_arg, o) for o in outs]


def reduce_scatter_expected(inputs, code, op, op_arg, nch, nthr, rings, buff_size=1 << 22):
    outs = rs_ref.expected(rs_ref.ELEM_REF, _inputs(code, op, op_arg, inputs), code, E.SUM, nch, nthr, rings,
                           buff_size)
    return [_outputs(code, op, op_arg, o) for o in outs]


def reduce_expected(inputs, code, op, op_arg, root, nch, nthr, rings, buff_size=1 << 22):
    out = rooted_ref.reduce_expected(rs_ref.ELEM_REF, _inputs(code, op, op_arg, inputs), code, E.SUM, root, nch,
                                     nthr, rings, buff_size)
    return _outputs(code, op, op_arg, out)


def sum_allreduce_expected(inputs, code, nch, nthr, rings, buff_size=1 << 22):
    """The plain Sum AllReduce (the control the new ops must differ from)."""
    return allreduce_expected(inputs, code, E.SUM, 0, nch, nthr, rings, buff_size)


# ---- the single-rounding alternative (the contraction fault) ----------------------------
def fused_first_hop(code, x, op_arg, acc):
    """round(x * s + acc) in exact arithmetic, one rounding: what a fused
    multiply-add computes where the contract demands round(round(x * s) + acc).
    Finite operands only (the rounding test's inputs)."""
    p, emin, emax, _, sign, inf = E.fp_fields(code)
    _, s = E.decode(code, scalar_bits(code, op_arg))
    sneg = bool(scalar_bits(code, op_arg) & sign)
    out = []
    for xb, ab in zip(E.bits_of(code, x).tolist(), E.bits_of(code, acc).tolist()):
        (sx, xv), (sa, av) = E.decode(code, xb), E.decode(code, ab)
        assert not isinstance(xv, str) and not isinstance(av, str)
        v = (-xv if sx != sneg else xv) * s + (-av if sa else av)
        out.append(0 if v == 0 else (sign if v < 0 else 0) | E.round_rne(v, p, emin, emax))
    return E.from_bits(code, out)
