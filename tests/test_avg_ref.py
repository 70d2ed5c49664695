"""CPU: pins tests/avg_ref.py itself (the reference the PreMulSum / SumPostDiv /
Avg tests compare against): the Avg scalars against exact rationals, truncation
on negative sums, wrap before divide, scalar decoding from the low bytes, and
that the library's host-side mapping (mccsAvgOp, mccsRedOpArgFromDouble)
returns the same values.
"""
from fractions import Fraction

import numpy as np
import pytest

import avg_ref as A
import elem_ref as E
from mccs_amd import comm as C

F16, F32, F64, BF16 = 6, 7, 8, 9


@pytest.mark.parametrize("n", [2, 3, 7, 8])
@pytest.mark.parametrize("code", [F16, F32, F64, BF16])
def test_avg_scalar_against_exact_rationals(code, n):
    p, emin, _, _, _, _ = E.fp_fields(code)
    bits = A.avg_scalar_bits(code, n)
    sign, v = E.decode(code, bits)
    assert sign == 0 and not isinstance(v, str)
    exact = Fraction(1, n)
    # within half an ulp of 1/n (a whisker more for the 16-bit types, rounded through binary32)
    e = -n.bit_length() if (1 << (n.bit_length() - 1)) != n else -(n.bit_length() - 1)
    ulp = Fraction(2) ** (e - p + 1)
    slack = Fraction(2) ** (e - 23) / 2 if code in (F16, BF16) else 0
    assert abs(v - exact) <= ulp / 2 + slack, (code, n, v)
    if n in (2, 8):
        assert v == exact
    # and the host's own arithmetic agrees for the two formats numpy divides in
    if code == F32:
        assert bits == int(np.array(np.float32(1.0) / np.float32(n), np.float32).view(np.uint32))
    if code == F64:
        assert bits == int(np.array(1.0 / n, np.float64).view(np.uint64))
    if code == F16:
        assert bits == int(np.array(np.float32(1.0) / np.float32(n), np.float32).astype(np.float16).view(np.uint16))
    assert A.avg_op(code, n) == (A.PREMULSUM, bits)


def test_avg_integers_divide_by_nranks():
    for code in E.INT_CODES:
        assert A.avg_op(code, 5) == (A.SUMPOSTDIV, 5)


def test_post_truncates_toward_zero():
    x = np.array([-7, -6, -1, 0, 1, 6, 7, -128, 127], np.int8)
    assert A.post(0, x, 3).tolist() == [-2, -2, 0, 0, 0, 2, 2, -42, 42]
    assert (x // 3).tolist() != A.post(0, x, 3).tolist()  # numpy floors
    x = np.array([-7, 7, -(1 << 31)], np.int32)
    assert A.post(2, x, 2).tolist() == [-3, 3, -(1 << 30)]
    x = np.array([-(1 << 63), -9, 9], np.int64)
    assert A.post(4, x, 7).tolist() == [-((1 << 63) // 7), -1, 1]


def test_post_unsigned_and_wrap_before_divide():
    # the sum wraps in T first: 200 + 100 = 44 in uint8, / 3 = 14
    s = E.ref_op(1, E.SUM, np.array([200], np.uint8), np.array([100], np.uint8))
    assert A.post(1, s, 3).tolist() == [14]
    s = E.ref_op(0, E.SUM, np.array([100], np.int8), np.array([100], np.int8))  # -56
    assert A.post(0, s, 3).tolist() == [-18]
    x = np.array([(1 << 32) - 1], np.uint32)
    assert A.post(3, x, 2).tolist() == [(1 << 31) - 1]
    x = np.array([(1 << 64) - 1], np.uint64)
    assert A.post(5, x, A.INT32_MAX).tolist() == [((1 << 64) - 1) // A.INT32_MAX]


def test_scalar_comes_from_the_low_bytes():
    arg = 0x1122334455667788
    assert A.scalar_bits(0, arg) == 0x88 and A.scalar(0, arg)[0] == np.int8(-120)
    assert A.scalar_bits(3, arg) == 0x55667788
    assert A.scalar_bits(5, arg) == arg
    assert A.scalar_bits(BF16, 0x3F80) == 0x3F80 and A.scalar_bits(F16, 0xABCD3C00) == 0x3C00
    assert A.divisor(7) == 7 and A.divisor(0xFFFFFFFF) == -1


def test_pre_rounds_once_and_wraps():
    third = A.avg_scalar_bits(F32, 3)
    x = np.array([3.0, 1.0, 0.1], np.float32)
    want = x * np.array(third, np.uint32).view(np.float32)
    assert np.array_equal(A.pre(F32, x, third).view(np.uint32), want.view(np.uint32))
    x = np.array([100, -3, 127], np.int8)
    assert A.pre(0, x, 3).tolist() == [44, -9, 125]
    assert A.pre(0, x, 0xFF).tolist() == [-100, 3, -127]  # -1
    assert A.pre(1, np.array([200], np.uint8), 255).tolist() == [56]
    # bf16: 1/3 (0x3eab) * 3 = 1.00195.. -> 1.0 after one rounding
    assert A.pre(BF16, np.array([0x4040], np.uint16), A.avg_scalar_bits(BF16, 3)).tolist() == [0x3F80]


def test_encode():
    assert A.encode(F32, 3) == 0x40400000 and A.encode(F16, 3) == 0x4200 and A.encode(BF16, 3) == 0x4040
    assert A.encode(F64, Fraction(-1, 2)) == 0xBFE0000000000000
    assert A.encode(0, -1) == 0xFF and A.encode(4, -1) == (1 << 64) - 1 and A.encode(3, 3) == 3


def test_library_mapping_matches():
    """mccsAvgOp and mccsRedOpArgFromDouble return avg_ref's values."""
    for code in range(10):
        for n in (1, 2, 3, 7, 8, 64):
            op, arg = C.avg_op(code, n)
            assert (int(op), arg) == A.avg_op(code, n), (code, n, hex(arg))
    for code in (F16, F32, F64, BF16):
        for v in (3.0, -0.5, 1.0, 0.0):
            assert C.red_op_arg(code, v) == A.encode(code, Fraction(v)), (code, v)
        assert C.red_op_arg(code, 1.0 / 3) == (A.avg_scalar_bits(code, 3) if code != F64 else A.avg_scalar_bits(F64, 3))
    for code in E.INT_CODES:
        for v in (3, 0, 1):
            assert C.red_op_arg(code, v) == A.encode(code, v)
    for code in A.SIGNED:
        assert C.red_op_arg(code, -1) == A.encode(code, -1)
    assert C.red_op_arg(1, 255) == 255 and C.red_op_arg(0, -128) == 0x80


def test_red_op_arg_refuses_what_the_type_cannot_hold():
    from mccs_amd._lib import MccsError

    for code, v in ((0, 128), (0, -129), (1, -1), (1, 256), (2, 0.5), (3, -1), (3, float(1 << 32)), (5, -1.0),
                    (4, float(1 << 63)), (2, float("nan")), (10, 1.0), (-1, 1.0)):
        with pytest.raises(MccsError) as ei:
            C.red_op_arg(code, v)
        assert ei.value.code == 4, (code, v)
