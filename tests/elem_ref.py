"""Independent two-operand reference of the element functors (test-only, CPU).

Written from the reference's functor table (src/collectives/src/
reduce_kernel.h), not from oracle/mccs_oracle.c, and without the assumption
the oracle and the kernels share (half types computed through binary32):

  integers        Sum/Prod modulo 2^w, Max/Min in the type's signedness
                  (:16-46, :72-235 for the byte types)
  fp32 / fp64     Sum/Prod are the host's IEEE add/multiply (numpy); Max/Min
                  are fmaxf/fminf/fmax/fmin (:435-463)
  fp16            Sum/Prod computed exactly in binary64 (every fp16 value is a
                  multiple of 2^-24 below 2^16: a sum needs 42 bits, a product
                  22) and rounded once by numpy's binary64 -> binary16
  bf16            Sum/Prod computed in exact rationals and rounded once by
                  round_rne below
  Max/Min, fp     CUDA fmaxf/fminf rules on the bit patterns: one NaN operand
                  yields the other operand, two NaNs yield NaN, +0 > -0
                  whatever the operand order (:338-463)

Arrays are raw storage (oracle.NP_DTYPE): bf16 is uint16 bits.  NaN results
are compared as "is NaN" only (same_bits); inputs carry quiet NaNs only.
"""
from __future__ import annotations

from fractions import Fraction
from functools import lru_cache

import numpy as np

SUM, PROD, MAX, MIN = 0, 1, 2, 3
NPDT = {0: np.int8, 1: np.uint8, 2: np.int32, 3: np.uint32, 4: np.int64, 5: np.uint64, 6: np.float16,
        7: np.float32, 8: np.float64, 9: np.uint16}
UINT = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}
# fp formats: code -> (significand bits p incl. the hidden one, emin, emax)
FMT = {6: (11, -14, 15), 7: (24, -126, 127), 8: (53, -1022, 1023), 9: (8, -126, 127)}
FP_CODES, INT_CODES = (6, 7, 8, 9), (0, 1, 2, 3, 4, 5)

# The fp32/fp64 references below are the host's own add and multiply: they
# must not flush subnormals.
assert np.float32(1e-45) * np.float32(1) != 0 and np.float64(5e-324) * np.float64(1) != 0


def is_fp(code):
    return code in FMT


def width(code):
    return np.dtype(NPDT[code]).itemsize * 8


def bits_of(code, a):
    """Raw storage -> unsigned integer bit patterns (a view)."""
    a = np.ascontiguousarray(a)
    return a.view(UINT[a.dtype.itemsize])


def from_bits(code, bits):
    """Python ints / unsigned array of bit patterns -> storage array."""
    u = UINT[np.dtype(NPDT[code]).itemsize]
    return np.array(bits, dtype=u).view(NPDT[code])


# ---- a generic round-to-nearest-even --------------------------------------------
def _units(v, p, emin):
    """v > 0 as n + twice/(2 den) units of the last place at its exponent e."""
    e = v.numerator.bit_length() - v.denominator.bit_length()  # floor(log2 v) or one above
    if Fraction(2) ** e > v:
        e -= 1
    e = max(e, emin)  # subnormals share emin's quantum
    q = v / Fraction(2) ** (e - p + 1)
    n, rem = divmod(q.numerator, q.denominator)
    return e, n, 2 * rem, q.denominator


def round_rne(value, p, emin, emax):
    """Bit pattern, without the sign, of |value| (an exact rational) rounded to
    nearest, ties to even, in the binary format with p significand bits and
    normal exponents emin..emax; overflow gives the Inf pattern."""
    v = abs(Fraction(value))
    if v == 0:
        return 0
    e, n, twice, den = _units(v, p, emin)
    if twice > den or (twice == den and (n & 1)):
        n += 1
    # subnormal: n < 2^(p-1), pattern n; normal: hidden bit adds one to the
    # exponent field; n == 2^p carries into the next exponent by itself
    bits = ((e - emin) << (p - 1)) + n
    return min(bits, (emax - emin + 2) << (p - 1))


def fp_fields(code):
    p, emin, emax = FMT[code]
    w = width(code)
    sign = 1 << (w - 1)
    inf = (emax - emin + 2) << (p - 1)
    return p, emin, emax, w, sign, inf


def decode(code, b):
    """One bit pattern -> (sign, 'nan' | 'inf' | exact Fraction magnitude)."""
    p, emin, _, _, sign, inf = fp_fields(code)
    s, m = int(b & sign != 0), b & (sign - 1)
    if m > inf:
        return s, "nan"
    if m == inf:
        return s, "inf"
    ef, frac = m >> (p - 1), m & ((1 << (p - 1)) - 1)
    if ef == 0:
        return s, Fraction(frac) * Fraction(2) ** (emin - p + 1)
    return s, Fraction(frac + (1 << (p - 1))) * Fraction(2) ** (ef - 1 + emin - p + 1)


def qnan(code):
    p, _, _, _, _, inf = fp_fields(code)
    return inf | (1 << (p - 2))


def _exact_op(code, op, xb, yb):
    """Sum / Prod of two bit patterns in exact rationals, rounded once."""
    p, emin, emax, _, sign, inf = fp_fields(code)
    (sx, x), (sy, y) = decode(code, xb), decode(code, yb)
    if x == "nan" or y == "nan":
        return qnan(code)
    if op == SUM:
        if x == "inf" or y == "inf":
            if x == "inf" and y == "inf" and sx != sy:
                return qnan(code)
            return (sign if (sx if x == "inf" else sy) else 0) | inf
        v = (-x if sx else x) + (-y if sy else y)
        if v == 0:  # exact zero: -0 only from -0 + -0 (round to nearest)
            return sign if (sx and sy) else 0
        return (sign if v < 0 else 0) | round_rne(v, p, emin, emax)
    s = sx ^ sy
    if x == "inf" or y == "inf":
        if x == 0 or y == 0:
            return qnan(code)
        return (sign if s else 0) | inf
    return (sign if s else 0) | round_rne(x * y, p, emin, emax)


@lru_cache(maxsize=None)
def _bf16_op(op, xb, yb):
    return _exact_op(9, op, xb, yb)


def exact_op(code, op, x, y):
    """Sum / Prod through exact rationals for any fp type (slow; bf16's route,
    and a cross-check of the other three)."""
    xb, yb = bits_of(code, x), bits_of(code, y)
    f = _bf16_op if code == 9 else (lambda o, a, b: _exact_op(code, o, a, b))
    return from_bits(code, [f(op, int(a), int(b)) for a, b in zip(xb.tolist(), yb.tolist())])


# ---- fmax / fmin on bit patterns --------------------------------------------------
def isnan_bits(code, a):
    _, _, _, _, sign, inf = fp_fields(code)
    b = bits_of(code, a)
    return (b & b.dtype.type(sign - 1)) > b.dtype.type(inf)


def _order_key(code, b):
    """Monotone unsigned key of a non-NaN pattern: -Inf < ... < -0 < +0 < ... < +Inf."""
    _, _, _, w, sign, _ = fp_fields(code)
    t = b.dtype.type
    return np.where(b & t(sign), ~b, b | t(sign))


def _fmaxmin(code, op, x, y):
    xb, yb = bits_of(code, x), bits_of(code, y)
    nx, ny = isnan_bits(code, x), isnan_bits(code, y)
    kx, ky = _order_key(code, xb), _order_key(code, yb)
    pick_x = (kx >= ky) if op == MAX else (kx <= ky)  # equal keys are equal bits
    r = np.where(nx, yb, np.where(ny, xb, np.where(pick_x, xb, yb)))  # two NaNs: y, a NaN
    return r.view(NPDT[code])


# ---- the reference ------------------------------------------------------------------
def ref_op(code, op, x, y):
    """fn(x, y) elementwise on raw storage arrays; returns storage of the same type."""
    npdt = NPDT[code]
    x = np.ascontiguousarray(x).view(npdt)
    y = np.ascontiguousarray(y).view(npdt)
    if not is_fp(code):
        if op in (SUM, PROD):
            u = UINT[x.dtype.itemsize]
            xu, yu = x.view(u), y.view(u)
            return (xu + yu if op == SUM else xu * yu).view(npdt)  # unsigned arrays wrap mod 2^w
        return np.maximum(x, y) if op == MAX else np.minimum(x, y)
    if op in (MAX, MIN):
        return _fmaxmin(code, op, x, y)
    with np.errstate(all="ignore"):
        if code in (7, 8):
            return x + y if op == SUM else x * y
        if code == 6:
            xd, yd = x.astype(np.float64), y.astype(np.float64)
            return (xd + yd if op == SUM else xd * yd).astype(np.float16)
    return exact_op(9, op, x, y)


def same_bits(code, got, ref):
    """got == ref bit for bit, NaNs (fp) compared as "is NaN" only.  Returns
    (ok, fraction of ref that is non-NaN)."""
    g, r = bits_of(code, got), bits_of(code, ref)
    if g.shape != r.shape:
        return False, 0.0
    if not is_fp(code):
        return bool(np.array_equal(g, r)), 1.0
    gn, rn = isnan_bits(code, got), isnan_bits(code, ref)
    ok = np.array_equal(gn, rn) and np.array_equal(g[~rn], r[~rn])
    return bool(ok), float(1.0 - rn.mean()) if rn.size else 1.0


def mismatches(code, got, ref):
    """Indices where same_bits fails (for assertion messages)."""
    g, r = bits_of(code, got), bits_of(code, ref)
    if not is_fp(code):
        return np.flatnonzero(g != r)
    gn, rn = isnan_bits(code, got), isnan_bits(code, ref)
    return np.flatnonzero((gn != rn) | (~rn & (g != r)))


# ---- edge values ---------------------------------------------------------------------
def _fp_edge_bits(code):
    p, emin, emax, w, sign, inf = fp_fields(code)

    def enc(v):  # exactly representable by construction
        b = round_rne(v, p, emin, emax)
        assert decode(code, b)[1] == abs(Fraction(v)), (code, v)
        return b

    two = Fraction(2)
    sub_min, sub_max, norm_min, fin_max = 1, (1 << (p - 1)) - 1, 1 << (p - 1), inf - 1
    half_top = two ** (emax - p)  # half an ulp of the largest finite: max + this ties up into Inf
    mags = [
        0, sub_min, sub_max, norm_min, fin_max, inf, enc(1),
        # Sum ties: 2^p + 1 ties down to 2^p (even), 2^p + 3 ties up to 2^p + 4
        enc(two ** p), enc(3), enc(two ** p + 2),
        # Sum into Inf, and just not: largest finite + half its ulp, and + the value below that
        enc(half_top), enc(half_top) - 1,
        # Prod onto subnormal ties: x * smallest subnormal = 0.5, 1.5, 2.5 (ties), 0.75, 0.25 units
        enc(Fraction(1, 2)), enc(Fraction(3, 2)), enc(Fraction(5, 2)), enc(Fraction(3, 4)), enc(Fraction(1, 4)),
        3,  # the subnormal 3 units: * 0.5 ties to 2 units
        norm_min + 1, sub_max - 1, enc(1) + 1, enc(1) - 1,  # neighbours: 1 +- ulp
        # Prod into Inf and just not: 2^ceil((emax+1)/2) squared overflows, the value below does not
        enc(two ** ((emax + 2) // 2)), enc(two ** ((emax + 2) // 2)) - 1, enc(2), fin_max - 1,
        # Prod underflow: 2^(emin/2)-ish squares land at the subnormal boundary
        enc(two ** ((emin - p + 1) // 2)), enc(two ** ((emin - p + 1) // 2 - 1)),
        enc(1) + (1 << (p - 1)) // 3, enc(10),  # 1.33.., 10
    ]
    out = []
    for m in mags:
        out += [m, m | sign]
    out += [qnan(code), qnan(code) | sign | 1]  # quiet NaNs, one with sign and payload
    return out


def _int_edge_bits(code):
    w = width(code)
    full = (1 << w) - 1
    top = 1 << (w - 1)
    alt = [int(("01" * 32)[-w:], 2), int(("10" * 32)[-w:], 2), int(("0011" * 16)[-w:], 2),
           int(("1100" * 16)[-w:], 2), int(("00001111" * 8)[-w:], 2), int(("11110000" * 8)[-w:], 2)]
    vals = [0, 1, full, 2, full - 1, 3, top, top + 1, top - 1, top - 2, full - 2] + alt
    h = 1 << (w // 2)
    vals += [h, h - 1, h + 1, full - h + 1, (1 << (w - 2)), 3 << (w - 2), 7, 10, 100 & full]
    if w == 32:
        vals += [46340, 46341, 65535, 65537]  # squares on either side of 2^31
    if w == 64:
        vals += [(1 << 31) - 1, 1 << 31, (1 << 32) - 1, 1 << 32, 0xFFFFFFFF00000000, 0x00000001FFFFFFFF,
                 0x8000000080000000, 0x7FFFFFFF80000000, 3037000499, 3037000500, 0xFFFFFFFF80000000]
    seen, out = set(), []
    for v in vals:
        if v not in seen:
            seen.add(v)
            out.append(v)
    return out


def edge_values(code):
    """At most 128 edge values of the dtype, as a storage array."""
    bits = _fp_edge_bits(code) if is_fp(code) else _int_edge_bits(code)
    assert len(bits) <= 128 and len(set(bits)) == len(bits), (code, len(bits))
    return from_bits(code, bits)


def random_bits(code, n, rng, exp_span=None):
    """n full-range random bit patterns.  fp: NaN patterns are made quiet; with
    exp_span the unbiased exponent is drawn from [-exp_span, exp_span] (finite
    normal values only), for products of several sources that would otherwise
    all be Inf or 0."""
    w = width(code)
    b = rng.integers(0, 1 << 64, n, dtype=np.uint64, endpoint=False) >> np.uint64(64 - w)
    if is_fp(code):
        p, emin, emax, _, sign, inf = fp_fields(code)
        if exp_span is not None:
            frac = b & np.uint64((1 << (p - 1)) - 1)
            ef = rng.integers(-exp_span, exp_span + 1, n).astype(np.int64) + (1 - emin)
            b = (b & np.uint64(sign)) | (ef.astype(np.uint64) << np.uint64(p - 1)) | frac
        nan = (b & np.uint64(sign - 1)) > np.uint64(inf)
        b = np.where(nan, b | np.uint64(1 << (p - 2)), b)
    return b.astype(UINT[w // 8]).view(NPDT[code])


N_RANDOM = 3001  # odd: with the cross product the count is no multiple of any pack


def edge_pairs(code, seed=0):
    """(x, y): the full cross product of edge_values (at most 16 384 pairs)
    followed by N_RANDOM pairs of random full-range bit patterns."""
    v = edge_values(code)
    rng = np.random.default_rng(1000 + code + seed)
    x = np.concatenate([np.repeat(v, v.size), random_bits(code, N_RANDOM, rng)])
    y = np.concatenate([np.tile(v, v.size), random_bits(code, N_RANDOM, rng)])
    return x, y


def _designed_columns(code, nsrcs):
    """A few fixed leading columns (one row per source) whose fold meets every
    targeted class whatever the op: all -0; zeros of alternating sign; a NaN
    first; all NaN; a Sum tie; a Sum into Inf; a Prod onto a subnormal tie;
    subnormals against zeros."""
    p, emin, emax, w, sign, inf = fp_fields(code)
    one = round_rne(1, p, emin, emax)
    cols = [
        [sign] * nsrcs,
        [sign if s & 1 else 0 for s in range(nsrcs)],
        [0 if s & 1 else sign for s in range(nsrcs)],
        [qnan(code), one] + [one | sign] * (nsrcs - 2),
        [qnan(code)] * nsrcs,
        [round_rne(Fraction(2) ** p, p, emin, emax), one] + [0] * (nsrcs - 2),
        [inf - 1, round_rne(Fraction(2) ** (emax - p), p, emin, emax)] + [sign] * (nsrcs - 2),
        [1, round_rne(Fraction(3, 2), p, emin, emax)] + [one] * (nsrcs - 2),
        [1] + [0] * (nsrcs - 1),
        [1 | sign] + [0] * (nsrcs - 1),
        [sign, 1 | sign] + [sign] * (nsrcs - 2),
    ]
    return np.array(cols, dtype=object).T  # [source][column]


def edge_sources(code, nsrcs, op, seed=0, reps=8, nrandom=N_RANDOM):
    """nsrcs arrays: (fp) the designed columns, then edge_values tiled `reps`
    times and shuffled per source, then random bits.  So that a fold over many
    sources is not mostly NaN, only one element in four carries Inf/NaN in
    every source; the others keep them in two sources (which two rotates with
    the index) and elsewhere clear the top exponent bit.  Prod narrows the
    random part's exponents to +-emax/nsrcs so that products of nsrcs values
    stay finite."""
    v = edge_values(code)
    rng = np.random.default_rng(2000 + 16 * code + nsrcs + seed)
    span = None
    if is_fp(code) and op == PROD:
        span = max(1, FMT[code][2] // nsrcs)
    out = []
    for s in range(nsrcs):
        a = np.concatenate([rng.permutation(np.tile(v, reps)), random_bits(code, nrandom, rng, span)])
        if is_fp(code):
            p, emin, emax, w, sign, inf = fp_fields(code)
            b = bits_of(code, a).copy()
            t = b.dtype.type
            col = np.arange(b.size)
            special = (b & t(sign - 1)) >= t(inf)
            allowed = (col % 4 == 0) | (col % nsrcs == s) | ((col + 1) % nsrcs == s)
            b = np.where(special & ~allowed, b & ~t(1 << (w - 2)), b)
            head = from_bits(code, [int(c) for c in _designed_columns(code, nsrcs)[s]])
            a = np.concatenate([head, b.view(NPDT[code])])
        out.append(a)
    return out


# ---- classes a reference output must contain (a test that never meets them is vacuous) ----
def is_tie(code, op, xb, yb):
    """True when the exact Sum/Prod of two finite patterns lies exactly half
    way between two neighbouring values of the format (Inf counted as the
    value after the largest finite one)."""
    p, emin, _, _, _, _ = fp_fields(code)
    (sx, x), (sy, y) = decode(code, xb), decode(code, yb)
    if isinstance(x, str) or isinstance(y, str):
        return False
    v = abs((-x if sx else x) + (-y if sy else y)) if op == SUM else x * y
    if v == 0:
        return False
    _, _, twice, den = _units(v, p, emin)
    return twice == den


def result_classes(code, op, x, y, r, tie_budget=4000):
    """Targeted classes present in r = ref_op(code, op, x, y).  fp: 'subnormal',
    'negzero', and for Sum/Prod 'inf' (overflow from finite operands) and 'tie'
    (looked for among the first tie_budget elements); integers: 'wrap'."""
    got = set()
    if not is_fp(code):
        if op in (SUM, PROD):
            xs = np.ascontiguousarray(x).view(NPDT[code]).astype(object)
            ys = np.ascontiguousarray(y).view(NPDT[code]).astype(object)
            rs = np.ascontiguousarray(r).view(NPDT[code]).astype(object)
            if np.any((xs + ys if op == SUM else xs * ys) != rs):
                got.add("wrap")
        return got
    p, _, _, _, sign, inf = fp_fields(code)
    rb, xb, yb = bits_of(code, r), bits_of(code, x), bits_of(code, y)
    t = rb.dtype.type
    mag = rb & t(sign - 1)
    if np.any((mag > 0) & (mag < t(1 << (p - 1)))):
        got.add("subnormal")
    if np.any(rb == t(sign)):
        got.add("negzero")
    if op in (SUM, PROD):
        fin = ((xb & t(sign - 1)) < t(inf)) & ((yb & t(sign - 1)) < t(inf))
        if np.any(fin & (mag == t(inf))):
            got.add("inf")
        if any(is_tie(code, op, a, b) for a, b in zip(xb[:tie_budget].tolist(), yb[:tie_budget].tolist())):
            got.add("tie")
    return got


def required_classes(code, op):
    if not is_fp(code):
        return {"wrap"} if op in (SUM, PROD) else set()
    return {"subnormal", "negzero", "inf", "tie"} if op in (SUM, PROD) else {"subnormal", "negzero"}


def fold_classes(code, op, srcs):
    """(fold result, union of result_classes over every step of the fold)."""
    acc = np.ascontiguousarray(srcs[0]).view(NPDT[code])
    got = set()
    for s in srcs[1:]:
        nxt = ref_op(code, op, acc, s)
        got |= result_classes(code, op, acc, s, nxt, tie_budget=64)
        acc = nxt
    return acc, got
