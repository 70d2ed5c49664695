"""The block-scaled FP8 AllReduce's definition (csrc/direct_quant.h), numpy only.
A block is 32 consecutive elements from a multiple of 32; QDQ gives it one E8M0
scale byte b = max(f - 7, 1), f the exponent field of its amax (255 with an Inf
or NaN: 32 NaN), and rounds y * 2^(127 - b) to nearest even onto E4M3FN.  Per
block, ranks in rank order: y_r = QDQ(f32(x_r)); t_r = y_r or fl32(y_r * f32(s));
acc = t_0; acc = fl32(acc + t_r); out = T(QDQ(acc)).  fp16 arrays are
np.float16, bf16 arrays the raw np.uint16 bits (tests/wide_ref.py).
"""
import numpy as np

from wide_ref import narrow, same, widen  # noqa: F401  (same: bit for bit, NaN payloads aside)


def e4m3(v):
    """Finite |v| < 256 (float64) rounded to nearest even onto E4M3FN: 3 mantissa
    bits, least normal exponent -6, subnormals and the sign of zero kept."""
    _, ex = np.frexp(np.abs(v))
    step = np.ldexp(1.0, np.maximum(ex - 1, -6) - 3)
    return np.copysign(np.rint(np.abs(v) / step) * step, v)


def qdq(y):
    """y: binary32, a whole number of blocks; returns the dequantised binary32."""
    y = np.asarray(y, np.float32).reshape(-1, 32)
    f = ((y.view(np.uint32) & 0x7FFFFFFF).max(axis=1) >> 23).astype(np.int64)
    b = np.maximum(f - 7, 1)[:, None]
    with np.errstate(all="ignore"):
        d = e4m3(np.where(np.isfinite(y), y, 0).astype(np.float64) * np.ldexp(1.0, 127 - b)) * np.ldexp(1.0, b - 127)
    return np.where((f == 255)[:, None], np.nan, d).astype(np.float32).reshape(-1)


def all_reduce(inputs, code, scalar=None):
    """inputs: one array per rank; scalar: the PreMulSum scalar as one T (None: Sum)."""
    cnt = inputs[0].size
    with np.errstate(all="ignore"):
        acc = None
        for x in inputs:
            t = qdq(np.pad(widen(x, code), (0, -cnt % 32)))
            if scalar is not None:
                t = (t * widen(np.array([scalar]), code)[0]).astype(np.float32)
            acc = t if acc is None else (acc + t).astype(np.float32)
        return narrow(qdq(acc)[:cnt], code)
