"""The wide-accumulate AllReduce's definition (csrc/direct_wide.h), numpy only.
Per element, ranks in rank order: t_r = f32(x_r), or fl32(f32(x_r) * f32(s))
for PreMulSum; acc = t_0; acc = fl32(acc + t_r); out = T(acc), nearest even.
fp16 arrays are np.float16, bf16 arrays the raw np.uint16 bits.
"""
import numpy as np

F16, BF16 = 6, 9


def widen(x, code):
    if code == BF16:
        return (np.asarray(x, np.uint16).astype(np.uint32) << 16).view(np.float32)
    return np.asarray(x, np.float16).astype(np.float32)


def narrow(acc, code):
    if code == F16:
        return acc.astype(np.float16)
    u = acc.view(np.uint32)
    out = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)  # nearest even on the bits
    return np.where(np.isnan(acc), np.uint16(0x7FC0), out)  # (the add would carry a NaN's payload away)


def all_reduce(inputs, code, scalar=None):
    """inputs: one array per rank; scalar: the PreMulSum scalar as one T (None: Sum)."""
    with np.errstate(all="ignore"):
        acc = None
        for x in inputs:
            t = widen(x, code)
            if scalar is not None:
                t = (t * widen(np.array([scalar]), code)[0]).astype(np.float32)
            acc = t if acc is None else (acc + t).astype(np.float32)
        return narrow(acc, code)


def same(got, want, code):
    """Bit for bit, except where both are NaN (payloads are not compared)."""
    g, w = widen(got, code), widen(want, code)
    return bool(np.all((np.isnan(g) & np.isnan(w)) | (np.asarray(got).view(np.uint16) == np.asarray(want).view(np.uint16))))
