"""The block-scaled FP8 streamed ReduceScatter's definition (csrc/direct_quant_stream.h), numpy only.  Quantisation
blocks of 32 count from the start of each ReduceScatter block of cnt elements; the owner's own input is never quantised.
"""
import numpy as np

from quant_ref import qdq
from wide_ref import narrow, widen


def reduce_scatter(inputs, code, scalar=None):
    """inputs: one array of n blocks per rank; returns the n output blocks, block t as rank t receives it."""
    n, cnt = len(inputs), inputs[0].size // len(inputs)
    out = []
    with np.errstate(all="ignore"):
        for t in range(n):
            acc = None
            for r, x in enumerate(inputs):
                y = widen(x[t * cnt:(t + 1) * cnt], code)
                y = y if r == t else qdq(np.pad(y, (0, -cnt % 32)))[:cnt]
                if scalar is not None:
                    y = (y * widen(np.array([scalar]), code)[0]).astype(np.float32)
                acc = y if acc is None else (acc + y).astype(np.float32)
            out.append(narrow(acc, code))
    return out
