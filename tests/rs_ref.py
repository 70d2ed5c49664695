"""Test helper: expected values of the ring ReduceScatter (test-only).

The reference has no ReduceScatter (task.rs:95-102 stops at unimplemented!()),
so the C oracle has no function for it.  The result is defined in words
(include/mccs_hip.h) and restated here with numpy and the
oracle's element functor only; nothing below calls the library under test
except `C.task_schema` through `vnode.Planner`, the host-only mirror of
get_task_schema.

  * `recvcount` elements per block are split over the selected channels:
    per loop, rcs = round_up(min(chunk, div_up(size - gridOffset, nch)), gran),
    channel bid owns [gridOffset + bid * rcs, + min(rcs, size - that)).
  * block D's piece on channel bid is folded along that channel's ring:
    acc = x[s1], acc = fn(x[sk], acc) for k = 2..n, s1..sn the successors of
    D on the ring and sn = D (the operand order of oracle ring_visit).

`orc` in fold / expected / expected_planned is anything with
`.apply(code, op, x, acc)`: the oracle module, or ELEM_REF below, which
evaluates the same schedule under the independent tests/elem_ref.py.
"""
from __future__ import annotations

import numpy as np

import vnode

ESIZE = vnode.ESIZE


def pieces(recvcount, code, nch, nthr, buff_size):
    """(bid, offset, nelem) of every non-empty piece of a block."""
    es = ESIZE[code]
    chunk = int(buff_size // 8 // es * 4)
    loop = nch * chunk
    gran = max(1, (nthr - 32) * 8 // es)
    out = []
    for g in range(0, recvcount, loop):
        rcs = min(chunk, -(-(recvcount - g) // nch))
        rcs = -(-rcs // gran) * gran
        for bid in range(nch):
            off = g + bid * rcs
            nelem = min(rcs, recvcount - off)
            if nelem > 0:
                out.append((bid, off, nelem))
    return out


def fold(orc, code, op, parts):
    """acc = parts[0]; acc = fn(parts[k], acc) for k = 1.., each hop rounded in the dtype."""
    acc = np.ascontiguousarray(parts[0]).copy()
    for x in parts[1:]:
        acc = orc.apply(code, op, np.ascontiguousarray(x), acc)
    return acc


def expected(orc, inputs, code, op, nch, nthr, rings, buff_size=1 << 22):
    """Per-rank results: out[D] = block D reduced in ring order.  inputs[r]
    holds n * recvcount elements; rings[bid] is channel bid's ring order."""
    n = len(inputs)
    cnt = inputs[0].size // n
    if n == 1:
        return [inputs[0][:cnt].copy()]
    out = [np.empty(cnt, inputs[0].dtype) for _ in range(n)]
    for bid, off, nelem in pieces(cnt, code, nch, nthr, buff_size):
        ring = list(rings[bid])
        for d in range(n):
            pos = ring.index(d)
            succ = [ring[(pos + k) % n] for k in range(1, n + 1)]
            lo = d * cnt + off
            out[d][off:off + nelem] = fold(orc, code, op, [inputs[s][lo:lo + nelem] for s in succ])
    return out


def expected_planned(orc, inputs, code, op, comm0, planner=None, buff_size=1 << 22):
    """`expected` with the channels, threads and rings the planner selects
    for this call (ring_enqueue: total = the bytes that enter the ring, load =
    one block's bytes per channel)."""
    n = len(inputs)
    cnt = inputs[0].size // n
    p = planner or vnode.Planner(comm0.nchannels, comm0.rings())
    nch, nthr, rings = p.select(cnt * ESIZE[code] * n, cnt * ESIZE[code])
    return expected(orc, inputs, code, op, nch, nthr, rings, buff_size)


def rank_order(orc, inputs, code, op):
    """Every block folded in plain rank order (acc = x[0], acc = fn(x[r], acc)):
    what a schedule-blind check would expect."""
    n = len(inputs)
    cnt = inputs[0].size // n
    return [fold(orc, code, op, [inputs[r][d * cnt:(d + 1) * cnt] for r in range(n)]) for d in range(n)]


class ElemRef:
    """Stands in for the oracle module in fold / expected / expected_planned:
    `.apply` is the independent reference of tests/elem_ref.py, on raw storage
    arrays (bf16 as uint16 bits), so the same schedule can be evaluated without
    the oracle's functor."""

    @staticmethod
    def apply(code, op, x, acc):
        import elem_ref as E

        return E.ref_op(code, op, x, acc)


ELEM_REF = ElemRef()


def fold_classes(code, op, parts, tie_budget=64):
    """(fold result, union of elem_ref.result_classes over every step) in this
    module's operand order, acc = fn(parts[k], acc): elem_ref.fold_classes
    folds fn(acc, s), which picks the other zero in Max / Min of +0 and -0."""
    import elem_ref as E

    acc = np.ascontiguousarray(parts[0]).view(E.NPDT[code])
    got = set()
    for x in parts[1:]:
        nxt = E.ref_op(code, op, x, acc)
        got |= E.result_classes(code, op, x, acc, nxt, tie_budget=tie_budget)
        acc = nxt
    return acc, got


# ---- edge-value inputs (tests/test_gpu_reduce_scatter_values.py, tests/test_reduce_scatter_cases.py) ----
_edge_cache = {}
BF16_RANDOM = 1001  # odd, as elem_ref.N_RANDOM


def edge_inputs(n, code, op):
    """Per-rank ReduceScatter inputs made of elem_ref's edge values.

    n = 2: rank 0 holds x and rank 1 holds y of edge_pairs(code, seed=d) in
    block d.  n > 2: block d is edge_sources(code, n, op, seed=d), rank r
    holding source (r - d - 1) % n, so that on the identity ring block d's
    fold visits the sources 0, 1, .., n-1 in that order.  bf16, whose Sum and
    Prod reference works in exact rationals element by element, gets a third
    of the random tail per block (n blocks of it cost what the AllReduce
    suite's single set does); designed columns and edge values stay whole.

    Returned read-only and checked once for vacuity on the identity ring's
    fold: every block's expected value is at least 75 % non-NaN, and the
    per-step classes contain elem_ref.required_classes(code, op)."""
    import elem_ref as E

    key = (n, code, op)
    if key in _edge_cache:
        return _edge_cache[key]
    if n == 2:
        blocks = [E.edge_pairs(code, seed=d) for d in range(n)]  # blocks[d][r]
    else:
        nrandom = BF16_RANDOM if code == 9 else E.N_RANDOM
        srcs = [E.edge_sources(code, n, op, seed=d, nrandom=nrandom) for d in range(n)]
        blocks = [[srcs[d][(r - d - 1) % n] for r in range(n)] for d in range(n)]
    inputs = [np.concatenate([blocks[d][r] for d in range(n)]) for r in range(n)]
    cnt = inputs[0].size // n
    assert all(x.size == n * cnt for x in inputs)
    for d in range(n):
        parts = [inputs[(d + k) % n][d * cnt:(d + 1) * cnt] for k in range(1, n + 1)]
        ref, classes = fold_classes(code, op, parts, tie_budget=4000 if n == 2 else 64)
        _, live = E.same_bits(code, ref, ref)
        assert live >= 0.75, (n, code, op, d, live)
        assert classes >= E.required_classes(code, op), (n, code, op, d, classes)
    for x in inputs:
        x.setflags(write=False)
    _edge_cache[key] = inputs
    return inputs
