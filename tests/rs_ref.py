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
