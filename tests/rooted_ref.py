"""Test helper: expected values of the ring Broadcast and Reduce (test-only).

The reference declares both functions and ships no kernel for either, so the
C oracle has none.  The results are defined in words (include/mccs_hip.h,
DESIGN.md §3.2) and restated here with numpy, tests/rs_ref.py and an element
functor; nothing below calls the library under test except `C.task_schema`
through `vnode.Planner`.

  * Broadcast: every rank ends with the root's bytes.
  * Reduce: the buffer of `count` elements is split over the selected channels
    like one ReduceScatter block (`rs_ref.pieces`); the piece of channel bid
    is folded along that channel's ring, acc = x[s1], acc = fn(x[sk], acc) for
    k = 2..n, s1..sn the successors of the root on the ring and sn = root.

`orc` is anything with `.apply(code, op, x, acc)`: the oracle module or
`rs_ref.ELEM_REF`.
"""
from __future__ import annotations

import numpy as np

import rs_ref
import vnode

ESIZE = vnode.ESIZE


def successors(ring, root):
    """s1..sn: the ranks after `root` along `ring`, ending with the root."""
    ring = list(ring)
    n = len(ring)
    pos = ring.index(root)
    return [ring[(pos + k) % n] for k in range(1, n + 1)]


def broadcast_expected(inputs, root):
    """What every rank's recvbuff holds: the root's bytes."""
    return np.ascontiguousarray(inputs[root]).copy()


def reduce_expected(orc, inputs, code, op, root, nch, nthr, rings, buff_size=1 << 22):
    """The root's result.  inputs[r] holds `count` elements; rings[bid] is
    channel bid's ring order."""
    n = len(inputs)
    cnt = inputs[0].size
    if n == 1:
        return inputs[0].copy()
    out = np.empty(cnt, inputs[0].dtype)
    for bid, off, nelem in rs_ref.pieces(cnt, code, nch, nthr, buff_size):
        succ = successors(rings[bid], root)
        out[off:off + nelem] = rs_ref.fold(orc, code, op, [inputs[s][off:off + nelem] for s in succ])
    return out


def select(nbytes, comm0=None, planner=None):
    """(channels, threads, rings) the planner gives a rooted call of `nbytes`
    (ring_enqueue: total = the buffer's bytes, load = the same per channel)."""
    p = planner or vnode.Planner(comm0.nchannels, comm0.rings())
    return p.select(nbytes, nbytes)


def reduce_expected_planned(orc, inputs, code, op, root, comm0, planner=None, buff_size=1 << 22):
    nch, nthr, rings = select(inputs[0].size * ESIZE[code], comm0, planner)
    return reduce_expected(orc, inputs, code, op, root, nch, nthr, rings, buff_size)


def rank_order(orc, inputs, code, op):
    """The buffer folded in plain rank order (acc = x[0], acc = fn(x[r], acc)):
    the control a schedule-blind check would expect, which must differ."""
    return rs_ref.fold(orc, code, op, list(inputs))
