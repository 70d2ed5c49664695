"""Expected values and models for the AllToAll tests (no library code here).

expected() is a numpy block transpose.  route() and calls() restate the
issue's route and call list in Python, written from the definitions
(DESIGN.md §3.2), not from the C++: tests hold mccs_alltoall_route, the fake
runtime's launch record and the host ring to them.
"""
from __future__ import annotations

import numpy as np

SENTINEL = 0xA5


def make_input(s: int, n: int, B: int) -> np.ndarray:
    """Rank s's send buffer: x_s[t*B + i] = (31*s + 7*t + i) % 251, so a wrong
    block, a wrong offset or a dropped hop shows."""
    t = np.repeat(np.arange(n, dtype=np.int64), B)
    i = np.tile(np.arange(B, dtype=np.int64), n)
    return ((31 * s + 7 * t + i) % 251).astype(np.uint8)


def make_inputs(n: int, B: int, salt: int = 0) -> list[np.ndarray]:
    return [((make_input(s, n, B).astype(np.int64) + salt) % 251).astype(np.uint8) for s in range(n)]


def expected(inputs: list[np.ndarray], B: int) -> list[np.ndarray]:
    """recv_r[s*B + i] = send_s[r*B + i]: the transpose of the n x n block matrix."""
    n = len(inputs)
    m = np.stack([x.reshape(n, B) for x in inputs])  # [s, t, i]
    return [np.ascontiguousarray(m[:, r, :]).reshape(n * B) for r in range(n)]


def route(n: int, rings: list[list[int]], force_relay: bool = False) -> dict:
    """One hop iff every ordered pair (s, t), s != t, is the arc s -> next of
    exactly m >= 1 channels, the same m for all pairs, and relay is not forced."""
    nch = len(rings)
    nxt = [{ring[i]: ring[(i + 1) % n] for i in range(n)} for ring in rings]
    prv = [{b: a for a, b in d.items()} for d in nxt]
    counts = {(s, t): sum(1 for d in nxt if d[s] == t) for s in range(n) for t in range(n) if s != t}
    vals = set(counts.values())
    one_hop = n > 1 and not force_relay and len(vals) == 1 and min(vals) >= 1
    if not one_hop:
        ident = [list(range(nch)) for _ in range(n)]
        return {"hops": n - 1, "m": 0, "send_bid": ident, "recv_bid": [list(x) for x in ident]}
    send_bid = [[sum(1 for k in range(c) if nxt[k][r] == nxt[c][r]) for c in range(nch)] for r in range(n)]
    recv_bid = [[sum(1 for k in range(c) if prv[k][r] == prv[c][r]) for c in range(nch)] for r in range(n)]
    return {"hops": 1, "m": vals.pop(), "send_bid": send_bid, "recv_bid": recv_bid}


def calls(hops: int) -> list[tuple[str, int]]:
    """The primitive calls of one loop: per distance d = 1 .. hops a send,
    d - 1 recvSend relays and a recv."""
    out = []
    for d in range(1, hops + 1):
        out.append(("send", d))
        out += [("recvSend", d)] * (d - 1)
        out.append(("recv", d))
    return out


def sentinel_frame(nbytes: int, lead: int, tail: int = 64) -> tuple[np.ndarray, slice]:
    """A 0xA5-filled host array with `nbytes` payload bytes starting `lead` bytes in."""
    a = np.full(lead + nbytes + tail, SENTINEL, np.uint8)
    return a, slice(lead, lead + nbytes)
