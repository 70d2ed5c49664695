"""Size tables and models for the AllToAllvDev tests (numpy only, no library code).

table():            rank r's size table from a count matrix and a layout of
                    tests/a2av_ref.py, written from the issue's text: 4 * n
                    64-bit words in bytes, word row * n + peer, row 0
                    sendcounts[t], 1 sdispls[t], 2 recvcounts[s], 3 rdispls[s].
sequence_layout():  one fixed layout for a sequence of matrices: every segment
                    gets the room of the element-wise maximum, packed in rank
                    order, so only the counts change from matrix to matrix.
want_elements():    rank r's work elements as the planner must queue them: per
                    channel the FIFO element (base pointers, count = the
                    table's address, redOpArg = 0, the route word with hops = 1,
                    recv_bid, successor and predecessor) and the self element.
"""
from __future__ import annotations

import numpy as np

import a2a_ref
import a2av_ref as V

ROWS = ("sendcounts", "sdispls", "recvcounts", "rdispls")


def index(row: int, n: int, peer: int) -> int:
    return row * n + peer


def table(cnt, lay, r: int) -> np.ndarray:
    n = len(cnt)
    t = np.zeros(4 * n, np.uint64)
    for k in range(n):
        t[index(0, n, k)] = cnt[r][k]
        t[index(1, n, k)] = lay["sdispls"][r][k]
        t[index(2, n, k)] = cnt[k][r]
        t[index(3, n, k)] = lay["rdispls"][r][k]
    return t


def tables(cnt, lay) -> list[np.ndarray]:
    return [table(cnt, lay, r) for r in range(len(cnt))]


def swap_rows(t: np.ndarray, a: int, b: int) -> np.ndarray:
    """The table with rows a and b exchanged: what a wrong row index would read."""
    n = t.size // 4
    out = t.copy()
    out[a * n:(a + 1) * n], out[b * n:(b + 1) * n] = t[b * n:(b + 1) * n], t[a * n:(a + 1) * n]
    return out


def sequence_layout(mats) -> dict:
    """Displacements that fit every matrix of `mats`: segment (r, k) has the
    room of the largest count any matrix gives it, packed in rank order."""
    n = len(mats[0])
    top = [[max(c[s][t] for c in mats) for t in range(n)] for s in range(n)]
    sd = [[sum(top[r][:t]) for t in range(n)] for r in range(n)]
    rd = [[sum(top[k][r] for k in range(s)) for s in range(n)] for r in range(n)]
    return {"sdispls": sd, "rdispls": rd, "send_len": [sum(top[r]) for r in range(n)],
            "recv_len": [sum(top[s][r] for s in range(n)) for r in range(n)]}


def want_elements(n: int, rings, r: int, send: int, recv: int, table_addr: int) -> list[dict]:
    """Rank r's elements in channel order, as the launch record's a2avd= key lists them."""
    if n == 1:
        nch = len(rings)
        return [{"hops": 0, "recv_bid": 0, "part": c, "parts": nch, "bid": c, "nch": nch, "count": table_addr,
                 "arg": 0, "send": send, "recv": recv} for c in range(nch)]
    model = a2a_ref.route(n, rings)
    nxt, prv = V.ring_next_prev(rings, n)
    out = []
    for c in range(len(rings)):
        # hops = 1: the part / parts bytes of the route word carry the successor and the predecessor
        out.append({"hops": 1, "recv_bid": model["recv_bid"][r][c], "part": nxt[c][r], "parts": prv[c][r],
                    "bid": model["send_bid"][r][c], "nch": model["m"], "count": table_addr, "arg": 0,
                    "send": send, "recv": recv})
        out.append({"hops": 0, "recv_bid": 0, "part": c, "parts": len(rings), "bid": 0, "nch": 1,
                    "count": table_addr, "arg": 0, "send": send, "recv": recv})
    return out
