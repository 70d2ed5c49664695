"""Expected bytes and models for the Send/Recv tests (numpy only, no library code).

A case is a list of Op(rank, kind, peer, nbytes, off): each rank's ops, in list
order, are the calls of one group; off is how many bytes the op's buffer starts
past 16-byte alignment.

matches():   per ordered pair (s, t) the k-th send of s to t meets the k-th
             receive of t from s (NCCL's rule).
expected():  each receive's buffer equals its send's payload; everything sits
             inside 0xA5 frames (a2av_ref.frame).
elements():  the per-channel work elements of one rank, written from the
             pairing rule: a send to t joins the send queue of every channel c
             with next_c(r) == t, a receive from p the receive queue of every
             channel with prev_c(r) == p, both in issue order; element k of a
             channel holds its k-th send (S = 0: none) and its k-th receive
             (R = 0: none); a zero-byte op keeps its queue position; a channel
             with no op gets one all-zero element.
patterns():  the named pattern lists (a)-(h) at n ranks.  Sizes come from
             a2av_ref.values(m): {0, 1, 15, 4099, C, C + 1, 2C + 999, 3C} at
             buffer_size = a2av_ref.BUFF, C one loop of a pair.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

import a2a_ref
import a2av_ref as V

SENTINEL = V.SENTINEL
BUFF = V.BUFF
NWARPS = (512 + 32) // 32  # the schema's largest thread count, in reference warps of 32

Op = namedtuple("Op", "rank kind peer nbytes off", defaults=(0,))


def S(rank, peer, nbytes, off=0):
    return Op(rank, "send", peer, nbytes, off)


def R(rank, peer, nbytes, off=0):
    return Op(rank, "recv", peer, nbytes, off)


# ---- matching and expected bytes -------------------------------------------
def matches(ops) -> list[tuple[int, int]]:
    """(send index, recv index) pairs; raises if a send has no receive of its size."""
    sends, recvs = {}, {}
    for i, o in enumerate(ops):
        key = (o.rank, o.peer) if o.kind == "send" else (o.peer, o.rank)
        (sends if o.kind == "send" else recvs).setdefault(key, []).append(i)
    assert sends.keys() == recvs.keys(), (sorted(sends), sorted(recvs))
    out = []
    for key, si in sends.items():
        ri = recvs[key]
        assert [ops[i].nbytes for i in si] == [ops[i].nbytes for i in ri], key
        out += list(zip(si, ri))
    return out


def payload(i: int, nbytes: int, salt: int = 0) -> np.ndarray:
    """Send op i's bytes: distinct from every other op's of the case at every
    position (i < 250); salt gives the case other bytes (a refill)."""
    assert i < 250
    return V.make_send(0, nbytes, salt=1 + i + salt)


def payloads(ops, salt: int = 0) -> dict:
    return {i: payload(i, o.nbytes, salt) for i, o in enumerate(ops) if o.kind == "send"}


def expected(ops, sent=None) -> dict:
    """recv op index -> the bytes its buffer must hold."""
    sent = payloads(ops) if sent is None else sent
    return {ri: sent[si] for si, ri in matches(ops)}


def frames(ops, salt: int = 0) -> list:
    """Per op (array, payload slice): 0xA5 all around, a send's payload filled in.
    The payload starts op.off bytes past a multiple of 16 of the array."""
    out = []
    for i, o in enumerate(ops):
        a, sl = V.frame(o.nbytes, lead=32 + o.off)
        if o.kind == "send":
            a[sl] = payload(i, o.nbytes, salt)
        out.append((a, sl))
    return out


def check(ops, bufs, salt: int = 0, only=None) -> None:
    """bufs[i]: op i's (array, slice) after the run (`only`: the ops to look
    at).  Receives hold their send's bytes, sends are untouched, every frame is
    intact."""
    want = expected(ops, payloads(ops, salt))
    for i in range(len(ops)) if only is None else only:
        o, (a, sl) = ops[i], bufs[i]
        a = np.asarray(a)
        w = want[i] if o.kind == "recv" else payload(i, o.nbytes, salt)
        bad = np.flatnonzero(a[sl] != w)
        assert bad.size == 0, f"op {i} {o}: {bad.size} wrong bytes, first at {bad[0]}"
        assert (a[:sl.start] == SENTINEL).all() and (a[sl.stop:] == SENTINEL).all(), f"op {i} {o}: frame written"


# ---- the element model ------------------------------------------------------------
def elements(ops, r: int, rings) -> list[list[dict]]:
    """Rank r's elements per channel: dicts with send / recv (op indices or
    None) and S / R (bytes)."""
    n = len(rings[0])
    nxt, prv = V.ring_next_prev(rings, n)
    out = []
    for c in range(len(rings)):
        sq = [i for i, o in enumerate(ops) if o.rank == r and o.kind == "send" and o.peer == nxt[c][r]]
        rq = [i for i, o in enumerate(ops) if o.rank == r and o.kind == "recv" and o.peer == prv[c][r]]
        es = []
        for k in range(max(len(sq), len(rq), 1)):
            s = sq[k] if k < len(sq) else None
            v = rq[k] if k < len(rq) else None
            es.append({"send": s, "S": ops[s].nbytes if s is not None else 0,
                       "recv": v, "R": ops[v].nbytes if v is not None else 0})
        out.append(es)
    return out


def work_elements(ops, r: int, rings, addr) -> list[list[dict]]:
    """The same with everything a work element carries: addr(i) is op i's
    buffer address.  Every element of channel c has the channel's parts of the
    one-hop route, nChannels = m, hops = 1 and the largest thread count."""
    n = len(rings[0])
    route = a2a_ref.route(n, rings)
    assert route["hops"] == 1
    out = []
    for c, es in enumerate(elements(ops, r, rings)):
        out.append([{"hops": 1, "recv_bid": route["recv_bid"][r][c], "part": 0, "parts": 0,
                     "bid": route["send_bid"][r][c], "nch": route["m"], "count": e["S"], "arg": e["R"],
                     "send": addr(e["send"]) if e["send"] is not None else 0,
                     "recv": addr(e["recv"]) if e["recv"] is not None else 0, "nwarps": NWARPS} for e in es])
    return out


def loop_cases(ops, rings, m) -> set:
    """(Ls, Lr) of every element of every rank."""
    n = len(rings[0])
    return {(V.loops(e["S"], m), V.loops(e["R"], m)) for r in range(n) for es in elements(ops, r, rings) for e in es}


def ranks_of(ops) -> list[int]:
    return sorted({o.rank for o in ops})


# ---- the pattern lists -------------------------------------------------------------
def _one_channel_cycle(rings):
    """Ranks (a, b, c) with a -> b -> c -> a on one channel (n = 3)."""
    ring = rings[0]
    return ring[0], ring[1], ring[2]


def patterns(n: int, m: int, rings) -> dict:
    C = V.loop_bytes(m)
    v = V.values(m)
    out = {}
    if n <= 4:  # (a) one message for every ordered pair, sizes through the whole set
        size = lambda s, t: v[(s * n + t + (s + t) // n) % len(v)]
        ops = []
        for r in range(n):
            for t in range(n):
                if t != r:
                    ops += [S(r, t, size(r, t)), R(r, t, size(t, r))]
        out["a_all_pairs"] = ops
    # (b) ring shift with 3C: the FIFO holds two chunks, so every send waits for its receiver
    out["b_shift_3C"] = [op for r in range(n) for op in (S(r, (r + 1) % n, 3 * C), R(r, (r - 1) % n, 3 * C))]
    # (c) pairwise exchange, the two directions of different sizes; with odd n the last rank stays out
    ops = []
    for a in range(0, n - 1, 2):
        ops += [S(a, a + 1, C + 1), R(a, a + 1, 4099), R(a + 1, a, C + 1), S(a + 1, a, 4099)]
    out["c_pairwise"] = ops
    # (d) fan-out from rank 0 and fan-in to rank 0
    ops = []
    for t in range(1, n):
        ops += [S(0, t, v[t % len(v)] or 15), R(0, t, v[(t + 3) % len(v)] or 1)]
    for t in range(1, n):
        ops += [R(t, 0, v[t % len(v)] or 15), S(t, 0, v[(t + 3) % len(v)] or 1)]
    out["d_fan"] = ops
    # (e) two messages on one pair in one group, different sizes: order kept, two elements;
    # and a zero-byte message in front of them, which keeps its place in the queue
    out["e_two_on_a_pair"] = [S(0, 1, 2 * C + 999), S(0, 1, 15), R(1, 0, 2 * C + 999), R(1, 0, 15), S(1, 0, 1),
                              R(0, 1, 1)]
    out["e_zero_first"] = [S(0, 1, 0), S(0, 1, C), S(0, 1, 4099), R(1, 0, 0), R(1, 0, C), R(1, 0, 4099)]
    if n == 3:
        # (f) on the channel a -> b -> c -> a: a sends two messages of >= 3 loops to b; b issues recv, recv and
        # only then its send to c, which the pairing must still put into element 0; c sends >= 2 loops to a
        a, b, c = _one_channel_cycle(rings)
        out["f_send_after_recvs"] = [S(a, b, 3 * C), S(a, b, 2 * C + 999), R(a, c, C + 1),
                                     R(b, a, 3 * C), R(b, a, 2 * C + 999), S(b, c, C + 1),
                                     S(c, a, C + 1), R(c, b, C + 1)]
    # (g) one message of three loops: the sender's channels have Ls = 3 / Lr = 0, the receiver's the reverse
    out["g_one_way"] = [S(0, 1, 2 * C + 999), R(1, 0, 2 * C + 999)]
    # (h) a shift and the reverse shift with every buffer 1-15 bytes off 16-byte alignment
    ops = []
    for r in range(n):
        o = lambda k: 1 + (4 * r + k) % 15
        ops += [S(r, (r + 1) % n, 4099, o(0)), R(r, (r - 1) % n, 4099, o(1))]
        if n > 2:
            ops += [S(r, (r - 1) % n, C + 1, o(2)), R(r, (r + 1) % n, C + 1, o(3))]
    out["h_misaligned"] = ops
    return out


def shift_matrix(n: int, nbytes: int) -> list[list[int]]:
    """The AllToAllv count matrix of a ring shift: s sends nbytes to s + 1."""
    return [[nbytes if t == (s + 1) % n else 0 for t in range(n)] for s in range(n)]
