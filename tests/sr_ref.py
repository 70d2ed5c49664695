"""Expected bytes and models for the Send/Recv tests (numpy only, no library
code; random_group() alone takes its engine draws, and with them the library's
default rings, from tests/test_gpu_all_to_all_v_fuzz.py).

A case is a list of Op(rank, kind, peer, nbytes, off, code): each rank's ops, in
list order, are the calls of one group; off is how many bytes the op's buffer
starts past 16-byte alignment.

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
random_group(): a seeded group under a seeded engine configuration: up to
             three messages on every ordered pair, sometimes a pair with more
             than one or two works of them, a rank's calls shuffled across its
             peers, typed counts.  chained(): the two hand-built groups with
             more than MAX_WORK_ELEMENTS elements on a channel.  An op's
             `code` is the element type its call names (the bytes are what
             counts: count = nbytes / ESIZE[code]).
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

import a2a_ref
import a2av_ref as V

SENTINEL = V.SENTINEL
BUFF = V.BUFF
NWARPS = (512 + 32) // 32  # the schema's largest thread count, in reference warps of 32

ESIZE = (1, 1, 4, 4, 8, 8, 2, 4, 8, 2)  # bytes per element of the ten type codes (int8, uint8, ... bfloat16)
U8 = 1
MAX_WORK_ELEMENTS = 10  # elements of one work (MCCS_MAX_WORK_ELEMENTS); a channel's further ones chain a work

Op = namedtuple("Op", "rank kind peer nbytes off code", defaults=(0, U8))


def S(rank, peer, nbytes, off=0, code=U8):
    return Op(rank, "send", peer, nbytes, off, code)


def R(rank, peer, nbytes, off=0, code=U8):
    return Op(rank, "recv", peer, nbytes, off, code)


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


# ---- queues and works ---------------------------------------------------------------
def queues(ops) -> dict:
    """(rank, kind, peer) -> that queue's op indices in issue order."""
    out = {}
    for i, o in enumerate(ops):
        out.setdefault((o.rank, o.kind, o.peer), []).append(i)
    return out


def works(ops, r: int, rings) -> list[int]:
    """Works per channel of rank r: MAX_WORK_ELEMENTS elements each, the last one the rest."""
    return [-(-len(es) // MAX_WORK_ELEMENTS) for es in elements(ops, r, rings)]


# ---- seeded groups ------------------------------------------------------------------
MAX_OPS = 249  # payload()'s limit
MAX_SENT = 8 << 20  # bytes a group sends in all
HEAVY = (11, 12, 21, 23)  # messages of a heavy pair: two works, and three works of ten
PAIR_COUNTS, PAIR_P = (0, 1, 2, 3), (0.4, 0.3, 0.15, 0.15)


def sizes(m: int) -> list[int]:
    return sorted(set(V.values(m)) | set(V.boundary_values(m)))


def interleave(rng, qs: list[list]) -> list:
    """A uniformly random interleaving of the lists qs that keeps each list's order."""
    left = [len(q) for q in qs]
    out = []
    while sum(left):
        k = int(rng.choice(len(qs), p=np.array(left) / sum(left)))
        out.append(qs[k][len(qs[k]) - left[k]])
        left[k] -= 1
    return out


def random_group(seed: int) -> dict:
    """n, cfg, slice2, fifo_works, relabelled, rings, m: the engine draws of
    test_gpu_all_to_all_v_fuzz (which names the library's constants and default
    rings).  ops: the group.  Every ordered pair of the ranks present draws 0-3
    messages; with probability 0.4 one pair is heavy (HEAVY messages, each of at
    most one loop); with probability 0.3 at n > 3 one rank is absent.  A size is
    one of sizes(m), or 0 one time in ten; the first message of the first pair
    has bytes.  The caps hold by construction: a pair gets no more messages
    than MAX_OPS leaves, a message no more bytes than MAX_SENT leaves (the
    largest size that fits).  Each rank's calls are a random interleaving of
    its (peer, direction) queues."""
    import test_gpu_all_to_all_v_fuzz as F

    rng = np.random.default_rng(seed)
    g = F.engine_case(rng)
    n, m = g["n"], g["m"]
    pool = sizes(m)
    assert pool[0] == 0
    absent = int(rng.integers(0, n)) if n > 3 and rng.random() < 0.3 else None
    live = [r for r in range(n) if r != absent]
    pairs = [(s, t) for s in live for t in live if s != t]
    first = pairs[int(rng.integers(0, len(pairs)))]
    heavy = pairs[int(rng.integers(0, len(pairs)))] if rng.random() < 0.4 else None
    nheavy = int(rng.choice(HEAVY))
    rest = [p for p in pairs if p not in (first, heavy)]
    order = [first] + ([heavy] if heavy not in (None, first) else [])
    order += [rest[int(k)] for k in rng.permutation(len(rest))]
    msgs_left, bytes_left = MAX_OPS // 2, MAX_SENT
    msgs = {}
    for p in order:
        k = nheavy if p == heavy else int(rng.choice(PAIR_COUNTS, p=PAIR_P))
        k = min(max(k, 1 if p == first else 0), msgs_left)
        msgs_left -= k
        own = [v for v in pool if v <= V.loop_bytes(m)] if p == heavy else pool
        msgs[p] = []
        for j in range(k):
            v = own[int(rng.integers(1, len(own)))]
            if rng.random() < 0.1 and not (p == first and j == 0):
                v = 0
            v = max(x for x in own if x <= min(v, bytes_left))
            bytes_left -= v
            code = int(rng.integers(0, len(ESIZE)))
            code = code if v % ESIZE[code] == 0 else U8
            msgs[p].append((v, code, int(rng.integers(0, 16)), int(rng.integers(0, 16))))
    ops = []
    for r in live:
        qs = [[S(r, t, v, so, code) for v, code, so, _ in msgs[(r, t)]] for t in live if t != r]
        qs += [[R(r, s, v, ro, code) for v, code, _, ro in msgs[(s, r)]] for s in live if s != r]
        ops += interleave(rng, qs)
    assert len(ops) <= MAX_OPS and any(o.nbytes for o in ops)
    assert sum(o.nbytes for o in ops if o.kind == "send") <= MAX_SENT
    return dict(seed=seed, **g, ops=ops, absent=absent, heavy=heavy)


# ---- the chained groups ---------------------------------------------------------------
def chain_sizes(k: int, m: int) -> list[int]:
    """k message sizes of one pair: a walk through the boundary values up to
    one loop, 2C + 999 in the middle, and zero bytes at positions 0, 9, 10 and
    last: the last element of a full work and the first of the chained one."""
    C = V.loop_bytes(m)
    walk = [v for v in V.boundary_values(m) if v <= C]
    out = [walk[(3 * j) % len(walk)] for j in range(k)]
    out[k // 2] = 2 * C + 999
    for j in (0, MAX_WORK_ELEMENTS - 1, MAX_WORK_ELEMENTS, k - 1):
        out[j] = 0
    return out


def chained(n: int, m: int) -> list:
    """n = 2: 23 messages 0 -> 1 and 12 messages 1 -> 0; every channel joins
    the pair, so each holds three works one way and two the other.  Rank 0
    issues its sends and then its receives, rank 1 takes them in turns.
    n = 4: 12 messages 0 -> 1, one of 3C 2 -> 3 and one 1 -> 2; rank 0 makes no
    call to 2 or 3, rank 1 issues its 12 receives before its single send."""
    C = V.loop_bytes(m)
    if n == 2:
        a, b = chain_sizes(23, m), chain_sizes(12, m)
        ops = [S(0, 1, v, j % 16) for j, v in enumerate(a)] + [R(0, 1, v, (5 + j) % 16) for j, v in enumerate(b)]
        for j, v in enumerate(a):
            ops.append(R(1, 0, v, (3 * j) % 16))
            if j < len(b):
                ops.append(S(1, 0, b[j], (7 * j + 1) % 16))
        return ops
    assert n == 4
    a = chain_sizes(12, m)
    ops = [S(0, 1, v, j % 16) for j, v in enumerate(a)]
    ops += [R(1, 0, v, (3 * j) % 16) for j, v in enumerate(a)] + [S(1, 2, C + 1, 9)]
    ops += [R(2, 1, C + 1, 2), S(2, 3, 3 * C), R(3, 2, 3 * C, 13)]
    return ops
