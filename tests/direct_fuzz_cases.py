"""Test helper: the seeded cases of the direct ReduceScatter / Reduce /
Broadcast fuzz (test-only; no GPU and no communicator: a case is a function of
its seed alone, and the only library call is comm.task_schema, the planner's
thread count for a size, which needs the built library).

tests/test_gpu_direct_collectives_fuzz.py runs what this module draws on the
virtual node; tests/test_direct_fuzz_cases.py asserts on the CPU what the
default lists cover, that every case plans as its `algo` says, and that every
case can fail.  The split is tests/test_gpu_reduce_scatter_fuzz.py's with
tests/test_reduce_scatter_cases.py.

Part one, `case(seed)`: one configuration per seed -- function, body, ranks,
dtype, op, root, a count at an edge of the cut, channels, permuted rings, FIFO
buffer size, slot sizes, MCCS_DIRECT_BLOCKS, a cached arena, in place and both
buffers' misalignment.  `calls(case)` is what runs on it: the case's call twice
with fresh payloads (both parities), then one direct call of another function
on the same communicators (E_IN and the launch count).

Part two, `sequence(seed, n)`: about 40 calls on communicators opted in to
everything, each with the `algo` its size must take under the limits below
(tests/test_gpu_rooted_direct_sequences.py's CFG), closed by a ring AllToAll.

The model of a launch (`geometry`) restates csrc/host/plan.cpp build_direct_rs
/ build_direct_rooted: the workgroups G and the two piece sizes; the CPU test
holds it to the planner's own record for every default case.
"""
from __future__ import annotations

import os

import numpy as np

import rooted_ref
import rs_ref
import vnode
from mccs_amd import comm as C

ESIZE = vnode.ESIZE
SUM, PROD, MAX, MIN = 0, 1, 2, 3
I8, F32 = 0, 7
FUNCS = ("rs", "rd", "bc")
VARIANTS = ("oneshot", "ll")
SLOTS = ((256 << 10, 128 << 10), (1 << 20, 1 << 20))  # (oneshot_bytes, ll_bytes)
BUFFERS = (1 << 16, 1 << 20, None)  # None: the library default
DEFAULT_BUFF = 1 << 22
BLOCKS = (None, 1, 2, 3, 5)  # MCCS_DIRECT_BLOCKS
COUNT_KINDS = ("one", "word-1", "word", "word+1", "127", "granule-1", "granule", "granule+1", "4099", "random", "cap")
THREADS = 512  # MCCS_DIRECT_THREADS
DEVICE_WORKGROUPS = 256  # one per CU of the MI355X (and of the fake device): a fused launch gets 256 / n per rank
DEFAULT_BLOCKS = 128
FOLLOW = {"rs": "bc", "rd": "rs", "bc": "rd"}  # the direct call of another function that closes a case
FOLLOW_COUNT = 1001  # fp32 elements (Broadcast: their bytes): within every cap

# tests/test_direct_fuzz_cases.py: the DEFAULT_CASES seeds from SEED_BASE meet its coverage list, one fewer do not
SEED_BASE = 245990
DEFAULT_CASES = 26
CASES = int(os.environ.get("MCCS_DIRECT_FUZZ_CASES", DEFAULT_CASES))


# =====================================================================================
# part one: one call per configuration
# =====================================================================================
def _granules(func, n, es, nch_cfg):
    """Element counts of one ring granule ((threads - 32) x 8 bytes) for each
    thread count the planner gives a call of about that size."""
    out = []
    for nthr in (96, 288, 544):
        g = (nthr - 32) * 8 // es
        total = g * es * (n if func == "rs" else 1)
        if C.task_schema(total, nch_cfg)[1] == nthr:
            out.append(g)
    return out


def case(seed):
    """The configuration of one seed, a dict: func, variant, n, code, op,
    root, count (elements; bytes for bc; per block for rs), count_kind, cfg
    (CommConfig keywords), rings, buffer_size, slots, blocks, fifo_device,
    inplace, soff, roff (bytes past a 16-byte boundary), null_other (the
    buffer a rank's role does not use is NULL), algo."""
    rng = np.random.default_rng([seed, 77])
    func = FUNCS[int(rng.integers(0, 3))]
    variant = VARIANTS[int(rng.integers(0, 2))]
    n = int(rng.integers(2, 9))
    code = I8 if func == "bc" else int(rng.integers(0, 10))
    op = SUM if func == "bc" else int(rng.choice([SUM, SUM, SUM, PROD, MAX, MIN]))
    root = int(rng.choice([0, n - 1, int(rng.integers(0, n))]))
    es = ESIZE[code]
    nch = int(rng.integers(1, 7))
    if rng.random() < 0.5:
        rings = [[int(v) for v in rng.permutation(n)] for _ in range(nch)]
        permuted = True
    else:
        rings, permuted = C.default_rings(n, nch), False
    buffer_size = BUFFERS[int(rng.integers(0, 3))]
    slots = SLOTS[int(rng.integers(0, 2))]
    blocks = BLOCKS[int(rng.integers(0, 5))]
    fifo_device = bool(rng.random() < 0.2)
    if fifo_device:  # the LL cap reads 0 on a cached arena: the count-based body, which must fence
        variant = "oneshot"
    inplace = bool(rng.random() < 0.3)
    offs = list(range(0, 16, es))
    soff = int(rng.choice(offs)) if rng.random() < 0.5 else 0
    roff = int(rng.choice(offs)) if rng.random() < 0.5 else 0
    cap = slots[0] if variant == "oneshot" else slots[1]
    top = cap // es
    kind = COUNT_KINDS[int(rng.integers(0, len(COUNT_KINDS)))]
    word = max(1, 8 // es)
    grans = _granules(func, n, es, len(rings))
    gran = grans[int(rng.integers(0, len(grans)))]
    frac = float(rng.random())
    count = {"one": 1, "word-1": max(1, word - 1), "word": word, "word+1": word + 1, "127": 127,
             "granule-1": gran - 1, "granule": gran, "granule+1": gran + 1, "4099": 4099,
             "random": max(1, int(top ** frac)), "cap": top}[kind]
    assert 1 <= count <= top
    if op in (MAX, MIN) and count < 16:
        op = SUM  # a Max of a few elements is one rank's input: a kernel that copied that rank would pass
    cfg = dict(oneshot_bytes=slots[0], ll_bytes=slots[1], direct_bytes=-1, rings=rings)
    if buffer_size is not None:
        cfg["buffer_size"] = buffer_size
    if fifo_device:
        cfg["fifo_memory"] = C.FIFO_DEVICE
    return dict(seed=seed, func=func, variant=variant, n=n, code=code, op=op, root=root, count=count,
                count_kind=kind, cfg=cfg, rings=rings, permuted=permuted, buffer_size=buffer_size or DEFAULT_BUFF,
                slots=slots, blocks=blocks, fifo_device=fifo_device, inplace=inplace, soff=soff, roff=roff,
                null_other=bool(seed & 1), algo=variant)


def calls(case):
    """The three calls of a case: itself twice, then FOLLOW[func], a direct
    call of another function at the same variant, aligned and out of place."""
    own = dict(kind=case["func"], code=case["code"], op=case["op"], count=case["count"], root=case["root"],
               inplace=case["inplace"], soff=case["soff"], roff=case["roff"], null_other=case["null_other"],
               algo=case["algo"])
    kind = FOLLOW[case["func"]]
    follow = dict(kind=kind, code=I8 if kind == "bc" else F32, op=SUM,
                  count=FOLLOW_COUNT * (4 if kind == "bc" else 1), root=(case["root"] + 1) % case["n"],
                  inplace=False, soff=0, roff=0, null_other=False, algo=case["algo"])
    return [dict(own, index=0), dict(own, index=1), dict(follow, index=2)]


def nbytes_of(call):
    """The bytes the call's limit is held to: one block (rs) or the buffer."""
    return call["count"] * (1 if call["kind"] == "bc" else ESIZE[call["code"]])


def select(case, call):
    """(channels, threads, rings) the planner gives the call on fresh, idle channels."""
    nb = nbytes_of(call)
    p = vnode.Planner(len(case["rings"]), case["rings"])
    return p.select(nb * case["n"], nb) if call["kind"] == "rs" else p.select(nb, nb)


def walk(case, call):
    """The non-empty (bid, offset, nelem) pieces of the ring walk the call's fold follows."""
    nch, nthr, _ = select(case, call)
    return rs_ref.pieces(call["count"], call["code"], nch, nthr, case["buffer_size"])


def loops(case, call):
    es = 1 if call["kind"] == "bc" else ESIZE[call["code"]]
    nch, _, _ = select(case, call)
    chunk = case["buffer_size"] // 8 // es * 4
    return -(-call["count"] // (nch * chunk))


def geometry(case, call, device_workgroups=DEVICE_WORKGROUPS):
    """(G, piece, piece2, units): the workgroups per rank of the launch, its two
    piece sizes in elements and the units of work its busiest phase deals over
    the workgroups (count-based: phase-2 pieces, a Broadcast's copies; LL:
    512-thread rounds of words)."""
    n, kind, ll = case["n"], call["kind"], call["algo"] == "ll"
    es = 1 if kind == "bc" else ESIZE[call["code"]]
    nb = call["count"] * es
    scatter = nb * (n - 1) if kind in ("rs", "bc") else nb
    blocks = case["blocks"] or DEFAULT_BLOCKS
    if ll:
        words = -(-nb // 8) * (n - 1 if kind == "rs" else 1)
        g = -(-words // THREADS)
    else:
        g = -(-scatter // 4096)
    g = max(1, min(g, blocks, device_workgroups // n))

    def piece(phase):
        p = -(-phase // g)
        return min(max(-(-p // 4096) * 4096, 4096), 65536) // es

    p1, p2 = piece(scatter), piece(nb)
    if ll:
        units = -(-(-(-nb // 8)) // THREADS)
    elif kind == "bc":
        units = -(-call["count"] // p2)
    else:
        units = sum(-(-ne // p2) for _, _, ne in walk(case, call))
    return g, p1, p2, units


def deals(case, call):
    """{deal: (G, pieces per group)} of a count-based launch: every loop of the
    kernels that starts at `j = bx >= base ? bx - base : bx + G - base`
    (csrc/direct_rs.h phases 1 and 2, csrc/direct_rooted.h direct_rd_body phase
    2 and direct_bc_body phase 1).  A group is what one such loop deals: one
    foreign block or copy in a phase 1, one chunk of the walk in a phase 2;
    `base` runs on from group to group.  The LL bodies are thread-linear and
    have no deal."""
    if call["algo"] != "oneshot":
        return {}
    n, kind, cnt = case["n"], call["kind"], call["count"]
    g, p1, p2, _ = geometry(case, call)
    out = {}
    if kind in ("rs", "bc"):
        out[f"{kind} phase 1"] = (g, [-(-cnt // p1)] * (n - 1))
    if kind in ("rs", "rd"):
        out[f"{kind} phase 2"] = (g, [-(-ne // p2) for _, _, ne in walk(case, call)])
    return out


def deal_wraps(g, groups):
    """(wraps, lands): whether some group starts at base != 0 (the workgroups
    below base take the `bx + G - base` branch), and whether one of those
    workgroups then gets a piece (G - base < the group's pieces)."""
    base, wraps, lands = 0, False, False
    for np_ in groups:
        if base:
            wraps = True
            lands = lands or g - base < np_
        base = (base + np_) % g
    return wraps, lands


def early_return(case, call):
    """Whether the fold leaves the walk through `if (coff >= w.size) return`: a
    chunk of the last loop is empty (count-based Reduce and ReduceScatter)."""
    if call["algo"] != "oneshot" or call["kind"] == "bc":
        return False
    return len(walk(case, call)) % select(case, call)[0] != 0


def pointers(case, call, send_base, recv_base):
    """Per-rank (send, recv) pointers of a call from the per-rank addresses of
    its send and receive payloads (0 = NULL): in place a ReduceScatter receives
    at send + rank * count, a rooted call's root at send; null_other leaves out
    the buffer a rank's role does not use."""
    n, kind, root = case["n"], call["kind"], call["root"]
    es = 1 if kind == "bc" else ESIZE[call["code"]]
    send, recv = list(send_base), list(recv_base)
    for r in range(n):
        if call["inplace"] and kind == "rs":
            recv[r] = send[r] + r * call["count"] * es
        elif call["inplace"] and r == root:
            recv[r] = send[r]
        if call["null_other"] and r != root:
            if kind == "rd":
                recv[r] = 0
            elif kind == "bc":
                send[r] = 0
    return send, recv


def issue(comms, call, send, recv, stream=None):
    """One grouped call on every communicator (0 is passed as NULL)."""
    kw = {} if stream is None else {"stream": stream}
    with C.group():
        for r, c in enumerate(comms):
            if call["kind"] == "rs":
                C.reduce_scatter(c, send[r], recv[r], call["count"], call["code"], call["op"], **kw)
            elif call["kind"] == "rd":
                C.reduce(c, send[r], recv[r] or None, call["count"], call["code"], call["op"], call["root"], **kw)
            else:
                C.broadcast(c, send[r] or None, recv[r], call["count"], call["root"], **kw)


def opt_in(comms, case):
    """Every communicator opted in to all three functions at the cap of the
    case's variant; asserts the caps (a cached arena closes the LL path)."""
    one, ll = case["slots"]
    for c in comms:
        want = (one, 0 if case["fifo_device"] else ll)
        assert c.reduce_scatter_direct_max() == want and c.rooted_direct_max() == want, (case["seed"], want)
        if case["variant"] == "oneshot":
            c.set_reduce_scatter_direct(block_bytes=one)
            c.set_rooted_direct(bcast_bytes=one, reduce_bytes=one)
        else:
            c.set_reduce_scatter_direct(ll_block_bytes=ll)
            c.set_rooted_direct(bcast_ll_bytes=ll, reduce_ll_bytes=ll)


def call_inputs(case, call, salt=0):
    """Per-rank inputs of one call (None: the rank has no input), seeded by
    the case, the call's place in it and `salt`."""
    n, kind, cnt = case["n"], call["kind"], call["count"]
    rng = np.random.default_rng([case["seed"], call["index"], salt, 5])
    if kind == "bc":
        x = rng.integers(1, 256, cnt, dtype=np.uint8)
        return [x if r == call["root"] else None for r in range(n)]
    return [vnode.gen(call["code"], cnt * (n if kind == "rs" else 1), rng) for _ in range(n)]


def call_expected(orc, case, call, xs):
    """Per-rank expected outputs (None: the rank has none), from rs_ref /
    rooted_ref with the planner's selection for the case's rings and buffer."""
    n, kind = case["n"], call["kind"]
    planner = vnode.Planner(len(case["rings"]), case["rings"])  # every launch starts from idle channels
    if kind == "rs":
        return rs_ref.expected_planned(orc, xs, call["code"], call["op"], None, planner=planner,
                                       buff_size=case["buffer_size"])
    if kind == "rd":
        exp = rooted_ref.reduce_expected_planned(orc, xs, call["code"], call["op"], call["root"], None,
                                                 planner=planner, buff_size=case["buffer_size"])
        return [exp if r == call["root"] else None for r in range(n)]
    return [rooted_ref.broadcast_expected(xs, call["root"])] * n


def needs_order_control(case, call):
    """Whether a schedule-blind fold must differ: fp32 Sum from four ranks on
    (vnode.gen's fp32 are multiples of 2^-23 below 1: a sum of two is exact and
    a sum of three rounds once, the same in any order).  A Reduce adds its root
    last on every ring and the rank-order fold adds rank n - 1 last: at n = 4
    with root 3 both are round(round(the other three) + the root's), whatever
    the rings, so there alone the control is impossible."""
    if call["kind"] == "bc" or call["code"] != F32 or call["op"] != SUM:
        return False
    if call["kind"] == "rd" and case["n"] == 4:
        return call["root"] != 3
    return case["n"] >= 4


def can_fail_message(orc, case, call, xs, exp):
    """'' when a wrong result would show: every expected output differs from a
    zero buffer and from each rank's input of that place, and (see
    needs_order_control) the rank-order fold differs from the ring-order one."""
    n, kind, cnt = case["n"], call["kind"], call["count"]
    for r in range(n):
        if exp[r] is None:
            continue
        e = np.ascontiguousarray(exp[r]).view(np.uint8).reshape(-1)
        if e.size == 0 or not e.any():
            return f"rank {r}: the expectation is all zeros"
        if kind == "bc":
            continue  # the only input is the root's: an undone Broadcast shows through the prefill
        for s in range(n):
            rival = xs[s][r * cnt:(r + 1) * cnt] if kind == "rs" else xs[s]
            if np.ascontiguousarray(rival).view(np.uint8).reshape(-1).tobytes() == e.tobytes():
                return f"rank {r}: the expectation equals rank {s}'s input"
    if needs_order_control(case, call):
        if kind == "rs":
            blind = rs_ref.rank_order(orc, xs, call["code"], call["op"])
            if all(b.tobytes() == w.tobytes() for b, w in zip(blind, exp)):
                return "the rank-order fold equals the ring-order one"
        elif rooted_ref.rank_order(orc, xs, call["code"], call["op"]).tobytes() == exp[call["root"]].tobytes():
            return "the rank-order fold equals the ring-order one"
    return ""


MAX_SALT = 200
DEALS = ("rs phase 1", "rs phase 2", "rd phase 2", "bc phase 1")


def call_payload(orc, case, call, first_salt=0):
    """(inputs, expected, salt): the first salt from `first_salt` whose inputs
    make a case that can fail (a one-element Sum is 0 now and then)."""
    msg = ""
    for salt in range(first_salt, first_salt + MAX_SALT):
        xs = call_inputs(case, call, salt)
        exp = call_expected(orc, case, call, xs)
        msg = can_fail_message(orc, case, call, xs, exp)
        if not msg:
            return xs, exp, salt
    raise AssertionError((case["seed"], call, msg))


def case_features(case):
    """The entries of the part-one coverage list this case meets."""
    c = calls(case)[0]
    f, v = case["func"], case["variant"]
    g, _, _, units = geometry(case, c)
    es = ESIZE[case["code"]]
    out = {f"{f}-{v}", f"n{case['n']}", f"blocks-{case['blocks']}", f"count-{case['count_kind']}"}
    if f != "bc":
        out |= {f"dtype{case['code']}", f"op{case['op']}"}
    if case["count"] == 1:
        out.add("count 1")
    if case["count_kind"] == "cap":
        out.add(f"cap-{v}")
    if loops(case, c) >= 3:
        out.add("three loops")
    if v == "ll" and case["count"] * es % 8:
        out.add("partial LL tail word")
    if case["inplace"]:
        out.add("in place")
    else:
        s, r = case["soff"] % 16 != 0, case["roff"] % 16 != 0
        out.add({(True, False): "send misaligned", (False, True): "recv misaligned",
                 (True, True): "both misaligned", (False, False): "aligned"}[s, r])
    if case["permuted"]:
        out.add("permuted rings")
    if case["fifo_device"]:
        out.add("FIFO_DEVICE")
    if v == "ll" and g > 1 and units > g:
        out.add("LL: more rounds of words than workgroups")  # the thread-linear loops run more than once
    if v == "oneshot" and g > 1 and units > g:
        out.add("more pieces than workgroups")
    for name, (dg, groups) in deals(case, c).items():
        wraps, lands = deal_wraps(dg, groups)
        if lands:
            out.add("a wrapped workgroup takes a piece")
        if wraps and dg in (2, 3, 5) and case["blocks"] == dg and sum(groups) > dg:
            out |= {f"deal wraps at G={dg}", f"{name} deal wraps"}
    if early_return(case, c):
        out.add("early return of the walk")
    if case["root"] == 0 and f != "rs":
        out.add("root 0")
    if case["root"] == case["n"] - 1 and f != "rs":
        out.add("root n-1")
    if needs_order_control(case, c) and case["count"] >= 127:
        out.add(f"rank-order control {f}")
    return out


REQUIRED = (
    {f"{f}-{v}" for f in FUNCS for v in VARIANTS} | {f"n{n}" for n in range(2, 9)}
    | {f"dtype{d}" for d in range(10)} | {f"op{o}" for o in range(4)}
    | {f"blocks-{b}" for b in BLOCKS} | {f"deal wraps at G={g}" for g in (2, 3, 5)}
    | {f"{d} deal wraps" for d in DEALS}
    | {"count 1", "cap-oneshot", "cap-ll", "three loops", "partial LL tail word", "in place", "send misaligned",
       "recv misaligned", "both misaligned", "permuted rings", "FIFO_DEVICE", "more pieces than workgroups",
       "LL: more rounds of words than workgroups", "a wrapped workgroup takes a piece", "early return of the walk",
       "rank-order control rs", "rank-order control rd",
       "root 0", "root n-1"})


def gaps(cases):
    """The entries of REQUIRED no case of `cases` meets."""
    got = set()
    for c in cases:
        got |= case_features(c)
    return REQUIRED - got


def default_cases(count=None):
    return [case(SEED_BASE + k) for k in range(CASES if count is None else count)]


# =====================================================================================
# part two: sequences
# =====================================================================================
# tests/test_gpu_rooted_direct_sequences.py's CFG and opt_in, which the GPU test holds these to
SEQ_BUFF = 1 << 16
ONESHOT, LL_BYTES, TWOSHOT = 256 << 10, 32 << 10, 2 << 20
SMALL_LL = 16 << 10  # the LL limit of ReduceScatter, Reduce and Broadcast
A2A_LL = 4099  # bytes per peer tests/test_gpu_rooted_direct_sequences.py sends through the LL AllToAll
SEQ_OPS = int(os.environ.get("MCCS_DIRECT_SEQ_OPS", "40"))
RD_TYPES = [(7, SUM), (6, MAX), (2, SUM), (9, MIN), (7, PROD), (8, SUM), (4, SUM), (6, SUM)]

# kind -> (call kind of tests/test_gpu_rooted_sequences.py, algo, smallest and largest size in bytes)
SEQ_KINDS = {
    "rs-oneshot": ("rs", "oneshot", SMALL_LL + 8, ONESHOT), "rs-ll": ("rs", "ll", 1, SMALL_LL),
    "rd-oneshot": ("rd", "oneshot", SMALL_LL + 8, ONESHOT), "rd-ll": ("rd", "ll", 1, SMALL_LL),
    "bc-oneshot": ("bc", "oneshot", SMALL_LL + 1, ONESHOT), "bc-ll": ("bc", "ll", 1, SMALL_LL),
    "ar-ll": ("ar", "ll", 1, LL_BYTES), "ar-oneshot": ("ar", "oneshot", LL_BYTES + 8, ONESHOT),
    "ar-direct": ("ar", "direct", ONESHOT + 8, 1 << 20), "ar-ring": ("ar", "ring", TWOSHOT + 8, 3 << 20),
    "ag-oneshot": ("ag", "oneshot", LL_BYTES + 1, ONESHOT), "ag-ll": ("ag", "ll", 1, LL_BYTES),
    "a2a-ll": ("a2a", "ll", 1, A2A_LL),
    "rs-ring": ("rs", "ring", ONESHOT + 8, 400 << 10), "rd-ring": ("rd", "ring", ONESHOT + 8, 400 << 10),
    "bc-ring": ("bc", "ring", ONESHOT + 1, 400 << 10),
}
# the draw: the three functions under test as often as everything else together
SEQ_DRAW = (["rs-oneshot", "rs-ll", "rd-oneshot", "rd-ll", "bc-oneshot", "bc-ll"] * 3
            + ["ar-ll", "ar-oneshot", "ar-direct", "ar-ring", "ag-oneshot", "ag-ll", "a2a-ll", "a2a-ll"]
            + ["rs-ring", "rd-ring", "bc-ring", "ar-ring"] * 2)
CLASSES = ("rs-direct", "rd-direct", "bc-direct", "other direct", "ring")


def predicted_algo(kind, nbytes):
    """The kernel a single call of `nbytes` (one block for rs, bytes per peer
    for a2a, bytes per rank otherwise) takes under the limits above; LL wins
    where both fit."""
    if kind in ("rs", "rd", "bc"):
        return "ll" if nbytes <= SMALL_LL else "oneshot" if nbytes <= ONESHOT else "ring"
    if kind == "a2a":
        return "ll" if nbytes <= A2A_LL else "ring"
    if nbytes <= LL_BYTES:
        return "ll"
    if nbytes <= ONESHOT:
        return "oneshot"
    return "direct" if kind == "ar" and nbytes <= TWOSHOT else "ring"


def klass(call):
    if call["algo"] == "ring":
        return "ring"
    return call["kind"] + "-direct" if call["kind"] in ("rs", "rd", "bc") else "other direct"


def sequence(seed, n, nops=None):
    """The calls of one sequence for n ranks, the same on every rank:
    tests/test_gpu_rooted_sequences.py's call dicts (kind, code, op, count --
    elements; bytes for bc / ag / a2a; per block for rs --, root, inplace; salt
    for a2a) plus `name` (a key of SEQ_KINDS) and `algo`, the kernel the call
    must take.  Every rooted call draws its root afresh; a ring AllToAll closes
    the sequence."""
    rng = np.random.default_rng([seed, n, 31])
    out = []
    for i in range(SEQ_OPS if nops is None else nops):
        name = SEQ_DRAW[int(rng.integers(0, len(SEQ_DRAW)))]
        kind, algo, lo, hi = SEQ_KINDS[name]
        code, op = 0, SUM
        if kind in ("rs", "rd", "ar"):
            code, op = RD_TYPES[int(rng.integers(0, len(RD_TYPES)))]
        es = 1 if kind in ("bc", "ag", "a2a") else ESIZE[code]
        lo = -(-lo // es) * es
        nbytes = int(lo * (hi / lo) ** float(rng.random()))
        if rng.random() < 0.15:
            nbytes = hi  # the limit itself
        count = min(max(nbytes // es, -(-lo // es)), hi // es)
        assert predicted_algo(kind, count * es) == algo, (name, count, es)
        call = dict(kind=kind, name=name, algo=algo, code=code, op=op, count=count, root=None, inplace=False)
        if kind in ("rd", "bc"):
            call["root"] = int(rng.integers(0, n))
            call["inplace"] = bool(rng.random() < 0.3)
        if kind == "a2a":
            call["salt"] = i
        out.append(call)
    out.append(dict(kind="a2a", name="a2a-ring", algo="ring", code=0, op=SUM, count=40000, root=None, inplace=False,
                    salt=len(out)))  # every FIFO connection in step
    return out


def sequence_features(seq):
    """Call kinds, ordered adjacencies of CLASSES, a root change between
    consecutive rooted calls, one parity of the slots reused by two functions."""
    out = {c["name"] for c in seq}
    for a, b in zip(seq, seq[1:]):
        out.add((klass(a), klass(b)))
        if a["root"] is not None and b["root"] is not None and a["root"] != b["root"]:
            out.add("root change")
    direct = [c for c in seq if c["algo"] != "ring"]  # launch k of these uses slot parity k & 1
    for a, b in zip(direct, direct[2:]):
        if a["kind"] != b["kind"] and {klass(a), klass(b)} & {"rs-direct", "rd-direct", "bc-direct"}:
            out.add("parity reused by two functions")
    return out


SEQ_REQUIRED = (set(SEQ_KINDS) | {"a2a-ring", "root change", "parity reused by two functions"}
                | {(a, b) for a in CLASSES for b in CLASSES})

# (seed, n) of the default runs: one stream, two streams, a replayed graph
SEQ_BASE = 0
ONE_STREAM = [(SEQ_BASE + k, n) for k, n in enumerate((2, 3, 4, 8))]
TWO_STREAMS = [(SEQ_BASE + 10, 3), (SEQ_BASE + 11, 5)]
GRAPH = [(SEQ_BASE + 20, 2), (SEQ_BASE + 21, 6)]


def sequence_gaps(runs):
    got = set()
    for seed, n in runs:
        got |= sequence_features(sequence(seed, n))
    return SEQ_REQUIRED - got
