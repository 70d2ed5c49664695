"""Test helper: the cases of the guarded mixed-alignment sweeps and a model
of the path every slice of a case takes (test-only).

tests/test_gpu_footprint_collectives.py runs the cases below on the virtual
node, tests/test_footprint_cases.py asserts on the CPU what they cover and
runs them on the host-thread ring.  Both build their buffers and check them
with `Buffers`, so the offsets, the in-place pointer arithmetic and the
expectations of the GPU tests are proven without a GPU.

The model restates, from the kernels' definitions, which path of
ring_stream.h reduce_copy_rows_dyn each slice reaches.  It uses no library
code beyond the host-only `C.ring_walk`, `C.task_schema`, `C.default_rings`
and `a2a_ref.route`.

  * A work element is a sequence of slices t = 0, 1, ..: loops of the walk,
    primitive calls of a loop (`calls`), one slice per call (slice_steps = 4,
    the library default).  Slice t uses the unit counter of parity t & 1.
  * A call touches a user operand only where its kind has kSrc / kDst
    (ring_kernel.h call_kind, slice_ptrs); a FIFO slot is always 16-byte
    aligned, so a recvSend slice is always aligned.  The user operand of a
    call sits at the user offset + (block base + chunk offset + lane offset)
    * element size; chunk and lane offsets are multiples of 16 bytes, the
    block base is not when a block's byte size is not.
  * The lanes cut a slice as `lane_parts` says.
  * A slice is "empty" (no element), "typed" (some operand misaligned: the
    typed loop, the unit counter does not move), "units" (aligned, at least
    one whole wave unit), "packs" (aligned, remainder packs only), either with
    "+tail" (typed elements past the last pack), or "no pack" (aligned, fewer
    elements than a pack).
  * A wave unit is 64 lanes x U packs of 16 bytes, U = MCCS_RING_UNROLL as
    the communicator launches are built: 8, and 4 for one-byte types
    (ring_kernel.h kUnroll).  The model uses this exact unit, not the "16 KiB
    holds whole units for every U <= 8" rule of `ring_paths`.
  * "alternation": on one rank, channel and lane, within one work element, a
    "units" slice, a "typed" slice and another "units" slice in that order on
    slices of one parity; reached by a case set when both parities have one.
    "alternation by block base": the same on 16-byte aligned user buffers,
    where only a block's byte size can misalign a call.
    With one slice per call a loop of n calls has fewer than three slices of
    a parity for n < 5: at n = 3 the cases take three loops of a 64 KiB FIFO
    buffer, at n = 8 one loop of the default buffer.
"""
from __future__ import annotations

import zlib
from dataclasses import dataclass, replace

import numpy as np

import a2a_ref
import footprint as F
import rooted_ref
import rs_ref
import vnode
from footprint import Guarded
from mccs_amd import comm as C

I8, I64, F16, F32, F64 = 0, 4, 6, 7, 8
SUM = 0
NPDT, ESIZE = vnode.NPDT, vnode.ESIZE
DEFAULT_BUFF = 1 << 22
SMALL_BUFF = 1 << 16  # a chunk is 32 KiB: a block of 76 KiB walks three loops
LOOPS_BUFF = 1 << 20  # tests/test_gpu_footprint.py test_ring_footprint_several_loops
# The walk of each function (ring_walk.h): Broadcast cuts its buffer and AllToAll a pair's block as
# AllGather cuts a block, Reduce its buffer as ReduceScatter cuts a block
FUNCS = {"rs": C.FUNC_REDUCE_SCATTER, "ag": C.FUNC_ALLGATHER, "bc": C.FUNC_ALLGATHER, "rd": C.FUNC_REDUCE_SCATTER,
         "a2a": C.FUNC_ALLGATHER}
BYTE_FUNCS = ("ag", "bc", "a2a")  # the int8 kernels: count is bytes


# =====================================================================================
# moved from tests/test_gpu_footprint.py, which imports them back
# =====================================================================================
def gen(code, count, rng):
    """Full-range integers (sums wrap), fp values with busy mantissas."""
    if code in (F16, F32, F64):
        return (rng.standard_normal(count) * 4).astype(NPDT[code])
    info = np.iinfo(NPDT[code])
    return rng.integers(info.min // 2, info.max // 2, count).astype(NPDT[code])


def offset_set(es):
    return sorted({0, es, 8, 16 - es})


def assignments(n, es):
    """(name, per-rank (send offset, receive offset), in place): every pair
    of {0, es, 8, 16 - es} on all ranks alike, then offsets that differ per
    rank, a single misaligned rank, and in place at nonzero offsets."""
    offs = offset_set(es)
    nz = [o for o in offs if o]
    out = [(f"send+{s} recv+{r}", [(s, r)] * n, False) for s in offs for r in offs]
    out.append(("per rank", [((r * es) % 16, offs[(r + 1) % len(offs)]) for r in range(n)], False))
    out.append(("only the last rank's send", [(es if r == n - 1 else 0, 0) for r in range(n)], False))
    out.append(("only rank 0's recv", [(0, 16 - es if r == 0 else 0) for r in range(n)], False))
    out.append(("in place, per rank", [(nz[r % len(nz)],) * 2 for r in range(n)], True))
    out.append(("in place, only rank 1", [(es if r == 1 else 0,) * 2 for r in range(n)], True))
    return out


def lane_parts(c, es, lanes, buff, spc):
    """Element counts of the parts ring_kernel.h's slice_ops cuts a chunk of c
    elements into: spc slices per chunk (1 by default, 2 with the reference's
    two-step slices), each over `lanes` workgroups at 256-byte multiples, a
    lane never more than its fixed share of the slot group."""
    step = buff // 8 // es
    span = step * (4 // spc)
    slice_size = max(-(-c // (16 * spc)) * 16, span // 32)
    align = 256 // es
    cap = span // lanes // align * align
    out = []
    for s in range(spc):
        real = max(min(c - s * slice_size, slice_size), 0)
        part = min(-(-(-(-real // lanes)) // align) * align, cap)
        for lane in range(lanes):
            lo = min(lane * part, real)
            hi = real if lane == lanes - 1 else min(lo + part, real)
            out.append(hi - lo)
    assert sum(out) == c
    return out


def ring_paths(chunks, es, aligned, lanes, buff):
    """The parts of reduce_copy_rows_dyn a bucket with these chunks reaches,
    whichever slicing is configured.  A wave unit is 64 lanes x U packs with
    U <= 8: a part of 16 KiB holds whole units, a part whose packs are no
    multiple of 64 leaves remainder packs, for every U."""
    out = set()
    pack = 16 // es
    if any(c <= 0 for c in chunks):
        out.add("empty chunk")
    if not aligned:
        out.add("typed fallback")
        return out
    per_slicing = []
    for spc in (1, 2):
        got = set()
        for c in chunks:
            for p in lane_parts(c, es, lanes, buff, spc) if c > 0 else ():
                if p * es >= 16 << 10:
                    got.add("wave units")
                if p // pack % 64:
                    got.add("remainder packs")
                if p % pack:
                    got.add("typed tail")
                if 0 < p < pack:
                    got.add("no pack")
        per_slicing.append(got)
    return out | (per_slicing[0] & per_slicing[1])


# =====================================================================================
# cases
# =====================================================================================
@dataclass(frozen=True)
class Case:
    func: str  # "rs", "ag", "bc", "rd", "a2a"
    n: int
    code: int  # dtype code; I8 for the byte functions
    count: int  # rs: elements per block; ag, a2a: bytes per block; bc: bytes; rd: elements
    offs: tuple  # per rank (send offset, receive offset), bytes past a 256-byte line
    inplace: bool = False  # rs: recv = send + r * count; ag: send = recv + r * count; bc, rd: at the root
    root: int = 0
    relay: bool = False  # a2a: MCCS_ALLTOALL_HOPS=relay
    channel_count: int = 0  # 0: the library's default ring set
    lanes: int = 2
    buffer_size: int = DEFAULT_BUFF
    block_threads: int = 0  # 0: the library's default
    name: str = ""

    @property
    def es(self):
        return ESIZE[self.code]

    def config(self):
        """CommConfig arguments of the communicators this case runs on."""
        out = dict(lanes=self.lanes, buffer_size=self.buffer_size)
        if self.channel_count:
            out["channel_count"] = self.channel_count
        if self.block_threads:
            out["block_threads"] = self.block_threads
        return out

    def comm_key(self):
        return (self.n, self.relay, tuple(sorted(self.config().items())))

    def tag(self):
        return (self.func, self.n, self.code, self.count, self.name, self.root)


def unit_packs(es):
    """16-byte packs of one wave unit (ring_kernel.h kUnroll)."""
    return 64 * (4 if es == 1 else 8)


def rings_of(case):
    return C.default_rings(case.n, case.channel_count)


def user_ranks(ring, r):
    """ring.userRanks of rank r: itself, then the ranks ahead of it."""
    pos = list(ring).index(r)
    return [ring[(pos + k) % len(ring)] for k in range(len(ring))]


def elements(case):
    """The work elements of the call, which every rank's launch carries:
    (threads, route, [(channel, bid, parts)]); bid None: the route's per-rank
    send_bid / recv_bid.  A fresh communicator's planner takes channels
    0 .. nch-1."""
    rings = rings_of(case)
    n, es = case.n, case.es
    total = case.count * es * (n if case.func in ("rs", "ag", "a2a") else 1)  # the bytes that enter the ring
    nch, nthr = C.task_schema(total, len(rings))
    if case.func != "a2a":
        return nthr, None, [(ch, ch, nch) for ch in range(nch)]
    route = a2a_ref.route(n, rings, case.relay)
    if route["hops"] == 1:  # every channel, each with this rank's parts of its neighbours' blocks
        return nthr, route, [(ch, None, route["m"]) for ch in range(len(rings))]
    return nthr, route, [(ch, ch, nch) for ch in range(nch)]


def selected(case):
    """(channels, threads, their rings) of a reducing case, for rs_ref / rooted_ref."""
    nthr, _, elems = elements(case)
    rings = rings_of(case)
    return len(elems), nthr, [rings[ch] for ch, _, _ in elems]


def bases(case, r):
    """Byte addresses modulo 16 of rank r's (send, receive) pointers; None
    for the null sendbuff of a Broadcast's non-root."""
    s, d = case.offs[r]
    es = case.es
    if case.func == "rs" and case.inplace:
        d = s + r * case.count * es
    elif case.func == "ag" and case.inplace:
        s = d + r * case.count
    elif case.func in ("bc", "rd") and case.inplace and r == case.root:
        d = s
    if case.func == "bc" and r != case.root:
        s = None
    return s, d


def calls(case, ur, r, send_part):
    """One loop's primitive calls of a rank with userRanks `ur`:
    (part of the block, source block or None, destination block or None).
    A block is an index into the user buffer in units of `count`."""
    n = case.n
    if case.func == "rs":  # send, recvReduceSend .., recvReduceCopy
        return [(send_part, ur[n - 1 - j], 0 if j == n - 1 else None) for j in range(n)]
    if case.func == "ag":  # directSend / directCopySend, recvCopySend .., recv
        first = (send_part, 0, None if case.inplace else ur[0])
        return [first] + [(send_part, None, ur[n - j] if j < n - 1 else ur[1]) for j in range(1, n)]
    if case.func == "bc":  # the root: send / copySend; the others: recvCopySend / recv
        if r == case.root:
            return [(send_part, 0, None if case.inplace else 0)]
        return [(send_part, None, 0)]
    if case.func == "rd":  # recvReduceCopy at the root, send / recvReduceSend elsewhere
        return [(send_part, 0, 0 if r == case.root else None)]
    raise AssertionError(case.func)


def a2a_calls(hops, ur, send_part, recv_part):
    n = len(ur)
    out = []
    for kind, d in a2a_ref.calls(hops):
        if kind == "send":
            out.append((send_part, ur[d], None))
        elif kind == "recv":
            out.append((recv_part, None, ur[n - d]))
        else:
            out.append((send_part, None, None))  # FIFO slot to FIFO slot
    return out


def part_path(p, es, aligned):
    if p <= 0:
        return "empty"
    if not aligned:
        return "typed"
    pack = 16 // es
    if p < pack:
        return "no pack"
    return ("units" if p // pack >= unit_packs(es) else "packs") + ("+tail" if p % pack else "")


def slice_paths(case):
    """{(rank, channel, lane): [path of slice 0, slice 1, ..]} of the case's
    one work element per rank and channel."""
    nthr, route, elems = elements(case)
    rings = rings_of(case)
    n, es = case.n, case.es
    wes = 1 if case.func in BYTE_FUNCS else es  # the walk's element size
    out = {}
    for ch, bid, parts in elems:
        rows = C.ring_walk(FUNCS[case.func], n, parts, wes, nthr, case.buffer_size, case.count)
        loops = sorted({g for g, _, _, _ in rows})
        assert len(rows) == len(loops) * parts
        for r in range(n):
            ur = user_ranks(rings[ch], r)
            send_part = route["send_bid"][r][ch] if bid is None else bid
            recv_part = route["recv_bid"][r][ch] if bid is None else bid
            sbase, dbase = bases(case, r)
            lanes = [[] for _ in range(case.lanes)]
            for li in range(len(loops)):
                if case.func == "a2a":
                    cl = a2a_calls(route["hops"], ur, send_part, recv_part)
                else:
                    cl = calls(case, ur, r, send_part)
                for part, sblock, dblock in cl:
                    _, _, off, nelem = rows[li * parts + part]
                    mis = 0
                    if sblock is not None:
                        mis |= sbase + (sblock * case.count + off) * wes
                    if dblock is not None:
                        mis |= dbase + (dblock * case.count + off) * wes
                    ps = lane_parts(max(nelem, 0), wes, case.lanes, case.buffer_size, 1)
                    for lane, p in enumerate(ps):
                        lanes[lane].append(part_path(p, wes, mis % 16 == 0))
            for lane in range(case.lanes):
                out[(r, ch, lane)] = lanes[lane]
    return out


def alternation_parities(paths):
    """Parities on which some rank, channel and lane has units, typed, units."""
    got = set()
    for seq in paths.values():
        for par in (0, 1):
            state = 0
            for p in seq[par::2]:
                if state in (0, 2) and p.startswith("units"):
                    state += 1
                elif state == 1 and p == "typed":
                    state = 2
            if state == 3:
                got.add(par)
    return got


def chain_paths(case):
    """Broadcast / Reduce: ranks of one chain on different paths."""
    paths = slice_paths(case)
    first = {r: paths[(r, 0, 0)][0] for r in range(case.n)}
    others = {p.split("+")[0] for r, p in first.items() if r != case.root}
    root = first[case.root].split("+")[0]
    if root == "typed" and others == {"units"}:
        return {"root typed, others units"}
    if root == "units" and others == {"typed"}:
        return {"root units, others typed"}
    return set()


def reached(cases):
    """The union of the paths the cases' slices take, "alternation" when both
    parities have one, and the rooted chains' mixed paths."""
    out, parities, by_base = set(), set(), set()
    for case in cases:
        paths = slice_paths(case)
        for seq in paths.values():
            for p in seq:
                out.update(p.split("+"))
        parities |= alternation_parities(paths)
        if all(o % 16 == 0 for pair in case.offs for o in pair):
            by_base |= alternation_parities(paths)
        if case.func in ("bc", "rd"):
            out |= chain_paths(case)
    if parities == {0, 1}:
        out.add("alternation")
    if by_base == {0, 1}:  # the block bases alone alternate: every user buffer is aligned
        out.add("alternation by block base")
    return out


SWEEP_PATHS = {"typed", "units", "packs", "tail", "no pack", "empty", "alternation", "alternation by block base"}
ROOTED_PATHS = {"typed", "units", "packs", "tail", "no pack", "empty", "root typed, others units",
                "root units, others typed"}


# ---- the case lists -------------------------------------------------------------------
def _cases(func, n, code, count, assigns, **kw):
    return [Case(func, n, code, count, tuple(map(tuple, offs)), inplace=inplace, name=name, **kw)
            for name, offs, inplace in assigns]


ONE_CH = dict(channel_count=1, lanes=2)
# The alternation blocks.  A block of 24 KiB + 8 bytes (fp16: count % 8 == 4)
# puts block 1 at +8 modulo 16 between the aligned blocks 0 and 2, and leaves
# both lanes one unit, remainder packs and a typed tail.  n = 3: two whole
# 32 KiB chunks of the 64 KiB buffer before it, so the walk has three loops.
# n = 8, int8: 12 KiB + 8 bytes, one loop of eight calls.  n = 2
# (two slices per loop, never three of a parity): the same block in int64.
ALT_RS = {2: (I64, 3073, DEFAULT_BUFF), 3: (F16, 2 * 16384 + 12292, SMALL_BUFF), 8: (I8, 12296, DEFAULT_BUFF)}
ALT_BLOCK = {F16: 12292, F32: 6146, I8: 24584, I64: 3073}  # 24 KiB + 8 bytes in one loop of the default buffer


def rs_counts(n, code):
    pack = 16 // ESIZE[code]
    return sorted({1, n - 1, pack + 1, 4097})


def rs_cases(n):
    """ReduceScatter, Sum: counts x types x assignments(n, es) on one channel
    of two lanes, then the alternation block."""
    out = []
    for code in (F16, F32, I8) + ((I64,) if n == 2 else ()):
        for count in rs_counts(n, code):
            out += _cases("rs", n, code, count, assignments(n, ESIZE[code]), **ONE_CH)
    code, count, buff = ALT_RS[n]
    out += _cases("rs", n, code, count, assignments(n, ESIZE[code]), buffer_size=buff, **ONE_CH)
    return out


def chain_end(n, root):
    """The rank whose successor on channel 0's ring is the root."""
    ring = C.default_rings(n, 1)[0]
    return ring[(ring.index(root) - 1) % n]


def rooted_assignments(n, es, root):
    end = chain_end(n, root)
    out = assignments(n, es)
    out.append(("only the root", [(es, es) if r == root else (0, 0) for r in range(n)], False))
    out.append(("only the chain's last rank", [(es, es) if r == end else (0, 0) for r in range(n)], False))
    out.append(("all but the root", [(0, 0) if r == root else (es, es) for r in range(n)], False))
    return out


def roots(n):
    return list(range(n)) if n == 3 else [0, n - 1]


def rooted_cases(func, n, root):
    out = []
    if func == "bc":
        for nbytes in (1, 13, 4099, ALT_BLOCK[I8]):
            out += _cases("bc", n, I8, nbytes, rooted_assignments(n, 1, root), root=root, **ONE_CH)
        return out
    for code in (F16, F32, I8) + ((I64,) if n == 2 else ()):
        for count in rs_counts(n, code) + [ALT_BLOCK[code]]:
            out += _cases("rd", n, code, count, rooted_assignments(n, ESIZE[code], root), root=root, **ONE_CH)
    return out


# AllToAll: (n, relay forced, channel_count, the alternation size, its buffer)
A2A_SHAPES = {"n2": (2, False, 0, ALT_BLOCK[I8], DEFAULT_BUFF), "n4": (4, False, 0, ALT_BLOCK[I8], DEFAULT_BUFF),
              "n8": (8, False, 0, ALT_BLOCK[I8], DEFAULT_BUFF), "n6": (6, False, 0, ALT_BLOCK[I8], DEFAULT_BUFF),
              "n3-relay": (3, True, 1, 2 * 32768 + 12296, SMALL_BUFF)}


def a2a_cases(shape):
    n, relay, cc, alt, buff = A2A_SHAPES[shape]
    assigns = [a for a in assignments(n, 1) if not a[2]]  # out of place only
    out = []
    for B in (1, 15, 4099):
        out += _cases("a2a", n, I8, B, assigns, relay=relay, channel_count=cc)
    return out + _cases("a2a", n, I8, alt, assigns, relay=relay, channel_count=cc, buffer_size=buff)


def ag_alternation_cases():
    """AllGather at the alternation size, n = 3, one channel of two lanes."""
    n, B = 3, 2 * 32768 + 12296
    out_of_place = [("out+0 send+0", [(0, 0)] * n, False), ("out+0 send+1", [(1, 0)] * n, False),
                    ("out+8 send+0", [(0, 8)] * n, False),
                    ("per rank", [((3 * r) % 16, 8 * (r % 2)) for r in range(n)], False)]
    in_place = [("in place, out+0", [(0, 0)] * n, True), ("in place, out+8", [(8, 8)] * n, True),
                ("in place, per rank", [(8 * (r % 2),) * 2 for r in range(n)], True)]
    return _cases("ag", n, I8, B, out_of_place + in_place, buffer_size=SMALL_BUFF, **ONE_CH)


LOOPS_ASSIGN = ("send+0 recv+0", "per rank", "only rank 0's recv", "in place, per rank")


def loops_cases(func, n):
    """A 1 MiB buffer on one channel of 4 lanes: two whole loops of 512 KiB
    chunks and a partial third, the block's byte size 8 modulo 16."""
    code = F16 if func == "rs" else I8
    es = ESIZE[code]
    chunk = LOOPS_BUFF // 2 // es
    count = 2 * chunk + (65536 + 4104) // es
    assigns = [a for a in assignments(n, es) if a[0] in LOOPS_ASSIGN and not (func == "a2a" and a[2])]
    return _cases(func, n, code, count, assigns, channel_count=1, lanes=4, buffer_size=LOOPS_BUFF,
                  )


SHAPE_ASSIGN = ("send+0 recv+0", "per rank", "only the last rank's send", "in place, per rank")
LAUNCH_SHAPES = {"64-lanes": (2, dict(lanes=64, channel_count=2)), "96-threads": (4, dict(block_threads=96, lanes=2))}


def launch_shape_cases(func, shape):
    n, cfg = LAUNCH_SHAPES[shape]
    code = F16 if func == "rs" else I8
    es = ESIZE[code]
    out = []
    for count in (5001, ALT_BLOCK[code]):
        assigns = [a for a in assignments(n, es) if a[0] in SHAPE_ASSIGN and not (func == "a2a" and a[2])]
        out += _cases(func, n, code, count, assigns, **cfg)
    return out


def two_element_cases():
    """Two ReduceScatters of one group: (typed throughout, aligned at a
    units-holding size); the tests issue them in both orders."""
    n, code = 3, F16
    typed = Case("rs", n, code, 6001, ((2, 2),) * n, name="misaligned", **ONE_CH)
    units = Case("rs", n, code, ALT_BLOCK[code], ((0, 0),) * n, name="aligned", **ONE_CH)
    return typed, units


# =====================================================================================
# inputs, expectations, buffers
# =====================================================================================
_inputs, _expected = {}, {}


def inputs(case):
    """Per-rank inputs of a case, the same for every offset assignment; read-only."""
    n = case.n
    key = (case.func, n, case.code, case.count)
    if key not in _inputs:
        rng = np.random.default_rng(zlib.crc32(repr(key).encode()))
        if case.func == "a2a":
            xs = a2a_ref.make_inputs(n, case.count, salt=case.count % 7)
        elif case.func in ("ag", "bc"):
            xs = [rng.integers(0, 256, case.count, dtype=np.uint8) for _ in range(n)]
        else:
            xs = [gen(case.code, case.count * (n if case.func == "rs" else 1), rng) for _ in range(n)]
        for x in xs:
            x.setflags(write=False)
        _inputs[key] = xs
    return _inputs[key]


def expected(orc, case):
    """Per-rank expected destination contents (None where a rank has none),
    computed once per (function, n, type, count, root, geometry)."""
    nch, nthr, rings = selected(case) if case.func in ("rs", "rd") else (0, 0, None)
    key = (case.func, case.n, case.code, case.count, case.root, nch, nthr, str(rings), case.buffer_size)
    if key in _expected:
        return _expected[key]
    xs, n = inputs(case), case.n
    if case.func == "rs":
        exp = rs_ref.expected(orc, xs, case.code, SUM, nch, nthr, rings, case.buffer_size)
    elif case.func == "rd":
        one = rooted_ref.reduce_expected(orc, xs, case.code, SUM, case.root, nch, nthr, rings, case.buffer_size)
        exp = [one if r == case.root else None for r in range(n)]
    elif case.func == "bc":
        exp = [rooted_ref.broadcast_expected(xs, case.root)] * n
    elif case.func == "ag":
        exp = [np.concatenate(xs)] * n
    else:
        exp = a2a_ref.expected(xs, case.count)
    _expected[key] = exp
    return exp


def can_fail_message(case, exp):
    """'' when a wrong result of the case would show: every destination's
    expectation differs from each single input that could have been left or
    copied there (the NOT prefill differs from it in every byte by
    construction, which the CPU test checks on the buffers themselves)."""
    xs, n, cnt = inputs(case), case.n, case.count
    for r in range(n):
        if exp[r] is None:
            continue
        e = np.ascontiguousarray(exp[r]).view(np.uint8).reshape(-1)
        if e.size == 0:
            return f"rank {r}: nothing expected"
        if case.func == "rs":
            rivals = [xs[s][r * cnt:(r + 1) * cnt] for s in range(n)]
        elif case.func == "rd":
            rivals = list(xs)
        elif case.func == "a2a":
            rivals = list(xs)
        elif case.func == "ag":  # every other order of the blocks
            rivals = [np.concatenate([xs[(s + k) % n] for s in range(n)]) for k in range(1, n)]
        else:  # a Broadcast left undone shows through the prefill alone; another rank's
            rivals = []  # bytes do not exist (null sendbuff)
        for k, x in enumerate(rivals):
            if np.array_equal(np.ascontiguousarray(x).view(np.uint8).reshape(-1), e):
                return f"rank {r}: the expectation equals input {k}"
    return ""


class Buffers:
    """The guarded buffers of one call of a case on `device`, filled: sources
    written, destinations prefilled with the NOT of their expectation.
    `send` / `recv` are the pointers the ranks pass (0 = null)."""

    def __init__(self, case, xs, exp, device="cpu"):
        n, es, cnt = case.n, 1 if case.func in BYTE_FUNCS else case.es, case.count
        self.case, self.exp = case, exp
        self.sends, self.recvs = [None] * n, [None] * n
        self.send, self.recv = [0] * n, [0] * n
        for r in range(n):
            so, ro = case.offs[r]
            x = np.ascontiguousarray(xs[r]).view(np.uint8).reshape(-1)
            if case.func == "rs":
                s = self.sends[r] = Guarded(x.size, so, device)
                s.write(x)
                self.send[r] = s.ptr
                if case.inplace:
                    self.recv[r] = s.ptr + r * cnt * es
                else:
                    d = self.recvs[r] = Guarded(cnt * es, ro, device)
                    d.prefill_not(exp[r])
                    self.recv[r] = d.ptr
            elif case.func == "ag":
                d = self.recvs[r] = Guarded(n * cnt, ro, device)
                d.prefill_not(exp[r])
                self.recv[r] = d.ptr
                if case.inplace:
                    d.poke(r * cnt, x)
                    self.send[r] = d.ptr + r * cnt
                else:
                    s = self.sends[r] = Guarded(cnt, so, device)
                    s.write(x)
                    self.send[r] = s.ptr
            elif case.func == "a2a":
                s = self.sends[r] = Guarded(n * cnt, so, device)
                s.write(x)
                d = self.recvs[r] = Guarded(n * cnt, ro, device)
                d.prefill_not(exp[r])
                self.send[r], self.recv[r] = s.ptr, d.ptr
            elif case.func == "bc":
                if r == case.root and case.inplace:
                    d = self.recvs[r] = Guarded(cnt, so, device)
                    d.write(x)
                    self.send[r] = d.ptr
                else:
                    d = self.recvs[r] = Guarded(cnt, ro, device)
                    d.prefill_not(exp[r])
                    if r == case.root:
                        s = self.sends[r] = Guarded(cnt, so, device)
                        s.write(x)
                        self.send[r] = s.ptr
                self.recv[r] = d.ptr
            else:  # rd: every rank passes a guarded recvbuff, only the root's may change
                s = self.sends[r] = Guarded(cnt * es, so, device)
                s.write(x)
                self.send[r] = s.ptr
                if r == case.root and case.inplace:
                    self.recv[r] = s.ptr
                else:
                    d = self.recvs[r] = Guarded(cnt * es, ro, device)
                    if r == case.root:
                        d.prefill_not(exp[r])
                    self.recv[r] = d.ptr

    def check(self):
        """{rank: what went wrong}: the result bit for bit, every pad, and
        every buffer that is no destination unchanged."""
        case, xs = self.case, inputs(self.case)
        n, cnt = case.n, case.count
        bad = {}
        for r in range(n):
            s, d, msg = self.sends[r], self.recvs[r], ""
            if case.func == "rs" and case.inplace:  # only the rank's own block may change
                want = xs[r].copy()
                want[r * cnt:(r + 1) * cnt] = self.exp[r]
                msg = F.diff_message(s.read(), want) or s.pads_message()
            elif case.func == "rd" and r == case.root and case.inplace:
                msg = F.diff_message(s.read(), self.exp[r]) or s.pads_message()
            elif case.func == "rd" and r != case.root:
                msg = d.source_message() or s.source_message()
            else:
                msg = F.diff_message(d.read(), self.exp[r]) or d.pads_message() or (s.source_message() if s else "")
            if msg:
                bad[r] = msg
        return bad


def host_run(case, b):
    """The case on the host-thread ring (no GPU), on the buffers `b`."""
    nthr, _, elems = elements(case)
    rings = rings_of(case)
    sel = [rings[ch] for ch, _, _ in elems]
    kw = dict(nthreads=nthr, buffer_size=case.buffer_size)
    null = lambda ps: [p or None for p in ps]
    if case.func == "rs":
        C.host_ring_reduce_scatter(b.send, b.recv, case.count, case.code, SUM, channels=len(sel), rings=sel, **kw)
    elif case.func == "rd":
        C.host_ring_reduce(b.send, b.recv, case.count, case.code, SUM, case.root, channels=len(sel), rings=sel, **kw)
    elif case.func == "bc":
        C.host_ring_broadcast(null(b.send), b.recv, case.count, case.root, channels=len(sel), rings=sel, **kw)
    elif case.func == "a2a":
        C.host_ring_all_to_all(b.send, b.recv, case.count, channels=len(rings), rings=rings, force_relay=case.relay,
                               **kw)
    else:
        raise AssertionError("the host ring has no AllGather of its own")


def with_count(case, count):
    return replace(case, count=count)
