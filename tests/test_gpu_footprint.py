"""GPU: no kernel writes outside its output, at every mix of alignments.

Every buffer is a footprint.Guarded one: 16 KiB of seeded noise on both sides
of the payload, the payload at a chosen byte offset from a 256-byte line, a
destination prefilled with the bitwise NOT of what is expected there.  After
each call the results equal the oracle's bit for bit (alignment only selects
the path: 16-byte packs, wave units, remainder packs, typed tail, the
all-or-nothing typed fallback, LL's partial last word), every destination's
pads are intact and every source that is no destination is unchanged.

The offsets of the operands are chosen independently of each other and differ
between ranks: the kernels decide between their pack and typed paths from the
alignment of all operands together (reduce.hip dispatch, ring_stream.h
reduce_copy_rows_dyn per slice, direct_kernel.h direct_reduce over every
peer's pointer, the LL words' in/out/segment alignment separately).

Which path a case reaches is worked out from its count (chunk_paths,
ring_paths, ll_paths below) and every test asserts that the paths it is
meant to reach were reached.  The last section calls the unmodified kernels
with count + 1 elements on buffers guarded for count: the checker must report
exactly the extra element.
"""
import numpy as np
import pytest

import footprint as F
import ring_sim
import vnode
from footprint import Guarded
from footprint_cases import assignments, gen, lane_parts, offset_set, ring_paths  # noqa: F401  (moved there)
from mccs_amd import comm as C

pytestmark = pytest.mark.gpu
DIRECT_DEFAULTS = True  # conftest: thresholds are set per communicator below

I8, I64, F16, F32, F64 = 0, 4, 6, 7, 8
SUM, MAX = 0, 2
NPDT, ESIZE = vnode.NPDT, vnode.ESIZE
RING_ONLY = dict(direct_bytes=-1, oneshot_bytes=-1, ll_bytes=-1)
DIRECT, LL_MAX = 8 << 20, 1 << 20
DEV = "cuda"


# =====================================================================================
# (a) chunk reduce, mccs_amd.reduce_copy with raw pointers
# =====================================================================================
# (U, S, W) the LDS loop is compiled for (reduce.hip launch_lds_cfg): the
# default for every type and op, the others for Sum over fp32 / fp16 / bf16
LDS_DEFAULT = (4, 2, 4)
LDS_GRID = {(4, 2, 4), (1, 3, 4), (2, 2, 4), (2, 3, 4), (4, 3, 4), (4, 4, 4), (8, 2, 4), (4, 3, 5), (2, 3, 6),
            (4, 2, 6), (4, 3, 6), (1, 2, 8), (2, 2, 8), (4, 2, 8)}
VARIANT_LDS = 2


def kernel_tile(code, op, nsrcs, ndsts):
    """(packs in one workgroup's tile, "lds" or "reg", LDS stages, packs in
    one wave's tile) of the main loop reduce.hip's dispatch picks for aligned
    operands under the current get_tune()."""
    import mccs_amd

    t = mccs_amd.get_tune()
    tuned = op == SUM and code in (F16, F32, 9)
    usw = (t["unroll"], t["stages"], t["waves"])
    if t["variant"] == VARIANT_LDS and (nsrcs, ndsts) == (2, 1) and (usw == LDS_DEFAULT or (tuned and usw in LDS_GRID)):
        return t["waves"] * 64 * t["unroll"], "lds", t["stages"], 64 * t["unroll"]
    unroll = t["unroll"] if t["variant"] != VARIANT_LDS else 4
    if not tuned or (nsrcs, ndsts) not in ((2, 1), (1, 1)) or unroll not in (2, 4, 8):
        unroll = 4
    return 256 * unroll, "reg", 0, 256 * unroll


def chunk_counts(code, op, nsrcs, ndsts):
    """(small counts, the count for one workgroup under tune_grid(1))."""
    pack = 16 // ESIZE[code]
    tile_packs, _, stages, _ = kernel_tile(code, op, nsrcs, ndsts)
    tile = tile_packs * pack
    small = sorted({1, pack - 1, pack, pack + 1, 255 * pack + 1, tile - pack + 1, tile, tile + 1})
    return small, ((stages or 2) + 2) * tile + pack + (pack - 1)


def chunk_paths(code, op, nsrcs, ndsts, count, aligned, one_block=False):
    """The parts of reduce.hip a case reaches, from its count."""
    if not aligned:
        return {"scalar kernel"}
    pack = 16 // ESIZE[code]
    tile_packs, kind, stages, wave_tile = kernel_tile(code, op, nsrcs, ndsts)
    npack = count // pack
    out = set()
    if npack >= tile_packs:
        out.add("full tile")
    if npack % tile_packs:
        out.add("partial tile")
    if count % pack:
        out.add("typed tail")
    if npack == 0:
        out.add("no pack")
    if kind == "lds" and one_block:
        waves = tile_packs // wave_tile
        tiles_per_wave = -(-npack // wave_tile) // waves
        if tiles_per_wave > stages:
            out.add("lds ring wraps")
    return out


PATTERNS = ["0", "es", "dst", "src1", "src0", "16-es", "8", "src1=8", "phase"]
ALIGNED_PATTERNS = ["0", "phase"]


def pattern_offsets(pattern, nsrcs, ndsts, es):
    """Byte offsets of (sources, destinations).  For two sources and one
    destination: "0" (0, 0, 0), "es" (es, es, es), "dst" (0, 0, es), "src1"
    (0, es, 0), "src0" (es, 0, 0), "16-es" (16 - es, 0, 0), "8" (8, 8, 8),
    "src1=8" (0, 8, 0), "phase" (16, 32, 48): aligned, at different phases
    of a 256-byte line."""
    s, d = [0] * nsrcs, [0] * ndsts
    if pattern == "es":
        s, d = [es] * nsrcs, [es] * ndsts
    elif pattern == "dst":
        d[-1] = es
    elif pattern == "src1":
        s[-1] = es
    elif pattern == "src0":
        s[0] = es
    elif pattern == "16-es":
        s[0] = 16 - es
    elif pattern == "8":
        s, d = [8] * nsrcs, [8] * ndsts
    elif pattern == "src1=8":
        s[-1] = 8
    elif pattern == "phase":
        s = [16 * (i + 1) for i in range(nsrcs)]
        d = [16 * (nsrcs + j + 1) for j in range(ndsts)]
    else:
        assert pattern == "0"
    return s, d


def patterns_for(es):
    return [p for p in PATTERNS if es < 8 or p not in ("8", "src1=8")]


def run_chunk(code, op, xs, exp, soffs, doffs, alias=None, count=None):
    """One reduce_copy on guarded buffers; alias = index of the destination
    that is src[0] itself (in place).  Returns '' or what went wrong."""
    import mccs_amd
    import torch

    count = xs[0].size if count is None else count
    srcs = [Guarded(x.nbytes, o, DEV) for x, o in zip(xs, soffs)]
    for g, x in zip(srcs, xs):
        g.write(x)
    dsts = []
    for j, o in enumerate(doffs):
        if j == alias:
            dsts.append(srcs[0])
        else:
            g = Guarded(exp[j].nbytes, o, DEV)
            g.prefill_not(exp[j])
            dsts.append(g)
    mccs_amd.reduce_copy([g.ptr for g in dsts], [g.ptr for g in srcs], count=count, dtype=code, op=op)
    torch.cuda.synchronize()
    for j, g in enumerate(dsts):
        msg = F.diff_message(g.read()[:exp[j].nbytes], exp[j]) or g.pads_message()
        if msg:
            return f"dst {j}: {msg}"
    for i, g in enumerate(srcs):
        if not (i == 0 and alias is not None) and g.source_message():
            return f"src {i}: {g.source_message()}"
    return ""


def sweep_chunk(orc, code, op, nsrcs, ndsts, patterns, alias=None, inplace_patterns=(), seed=0):
    """Every count x offset pattern for one type, op and fan under the current
    tune; the one-workgroup count under tune_grid(1).  Returns (failures,
    paths reached)."""
    import mccs_amd

    es = ESIZE[code]
    rng = np.random.default_rng(1000 * code + 10 * nsrcs + ndsts + seed)
    small, big = chunk_counts(code, op, nsrcs, ndsts)
    bad, reached = {}, set()

    def one(count, one_block):
        xs = [gen(code, count, rng) for _ in range(nsrcs)]
        exp = orc.reduce_copy(code, op, xs, ndsts)
        for pat in patterns:
            soffs, doffs = pattern_offsets(pat, nsrcs, ndsts, es)
            modes = [alias] if alias is not None else [None] + ([0] if pat in inplace_patterns else [])
            for al in modes:
                if al is not None:
                    doffs = list(doffs)
                    doffs[al] = soffs[0]
                aligned = all(o % 16 == 0 for o in soffs + list(doffs))
                reached.update(chunk_paths(code, op, nsrcs, ndsts, count, aligned, one_block))
                if al is not None:
                    reached.add("in place" + (", lds" if aligned and one_block and
                                              kernel_tile(code, op, nsrcs, ndsts)[1] == "lds" else ""))
                msg = run_chunk(code, op, xs, exp, soffs, doffs, alias=al)
                if msg:
                    bad[(count, pat, al)] = msg

    for count in small:
        one(count, False)
    mccs_amd.tune_grid(1)
    try:
        one(big, True)
    finally:
        mccs_amd.tune_grid(0)
    return bad, reached


@pytest.mark.parametrize("code,op", [(I8, SUM), (F16, SUM), (F32, SUM), (F64, SUM), (F16, MAX)],
                         ids=["int8", "fp16", "fp32", "fp64", "fp16-max"])
def test_chunk_reduce_footprint(orc, code, op):
    """Two sources, one destination under the default tune: the LDS loop, its
    last block's typed tail and, for any misaligned operand, the scalar
    kernel; out of place and in place."""
    import mccs_amd

    mccs_amd.tune()
    mccs_amd.tune_grid(0)
    assert kernel_tile(code, op, 2, 1)[1] == "lds"
    bad, reached = sweep_chunk(orc, code, op, 2, 1, patterns_for(ESIZE[code]),
                               inplace_patterns=("0", "es", "src1", "phase"))
    assert not bad, F.brief(bad)
    assert reached >= {"scalar kernel", "full tile", "partial tile", "typed tail", "no pack", "lds ring wraps",
                       "in place", "in place, lds"}, reached


# (variant, unroll, policy, blocks_per_cu, stages, waves) of test_reduce_variants
# with the most distinct tile shapes: REG 512 and 2048 packs per tile, LDS
# 256 (3 stages), 2048 (2 stages), 768 (6 waves) and 1024 (4 stages), the
# blocked and the wave-row REG maps
VARIANT_ROWS = [(1, 2, 0, 4, 0, 0), (1, 8, 1, 2, 0, 0), (2, 1, 1, 1, 3, 4), (2, 8, 1, 1, 2, 4), (2, 2, 2, 2, 3, 6),
                (2, 4, 1, 1, 4, 4), (3, 4, 1, 16, 0, 0), (4, 8, 1, 16, 0, 0)]


@pytest.mark.parametrize("row", VARIANT_ROWS, ids=[str(r) for r in VARIANT_ROWS])
def test_chunk_reduce_footprint_variants(orc, row):
    import mccs_amd

    mccs_amd.tune(*row)
    try:
        for code in (F16, F32):
            tile_packs, kind, stages, _ = kernel_tile(code, SUM, 2, 1)
            assert kind == ("lds" if row[0] == VARIANT_LDS else "reg")
            assert tile_packs == (row[5] * 64 * row[1] if kind == "lds" else 256 * row[1])
            bad, reached = sweep_chunk(orc, code, SUM, 2, 1, ALIGNED_PATTERNS, inplace_patterns=("0",), seed=row[1])
            assert not bad, (code, F.brief(bad))
            want = {"full tile", "partial tile", "typed tail", "no pack", "in place"}
            assert reached >= (want | {"lds ring wraps", "in place, lds"} if kind == "lds" else want), reached
    finally:
        mccs_amd.tune()
        mccs_amd.tune_grid(0)


@pytest.mark.parametrize("nsrcs,ndsts,alias", [(1, 1, None), (3, 2, None), (8, 4, None), (2, 2, 0)],
                         ids=["1to1", "3to2", "8to4", "2to2-dst0-is-src0"])
def test_chunk_reduce_footprint_fans(orc, nsrcs, ndsts, alias):
    """Copies and fan-outs (the run-time REG loop), and the header's "dst may
    alias src[0]" with a second destination."""
    import mccs_amd

    mccs_amd.tune()
    mccs_amd.tune_grid(0)
    for code in (I8, F16, F32, F64):
        assert kernel_tile(code, SUM, nsrcs, ndsts)[1] == "reg"
        bad, reached = sweep_chunk(orc, code, SUM, nsrcs, ndsts, patterns_for(ESIZE[code]), alias=alias)
        assert not bad, (code, F.brief(bad))
        assert reached >= {"scalar kernel", "full tile", "partial tile", "typed tail", "no pack"}, reached


# =====================================================================================
# (b), (c) collectives on the virtual node
# =====================================================================================
def run_allreduce(comms, inputs, exp, code, offs, inplace, want_algo, count=None):
    """One grouped AllReduce on guarded buffers; returns {rank: what went wrong}."""
    n, nbytes = len(comms), exp.nbytes
    count = exp.size if count is None else count
    send = [Guarded(inputs[r].nbytes, offs[r][0], DEV) for r in range(n)]
    recv = send if inplace else [Guarded(nbytes, offs[r][1], DEV) for r in range(n)]
    for r in range(n):
        send[r].write(inputs[r])
        if not inplace:
            recv[r].prefill_not(exp)
    with C.group():
        for r in range(n):
            C.all_reduce(comms[r], send[r].ptr, recv[r].ptr, count, code, SUM)
    for c in comms:
        c.sync()
    algos = {c.last_algo() for c in comms}
    assert algos == {want_algo}, (algos, want_algo)
    bad = {}
    for r in range(n):
        msg = (F.diff_message(recv[r].read()[:nbytes], exp) or recv[r].pads_message()
               or ("" if inplace else send[r].source_message()))
        if msg:
            bad[r] = msg
    return bad


def ring_chunks(n, count, nch, nthr, buff, es):
    """Element counts of the chunks of every loop of every channel."""
    out = []
    for bid in range(nch):
        for prim, off, nelem in ring_sim.rank_program(0, n, count, nch, bid, nthr, buff, es):
            if prim in ("send", "recvReduceSend", "recvReduceCopySend"):  # each chunk once
                out.append(max(nelem, 0))
    return out


def ring_loops(n, count, nch, nthr, buff, es):
    return len(list(ring_sim.rank_program(0, n, count, nch, 0, nthr, buff, es))) // (2 * n - 1)


def sweep_ring(orc, comms, cases, buff=1 << 22, only=None, seed=0):
    """cases: (dtype code, count); every offset assignment for each.  Returns
    (failures, paths reached)."""
    n = len(comms)
    rng = np.random.default_rng(seed + n)
    bad, reached = {}, set()
    for code, count in cases:
        es = ESIZE[code]
        inputs = [gen(code, count, rng) for _ in range(n)]
        exp = vnode.expected_allreduce(orc, inputs, code, SUM, comms[0], buff_size=buff)
        nch, nthr, _ = vnode.Planner(comms[0].nchannels, comms[0].rings()).select(count * es, count * es)
        chunks = ring_chunks(n, count, nch, nthr, buff, es)
        assert sum(chunks) == count
        for name, offs, inplace in assignments(n, es):
            if only is not None and name not in only:
                continue
            aligned = all(o % 16 == 0 for pair in offs for o in pair)
            reached.update(ring_paths(chunks, es, aligned, comms[0].lanes, buff))
            for r, msg in run_allreduce(comms, inputs, exp, code, offs, inplace, "ring").items():
                bad[(code, count, name, r)] = msg
    return bad, reached


def ring_cases(n):
    out = []
    for code in (F16, F32, I8) + ((I64,) if n == 2 else ()):
        pack = 16 // ESIZE[code]
        out += [(code, c) for c in sorted({1, n - 1, pack + 1, n * pack + 1, 4097})]
    return out


@pytest.mark.parametrize("n", [2, 3, 8])
def test_ring_footprint(orc, n):
    comms = C.init_all([0] * n, C.CommConfig(**RING_ONLY))
    try:
        bad, reached = sweep_ring(orc, comms, ring_cases(n))
        assert not bad, F.brief(bad)
        want = {"typed fallback", "remainder packs", "typed tail", "no pack"} | ({"empty chunk"} if n > 2 else set())
        assert reached >= want, reached
    finally:
        vnode.destroy(comms)


@pytest.mark.parametrize("n", [2, 3, 8])
def test_ring_footprint_several_loops(orc, n):
    """A 1 MiB FIFO buffer on one channel of 4 lanes: two whole loops of n
    chunks of 512 KiB and a partial third, so every lane's part of a slice
    holds whole wave units and a slice's base moves through the user buffers."""
    buff, code = 1 << 20, F16
    comms = C.init_all([0] * n, C.CommConfig(buffer_size=buff, channel_count=1, lanes=4, **RING_ONLY))
    try:
        chunk = ring_sim.chunk_size_elems(buff, ESIZE[code])
        assert comms[0].nchannels == 1 and comms[0].lanes == 4
        count = 2 * n * chunk + chunk + 4099
        nch, nthr, _ = vnode.Planner(1, comms[0].rings()).select(count * ESIZE[code], count * ESIZE[code])
        assert nch == 1 and ring_loops(n, count, nch, nthr, buff, ESIZE[code]) == 3 and count % (n * chunk) != 0
        bad, reached = sweep_ring(orc, comms, [(code, count)], buff=buff,
                                  only=("send+0 recv+0", "per rank", "only rank 0's recv", "in place, per rank"))
        assert not bad, F.brief(bad)
        assert reached >= {"wave units", "typed tail", "typed fallback"}, reached
    finally:
        vnode.destroy(comms)


@pytest.mark.parametrize("cfg,n,counts", [(dict(lanes=64, channel_count=2), 2, (5000, 5001)),
                                          (dict(block_threads=96, lanes=2), 4, (4097,))],
                         ids=["64-lanes", "96-threads"])
def test_ring_footprint_launch_shapes(orc, cfg, n, counts):
    """test_wide_lanes' shape (each lane a fixed region of a slot group; 5000
    elements leave every lane whole packs, 5001 a typed tail too) and a block
    that is not whole waves."""
    comms = C.init_all([0] * n, C.CommConfig(**cfg, **RING_ONLY))
    try:
        assert comms[0].lanes == cfg["lanes"]
        bad, reached = sweep_ring(orc, comms, [(code, c) for c in counts for code in (F32, F16)])
        assert not bad, F.brief(bad)
        assert reached >= {"remainder packs", "typed tail", "typed fallback"}, reached
    finally:
        vnode.destroy(comms)


def run_allgather(comms, data, out_offs, send_offs, inplace, want_algo, nbytes=None):
    """One grouped AllGather; in place the send pointer is the rank's own
    segment of its output."""
    n = len(comms)
    size = data[0].size
    nbytes = size if nbytes is None else nbytes
    exp = np.concatenate(data)
    outs = [Guarded(n * size, out_offs[r], DEV) for r in range(n)]
    sends = [None if inplace else Guarded(size, send_offs[r], DEV) for r in range(n)]
    for r in range(n):
        outs[r].prefill_not(exp)
        if inplace:
            outs[r].poke(r * size, data[r])
        else:
            sends[r].write(data[r])
    with C.group():
        for r in range(n):
            C.all_gather(comms[r], outs[r].ptr + r * size if inplace else sends[r].ptr, outs[r].ptr, nbytes)
    for c in comms:
        c.sync()
    algos = {c.last_algo() for c in comms}
    assert algos == {want_algo}, (algos, want_algo)
    bad = {}
    for r in range(n):
        msg = (F.diff_message(outs[r].read(), exp) or outs[r].pads_message()
               or ("" if inplace else sends[r].source_message()))
        if msg:
            bad[r] = msg
    return bad


def sweep_allgather(comms, want_algo):
    n = len(comms)
    rng = np.random.default_rng(n)
    bad = {}
    for nbytes in (1, 13, 1000, 65539):
        data = [rng.integers(0, 256, nbytes, dtype=np.uint8) for _ in range(n)]
        for name, out_offs, send_offs, inplace in (
                ("out+0 send+0", [0] * n, [0] * n, False), ("out+1 send+0", [1] * n, [0] * n, False),
                ("out+0 send+1", [0] * n, [1] * n, False), ("out+1 send+8", [1] * n, [8] * n, False),
                ("per rank", [r % 2 for r in range(n)], [(3 * r) % 16 for r in range(n)], False),
                ("in place, out+0", [0] * n, None, True), ("in place, out+1", [1] * n, None, True),
                ("in place, per rank", [(r + 1) % 2 for r in range(n)], None, True)):
            for r, msg in run_allgather(comms, data, out_offs, send_offs, inplace, want_algo).items():
                bad[(nbytes, name, r)] = msg
    return bad


@pytest.mark.parametrize("n", [2, 8])
def test_ring_allgather_footprint(n):
    """Segments other than 0 start at odd addresses for odd sizes."""
    comms = C.init_all([0] * n, C.CommConfig(**RING_ONLY))
    try:
        bad = sweep_allgather(comms, "ring")
        assert not bad, F.brief(bad)
    finally:
        vnode.destroy(comms)


def _cfg(variant):
    """One direct kernel per communicator set, as test_gpu_direct._cfg."""
    return C.CommConfig(direct_bytes=DIRECT if variant == "direct" else -1,
                        oneshot_bytes=DIRECT if variant in ("oneshot", "ll") else -1,
                        ll_bytes=LL_MAX if variant == "ll" else -1)


# test_ll_ragged_and_in_place's ragged buckets, and one above a single
# workgroup's span (4 KiB: 512 threads x one 8-byte LL word, and the direct
# kernels' 4 KiB of phase-1 bytes per workgroup) whatever n
DIRECT_CASES = [(I8, 1), (I8, 13), (F16, 3), (F16, 4099), (F32, 7), (F64, 5), (F32, 5003)]
WG_SPAN = 4096


def ll_paths(code, count, offs):
    """ll_load_word / ll_store_word per operand: whole 8-byte words when the
    pointer is 8-byte aligned, a partial last word, typed elements otherwise."""
    out = set()
    nbytes = count * ESIZE[code]
    for pair in offs:
        for o in pair:
            if o % 8:
                out.add("typed words")
            else:
                if nbytes >= 8:
                    out.add("whole words")
                if nbytes % 8:
                    out.add("partial last word")
    return out


@pytest.mark.parametrize("n", [2, 3, 5])
@pytest.mark.parametrize("variant", ["direct", "oneshot", "ll"])
def test_direct_footprint(orc, variant, n):
    comms = C.init_all([0] * n, _cfg(variant))
    try:
        rng = np.random.default_rng(n)
        bad, reached = {}, set()
        assert any(c * ESIZE[code] * (n - 1) // n > WG_SPAN for code, c in DIRECT_CASES)
        for code, count in DIRECT_CASES:
            inputs = [gen(code, count, rng) for _ in range(n)]
            exp = vnode.expected_allreduce(orc, inputs, code, SUM, comms[0])
            for name, offs, inplace in assignments(n, ESIZE[code]):
                reached.update(ll_paths(code, count, offs))
                for r, msg in run_allreduce(comms, inputs, exp, code, offs, inplace, variant).items():
                    bad[(code, count, name, r)] = msg
        assert not bad, F.brief(bad)
        if variant == "ll":
            assert reached >= {"typed words", "whole words", "partial last word"}, reached
    finally:
        vnode.destroy(comms)


@pytest.mark.parametrize("n", [2, 3, 5])
@pytest.mark.parametrize("variant", ["oneshot", "ll"])
def test_direct_allgather_footprint(variant, n):
    comms = C.init_all([0] * n, _cfg(variant))
    try:
        bad = sweep_allgather(comms, variant)
        assert not bad, F.brief(bad)
    finally:
        vnode.destroy(comms)


# =====================================================================================
# (d) positive controls: the unmodified kernels asked for one element more
# =====================================================================================
def extra_element(exp_plus, count, es):
    """Bytes of element `count` of the count + 1 result, their NOT (what the
    destination's pad holds there before the call) and the offsets they fill."""
    last = exp_plus.view(np.uint8)[count * es:(count + 1) * es]
    return ~last, list(range(count * es, (count + 1) * es))


@pytest.mark.parametrize("code,count,off,path", [(F16, 4 * 8 - 1, 0, "pack"), (F32, 4 + 1, 0, "typed tail"),
                                                 (F32, 37, 4, "scalar kernel"), (I8, 1000, 1, "scalar kernel")])
def test_control_chunk_reduce_one_element_too_many(orc, code, count, off, path):
    """The extra element lies inside the destination's right pad: check()
    reports exactly its bytes, the payload is still the oracle's."""
    import mccs_amd
    import torch

    mccs_amd.tune()
    mccs_amd.tune_grid(0)
    es, pack = ESIZE[code], 16 // ESIZE[code]
    if path == "pack":  # the last element is stored as part of a 16-byte pack
        assert off == 0 and (count + 1) % pack == 0
    elif path == "typed tail":
        assert off == 0 and (count + 1) % pack != 0
    else:
        assert off % 16
    rng = np.random.default_rng(count)
    xs = [gen(code, count + 1, rng) for _ in range(2)]
    (exp,) = orc.reduce_copy(code, SUM, xs)
    srcs = [Guarded(x.nbytes, off, DEV) for x in xs]
    for g, x in zip(srcs, xs):
        g.write(x)
    dst = Guarded(count * es, off, DEV)
    dst.prefill_not(exp[:count])
    planted, where = extra_element(exp, count, es)
    dst.poke(count * es, planted)
    mccs_amd.reduce_copy([dst.ptr], [g.ptr for g in srcs], count=count + 1, dtype=code, op=SUM)
    torch.cuda.synchronize()
    assert dst.check().tolist() == where
    assert "wrote outside" in dst.pads_message() and str(where[0]) in dst.pads_message()
    assert not F.diff_message(dst.read(), exp[:count])
    assert all(g.unchanged() for g in srcs)


@pytest.mark.parametrize("variant,code,count,off", [("ring", F16, 4097, 0), ("ring", F32, 4097, 4),
                                                    ("ll", F16, 4099, 0), ("ll", I8, 13, 1)])
def test_control_allreduce_one_element_too_many(orc, variant, code, count, off):
    n, es = 2, ESIZE[code]
    comms = C.init_all([0] * n, C.CommConfig(**RING_ONLY) if variant == "ring" else _cfg("ll"))
    try:
        rng = np.random.default_rng(count)
        inputs = [gen(code, count + 1, rng) for _ in range(n)]
        exp = vnode.expected_allreduce(orc, inputs, code, SUM, comms[0])
        send = [Guarded(x.nbytes, off, DEV) for x in inputs]
        recv = [Guarded(count * es, off, DEV) for _ in range(n)]
        planted, where = extra_element(exp, count, es)
        for r in range(n):
            send[r].write(inputs[r])
            recv[r].prefill_not(exp[:count])
            recv[r].poke(count * es, planted)
        with C.group():
            for r in range(n):
                C.all_reduce(comms[r], send[r].ptr, recv[r].ptr, count + 1, code, SUM)
        for c in comms:
            c.sync()
        assert {c.last_algo() for c in comms} == {variant}
        for r in range(n):
            assert recv[r].check().tolist() == where, r
            assert not F.diff_message(recv[r].read(), exp[:count]), r
            assert send[r].unchanged(), r
    finally:
        vnode.destroy(comms)
