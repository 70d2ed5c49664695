"""CPU: the one chunk walk every path shares (mccs_amd/csrc/ring_walk.h).

mccs_ring_walk prints the walk of one work element with the header's own
functions, in the ring's 64-bit and the direct kernels' 32-bit arithmetic.
Here the 64-bit walk is held to the Python models, which never call the
library: ring_sim.rank_program for AllReduce, rs_ref.pieces for
ReduceScatter, and for AllGather all_gather.h:14-36 restated below together
with what the oracle's AllGather (a whole-block copy) needs of a walk, that
its non-empty chunks tile the block exactly once.  Then the 32-bit walk is
held to the 64-bit one, up to the largest bucket the direct path accepts.
"""
import ctypes
import itertools

import numpy as np
import pytest

from mccs_amd import comm as C
import ring_sim
import rs_ref

NS, NCHS, ESIZES, THREADS, BUFFS = (2, 3, 8), (1, 2, 7), (1, 2, 8), (96, 544), (8192, 4 << 20)
FUNCS = (C.FUNC_ALLREDUCE, C.FUNC_ALLGATHER, C.FUNC_REDUCE_SCATTER)
CODE_OF_ESIZE = {1: 0, 2: 6, 8: 4}  # a dtype code of that size for rs_ref.pieces (int8, float16, int64)
GRID = list(itertools.product(NS, NCHS, ESIZES, THREADS, BUFFS))


def geometry(func, n, nch, es, thr, buff):
    """(chunk, gran, parts, loop) in elements, from all_reduce.h:17-21,34 / all_gather.h:14-18,31."""
    chunk = buff // 8 // es * 4
    gran = max(1, (thr - 32) * 8 // es)
    parts = nch * n if func == C.FUNC_ALLREDUCE else nch
    return chunk, gran, parts, parts * chunk


def counts(func, n, nch, es, thr, buff):
    """The smallest counts at which each branch of the walk can go wrong."""
    chunk, gran, parts, loop = geometry(func, n, nch, es, thr, buff)
    out = [1, gran - 1, gran, gran + 1, parts * gran - 1, parts * gran + 1,
           loop - 1, loop, loop + 1,
           2 * loop + gran + 1]  # two loops and a tail of two chunks: the other parts of its loop are empty
    if func != C.FUNC_ALLREDUCE:
        out.append((nch - 1) * gran - 1)  # a block shorter than nch * gran: trailing channels get nelem <= 0
    return sorted({c for c in out if c >= 1})


def cases(funcs=FUNCS):
    for func in funcs:
        for g in GRID:
            for count in counts(func, *g):
                yield (func, *g, count)


def model_allreduce(n, nch, es, thr, buff, count):
    """Rows from ring_sim.rank_program: the rank at ring index r of channel bid
    owns chunk r, the one its recvReduceCopySend call works on."""
    per_loop = {}
    for bid in range(nch):
        for r in range(n):
            prog = list(ring_sim.rank_program(r, n, count, nch, bid, thr, buff, es))
            assert len(prog) % (2 * n - 1) == 0
            for loop_ix in range(len(prog) // (2 * n - 1)):
                calls = prog[loop_ix * (2 * n - 1):(loop_ix + 1) * (2 * n - 1)]
                assert calls[n - 1][0] == "recvReduceCopySend"
                per_loop.setdefault(loop_ix, {})[bid * n + r] = (calls[n - 1][1], max(0, calls[n - 1][2]))
                # the n reducing calls visit the channel's n chunks once each
                per_loop[loop_ix].setdefault(("visited", bid), set()).add(
                    tuple(sorted((o, max(0, m)) for _, o, m in calls[:n])))
    return per_loop


def model_allgather(nch, es, thr, buff, count):
    """all_gather.h:14-36: (gridOffset, realChunkSize, chunkOffset, nelem) per loop and channel."""
    chunk = buff // 8 // es * 4
    loop = nch * chunk
    gran = (thr - 32) * 8 // es
    rows = []
    for g in range(0, count, loop):
        rcs = min(chunk, -(-(count - g) // nch))
        rcs = -(-rcs // gran) * gran
        for bid in range(nch):
            off = g + bid * rcs
            rows.append((g, rcs, off, max(0, min(rcs, count - off))))
    return rows


@pytest.mark.parametrize("n,nch,es,thr,buff", GRID)
def test_walk_matches_the_models(lib, n, nch, es, thr, buff):
    for count in counts(C.FUNC_ALLREDUCE, n, nch, es, thr, buff):
        rows = C.ring_walk(C.FUNC_ALLREDUCE, n, nch, es, thr, buff, count)
        model = model_allreduce(n, nch, es, thr, buff, count)
        assert len(rows) == len(model) * nch * n, (count, len(rows))
        for i, (g, rcs, off, nelem) in enumerate(rows):
            loop_ix, part = divmod(i, nch * n)
            assert (off, nelem) == model[loop_ix][part], (count, i, rows[i], model[loop_ix][part])
        for loop_ix, m in model.items():
            for bid in range(nch):
                got = tuple(sorted((o, ne) for _, _, o, ne in rows[(loop_ix * nch + bid) * n:(loop_ix * nch + bid + 1) * n]))
                assert m[("visited", bid)] == {got}, (count, loop_ix, bid)
    for count in counts(C.FUNC_REDUCE_SCATTER, n, nch, es, thr, buff):
        rows = C.ring_walk(C.FUNC_REDUCE_SCATTER, n, nch, es, thr, buff, count)
        got = [(i % nch, off, nelem) for i, (_, _, off, nelem) in enumerate(rows) if nelem > 0]
        assert got == rs_ref.pieces(count, CODE_OF_ESIZE[es], nch, thr, buff), count
        assert all(nelem == 0 for _, rcs, off, nelem in rows if off >= count), count
    for count in counts(C.FUNC_ALLGATHER, n, nch, es, thr, buff):
        rows = C.ring_walk(C.FUNC_ALLGATHER, n, nch, es, thr, buff, count)
        assert rows == model_allgather(nch, es, thr, buff, count), count
        # the oracle copies each block whole: the non-empty chunks tile [0, count) once, in order
        end = 0
        for _, _, off, nelem in rows:
            if nelem:
                assert off == end, (count, off, end)
                end += nelem
        assert end == count, count


def test_counts_reach_every_branch():
    """The count list is not vacuous: over the grid it holds single-chunk and
    multi-loop walks, walks whose last chunks are empty, rounded and capped
    chunk sizes, and block walks with channels past the end."""
    seen = set()
    for func, n, nch, es, thr, buff, count in cases():
        chunk, gran, parts, loop = geometry(func, n, nch, es, thr, buff)
        rows = C.ring_walk(func, n, nch, es, thr, buff, count)
        seen.add("loops>1" if len(rows) > parts else "one loop")
        for g, rcs, off, nelem in rows:
            if rcs == chunk:
                seen.add("capped")
            if rcs > min(chunk, -(-(count - g) // parts)):
                seen.add("rounded up")
            if off >= count and parts > 1:
                seen.add("empty part, AllReduce" if func == C.FUNC_ALLREDUCE else "empty part, block")
            if 0 < nelem < rcs:
                seen.add("partial chunk")
    assert seen == {"loops>1", "one loop", "capped", "rounded up", "empty part, AllReduce", "empty part, block",
                    "partial chunk"}, seen


# the largest buckets the direct path accepts: validate_cfg caps direct_bytes at 1 GiB
LARGEST = [(1, 1 << 30), (2, 1 << 29), (8, 1 << 27)]


def walk_array(lib, width, *args):
    """The walk as an (rows, 4) int64 array (up to 2^18 rows at the largest buckets)."""
    n = lib.mccs_ring_walk(*args, width, None, 0)
    assert n > 0, args
    rows = np.empty((n, 4), dtype=np.int64)
    assert lib.mccs_ring_walk(*args, width, rows.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong)), n) == n
    return rows


def test_32_bit_walk_equals_the_64_bit_walk(lib):
    for func, n, nch, es, thr, buff, count in cases():
        assert C.ring_walk(func, n, nch, es, thr, buff, count, 32) == \
            C.ring_walk(func, n, nch, es, thr, buff, count, 64), (func, n, nch, es, thr, buff, count)
    for (es, count), n, nch, thr, buff in itertools.product(LARGEST, NS, NCHS + (32,), THREADS, BUFFS):
        for c in (count, count - 1):
            w32 = walk_array(lib, 32, C.FUNC_ALLREDUCE, n, nch, es, thr, buff, c)
            w64 = walk_array(lib, 64, C.FUNC_ALLREDUCE, n, nch, es, thr, buff, c)
            assert np.array_equal(w32, w64), (n, nch, es, thr, buff, c)
            assert int(w64[:, 3].sum()) == c


def test_invalid_arguments(lib):
    ok = (C.FUNC_ALLREDUCE, 2, 1, 4, 96, 8192, 100)
    assert len(C.ring_walk(*ok)) == 2
    for bad in [(0,) + ok[1:], ok[:1] + (0,) + ok[2:], ok[:2] + (0,) + ok[3:], ok[:3] + (0,) + ok[4:],
                ok[:4] + (32,) + ok[5:], ok[:5] + (1000,) + ok[6:]]:
        with pytest.raises(ValueError):
            C.ring_walk(*bad)
    with pytest.raises(ValueError):
        C.ring_walk(*ok, width=16)
    with pytest.raises(ValueError):
        C.ring_walk(*ok[:6], 1 << 31, width=32)
