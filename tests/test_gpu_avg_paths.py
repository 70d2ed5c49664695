"""GPU: the code paths of the PreMulSum / SumPostDiv ring kernels, bit for bit
against tests/avg_ref.py.

One fp pair (fp32 PreMulSum by 1/3) and one integer pair (int32 SumPostDiv by
3) on communicators of n = 2 ranks on one GPU: one channel of one lane with
the default FIFO (a slice is one lane's piece: whole wave units, then packs,
then a tail shorter than a pack), the defaults, and one channel of one lane
with a 64 KiB FIFO (several loops).  Shapes: 21 003 elements; 3 elements (less
than a pack); both buffers one element past a 16-byte boundary (the unaligned
typed loop); in place.  Every buffer is canary-framed (tests/footprint.py):
nothing outside the receive range is written and, out of place, the send
buffer is unchanged.  Further: one rank, 96-thread workgroups, a non-identity
ring order at n = 4, a sequence with rooted calls in between, two calls of
different op_arg batched in one group, a replayed HIP graph, and one external
launch of a reference-named kernel.
"""
import ctypes

import numpy as np
import pytest

import avg_ref as A
import elem_ref as E
import rooted_ref
import vnode
from footprint import Guarded
from mccs_amd import _lib
from mccs_amd import comm as C
from test_gpu_avg_values import diff

pytestmark = pytest.mark.gpu
DIRECT_DEFAULTS = True

TIMEOUT_MS = 8000
F32, I32 = 7, 2
PAIRS = [(F32, A.PREMULSUM, A.avg_scalar_bits(F32, 3)), (I32, A.SUMPOSTDIV, 3)]
PAIR_IDS = ["fp32-premulsum", "int32-sumpostdiv"]
CONFIGS = {
    "one-lane": dict(channel_count=1, lanes=1),
    "defaults": dict(),
    "one-lane-64k": dict(channel_count=1, lanes=1, buffer_size=1 << 16),
}
FUNCS = ("all_reduce", "reduce_scatter", "reduce")
BIG = 21003  # per rank (per block for ReduceScatter): no multiple of a pack


def gen(code, count, rng):
    if code == F32:
        return rng.standard_normal(count).astype(np.float32)
    return rng.integers(-100000, 100000, count).astype(vnode.NPDT[code])


def plan_of(planner, func, code, n, count):
    """(nch, nthr, rings) for a call of `count` elements (per block for ReduceScatter)."""
    es = vnode.ESIZE[code]
    if func == "reduce_scatter":
        return planner.select(count * es * n, count * es)
    return planner.select(count * es, count * es)


def expected(func, inputs, code, op, arg, root, sel, buff):
    nch, nthr, rings = sel
    if func == "all_reduce":
        return A.allreduce_expected(inputs, code, op, arg, nch, nthr, rings, buff)
    if func == "reduce_scatter":
        return A.reduce_scatter_expected(inputs, code, op, arg, nch, nthr, rings, buff)
    out = A.reduce_expected(inputs, code, op, arg, root, nch, nthr, rings, buff)
    return [out if r == root else None for r in range(len(inputs))]


def issue(comms, func, send, recv, count, code, op, arg, root, stream=None):
    """One grouped call; send / recv are per-rank device addresses (recv None where unused)."""
    with C.group():
        for r, c in enumerate(comms):
            if func == "all_reduce":
                C.all_reduce(c, send[r], recv[r], count, code, op, stream=stream, op_arg=arg)
            elif func == "reduce_scatter":
                C.reduce_scatter(c, send[r], recv[r], count, code, op, stream=stream, op_arg=arg)
            else:
                C.reduce(c, send[r], recv[r] if r == root else None, count, code, op, root, stream=stream, op_arg=arg)


def framed_case(comms, func, code, op, arg, count, off_elems, inplace, buff, seed):
    """One call on canary-framed buffers; returns '' or what went wrong."""
    n, es = len(comms), vnode.ESIZE[code]
    root = n - 1
    rng = np.random.default_rng(seed)
    per_rank = count * (n if func == "reduce_scatter" else 1)
    inputs = [gen(code, per_rank, rng) for _ in range(n)]
    sel = plan_of(vnode.Planner(comms[0].nchannels, comms[0].rings()), func, code, n, count)
    exp = expected(func, inputs, code, op, arg, root, sel, buff)
    off = off_elems * es
    sbuf = [Guarded(per_rank * es, off, "cuda") for _ in range(n)]
    for r in range(n):
        sbuf[r].write(inputs[r])
    if inplace:
        rbuf = None
        recv = [sbuf[r].ptr + (r * count * es if func == "reduce_scatter" else 0) for r in range(n)]
    else:
        rbuf = [Guarded(count * es, off, "cuda") if exp[r] is not None else None for r in range(n)]
        for r in range(n):
            if rbuf[r] is not None:
                rbuf[r].prefill_not(exp[r])
        recv = [b.ptr if b is not None else None for b in rbuf]
    issue(comms, func, [b.ptr for b in sbuf], recv, count, code, op, arg, root)
    for c in comms:
        c.sync()
    assert {c.last_algo() for c in comms} == {"ring"}
    msgs = []
    for r in range(n):
        if inplace:
            msgs.append(sbuf[r].pads_message())
            if exp[r] is None:
                msgs.append(sbuf[r].source_message())
                continue
            lo = r * count if func == "reduce_scatter" else 0
            whole = sbuf[r].read(vnode.NPDT[code])
            msgs.append(diff(code, whole[lo:lo + count], exp[r]))
            if func == "reduce_scatter":  # the other blocks of the send buffer stay
                keep = np.ones(per_rank, bool)
                keep[lo:lo + count] = False
                msgs.append(diff(code, whole[keep], inputs[r][keep]))
        else:
            msgs.append(sbuf[r].source_message())
            if rbuf[r] is not None:
                msgs.append(rbuf[r].pads_message())
                msgs.append(diff(code, rbuf[r].read(vnode.NPDT[code]), exp[r]))
    return "; ".join(m for m in msgs if m)


_sets = {}


@pytest.fixture(scope="module")
def node():
    def get(name, n=2, **extra):
        key = (name, n)
        if key not in _sets:
            _sets[key] = C.init_all([0] * n, C.CommConfig(timeout_ms=TIMEOUT_MS, **CONFIGS.get(name, {}), **extra))
        return _sets[key]

    yield get
    for comms in _sets.values():
        vnode.destroy(comms)
    _sets.clear()


SHAPES = [("units-packs-tail", BIG, 0, False), ("below-a-pack", 3, 0, False), ("misaligned", BIG, 1, False),
          ("in-place", BIG, 0, True), ("in-place-misaligned", 1001, 1, True)]


@pytest.mark.parametrize("cfg", list(CONFIGS))
@pytest.mark.parametrize("code,op,arg", PAIRS, ids=PAIR_IDS)
def test_code_sites_and_footprint(node, cfg, code, op, arg):
    comms = node(cfg)
    buff = CONFIGS[cfg].get("buffer_size", 1 << 22)
    if cfg == "one-lane":
        # a slice is one lane's: at least two whole 8 KiB wave units, then packs, then a tail under a pack
        assert BIG * 4 // 4 >= 2 * 8192 + 3 * 16 and BIG % 4 != 0
    if cfg == "one-lane-64k":
        assert BIG * 4 > 2 * (buff // 2)  # several loops of the 32 KiB chunk
    bad = {}
    for func in FUNCS:
        for k, (name, count, off, inplace) in enumerate(SHAPES):
            msg = framed_case(comms, func, code, op, arg, count, off, inplace, buff, seed=100 * k + code)
            if msg:
                bad[(func, name)] = msg
    assert not bad, bad


@pytest.mark.parametrize("code,op,arg", PAIRS, ids=PAIR_IDS)
def test_one_rank(code, op, arg):
    """nranks == 1: recv = post(pre(send)), out of place and in place."""
    comms = C.init_all([0], C.CommConfig(timeout_ms=TIMEOUT_MS))
    try:
        for func in FUNCS:
            for inplace in (False, True):
                x = gen(code, 5003, np.random.default_rng(code))
                want = A.apply_one(code, op, arg, x)
                assert E.mismatches(code, want, x).size >= x.size // 2
                s = Guarded(x.nbytes, 0, "cuda")
                s.write(x)
                d = s if inplace else Guarded(x.nbytes, 0, "cuda")
                if not inplace:
                    d.prefill_not(want)
                issue(comms, func, [s.ptr], [d.ptr], x.size, code, op, arg, 0)
                comms[0].sync()
                assert not diff(code, d.read(vnode.NPDT[code]), want), (func, inplace)
                assert not d.pads_message(), (func, inplace, d.pads_message())
                if not inplace:
                    s.assert_unchanged()
    finally:
        vnode.destroy(comms)


@pytest.mark.parametrize("code,op,arg", PAIRS, ids=PAIR_IDS)
def test_96_thread_workgroups(code, op, arg):
    comms = C.init_all([0] * 2, C.CommConfig(timeout_ms=TIMEOUT_MS, block_threads=96))
    try:
        assert comms[0].block_threads == 96
        for func in FUNCS:
            assert not framed_case(comms, func, code, op, arg, BIG, 0, False, 1 << 22, seed=7), func
    finally:
        vnode.destroy(comms)


@pytest.mark.parametrize("code,op,arg", PAIRS, ids=PAIR_IDS)
def test_non_identity_ring_of_four(code, op, arg):
    rings = [[0, 2, 1, 3], [0, 3, 1, 2]]
    comms = C.init_all([0] * 4, C.CommConfig(timeout_ms=TIMEOUT_MS, rings=rings))
    try:
        assert comms[0].rings() == rings
        for func in FUNCS:
            assert not framed_case(comms, func, code, op, arg, 40001, 0, False, 1 << 22, seed=9), func
    finally:
        vnode.destroy(comms)


# ---- sequences -------------------------------------------------------------------------------
SEQ_N, SEQ_COUNT = 3, 300000  # every call takes every channel, so one Planner carried through stays exact


def _sequence(code, batched):
    """(func, op, op_arg(s), root) steps: Sum AllReduce, Avg AllReduce (or two of
    different op_arg in one group), Broadcast, Avg ReduceScatter, Avg Reduce with
    rotating roots, Sum AllReduce."""
    op, avg = A.avg_op(code, SEQ_N)
    other = A.encode(code, 3) if op == A.PREMULSUM else 7
    steps = [("all_reduce", E.SUM, [0], 0), ("all_reduce", op, [avg, other] if batched else [avg], 0),
             ("broadcast", 0, [0], 1), ("reduce_scatter", op, [avg], 0)]
    steps += [("reduce", op, [avg], root) for root in (2, 0, 1)]
    return steps + [("all_reduce", E.SUM, [0], 0)]


@pytest.mark.parametrize("batched", [False, True], ids=["sequence", "batched-group"])
@pytest.mark.parametrize("code", [F32, I32], ids=["fp32", "int32"])
def test_sequence_on_one_communicator(code, batched):
    """No sync between the calls: the rooted ones leave the connections at
    different FIFO steps and the new kernels start from there like the old."""
    import torch

    n, es = SEQ_N, vnode.ESIZE[code]
    # the Sum AllReduces take the ring too, so every call of the sequence shares the FIFO connections
    comms = C.init_all([0] * n, C.CommConfig(timeout_ms=TIMEOUT_MS, direct_bytes=-1, oneshot_bytes=-1, ll_bytes=-1))
    try:
        planner = vnode.Planner(comms[0].nchannels, comms[0].rings())
        rng = np.random.default_rng(code + batched)
        staged = []
        for func, op, args, root in _sequence(code, batched):
            calls = []
            for arg in args:
                cnt = SEQ_COUNT // n if func == "reduce_scatter" else SEQ_COUNT
                if func == "broadcast":
                    xs = [rng.integers(0, 256, SEQ_COUNT * es, dtype=np.uint8) for _ in range(n)]
                    sel = rooted_ref.select(SEQ_COUNT * es, planner=planner)
                    exp = [rooted_ref.broadcast_expected(xs, root)] * n
                else:
                    xs = [gen(code, SEQ_COUNT, rng) for _ in range(n)]
                    sel = plan_of(planner, func, code, n, cnt)
                    exp = expected(func, xs, code, op, arg, root, sel, 1 << 22)
                assert sel[0] == comms[0].nchannels, (func, sel[0])
                send = [vnode.to_dev(x) for x in xs]
                recv = [vnode.to_dev(np.zeros(e.nbytes, np.uint8)) if e is not None else None for e in exp]
                calls.append((arg, cnt, send, recv, exp))
            staged.append((func, op, root, calls))
        torch.cuda.synchronize()
        for func, op, root, calls in staged:
            with C.group():
                for arg, cnt, send, recv, exp in calls:
                    for r, c in enumerate(comms):
                        if func == "broadcast":
                            C.broadcast(c, send[r] if r == root else None, recv[r], cnt * es, root)
                        elif func == "all_reduce":
                            C.all_reduce(c, send[r], recv[r], cnt, code, op, op_arg=arg)
                        elif func == "reduce_scatter":
                            C.reduce_scatter(c, send[r], recv[r], cnt, code, op, op_arg=arg)
                        else:
                            C.reduce(c, send[r], recv[r], cnt, code, op, root, op_arg=arg)
            assert comms[0].last_algo() == "ring"
        for c in comms:
            c.sync()
        for i, (func, op, root, calls) in enumerate(staged):
            for arg, cnt, send, recv, exp in calls:
                for r in range(n):
                    if exp[r] is None:
                        continue
                    if func == "broadcast":
                        assert recv[r].cpu().numpy().tobytes() == exp[r].tobytes(), (i, func, r)
                    else:
                        d = diff(code, vnode.from_dev(recv[r], code), exp[r])
                        assert not d, (i, func, op, hex(arg), r, d)
    finally:
        vnode.destroy(comms)


@pytest.mark.parametrize("code", [F32, I32], ids=["fp32", "int32"])
def test_graph_replay_keeps_the_scalar(code):
    """One Avg AllReduce captured and replayed three times on changing inputs:
    the scalar lives in the captured work list."""
    import torch

    n, count = 3, 100003
    op, arg = A.avg_op(code, n)
    comms = C.init_all([0] * n, C.CommConfig(timeout_ms=TIMEOUT_MS))
    try:
        rng = np.random.default_rng(5 + code)
        send = [vnode.to_dev(gen(code, count, rng)) for _ in range(n)]
        recv = [vnode.to_dev(np.zeros(count, vnode.NPDT[code])) for _ in range(n)]
        sp, rp = [t.data_ptr() for t in send], [t.data_ptr() for t in recv]
        issue(comms, "all_reduce", sp, rp, count, code, op, arg, 0)  # eager first: loads the code object
        for c in comms:
            c.sync()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            issue(comms, "all_reduce", sp, rp, count, code, op, arg, 0)
        sel = plan_of(vnode.Planner(comms[0].nchannels, comms[0].rings()), "all_reduce", code, n, count)
        for rep in range(3):
            xs = [gen(code, count, rng) for _ in range(n)]
            for r in range(n):
                send[r].copy_(vnode.to_dev(xs[r]))
                recv[r].zero_()
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            for c in comms:
                c.sync()
            exp = expected("all_reduce", xs, code, op, arg, 0, sel, 1 << 22)
            for r in range(n):
                d = diff(code, vnode.from_dev(recv[r], code), exp[r])
                assert not d, (rep, r, d)
        del g
    finally:
        vnode.destroy(comms)


def test_external_launch_of_a_reference_named_kernel():
    """mccs_hip_launch_coll of mccsKernel_AllReduce_RING_SIMPLE_PreMulSum_float
    with redOpArg set in a hand-built work element.  One GPU runs one
    externally launched rank (co-located ranks need the fused launch), so the
    communicator has one rank: recv = send * s."""
    import torch
    from test_gpu_external_launch import _works

    lib = _lib.load()
    assert lib.mccs_hip_set_ref_watchdog(30000) == 0
    comms = C.init_all([0], C.CommConfig(lanes=1, fifo_slots=8, timeout_ms=TIMEOUT_MS))
    try:
        nch, nthr, count = comms[0].nchannels, 544, 70001
        arg = A.avg_scalar_bits(F32, 3)
        x = gen(F32, count, np.random.default_rng(3))
        want = A.pre(F32, x, arg)
        s, d = Guarded(x.nbytes, 0, "cuda"), Guarded(x.nbytes, 0, "cuda")
        s.write(x)
        d.prefill_not(want)
        works = _works(nch, s.ptr, d.ptr, count, nthr)
        for c in range(nch):
            works[c].elems[0].redOpArg = arg
        wb = torch.frombuffer(bytearray(bytes(works)), dtype=torch.uint8).cuda()
        torch.cuda.synchronize()
        assert lib.mccs_hip_coll_kernel(4, F32, A.PREMULSUM)
        rc = lib.mccs_hip_launch_coll(4, F32, A.PREMULSUM, comms[0].dev_comm(), (1 << nch) - 1, wb.data_ptr(), nch, nthr,
                                      torch.cuda.current_stream().cuda_stream)
        assert rc == 0, rc
        torch.cuda.synchronize()
        comms[0].sync()
        assert not diff(F32, d.read(np.float32), want)
        d.assert_pads()
        s.assert_unchanged()
    finally:
        torch.cuda.synchronize()
        for c in comms:
            c.destroy()
