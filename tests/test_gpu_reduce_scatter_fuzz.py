"""GPU: ring ReduceScatter under random configurations and inside random
sequences of collectives.

Part one draws, per seed, a rank count, dtype, op, count per block (tiny,
ragged, or three loops of a 64 KiB FIFO buffer), channels, lanes, block size,
FIFO memory, data placement, buffer size, permuted rings, FIFO slots, slicing
and the work-list route, runs one grouped ReduceScatter on a virtual node and
compares every rank bit for bit with tests/rs_ref.py.  The lane partition
depends on lanes x slots x slicing, and the ReduceScatter walk has one call
per loop (recvReduceCopy) that takes a receive step without posting a send
step; test_gpu_ring_fuzz.py draws these settings for AllReduce / AllGather
only.

Part two issues ReduceScatters between AllReduces (LL, one-shot, two-shot,
ring), AllGathers and grouped calls on one communicator set without a sync in
between, as test_gpu_sequence_fuzz.py does for the other collectives: saved
steps in the flag lines, the work FIFO, the LL launch sequence, the direct
counters and the arena all carry from one launch to the next.  The same
sequences run on three streams, inside a replayed HIP graph and with one rank
per process (tests/ipc_worker.py "rsseq": the multi-rank kernel launched by a
single rank over IPC-mapped arenas).

The case lists are pure functions of the seeds; tests/test_reduce_scatter_cases.py
asserts on the CPU what they cover.
"""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from mccs_amd import comm as C
import rs_ref
import vnode

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
DIRECT_DEFAULTS = True  # part two runs the library's default routing; part one never leaves the ring (ReduceScatter)

TIMEOUT_MS = 8000
DEFAULT_CASES = 32  # the smallest number that meets the coverage list
CASES = int(os.environ.get("MCCS_RS_FUZZ_CASES", DEFAULT_CASES))
SEED_BASE = 9100  # tests/test_reduce_scatter_cases.py: the 32 cases from here meet the coverage list
LOOP_BUFFER = 1 << 16

SEQ_OPS = int(os.environ.get("MCCS_RS_SEQ_OPS", "40"))
SEQ_SEEDS, SEQ_BASE = 8, 17000
STREAM_SEEDS, STREAM_BASE = 4, 19000
GRAPH_SEEDS, GRAPH_BASE, GRAPH_OPS = 3, 21000, 30
IPC_BASE = 23000
MAX_BYTES = 16 << 20
GROUP_BYTES = 4 << 20


# ---- part one: one ReduceScatter per configuration -------------------------------------
def _case(seed):
    """A dict: n, code, op, count (elements per block), cfg (CommConfig
    keywords), slice2, fifo_works, inplace."""
    rng = np.random.default_rng(seed)
    n = int(rng.integers(2, 9))
    code = int(rng.integers(0, 10))
    op = int(rng.choice([0, 0, 0, 1, 2, 3]))
    esize = vnode.ESIZE[code]
    kind = int(rng.integers(0, 6))
    cfg = {}
    if rng.random() < 0.5:
        cfg["channel_count"] = int(rng.integers(1, 7))
    if rng.random() < 0.5:
        cfg["lanes"] = int(rng.choice([1, 2, 3]))
    if rng.random() < 0.3:
        cfg["block_threads"] = int(rng.choice([128, 256, 544, 576]))
    if rng.random() < 0.3:
        cfg["fifo_memory"] = C.FIFO_DEVICE
    if rng.random() < 0.3:
        cfg["locality"] = C.LOCALITY_SENDER
    if rng.random() < 0.3:
        cfg["buffer_size"] = int(rng.choice([1 << 20, 1 << 21]))
    if rng.random() < 0.3:
        nch = cfg.setdefault("channel_count", 2)
        cfg["rings"] = [[int(v) for v in rng.permutation(n)] for _ in range(nch)]
    if rng.random() < 0.5:
        cfg["fifo_slots"] = int(rng.choice([8, 16, 32]))
    slice2 = bool(rng.random() < 0.25)
    fifo_works = bool(rng.random() < 0.3)  # MCCS_INLINE_WORKS=0: the work list goes through the FIFO
    inplace = bool(rng.random() < 0.3)
    if kind == 5:  # three loops, the last one ragged (test_gpu_reduce_scatter.test_more_than_one_loop)
        cfg["buffer_size"] = LOOP_BUFFER
        nch = cfg.get("channel_count") or len(C.default_rings(n))
        count = 2 * nch * (LOOP_BUFFER // 2 // esize) + 77
    else:
        count = [1, 3, 127, 4099, int(rng.integers(1, (1 << 18) + 1))][kind]
    return dict(seed=seed, n=n, code=code, op=op, count=count, cfg=cfg, slice2=slice2, fifo_works=fifo_works,
                inplace=inplace)


def case_rings(case):
    """The rings the communicator of a case gets (host-only)."""
    cfg = case["cfg"]
    return cfg["rings"] if "rings" in cfg else C.default_rings(case["n"], cfg.get("channel_count", 0))


def case_inputs(case):
    n, code, count = case["n"], case["code"], case["count"]
    rng = np.random.default_rng([case["seed"], 1])
    return [vnode.gen(code, n * count, rng) for _ in range(n)]


def case_expected(orc, case, inputs):
    rings = case_rings(case)
    planner = vnode.Planner(len(rings), rings)
    return rs_ref.expected_planned(orc, inputs, case["code"], case["op"], None, planner=planner,
                                   buff_size=case["cfg"].get("buffer_size", 1 << 22))


@pytest.mark.parametrize("k", range(CASES))
def test_random_reduce_scatter_case(orc, k, monkeypatch):
    case = _case(SEED_BASE + k)
    n, code, op, count, cfg = case["n"], case["code"], case["op"], case["count"], case["cfg"]
    if case["slice2"]:
        monkeypatch.setenv("MCCS_SLICE_STEPS", "2")
    if case["fifo_works"]:
        monkeypatch.setenv("MCCS_INLINE_WORKS", "0")
    inputs = case_inputs(case)
    exp = case_expected(orc, case, inputs)
    comms = C.init_all([0] * n, C.CommConfig(timeout_ms=TIMEOUT_MS, **cfg))
    try:
        assert comms[0].rings() == [list(r) for r in case_rings(case)]  # what the CPU-side coverage test assumed
        es = vnode.ESIZE[code]
        send = [vnode.to_dev(x) for x in inputs]
        if case["inplace"]:
            recv = [send[r].data_ptr() + r * count * es for r in range(n)]
        else:
            recv = [vnode.to_dev(np.zeros(count, vnode.NPDT[code])) for _ in range(n)]
        with C.group():
            for r, c in enumerate(comms):
                C.reduce_scatter(c, send[r], recv[r], count, code, op)
        for c in comms:
            c.sync()
        assert all(c.last_algo() == "ring" for c in comms)
        tag = case
        for r in range(n):
            got = (vnode.from_dev(send[r], code)[r * count:(r + 1) * count] if case["inplace"]
                   else vnode.from_dev(recv[r], code))
            assert got.tobytes() == exp[r].tobytes(), (tag, r)
            if case["inplace"]:  # only the rank's own block may change
                whole = vnode.from_dev(send[r], code).copy()
                whole[r * count:(r + 1) * count] = inputs[r][r * count:(r + 1) * count]
                assert whole.tobytes() == inputs[r].tobytes(), (tag, r, "outside the block")
    finally:
        vnode.destroy(comms)


# ---- part two: sequences -----------------------------------------------------------------
def _frac(rng):
    """Where in a log-uniform size range a call lies; sized() turns it into a
    count once the rank count is known."""
    return float(rng.random())


def sized(frac, esize, cap):
    """Elements of `esize` bytes: log-uniform from one element to `cap` bytes."""
    cap = max(esize, cap)
    return max(1, int(esize * (cap / esize) ** frac) // esize)


def rs_sequence(rng, nops):
    """The same list on every rank: dicts with kind ar / ag / group (as
    test_gpu_sequence_fuzz.sequence) and rs / rsgroup, about 35 % of the draws.
    Sizes are fractions of a log-uniform range: resolve() fixes them for a
    rank count (a ReduceScatter block is at most 16 MiB / n)."""
    ops = []
    for _ in range(nops):
        u = rng.random()
        code = int(rng.choice([0, 2, 4, 6, 7, 8, 9]))
        frac = _frac(rng)
        if u < 0.40:
            ops.append(dict(kind="ar", code=code, op=int(rng.choice([0, 0, 0, 1, 2, 3])), frac=frac,
                            inplace=bool(rng.random() < 0.25)))
        elif u < 0.52:
            ops.append(dict(kind="ag", frac=frac))
        elif u < 0.65:
            ops.append(dict(kind="group", code=int(rng.choice([0, 2, 4])), op=int(rng.choice([0, 2, 3])),
                            fracs=[_frac(rng) for _ in range(int(rng.integers(2, 5)))]))
        elif u < 0.90:
            ops.append(dict(kind="rs", code=int(rng.integers(0, 10)), op=int(rng.integers(0, 4)), frac=frac,
                            inplace=bool(rng.random() < 0.25)))
        else:  # one dtype and op per group: plan.cpp refuses a mixed one
            ops.append(dict(kind="rsgroup", code=int(rng.integers(0, 6)), op=int(rng.choice([0, 2, 3])),
                            fracs=[_frac(rng) for _ in range(int(rng.integers(2, 5)))]))
    return ops


def resolve(o, n):
    """The calls of one sequence entry for n ranks: a list of dicts with kind,
    code, op, count (elements; bytes for ag; elements per block for rs) and
    inplace.  More than one call = one group."""
    kind = o["kind"]
    if kind == "ag":
        return [dict(kind="ag", code=None, op=None, count=sized(o["frac"], 1, MAX_BYTES), inplace=False)]
    es = vnode.ESIZE[o["code"]]
    if kind == "ar":
        return [dict(kind="ar", code=o["code"], op=o["op"], count=sized(o["frac"], es, MAX_BYTES), inplace=o["inplace"])]
    if kind == "rs":
        return [dict(kind="rs", code=o["code"], op=o["op"], count=sized(o["frac"], es, MAX_BYTES // n),
                     inplace=o["inplace"])]
    cap = GROUP_BYTES if kind == "group" else GROUP_BYTES // n
    return [dict(kind=kind, code=o["code"], op=o["op"], count=sized(f, es, cap), inplace=False) for f in o["fracs"]]


def predicted_algo(call, n, uncached=True):
    """The kernel the library's defaults give a single call (groups and
    ReduceScatters: the ring; AllGather has a kernel choice of its own and is
    reported as "ag")."""
    if call["kind"] == "ar":
        return vnode.ddp_expected_algo(call["count"] * vnode.ESIZE[call["code"]], n, uncached)
    return "ag" if call["kind"] == "ag" else "ring"


def neighbours(seq, n):
    """(what directly preceded an rs, what directly followed one): sets of
    "ll" / "oneshot" / "direct" / "ring" (single AllReduces) and "ag"."""
    before, after = set(), set()
    tags = []
    for o in seq:
        calls = resolve(o, n)
        tags.append((o["kind"], predicted_algo(calls[0], n) if o["kind"] in ("ar", "ag") else None))
    for (ka, ta), (kb, tb) in zip(tags, tags[1:]):
        if kb == "rs" and ta:
            before.add(ta)
        if ka == "rs" and tb:
            after.add(tb)
    return before, after


def seq_setup(seed):
    """(rng, n, cfg) as test_gpu_sequence_fuzz draws them."""
    rng = np.random.default_rng(seed)
    n = int(rng.integers(2, 9))
    cfg = {}
    if rng.random() < 0.3:
        cfg["channel_count"] = int(rng.integers(1, 7))
    if rng.random() < 0.3:
        cfg["lanes"] = int(rng.choice([1, 2, 4]))
    return rng, n, cfg


def call_input(call, n, rng):
    """One rank's input of a call among n ranks."""
    if call["kind"] == "ag":
        return rng.integers(0, 256, call["count"], dtype=np.uint8)
    mult = n if call["kind"] in ("rs", "rsgroup") else 1
    return vnode.gen(call["code"], mult * call["count"], rng)


def call_inputs(call, n, rng):
    return [call_input(call, n, rng) for _ in range(n)]


def _int_reduce(xs, op):
    acc = xs[0].copy()
    for x in xs[1:]:
        acc = (acc + x).astype(acc.dtype) if op == 0 else np.maximum(acc, x) if op == 2 else np.minimum(acc, x)
    return acc


def call_expected(orc, call, xs, nch_cfg, rings):
    """Per-rank expected outputs of one call (integer groups are order-free,
    so they need no channel plan)."""
    n, kind, code, op, cnt = len(xs), call["kind"], call["code"], call["op"], call["count"]
    if kind == "ag":
        return [orc.ring_allgather(xs)] * n
    if kind == "group":
        return [_int_reduce(xs, op)] * n
    if kind == "rsgroup":
        return [_int_reduce([x[d * cnt:(d + 1) * cnt] for x in xs], op) for d in range(n)]
    planner = vnode.Planner(nch_cfg, rings)
    if kind == "rs":
        return rs_ref.expected_planned(orc, xs, code, op, None, planner=planner)
    nch, nthr, sel = planner.select(cnt * vnode.ESIZE[code], cnt * vnode.ESIZE[code])
    return [orc.ring_allreduce(code, op, xs, nchannels=nch, nthreads=nthr, ring_orders=sel)] * n


class Staged:
    """Device buffers of one call on the virtual node."""

    def __init__(self, call, n):
        self.call, self.n = call, n
        kind, cnt = call["kind"], call["count"]
        es = 1 if kind == "ag" else vnode.ESIZE[call["code"]]
        smult = n if kind in ("rs", "rsgroup") else 1
        rmult = n if kind == "ag" else 1
        self.send = [vnode.to_dev(np.zeros(smult * cnt * es, np.uint8)) for _ in range(n)]
        if not call["inplace"]:
            self.recv = [vnode.to_dev(np.zeros(rmult * cnt * es, np.uint8)) for _ in range(n)]
            self.out = lambda r: self.recv[r].cpu().numpy()
        elif kind == "rs":
            self.recv = [self.send[r].data_ptr() + r * cnt * es for r in range(n)]
            self.out = lambda r: self.send[r].cpu().numpy()[r * cnt * es:(r + 1) * cnt * es]
        else:
            self.recv = self.send
            self.out = lambda r: self.send[r].cpu().numpy()

    def fill(self, xs):
        import torch

        self.xs = xs
        for r in range(self.n):
            self.send[r].copy_(torch.from_numpy(np.ascontiguousarray(xs[r]).view(np.uint8)).cuda())

    def issue(self, comms, stream=None):
        c = self.call
        for r in range(self.n):
            if c["kind"] == "ag":
                C.all_gather(comms[r], self.send[r], self.recv[r], c["count"], stream=stream)
            elif c["kind"] in ("rs", "rsgroup"):
                C.reduce_scatter(comms[r], self.send[r], self.recv[r], c["count"], c["code"], c["op"], stream=stream)
            else:
                C.all_reduce(comms[r], self.send[r], self.recv[r], c["count"], c["code"], c["op"], stream=stream)

    def check(self, orc, comm0, tag):
        exp = call_expected(orc, self.call, self.xs, comm0.nchannels, comm0.rings())
        for r in range(self.n):
            assert self.out(r).tobytes() == exp[r].tobytes(), (tag, self.call, r)


def stage(seq, n, rng=None):
    """[[Staged, ..] per sequence entry]; filled with inputs when rng is given."""
    items = []
    for o in seq:
        group = [Staged(call, n) for call in resolve(o, n)]
        if rng is not None:
            for s in group:
                s.fill(call_inputs(s.call, n, rng))
        items.append(group)
    return items


def issue(group, comms, stream=None):
    with C.group():
        for s in group:
            s.issue(comms, stream)


@pytest.mark.parametrize("seed", range(SEQ_SEEDS))
def test_rs_sequence(orc, seed):
    """40 collectives, no sync in between, one sync, every output exact.  The
    kernel each single AllReduce took must be the one predicted_algo names:
    tests/test_reduce_scatter_cases.py derives from that which algorithms ran
    next to a ReduceScatter over the eight seeds together."""
    import torch

    rng, n, cfg = seq_setup(SEQ_BASE + seed)
    seq = rs_sequence(rng, SEQ_OPS)
    comms = C.init_all([0] * n, C.CommConfig(timeout_ms=TIMEOUT_MS, **cfg))
    try:
        uncached = comms[0].fifo_memory != C.FIFO_DEVICE
        items = stage(seq, n, rng)
        torch.cuda.synchronize()
        took = []
        for o, group in zip(seq, items):
            issue(group, comms)
            algo = comms[0].last_algo()
            took.append((o["kind"], algo, predicted_algo(group[0].call, n, uncached)))
            if o["kind"] in ("rs", "rsgroup"):
                assert all(c.last_algo() == "ring" for c in comms), o
        torch.cuda.synchronize()
        for c in comms:
            c.sync()
        for i, group in enumerate(items):
            for s in group:
                s.check(orc, comms[0], (seed, n, cfg, i))
        line = [f"{k}:{a}" for k, a, _ in took]
        print(f"seed {seed} n {n} {cfg}: {' '.join(line)}")
        print(f"seed {seed}: next to an rs (predicted): before {sorted(neighbours(seq, n)[0])} "
              f"after {sorted(neighbours(seq, n)[1])}")
        wrong = [(i, t) for i, t in enumerate(took) if t[0] == "ar" and t[1] != t[2]]
        assert not wrong, wrong
    finally:
        vnode.destroy(comms)


@pytest.mark.parametrize("seed", range(STREAM_SEEDS))
def test_rs_sequence_mixed_streams(orc, seed):
    """Every entry on one of three streams at random, inputs staged and
    synchronised first: a communicator's launches still run in issue order."""
    import torch

    rng, n, _ = seq_setup(STREAM_BASE + seed)
    seq = rs_sequence(rng, SEQ_OPS)
    comms = C.init_all([0] * n, C.CommConfig(timeout_ms=TIMEOUT_MS))
    streams = [torch.cuda.current_stream(), torch.cuda.Stream(), torch.cuda.Stream()]
    try:
        items = stage(seq, n, rng)
        torch.cuda.synchronize()
        for group in items:
            issue(group, comms, streams[int(rng.integers(0, 3))])
        torch.cuda.synchronize()
        for c in comms:
            c.sync()
        for i, group in enumerate(items):
            for s in group:
                s.check(orc, comms[0], (seed, n, i))
    finally:
        vnode.destroy(comms)


@pytest.mark.parametrize("seed", range(GRAPH_SEEDS))
def test_rs_sequence_graph_replay(orc, seed):
    """30 entries without AllGathers, issued once eagerly (the first launch of
    a kernel loads its code object, which a capture cannot), then captured
    into one HIP graph and replayed three times with fresh inputs: the
    replays pick the FIFO steps up where the previous launch left them."""
    import torch

    rng, n, _ = seq_setup(GRAPH_BASE + seed)
    seq = [o for o in rs_sequence(rng, GRAPH_OPS) if o["kind"] != "ag"]
    comms = C.init_all([0] * n, C.CommConfig(timeout_ms=TIMEOUT_MS))
    try:
        items = stage(seq, n)
        torch.cuda.synchronize()
        for group in items:
            issue(group, comms)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for group in items:
                issue(group, comms)
        for rep in range(3):
            for group in items:
                for s in group:
                    s.fill(call_inputs(s.call, n, rng))
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            for i, group in enumerate(items):
                for s in group:
                    s.check(orc, comms[0], (seed, n, rep, i))
        for c in comms:
            c.sync()
        del g
    finally:
        vnode.destroy(comms)


def _free_port() -> int:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


@pytest.mark.parametrize("world,mode", [(2, "rsseq"), (3, "rsseq"), (4, "rsseq"), (2, "rsseqs"), (4, "rsseqs")])
def test_rs_sequence_across_processes(world, mode):
    """One rank per process: every ReduceScatter is the multi-rank kernel
    launched for a single rank, over IPC-mapped arenas."""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.join(HERE, "ipc_worker.py")]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", IPC_MODES=mode)  # rsseqs: random streams per call
    for k in ("MCCS_ONESHOT_BYTES", "MCCS_DIRECT_BYTES", "MCCS_LL_BYTES"):
        env.pop(k, None)
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env, cwd=os.path.dirname(HERE))
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    lib_lines = "\n".join(l for l in (r.stdout + r.stderr).splitlines() if "mccs" in l.lower() or "hip" in l)[-3000:]
    assert r.returncode == 0 and lines, lib_lines + "\n----\n" + r.stdout[-2000:] + r.stderr[-2000:]
    res = json.loads(lines[-1])
    bad = [k for k, v in res["fifo_modes"].items() if not v]
    assert res["all_ok"] and not bad, bad
    nrs = [k for k in res["fifo_modes"] if "/rs/" in k]
    assert nrs and "rsseq/rs_algos:ring" in res["fifo_modes"], sorted(res["fifo_modes"])
    print(f"{world} processes: {len(nrs)} ReduceScatters,",
          [k for k in res["fifo_modes"] if k.startswith(("rsseq/algos", "rsseq/rs_algos"))])
