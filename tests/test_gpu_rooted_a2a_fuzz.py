"""GPU: ring Broadcast, Reduce and AllToAll under random engine configurations,
and the rooted / AllToAll sequences under a fixed list of them.

Part one draws, per seed, a rank count, a size (tiny, ragged, up to 256 KiB,
1 .. 2 MiB, or three loops of a 64 KiB FIFO buffer), channels, lanes, block
size, FIFO memory, data placement, buffer size, permuted rings, FIFO slots,
two-step slicing and the work-list route, runs one grouped call on a virtual
node and compares every byte with tests/rooted_ref.py, tests/avg_ref.py and
tests/a2a_ref.py.  tests/test_gpu_ring_fuzz.py and
tests/test_gpu_reduce_scatter_fuzz.py draw these settings for AllReduce,
AllGather and ReduceScatter only: the rooted kernels (root and role in every
work element, a chain that leaves one connection standing) and the AllToAll
kernel (the route in every work element, recvSend from FIFO slot to FIFO slot)
otherwise meet the default configuration alone.

Part two runs the sequences of tests/test_gpu_rooted_sequences.py and
tests/test_gpu_all_to_all_sequences.py, where the connections' FIFO steps drift
furthest apart, under six overrides of their configuration: the slot index is
step & (fifo_slots - 1) and the send window depends on slots and slicing, so
drifted steps must stay consistent with 8 and 32 slots, with two-step slices,
with the cached arena's acquire / release hand-off, with sender-side placement
and a work list read through the work FIFO, and on permuted rings.

The case lists are pure functions of the seeds; tests/test_rooted_a2a_fuzz_cases.py
asserts on the CPU what they cover.
"""
import os

import numpy as np
import pytest

import a2a_ref
import avg_ref
from mccs_amd import comm as C
import rooted_ref
import test_gpu_all_to_all_sequences as A
import test_gpu_rooted_sequences as S
import vnode

pytestmark = pytest.mark.gpu
DIRECT_DEFAULTS = True  # part two sets every threshold through S.CFG; part one passes RING_ONLY itself

TIMEOUT_MS = 8000
RING_ONLY = dict(oneshot_bytes=-1, direct_bytes=-1, ll_bytes=-1)
LOOP_BUFFER = 1 << 16
SENTINEL = a2a_ref.SENTINEL
FP = (6, 7, 8, 9)
BF16 = 9
ENV = ("MCCS_SLICE_STEPS", "MCCS_INLINE_WORKS", "MCCS_ALLTOALL_HOPS")

# tests/test_rooted_a2a_fuzz_cases.py: per list, the smallest number of cases from its seed base that meets
# the coverage list and the sensitivity properties (found on the CPU by counting up from one)
SEED_BASE = {"bc": 42700, "rd": 43100, "a2a": 46300}
DEFAULT_CASES = {"bc": 22, "rd": 31, "a2a": 24}
CASES = {k: int(os.environ.get("MCCS_ROOTED_A2A_FUZZ_CASES", v)) for k, v in DEFAULT_CASES.items()}
KINDS = ("one", "three", "ragged", "random", "big", "loops")


# ---- part one: the case lists ------------------------------------------------------------------
def _common(rng, n):
    """The draws every list shares: (cfg, slice2, fifo_works, kind).  The value
    sets are those of test_gpu_reduce_scatter_fuzz._case."""
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
    slice2 = bool(rng.random() < 0.3)  # MCCS_SLICE_STEPS=2
    fifo_works = bool(rng.random() < 0.3)  # MCCS_INLINE_WORKS=0: the work list goes through the FIFO
    kind = KINDS[int(rng.integers(0, 6))]
    if kind == "loops":
        cfg["buffer_size"] = LOOP_BUFFER
    return cfg, slice2, fifo_works, kind


def _nbytes(rng, kind):
    """The byte size of every kind but "loops" (drawn whether used or not)."""
    ragged = int(rng.choice([127, 4099]))
    random = int(rng.integers(1, (256 << 10) + 1))
    big = int(rng.integers(1 << 20, (2 << 20) + 1))  # every channel and lane carries whole wave units
    return {"one": 1, "three": 3, "ragged": ragged, "random": random, "big": big}.get(kind)


def case_rings(case):
    """The rings the communicator of a case gets (host-only)."""
    cfg = case["cfg"]
    return cfg["rings"] if "rings" in cfg else C.default_rings(case["n"], cfg.get("channel_count", 0))


def bc_case(seed):
    """A dict: n, root, size (bytes), cfg (CommConfig keywords), slice2,
    fifo_works, kind, inplace, recv_off (per rank, bytes past a 16-byte
    boundary)."""
    rng = np.random.default_rng(seed)
    n = int(rng.integers(2, 9))
    cfg, slice2, fifo_works, kind = _common(rng, n)
    size = _nbytes(rng, kind)
    root = int(rng.integers(0, n))
    inplace = bool(rng.random() < 0.3)
    recv_off = [int(v) for v in rng.integers(0, 16, n)]
    case = dict(seed=seed, n=n, root=root, cfg=cfg, slice2=slice2, fifo_works=fifo_works, kind=kind, inplace=inplace,
                recv_off=recv_off)
    if kind == "loops":  # two full loops of every channel (test_gpu_rooted.test_more_than_one_loop) and a ragged tail
        size = 2 * len(case_rings(case)) * (LOOP_BUFFER // 2) + 4 * 999 + 1
    return dict(case, size=size)


def rd_case(seed):
    """A dict: n, root, code, op, op_arg (None for the four plain ops), count
    (elements), cfg, slice2, fifo_works, kind, inplace."""
    rng = np.random.default_rng(seed)
    n = int(rng.integers(2, 9))
    cfg, slice2, fifo_works, kind = _common(rng, n)
    nbytes = _nbytes(rng, kind)
    code = int(rng.integers(0, 10))
    op = int(rng.choice([0, 0, 1, 2, 3, avg_ref.PREMULSUM, avg_ref.PREMULSUM, avg_ref.SUMPOSTDIV]))
    if op == avg_ref.SUMPOSTDIV and code in FP:  # defined for the integer types only
        op = avg_ref.PREMULSUM
    which = int(rng.integers(0, 2))
    op_arg = avg_ref.case_args(code, op, n)[which] if op >= avg_ref.PREMULSUM else None
    root = int(rng.integers(0, n))
    inplace = bool(rng.random() < 0.3)
    case = dict(seed=seed, n=n, root=root, code=code, op=op, op_arg=op_arg, cfg=cfg, slice2=slice2,
                fifo_works=fifo_works, kind=kind, inplace=inplace)
    es = vnode.ESIZE[code]
    if kind == "loops":
        count = 2 * len(case_rings(case)) * (LOOP_BUFFER // 2 // es) + 77
    elif kind in ("random", "big"):  # byte sizes: as many whole elements
        count = max(1, nbytes // es)
    else:
        count = nbytes
    return dict(case, count=count)


def a2a_case(seed):
    """A dict: n, size (bytes per peer), relay (MCCS_ALLTOALL_HOPS=relay), cfg,
    slice2, fifo_works, kind, send_off / recv_off (per rank)."""
    rng = np.random.default_rng(seed)
    n = int(rng.integers(2, 9))
    cfg, slice2, fifo_works, kind = _common(rng, n)
    size = _nbytes(rng, kind)
    relay = bool(rng.random() < 0.3)
    send_off = [int(v) for v in rng.integers(0, 16, n)]
    recv_off = [int(v) for v in rng.integers(0, 16, n)]
    case = dict(seed=seed, n=n, relay=relay, cfg=cfg, slice2=slice2, fifo_works=fifo_works, kind=kind,
                send_off=send_off, recv_off=recv_off)
    if kind == "loops":  # test_gpu_all_to_all.test_three_loops: two full loops of a block's channels, a short third
        rings = case_rings(case)
        m = a2a_ref.route(n, rings, force_relay=relay)["m"] or len(rings)
        size = 2 * m * (LOOP_BUFFER // 2) + 999
    return dict(case, size=size)


MAKE = {"bc": bc_case, "rd": rd_case, "a2a": a2a_case}


def cases(which, count=None):
    return [MAKE[which](SEED_BASE[which] + k) for k in range(DEFAULT_CASES[which] if count is None else count)]


def buffer_size(case):
    return case["cfg"].get("buffer_size", 1 << 22)


def rooted_plan(case):
    """(channels, threads, rings) the planner gives a bc / rd case's call."""
    rings = case_rings(case)
    nbytes = case["size"] if "size" in case else case["count"] * vnode.ESIZE[case["code"]]
    return vnode.Planner(len(rings), rings).select(nbytes, nbytes)


def bc_data(root, size):
    """`size` bytes of 32-bit words naming root and index (the last word cut)."""
    i = np.arange(-(-size // 4), dtype=np.int64)
    return ((root + 1) * 16777259 + i).astype(np.int32).view(np.uint8)[:size].copy()


def rd_inputs(case):
    rng = np.random.default_rng([case["seed"], 1])
    return [vnode.gen(case["code"], case["count"], rng) for _ in range(case["n"])]


def rd_expected(orc, case, inputs):
    """The root's result.  The four plain ops: rooted_ref under the oracle's
    functor.  PreMulSum / SumPostDiv: avg_ref.reduce_expected, which folds
    under tests/elem_ref.py; its bf16 Sum works in exact rationals element by
    element, so a bf16 case above 4099 elements folds the pre-scaled inputs
    (avg_ref.pre, the same first step) under the oracle's Sum instead.
    tests/test_rooted_a2a_fuzz_cases.py holds that route to
    avg_ref.reduce_expected on the cases small enough for both."""
    nch, nthr, rings = rooted_plan(case)
    code, op, root, buff = case["code"], case["op"], case["root"], buffer_size(case)
    if op < avg_ref.PREMULSUM:
        return rooted_ref.reduce_expected(orc, inputs, code, op, root, nch, nthr, rings, buff)
    if code == BF16 and case["count"] > 4099:
        return rd_expected_scaled(orc, case, inputs)
    return avg_ref.reduce_expected(inputs, code, op, case["op_arg"], root, nch, nthr, rings, buff)


def rd_expected_scaled(orc, case, inputs):
    """PreMulSum as the Sum Reduce over elementwise pre-scaled inputs, the sum
    under the oracle's functor."""
    assert case["op"] == avg_ref.PREMULSUM
    nch, nthr, rings = rooted_plan(case)
    scaled = [avg_ref.pre(case["code"], x, case["op_arg"]) for x in inputs]
    return rooted_ref.reduce_expected(orc, scaled, case["code"], 0, case["root"], nch, nthr, rings, buffer_size(case))


def a2a_route(case):
    return a2a_ref.route(case["n"], case_rings(case), force_relay=case["relay"])


def _env(monkeypatch, case):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    if case["slice2"]:
        monkeypatch.setenv("MCCS_SLICE_STEPS", "2")
    if case["fifo_works"]:
        monkeypatch.setenv("MCCS_INLINE_WORKS", "0")
    if case.get("relay"):
        monkeypatch.setenv("MCCS_ALLTOALL_HOPS", "relay")


def _comms(case):
    return C.init_all([0] * case["n"], C.CommConfig(timeout_ms=TIMEOUT_MS, **{**RING_ONLY, **case["cfg"]}))


def _same_rings(comms, case):
    assert comms[0].rings() == [list(r) for r in case_rings(case)]  # what the CPU-side coverage test assumed
    _as_configured(comms, case["cfg"])


def _as_configured(comms, cfg):
    """The drawn lanes, block size and FIFO memory are what the communicators run."""
    for c in comms:
        assert c.lanes == cfg.get("lanes", c.lanes) and c.block_threads == cfg.get("block_threads", c.block_threads)
        assert (c.fifo_memory == C.FIFO_DEVICE) == (cfg.get("fifo_memory") == C.FIFO_DEVICE)


def _framed(nbytes, off):
    """(device tensor of a 0xA5 frame, slice of the payload, host copy)."""
    import torch

    host, sl = a2a_ref.sentinel_frame(nbytes, 16 + off)
    return torch.from_numpy(host).cuda(), sl, host


def _sync(comms):
    import torch

    torch.cuda.synchronize()
    for c in comms:
        c.sync()
    assert all(c.last_algo() == "ring" for c in comms)


def _diff(got, want, tag):
    if got.tobytes() != want.tobytes():
        bad = np.flatnonzero(np.ascontiguousarray(got).view(np.uint8) != np.ascontiguousarray(want).view(np.uint8))
        raise AssertionError(f"{tag}: {bad.size} bytes differ, first at byte {bad[0]}")


@pytest.mark.parametrize("k", range(CASES["bc"]))
def test_random_broadcast_case(k, monkeypatch):
    import torch

    case = bc_case(SEED_BASE["bc"] + k)
    n, root, size = case["n"], case["root"], case["size"]
    _env(monkeypatch, case)
    data = bc_data(root, size)
    want = rooted_ref.broadcast_expected([bc_data(r, size) for r in range(n)], root)
    comms = _comms(case)
    try:
        _same_rings(comms, case)
        frames = [_framed(size, case["recv_off"][r]) for r in range(n)]
        recv = [t.data_ptr() + sl.start for t, sl, _ in frames]
        src = vnode.to_dev(data)
        send = [None] * n
        send[root] = src.data_ptr()
        if case["inplace"]:
            t, sl, _ = frames[root]
            t[sl].copy_(src)
            send[root] = recv[root]
        torch.cuda.synchronize()
        with C.group():
            for r, c in enumerate(comms):
                C.broadcast(c, send[r], recv[r], size, root)
        _sync(comms)
        for r, (t, sl, host) in enumerate(frames):
            host[sl] = want
            _diff(t.cpu().numpy(), host, (case, r))  # the payload and both bands
        assert src.cpu().numpy().tobytes() == data.tobytes(), (case, "the root's sendbuff was written")
    finally:
        vnode.destroy(comms)


@pytest.mark.parametrize("k", range(CASES["rd"]))
def test_random_reduce_case(orc, k, monkeypatch):
    import torch

    case = rd_case(SEED_BASE["rd"] + k)
    n, root, code, count = case["n"], case["root"], case["code"], case["count"]
    _env(monkeypatch, case)
    inputs = rd_inputs(case)
    want = rd_expected(orc, case, inputs)
    comms = _comms(case)
    try:
        _same_rings(comms, case)
        nbytes = count * vnode.ESIZE[code]
        keep = [vnode.to_dev(x) for x in inputs]
        out = [torch.full((nbytes,), SENTINEL, dtype=torch.uint8, device="cuda") for _ in range(n)]
        recv = [t.data_ptr() for t in out]
        if case["inplace"]:
            recv[root] = keep[root].data_ptr()
        torch.cuda.synchronize()
        with C.group():
            for r, c in enumerate(comms):
                C.reduce(c, keep[r], recv[r], count, code, case["op"], root, op_arg=case["op_arg"])
        _sync(comms)
        _diff((keep if case["inplace"] else out)[root].cpu().numpy(), want, (case, "the root's result"))
        for r in range(n):
            if r != root or case["inplace"]:
                assert bool((out[r] == SENTINEL).all()), (case, r, "an unused recvbuff was written")
            if r != root or not case["inplace"]:
                _diff(keep[r].cpu().numpy(), inputs[r], (case, r, "sendbuff written"))
    finally:
        vnode.destroy(comms)


@pytest.mark.parametrize("k", range(CASES["a2a"]))
def test_random_all_to_all_case(k, monkeypatch):
    import torch

    case = a2a_case(SEED_BASE["a2a"] + k)
    n, B = case["n"], case["size"]
    _env(monkeypatch, case)
    inputs = a2a_ref.make_inputs(n, B, salt=case["seed"] % 7)
    want = a2a_ref.expected(inputs, B)
    route = a2a_route(case)
    comms = _comms(case)
    try:
        _same_rings(comms, case)
        assert all(c.all_to_all_route() == {"hops": route["hops"], "m": route["m"]} for c in comms), (case, route)
        sends = [_framed(n * B, case["send_off"][r]) for r in range(n)]
        recvs = [_framed(n * B, case["recv_off"][r]) for r in range(n)]
        for r, (t, sl, host) in enumerate(sends):
            host[sl] = inputs[r]
            t.copy_(torch.from_numpy(host))
        torch.cuda.synchronize()
        with C.group():
            for r in range(n):
                C.all_to_all(comms[r], sends[r][0].data_ptr() + sends[r][1].start,
                             recvs[r][0].data_ptr() + recvs[r][1].start, B)
        _sync(comms)
        for r in range(n):
            t, sl, host = recvs[r]
            host[sl] = want[r]
            _diff(t.cpu().numpy(), host, (case, r))  # the blocks and both bands
            _diff(sends[r][0].cpu().numpy(), sends[r][2], (case, r, "send buffer written"))
    finally:
        vnode.destroy(comms)


# The Reduce case of seed 43125 (float64 PreMulSum by 1/7 = 0x3fc2492492492492) gave NaN everywhere: the ring
# kernels put the scalar together from two 32-bit halves and the low one sign-extended over the high one.
# tests/avg_ref.py's case_args at n = 2 .. 4 (1/2, 1/3, 1/4, 3, -1) never set bit 31 below a high half
# that is not all ones; these do, for the three 64-bit types and every function that takes the scalar.
WIDE_SCALARS = [(8, 0x3fc2492492492492), (8, 0x3fc999999999999a), (4, 0x0000000180000001), (5, 0x92492492)]


@pytest.mark.parametrize("code,arg", WIDE_SCALARS, ids=[f"dt{c}-{a:#x}" for c, a in WIDE_SCALARS])
def test_premulsum_scalar_with_bit_31_set(code, arg):
    """AllReduce, ReduceScatter and Reduce (root 1) of 4099 elements per rank
    or block on three ranks (whole wave units, packs and a tail), and of 3."""
    import test_gpu_avg_paths as P

    n, root, op = 3, 1, avg_ref.PREMULSUM
    comms = C.init_all([0] * n, C.CommConfig(timeout_ms=TIMEOUT_MS, **RING_ONLY))
    try:
        rng = np.random.default_rng(code)
        for func in P.FUNCS:
            for count in (4099, 3):
                per_rank = count * (n if func == "reduce_scatter" else 1)
                inputs = [vnode.gen(code, per_rank, rng) for _ in range(n)]
                sel = P.plan_of(vnode.Planner(comms[0].nchannels, comms[0].rings()), func, code, n, count)
                exp = P.expected(func, inputs, code, op, arg, root, sel, 1 << 22)
                send = [vnode.to_dev(x) for x in inputs]
                recv = [vnode.to_dev(np.zeros(count, vnode.NPDT[code])) for _ in range(n)]
                P.issue(comms, func, [t.data_ptr() for t in send], [t.data_ptr() for t in recv], count, code, op, arg,
                        root)
                _sync(comms)
                for r in range(n):
                    if exp[r] is not None:
                        _diff(vnode.from_dev(recv[r], code), exp[r], (func, count, r))
    finally:
        vnode.destroy(comms)


# ---- part two: the sequences under engine overrides ----------------------------------------------
SEQ_NS = (4, 8)
# name -> (CommConfig keywords layered on S.CFG, environment)
OVERRIDES = {
    "slots8-lanes3": (dict(fifo_slots=8, lanes=3), {}),
    "slots32-lanes1": (dict(fifo_slots=32, lanes=1), {}),
    "slots8-slice2": (dict(fifo_slots=8), {"MCCS_SLICE_STEPS": "2"}),
    "device-slots8": (dict(fifo_memory=C.FIFO_DEVICE, fifo_slots=8), {}),
    "sender-fifo-works": (dict(locality=C.LOCALITY_SENDER), {"MCCS_INLINE_WORKS": "0"}),
    "permuted-rings": (dict(rings="permuted"), {}),
}


def permuted_rings(n):
    """Two channels, each an independent permutation of the ranks."""
    rng = np.random.default_rng([S.SEED, n, 2])
    return [[int(v) for v in rng.permutation(n)] for _ in range(2)]


def override(name, n):
    """(CommConfig keywords: S.CFG with the override on top, environment, the rings that gives)."""
    kw, env = OVERRIDES[name]
    cfg = {**S.CFG, **kw}
    if cfg.get("rings") == "permuted":
        cfg["rings"] = permuted_rings(n)
    return cfg, env, cfg.get("rings") or C.default_rings(n)


def seq_algo(call, cfg):
    """The kernel a call of the sequences takes under `cfg`: a cached arena
    never takes the LL one-shot (test_gpu_direct.test_direct_hand_off_modes),
    so the direct-sized AllReduces take the one-shot kernel there."""
    if call["kind"] == "a2a":
        return "ring"
    if call["kind"] == "ard" and cfg.get("fifo_memory") == C.FIFO_DEVICE:
        return "oneshot"
    return S.expected_algo(call)


def _run_sequence(orc, monkeypatch, n, name, stage, tag):
    import torch

    cfg, env, rings = override(name, n)
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    comms = C.init_all([0] * n, C.CommConfig(timeout_ms=TIMEOUT_MS, **cfg))
    try:
        assert comms[0].rings() == [list(r) for r in rings]  # S.Staged.check takes its expected values from these
        _as_configured(comms, cfg)
        route = a2a_ref.route(n, rings)
        assert comms[0].all_to_all_route() == {"hops": route["hops"], "m": route["m"]}
        items = stage(n, np.random.default_rng([n, list(OVERRIDES).index(name)]))
        torch.cuda.synchronize()
        took = []
        for s in items:
            s.issue(comms)
            took.append((s.call["kind"], comms[0].last_algo(), seq_algo(s.call, cfg)))
        S._finish(orc, comms, items, (tag, n, name))
        print(f"{name} n {n}:", " ".join(f"{k}:{a}" for k, a, _ in took))
        assert not [t for t in took if t[1] != t[2]], took
        return took
    finally:
        vnode.destroy(comms)


@pytest.mark.parametrize("name", list(OVERRIDES))
@pytest.mark.parametrize("n", SEQ_NS)
def test_rooted_sequence_under(orc, monkeypatch, n, name):
    """S.sequence, no sync between the calls, one final check, every result exact."""
    took = _run_sequence(orc, monkeypatch, n, name, S._stage, "rooted")
    assert {k for k, _, _ in took} == {"bc", "rd", "ar", "ard", "ag", "rs"}


@pytest.mark.parametrize("name", list(OVERRIDES))
@pytest.mark.parametrize("n", SEQ_NS)
def test_all_to_all_sequence_under(orc, monkeypatch, n, name):
    """A.sequence: the same calls with seven AllToAlls woven in (relayed on the permuted rings)."""
    took = _run_sequence(orc, monkeypatch, n, name, A._stage, "a2a")
    assert sum(1 for t in took if t[0] == "a2a") == 7
