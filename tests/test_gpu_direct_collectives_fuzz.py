"""GPU: the direct and LL ReduceScatter, Reduce and Broadcast under seeded
configurations and inside seeded sequences of collectives.

The three other fuzz files (tests/test_gpu_sequence_fuzz.py,
tests/test_gpu_reduce_scatter_fuzz.py, tests/test_gpu_rooted_a2a_fuzz.py) never
opt in, and the direct kernels' own tests run the default geometry plus a few
fixed variations.  The cases are tests/direct_fuzz_cases.py's, pure functions
of their seeds; tests/test_direct_fuzz_cases.py asserts on the CPU what they
cover, that each plans as its `algo` says and that each can fail.

Part one draws, per seed, the function, the body, 2..8 ranks, dtype, op,
root, a count at an edge of the cut (1, an 8-byte word +- 1 element, a ring
granule +- 1, the cap of the variant, ..), 1..6 channels, permuted rings, the
FIFO buffer size (64 KiB: several loops of the walk inside the cap), the slot
sizes, MCCS_DIRECT_BLOCKS (G = 2, 3, 5: the count-based bodies' round-robin deal
of pieces wraps; the default list holds one such launch per G and per loop that
deals, and a count-based fold that leaves the walk by its early return), a
cached arena (the LL cap reads 0 and the count-based body fences), in place,
and both buffers' misalignment.  The call runs twice back to back with fresh
payloads, so both slot parities are used, then one direct call of another
function runs on the same communicators (E_IN and the launch count), all
without a sync.  Every buffer is a footprint.Guarded one (16 KiB pseudo-random
pads, destinations prefilled with the NOT of their expectation): every rank is
compared byte for byte, every pad and every buffer that is no destination must
be unchanged.  On odd seeds a Reduce's non-roots pass no recvbuff and a
Broadcast's non-roots no sendbuff.  Expected values: rs_ref / rooted_ref with a
vnode.Planner built from the case's rings and buffer size.

Part two issues about 40 calls per sequence without a sync in between --
direct and LL ReduceScatters, Reduces and Broadcasts with freshly drawn roots,
LL / one-shot / two-shot / ring AllReduces, both AllGathers, LL AllToAlls and
oversized (ring) ReduceScatters, Reduces and Broadcasts in random order, closed
by a ring AllToAll -- on communicators opted in as
tests/test_gpu_rooted_direct_sequences.py's, on one stream at n = 2, 3, 4, 8,
across two streams, and in a HIP graph replayed three times with rewritten
inputs.  What keeps the slots' parity reuse and the single E_IN word valid is
that every ordered pair hands off in every launch; these sequences are the
seeded test of that.  Expected values: tests/test_gpu_rooted_sequences.py's
call_expected.  Every call asserts last_algo() on every rank; every
communicator has an 8 s watchdog.
"""
import numpy as np
import pytest

import direct_fuzz_cases as K
import test_gpu_all_to_all_sequences as A
import test_gpu_rooted_direct_sequences as RDS
import test_gpu_rooted_sequences as S
import vnode
from footprint import Guarded
from mccs_amd import comm as C

pytestmark = pytest.mark.gpu
DIRECT_DEFAULTS = True  # every threshold is set per communicator

TIMEOUT_MS = 8000
DEV = "cuda"


# ---- part one: one call per configuration -------------------------------------------
class Staged:
    """The guarded buffers of one call of a case, filled; `expect` records what
    each must hold after the call (everything else: what it holds now)."""

    def __init__(self, orc, case, call):
        self.case, self.call = case, call
        n, kind, cnt, root = case["n"], call["kind"], call["count"], call["root"]
        es = 1 if kind == "bc" else vnode.ESIZE[call["code"]]
        xs, exp, self.salt = K.call_payload(orc, case, call)
        self.sends = [Guarded(cnt * es * (n if kind == "rs" else 1), call["soff"], DEV) for _ in range(n)]
        self.recvs = [Guarded(cnt * es, call["roff"], DEV) for _ in range(n)]
        for r in range(n):
            if xs[r] is not None:
                self.sends[r].write(xs[r])
        self.send, self.recv = K.pointers(case, call, [g.ptr for g in self.sends], [g.ptr for g in self.recvs])
        self.after = []  # (buffer, position, bytes) the call must leave
        for r in range(n):
            if exp[r] is None:
                continue
            if self.recv[r] == self.recvs[r].ptr:  # out of place
                self.recvs[r].prefill_not(exp[r])
                self.after.append((self.recvs[r], 0, exp[r]))
            else:  # in place: inside this rank's send buffer
                at = self.recv[r] - self.sends[r].ptr
                assert at == (r * cnt * es if kind == "rs" else 0) and (kind == "rs" or r == root)
                self.after.append((self.sends[r], at, exp[r]))

    def check(self):
        """{(buffer, rank): what went wrong}: results bit for bit, every pad
        intact, everything that is no destination unchanged."""
        for g, at, data in self.after:
            b = np.ascontiguousarray(data).view(np.uint8).reshape(-1)
            g.want[g.lo + at:g.lo + at + b.size] = b
        bad = {}
        for name, bufs in (("send", self.sends), ("recv", self.recvs)):
            for r, g in enumerate(bufs):
                msg = g.source_message()
                if msg:
                    bad[(self.call["index"], self.call["kind"], name, r)] = msg
        return bad


@pytest.mark.parametrize("k", range(K.CASES))
def test_random_direct_case(orc, monkeypatch, k):
    import torch

    case = K.case(K.SEED_BASE + k)
    n = case["n"]
    if case["blocks"] is None:
        monkeypatch.delenv("MCCS_DIRECT_BLOCKS", raising=False)
    else:
        monkeypatch.setenv("MCCS_DIRECT_BLOCKS", str(case["blocks"]))
    comms = C.init_all([0] * n, C.CommConfig(timeout_ms=TIMEOUT_MS, **case["cfg"]))
    try:
        assert comms[0].rings() == case["rings"]  # what the CPU-side coverage test assumed
        assert (comms[0].fifo_memory == C.FIFO_DEVICE) == case["fifo_device"]
        K.opt_in(comms, case)  # asserts the caps: on a cached arena the LL cap reads 0
        items = [Staged(orc, case, call) for call in K.calls(case)]
        torch.cuda.synchronize()
        for s in items:  # no sync in between
            K.issue(comms, s.call, s.send, s.recv)
            algos = [c.last_algo() for c in comms]
            assert algos == [s.call["algo"]] * n, (case, s.call, algos)
        torch.cuda.synchronize()
        for c in comms:
            c.sync()
        bad = {}
        for s in items:
            bad.update(s.check())
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        g, piece, piece2, units = K.geometry(case, items[0].call, device_workgroups=cus)
        print(f"seed {case['seed']} {case['func']}-{case['variant']} n={n} dtype={case['code']} op={case['op']} "
              f"count={case['count']} ({case['count_kind']}) blocks={case['blocks']}: G={g} units={units} "
              f"loops={K.loops(case, items[0].call)} salts={[s.salt for s in items]}")
        assert not bad, (case, bad)
    finally:
        vnode.destroy(comms)


# ---- part two: sequences ---------------------------------------------------------------
def _stage(seed, n, rng):
    return [A.A2AStaged(call, n) if call["kind"] == "a2a"
            else S.Staged(call, n, [S.call_input(call, n, rng) for _ in range(n)]) for call in K.sequence(seed, n)]


def _issue_all(items, comms, pick_stream=lambda: None):
    n = len(comms)
    for s in items:
        s.issue(comms, pick_stream())
        algos = [c.last_algo() for c in comms]
        assert algos == [s.call["algo"]] * n, (s.call, algos)


def _comms(n):
    assert RDS.CFG == dict(buffer_size=K.SEQ_BUFF, oneshot_bytes=K.ONESHOT, ll_bytes=K.LL_BYTES,
                           direct_bytes=K.TWOSHOT) and RDS.ROOTED_LL == K.SMALL_LL and S.TIMEOUT_MS == TIMEOUT_MS
    comms = RDS._comms(n)  # opted in to every direct ReduceScatter, Reduce, Broadcast and the LL AllToAll
    assert comms[0].all_to_all_ll_max() >= K.A2A_LL
    return comms


@pytest.mark.parametrize("seed,n", K.ONE_STREAM, ids=[f"seed{s}-n{n}" for s, n in K.ONE_STREAM])
def test_sequence(orc, seed, n):
    import torch

    comms = _comms(n)
    try:
        items = _stage(seed, n, np.random.default_rng([seed, n]))
        torch.cuda.synchronize()
        _issue_all(items, comms)
        S._finish(orc, comms, items, ("direct fuzz sequence", seed, n))
        print(f"seed {seed} n {n}:", " ".join(s.call["name"] for s in items))
    finally:
        vnode.destroy(comms)


@pytest.mark.parametrize("seed,n", K.TWO_STREAMS, ids=[f"seed{s}-n{n}" for s, n in K.TWO_STREAMS])
def test_sequence_across_two_streams(orc, seed, n):
    """Every call on one of two streams, inputs staged and synchronised first:
    a communicator's launches still run in issue order."""
    import torch

    comms = _comms(n)
    streams = [torch.cuda.current_stream(), torch.cuda.Stream()]
    try:
        rng = np.random.default_rng([seed, n])
        items = _stage(seed, n, rng)
        torch.cuda.synchronize()
        _issue_all(items, comms, lambda: streams[int(rng.integers(0, 2))])
        S._finish(orc, comms, items, ("direct fuzz streams", seed, n))
    finally:
        vnode.destroy(comms)


@pytest.mark.parametrize("seed,n", K.GRAPH, ids=[f"seed{s}-n{n}" for s, n in K.GRAPH])
def test_sequence_graph_replayed_three_times(orc, seed, n):
    """Issued once eagerly (the first launch of a kernel loads its code
    object, which a capture cannot), then captured into one HIP graph and
    replayed three times with rewritten inputs: E_IN, the launch count and the
    parity in the control block keep counting across the replays."""
    import torch

    comms = _comms(n)
    try:
        rng = np.random.default_rng([seed, n])
        items = _stage(seed, n, rng)
        torch.cuda.synchronize()
        _issue_all(items, comms)
        S._finish(orc, comms, items, ("direct fuzz eager", seed, n))
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            _issue_all(items, comms)
        for rep in range(3):
            RDS._refill(items, n, rng, rep)
            torch.cuda.synchronize()
            g.replay()
            S._finish(orc, comms, items, ("direct fuzz graph", seed, n, rep))
        del g
    finally:
        vnode.destroy(comms)
