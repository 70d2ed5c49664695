"""CPU: what the ReduceScatter GPU suites' generated cases cover, and the host
ring on edge values.

tests/test_gpu_reduce_scatter_fuzz.py's case lists are pure functions of their
seeds: the coverage and sensitivity they are meant to have is asserted here,
without a GPU.  tests/test_gpu_reduce_scatter_values.py's inputs are checked
for vacuity, and mccs_host_ring_reduce_scatter, which shares the walk with the
gfx950 kernels, runs them against tests/rs_ref.py evaluated with the
independent element reference (tests/elem_ref.py).
"""
import hashlib
import json

import numpy as np
import pytest

import elem_ref as E
import rs_ref
import test_gpu_reduce_scatter_fuzz as F
import test_gpu_sequence_fuzz as S
import vnode
from mccs_amd import comm as C

CODES = list(range(10))
OPS = [E.SUM, E.PROD, E.MAX, E.MIN]
FP = (6, 7, 8, 9)


# ---- the existing generator is untouched --------------------------------------------------
def test_existing_sequence_draws_are_unchanged():
    """sha256 of sequence(default_rng(7000), 40) as JSON, computed before
    rs_sequence was added: ipc_worker.py's "seq" modes and the existing seeds
    depend on these draws."""
    seq = S.sequence(np.random.default_rng(7000), 40)
    digest = hashlib.sha256(json.dumps(seq, sort_keys=True).encode()).hexdigest()
    assert digest == "98a6e5f8eebeea98461cc3fe2cc7e74586a0939d0ed6efa81fde3bce5ad1c2dc"


# ---- the adapter ------------------------------------------------------------------------------
@pytest.mark.parametrize("code", CODES)
def test_adapter_agrees_with_the_oracle_on_mid_range_inputs(orc, code):
    rng = np.random.default_rng(40 + code)
    x, acc = vnode.gen(code, 4099, rng), vnode.gen(code, 4099, rng)
    for op in OPS:
        a, b = rs_ref.ELEM_REF.apply(code, op, x, acc), orc.apply(code, op, x, acc)
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), (code, op)
    inputs = [vnode.gen(code, 3 * 1001, rng) for _ in range(3)]
    rings = [[0, 2, 1]]
    for op in OPS:
        a = rs_ref.expected(rs_ref.ELEM_REF, inputs, code, op, 1, 96, rings, 16384)
        b = rs_ref.expected(orc, inputs, code, op, 1, 96, rings, 16384)
        assert all(u.tobytes() == v.tobytes() for u, v in zip(a, b)), (code, op)


def test_fold_keeps_the_ring_operand_order():
    """fold calls fn(x[s_k], acc), the new source first: pinned with a functor
    that does not commute.  The reference's own functors hide the order (Sum /
    Prod commute, fmax / fmin put +0 above -0 from either side), so a functor
    that picked equal operands by position would show only here and in the
    signed-zero columns of the edge inputs."""

    class Positional:
        @staticmethod
        def apply(code, op, x, acc):
            return (2 * acc + x).astype(x.dtype)

    a, b, c = (np.array([v], np.int64) for v in (1, 10, 100))
    assert rs_ref.fold(Positional, 4, 0, [a, b, c]).tolist() == [2 * (2 * 1 + 10) + 100]
    for code in FP:
        pz, nz = E.from_bits(code, [0]), E.from_bits(code, [E.fp_fields(code)[4]])
        for op, want in ((E.MAX, pz), (E.MIN, nz)):
            for parts in ([pz, nz], [nz, pz], [nz, pz, nz], [pz, nz, pz]):
                got, _ = rs_ref.fold_classes(code, op, parts)
                assert got.tobytes() == want.tobytes(), (code, op)
    # the classes are those of every step, not of the end result alone
    code = 7
    one, big = np.array([1.0], np.float32), np.array([3.4e38], np.float32)
    _, classes = rs_ref.fold_classes(code, E.SUM, [big, big, -big, one])
    assert "inf" in classes


# ---- section 2's inputs -------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 4])
def test_edge_inputs_are_not_vacuous(n):
    """edge_inputs asserts, per block: >= 75 % of the expected elements
    non-NaN and every required class met in some step.  Here also: the layout
    (block d folds sources 0, 1, .. on the identity ring) and that the blocks
    differ from each other."""
    for code in CODES:
        for op in OPS:
            inputs = rs_ref.edge_inputs(n, code, op)
            cnt = inputs[0].size // n
            if n == 2:
                for d in range(2):
                    x, y = E.edge_pairs(code, seed=d)
                    assert inputs[0][d * cnt:(d + 1) * cnt].tobytes() == x.tobytes()
                    assert inputs[1][d * cnt:(d + 1) * cnt].tobytes() == y.tobytes()
            else:
                for d in range(n):
                    srcs = E.edge_sources(code, n, op, seed=d,
                                          nrandom=rs_ref.BF16_RANDOM if code == 9 else E.N_RANDOM)
                    for k in range(n):  # the k-th rank block d's fold visits holds source k
                        r = (d + 1 + k) % n
                        assert inputs[r][d * cnt:(d + 1) * cnt].tobytes() == srcs[k].tobytes(), (code, op, d, k)
            exp = rs_ref.expected(rs_ref.ELEM_REF, inputs, code, op, 1, 96, [list(range(n))], 1 << 22)
            assert len({e.tobytes() for e in exp}) == n, (code, op)


# ---- the host ring on those inputs ----------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 4])
def test_host_ring_reduce_scatter_on_edge_values(n):
    """All forty (dtype, op) pairs, two channels, several loops (16 KiB
    buffer), against rs_ref under elem_ref: NaNs as "is NaN", the rest bit
    for bit."""
    rings = [list(range(n))] * 2
    bad = {}
    for code in CODES:
        for op in OPS:
            inputs = rs_ref.edge_inputs(n, code, op)
            cnt = inputs[0].size // n
            exp = rs_ref.expected(rs_ref.ELEM_REF, inputs, code, op, 2, 96, rings, 16384)
            assert len({b for b, _, _ in rs_ref.pieces(cnt, code, 2, 96, 16384)}) == 2
            sends = [x.copy() for x in inputs]
            recvs = [np.zeros(cnt, vnode.NPDT[code]) for _ in range(n)]
            C.host_ring_reduce_scatter(sends, recvs, cnt, code, op, channels=2, nthreads=96, buffer_size=16384,
                                       rings=rings)
            for r in range(n):
                ok, live = E.same_bits(code, recvs[r], exp[r])
                assert live >= 0.75
                if not ok:
                    i = E.mismatches(code, recvs[r], exp[r])
                    bad[(code, op, r)] = (i.size, i[:4].tolist(),
                                          [hex(v) for v in E.bits_of(code, recvs[r])[i[:4]].tolist()],
                                          [hex(v) for v in E.bits_of(code, exp[r])[i[:4]].tolist()])
                assert sends[r].tobytes() == inputs[r].tobytes(), (code, op, r, "sendbuff written")
    assert not bad, bad


# ---- part one of the fuzz: coverage of the case list -------------------------------------------------
def _plan(case):
    rings = F.case_rings(case)
    es = vnode.ESIZE[case["code"]]
    nch, nthr, sel = vnode.Planner(len(rings), rings).select(case["count"] * es * case["n"], case["count"] * es)
    buff = case["cfg"].get("buffer_size", 1 << 22)
    pieces = rs_ref.pieces(case["count"], case["code"], nch, nthr, buff)
    loops = -(-case["count"] // (nch * (buff // 8 // es * 4)))
    return nch, pieces, loops


def test_fuzz_cases_cover_the_list(orc):
    cases = [F._case(F.SEED_BASE + k) for k in range(F.DEFAULT_CASES)]
    assert {c["code"] for c in cases} == set(CODES)
    assert {c["op"] for c in cases} == set(OPS)
    ns = {c["n"] for c in cases}
    assert 2 in ns and 8 in ns and ns & {3, 5, 7}
    plans = [_plan(c) for c in cases]
    assert sum(loops == 3 for _, _, loops in plans) >= 3
    assert sum({b for b, _, _ in pieces} != set(range(nch)) for nch, pieces, _ in plans) >= 2
    assert sum(c["cfg"].get("lanes", 0) > 1 and c["cfg"].get("fifo_slots") == 8 for c in cases) >= 3
    assert sum(c["slice2"] for c in cases) >= 2
    assert sum(c["inplace"] for c in cases) >= 3
    assert any(c["fifo_works"] for c in cases)
    for key, vals in (("block_threads", {128, 256, 544, 576}), ("buffer_size", {1 << 16, 1 << 20, 1 << 21}),
                      ("fifo_slots", {8, 16, 32}), ("lanes", {1, 2, 3})):
        assert {c["cfg"][key] for c in cases if key in c["cfg"]} == vals, key
    assert any(c["cfg"].get("fifo_memory") == C.FIFO_DEVICE for c in cases)
    assert any(c["cfg"].get("locality") == C.LOCALITY_SENDER for c in cases)
    assert any("rings" in c["cfg"] for c in cases)
    # sensitivity of the expected values on the generated inputs
    order_seen = 0
    for c in cases:
        inputs = F.case_inputs(c)
        exp = F.case_expected(orc, c, inputs)
        n = c["n"]
        if c["count"] >= 2:
            for r in range(n):
                assert exp[r].tobytes() != exp[(r + 1) % n].tobytes(), (c, r)
        if c["code"] in FP and n >= 3:
            plain = rs_ref.rank_order(orc, inputs, c["code"], c["op"])
            order_seen += any(e.tobytes() != p.tobytes() for e, p in zip(exp, plain))
    assert order_seen >= 5, order_seen


# ---- part two: the sequences ------------------------------------------------------------------------------
def test_rs_sequences_put_every_algorithm_next_to_a_reduce_scatter():
    want = {"ll", "oneshot", "direct", "ring", "ag"}
    before, after = set(), set()
    kinds = []
    for seed in range(F.SEQ_SEEDS):
        rng, n, cfg = F.seq_setup(F.SEQ_BASE + seed)
        seq = F.rs_sequence(rng, 40)
        b, a = F.neighbours(seq, n)
        before |= b
        after |= a
        kinds += [o["kind"] for o in seq]
    assert before >= want and after >= want, (before, after)
    share = sum(k in ("rs", "rsgroup") for k in kinds) / len(kinds)
    assert 0.28 <= share <= 0.42, share  # about 35 % of the draws
    assert {"ar", "ag", "group", "rs", "rsgroup"} <= set(kinds)


def test_rs_sequence_sizes_and_groups():
    """A ReduceScatter block is between one element and 16 MiB / n; a group
    is one dtype and op (plan.cpp refuses a mixed one); every dtype and op
    occurs in an rs over the seeds the GPU tests use."""
    pairs = set()
    setups = ([(F.SEQ_BASE + s, 40) for s in range(F.SEQ_SEEDS)] + [(F.STREAM_BASE + s, 40) for s in range(F.STREAM_SEEDS)]
              + [(F.GRAPH_BASE + s, F.GRAPH_OPS) for s in range(F.GRAPH_SEEDS)])
    for seed, nops in setups:
        rng, n, _ = F.seq_setup(seed)
        for o in F.rs_sequence(rng, nops):
            calls = F.resolve(o, n)
            assert len({(c["kind"], c["code"], c["op"]) for c in calls}) == 1
            for c in calls:
                es = 1 if c["kind"] == "ag" else vnode.ESIZE[c["code"]]
                cap = F.MAX_BYTES // n if c["kind"] == "rs" else F.GROUP_BYTES // n if c["kind"] == "rsgroup" else \
                    F.GROUP_BYTES if c["kind"] == "group" else F.MAX_BYTES
                assert 1 <= c["count"] and c["count"] * es <= max(es, cap), (c, n)
            if o["kind"] == "rs":
                pairs.add((o["code"], o["op"]))
            if o["kind"] == "rsgroup":
                assert 2 <= len(calls) <= 4 and o["code"] in range(6)
    assert {c for c, _ in pairs} == set(CODES) and {o for _, o in pairs} == set(OPS)
    for world in (2, 3, 4):  # tests/ipc_worker.py "rsseq"
        seq = F.rs_sequence(np.random.default_rng(F.IPC_BASE + world), 40)
        assert sum(o["kind"] == "rs" for o in seq) >= 5 and any(o["kind"] == "rsgroup" for o in seq)
        assert F.sized(0.0, 4, F.MAX_BYTES // world) == 1
        assert F.sized(1.0, 4, F.MAX_BYTES // world) * 4 <= F.MAX_BYTES // world
