"""Test helper: the cases of tests/refdrv_worker.py's mode "avg" (CPU only).

The sixteen reference-named PreMulSum / SumPostDiv AllReduce kernels are
launched by symbol, one rank per process, by the worker; what they are
launched on, and what must come out, is decided here, as pure functions of
the world size and the plan, so tests/test_refdrive_avg_cases.py can assert
without a GPU that every case is able to fail:

  edge      rs_ref.edge_inputs(n, code, SUM) under both avg_ref.case_args of
            each of avg_ref.PAIRS; each expected array is >= 75 % non-NaN and
            differs from the plain Sum's in >= half its elements
            (test_gpu_avg_values.can_fail)
  rounding  test_gpu_avg_rounding's standard-normal inputs at n = 3 with the
            scalar 1/3: the contract round(round(x*s) + acc) and the single
            rounding round(x*s + acc) differ in >= 10 % of each rank's elements
  buckets   the byte sizes that make get_task_schema pick 96, 160, 288 and 544
            threads, random full-range bits
  batched   one plan whose tasks carry different scalars: two tasks in one
            work, one in a chained work of a 544-thread block; a task's
            expected output under any other scalar of the plan differs in
            >= half its elements (a swapped redOpArg cannot pass)
  odd       count 4097, both buffers one element past a 16-byte boundary
  sequence  six launches on the same buffers, the ops alternating; each
            expected output differs from the one before in >= half its elements

Expected values: avg_ref.allreduce_expected (tests/elem_ref.py underneath)
for Sum, PreMulSum and SumPostDiv; the same FIFO simulation under
elem_ref.ref_op for the sequence's one Max.  A plan is (k, nthreads, [ring of
each selected channel]), what RefDrivenRank.last_plan holds.
"""
from __future__ import annotations

from fractions import Fraction

import numpy as np

import avg_ref as A
import elem_ref as E
import ring_sim
import rs_ref
import test_gpu_avg_rounding as R
import vnode
from test_gpu_avg_values import can_fail, diff

# comm_patterns_override: tests/test_gpu_ring.py's two channels whose orders do
# not start at rank 0 and are no rotations of each other, cut down to the world
OVERRIDE8 = [[3, 0, 6, 1, 7, 2, 5, 4], [4, 5, 2, 7, 1, 6, 0, 3]]
NTHR_OF_BUCKET = {5000: 96, 10000: 160, 20000: 288, 40000: 544}  # get_task_schema, plan.rs:602-635
F16, BF16, F32, I32, I8 = 6, 9, 7, 2, 0
NCH = 2
BUFF = 1 << 22  # RefDrivenRank's default buffer_size, and ring_sim's
ESIZE = vnode.ESIZE

_cache = {}


def variant_rings(n):
    """The two configurations every mode of the worker runs."""
    return {"ref_sender": [list(range(n))] * NCH,
            "override_receiver": [[r for r in ring if r < n] for ring in OVERRIDE8]}


def planner(rings):
    return vnode.Planner(NCH, rings)


def plan_of(rings, nbytes):
    """The plan of one task launched alone (channel loads start at zero)."""
    return tuple(planner(rings).select(nbytes, nbytes))


def _key(plan):
    k, nthr, rings = plan
    return k, nthr, tuple(tuple(r) for r in rings)


def expected(inputs, code, op, arg, plan, buff=BUFF):
    """Per-rank outputs of one AllReduce under `plan`."""
    k, nthr, rings = plan
    if op in (E.SUM, A.PREMULSUM, A.SUMPOSTDIV):
        return A.allreduce_expected(inputs, code, op, arg, k, nthr, rings, buff_size=buff)
    return ring_sim.simulate([np.ascontiguousarray(x) for x in inputs], op, k, nthr, buff, ring=rings,
                             fn=lambda o, x, y: E.ref_op(code, o, x, y))


def differing(code, a, b):
    """Smallest share, over the ranks, of elements in which a and b differ."""
    return min(E.mismatches(code, x, y).size / x.size for x, y in zip(a, b))


# ---- a. edge values ------------------------------------------------------------------------
def edge_inputs(n, code):
    """rs_ref.edge_inputs(n, code, SUM), without its last element where the
    count is a multiple of a 16-byte pack (the 8-byte types at n = 2): the
    AllReduce count decides whether the last chunk ends in a typed tail."""
    inputs = rs_ref.edge_inputs(n, code, E.SUM)
    count, pack = inputs[0].size, 16 // ESIZE[code]
    if n == 2:  # edge_pairs: no block is a multiple of a pack either
        assert (count // n) % pack != 0
    if count % pack == 0:
        count -= 1
    assert count % pack != 0
    return [x[:count] for x in inputs]


def edge_cases(n):
    return [(code, op, arg) for code, op in A.PAIRS for arg in A.case_args(code, op, n)]


def edge_expected(n, code, op, arg, plan, buff=BUFF):
    """Expected per-rank outputs, checked once per plan against the plain Sum's."""
    key = ("edge", n, code, op, arg, _key(plan), buff)
    if key not in _cache:
        inputs = edge_inputs(n, code)
        pkey = ("edge_sum", n, code, _key(plan), buff)
        if pkey not in _cache:
            _cache[pkey] = expected(inputs, code, E.SUM, 0, plan, buff)
        exp = expected(inputs, code, op, arg, plan, buff)
        can_fail(code, exp, _cache[pkey], ("edge", n, code, op, hex(arg)))
        _cache[key] = exp
    return _cache[key]


# ---- b. the two roundings (n = 3) --------------------------------------------------------------
ROUNDING_CODES = (F16, BF16, F32, 8)
ROUNDING_SEED = {F16: 1, BF16: 1, F32: 1, 8: 1}
ROUNDING_FLOOR = 0.10


def rounding_inputs(code):
    key = ("rounding_inputs", code)
    if key not in _cache:
        rng = np.random.default_rng(ROUNDING_SEED[code])
        _cache[key] = [R.normal(code, R.N * R.CNT, rng) for _ in range(R.N)]
    return _cache[key]


def rounding_expected(code, plan, buff=BUFF):
    """(the contract's per-rank outputs, per rank the share of elements in which
    the single-rounding alternative differs).  The contract is computed twice,
    by avg_ref and from the fold order read off the schedule; the two agree."""
    key = ("rounding", code, _key(plan), buff)
    if key not in _cache:
        assert buff == BUFF, "test_gpu_avg_rounding.orders walks the default buffer size"
        k, nthr, rings = plan
        inputs = rounding_inputs(code)
        op, arg = A.avg_op(code, R.N)
        assert op == A.PREMULSUM
        exp = A.allreduce_expected(inputs, code, op, arg, k, nthr, rings, buff_size=buff)
        told_apart = []
        for e, o in zip(exp, R.orders("all_reduce", code, 0, k, nthr, rings)):
            contract, fused = R.both(inputs, code, arg, "all_reduce", o, 0)
            assert not diff(code, contract, e), "the fold order read off the schedule disagrees with avg_ref"
            told_apart.append(E.mismatches(code, fused, contract).size / contract.size)
        assert min(told_apart) >= ROUNDING_FLOOR, (code, told_apart)
        _cache[key] = (exp, told_apart)
    return _cache[key]


# ---- c. every block size -------------------------------------------------------------------------
def bucket_cases(n):
    """(code, op, arg, nbytes, inputs): bf16 PreMulSum by 1/3 and int32
    SumPostDiv by 7 at each bucket."""
    out = []
    for code, op, arg in ((BF16, A.PREMULSUM, A.avg_scalar_bits(BF16, 3)), (I32, A.SUMPOSTDIV, 7)):
        for nbytes in NTHR_OF_BUCKET:
            count = nbytes // ESIZE[code]
            inputs = [E.random_bits(code, count, np.random.default_rng([3, code, count, r])) for r in range(n)]
            out.append((code, op, arg, nbytes, inputs))
    return out


def bucket_expected(n, code, op, arg, nbytes, inputs, plan, buff=BUFF):
    key = ("bucket", n, code, nbytes, _key(plan), buff)
    if key not in _cache:
        assert plan[:2] == (1, NTHR_OF_BUCKET[nbytes]), plan
        exp = expected(inputs, code, op, arg, plan, buff)
        can_fail(code, exp, expected(inputs, code, E.SUM, 0, plan, buff), ("bucket", n, code, nbytes))
        _cache[key] = exp
    return _cache[key]


# ---- d. one plan, several scalars ------------------------------------------------------------------
# Task 0 (40 000 bytes, one channel, 544 threads) loads channel 0; tasks 1 and
# 2 (5 000 bytes, 96 threads) then both go to channel 1 and share its first
# work; task 3 (10 000 bytes, 160 threads) follows them there into a chained
# second work.  Tasks 1 and 2 have the same inputs: they differ in scalar only.
BATCH_BYTES = (40000, 5000, 5000, 10000)
BATCH_ARGS = {
    (F32, A.PREMULSUM): (A.encode(F32, Fraction(-3, 4)), A.avg_scalar_bits(F32, 3), 0, A.encode(F32, 3)),
    (I32, A.SUMPOSTDIV): (3, 2, 3, 7),
}


def batch_tasks(n, code, op):
    """[(count, arg, inputs)].  fp32: finite values of both signs that fill the
    mantissa (the all-zero scalar then leaves signed zeros to add up); int32:
    random full-range bits."""
    out = []
    for nbytes, arg in zip(BATCH_BYTES, BATCH_ARGS[(code, op)]):
        count = nbytes // ESIZE[code]
        if code == F32:
            inputs = [vnode.gen(F32, count, np.random.default_rng([4, count, r])) * np.float32(0.7) for r in range(n)]
            assert all(np.isfinite(x).all() and (x > 0).any() and (x < 0).any() for x in inputs)
        else:
            inputs = [E.random_bits(code, count, np.random.default_rng([4, count, r])) for r in range(n)]
        out.append((count, arg, inputs))
    assert op != A.SUMPOSTDIV or all(A.divisor(arg) != 0 for _, arg, _ in out)
    return out


def batch_plans(rings, code, op):
    """Per task the plan the merge gives it: channels by the plan's running load."""
    p = planner(rings)
    return [tuple(p.select(nbytes, nbytes)) for nbytes in BATCH_BYTES]


def batch_expected(n, code, op, plans, buff=BUFF):
    """Per task the expected per-rank outputs; a task's output under every
    other scalar of the plan differs from it in at least half the elements."""
    key = ("batch", n, code, op, tuple(_key(p) for p in plans), buff)
    if key not in _cache:
        tasks = batch_tasks(n, code, op)
        args = sorted({arg for _, arg, _ in tasks})
        assert len(args) >= 3
        out = []
        for (count, arg, inputs), plan in zip(tasks, plans):
            exp = expected(inputs, code, op, arg, plan, buff)
            for other in args:
                if other != arg:
                    share = differing(code, exp, expected(inputs, code, op, other, plan, buff))
                    assert share >= 0.5, ("batch", code, op, hex(arg), hex(other), share)
            out.append(exp)
        _cache[key] = out
    return _cache[key]


# ---- e. misaligned buffers ---------------------------------------------------------------------------
ODD_COUNT = 4097


def odd_cases(n):
    """(code, op, arg, inputs): fp16 PreMulSum by 1/3 on uniform values, int8
    SumPostDiv by 7 on random bits."""
    f16 = [vnode.gen(F16, ODD_COUNT, np.random.default_rng([5, F16, r])) for r in range(n)]
    i8 = [E.random_bits(I8, ODD_COUNT, np.random.default_rng([5, I8, r])) for r in range(n)]
    return [(F16, A.PREMULSUM, A.avg_scalar_bits(F16, 3), f16), (I8, A.SUMPOSTDIV, 7, i8)]


def odd_expected(n, code, op, arg, inputs, plan, buff=BUFF):
    key = ("odd", n, code, _key(plan), buff)
    if key not in _cache:
        exp = expected(inputs, code, op, arg, plan, buff)
        can_fail(code, exp, expected(inputs, code, E.SUM, 0, plan, buff), ("odd", n, code))
        _cache[key] = exp
    return _cache[key]


# ---- f. six launches on the same buffers ----------------------------------------------------------------
SEQ_COUNT = 2503  # int32: 10 012 bytes, one channel, 160 threads
SEQUENCE = [(E.SUM, 0), (A.PREMULSUM, A.encode(I32, 3)), (E.MAX, 0), (A.SUMPOSTDIV, 7),
            (A.PREMULSUM, A.encode(I32, -1)), (E.SUM, 0)]


def sequence_inputs(n):
    return [E.random_bits(I32, SEQ_COUNT, np.random.default_rng([6, r])) for r in range(n)]


def sequence_expected(n, plan, buff=BUFF):
    """Per launch the expected per-rank outputs; consecutive launches differ in
    at least half the elements, so a launch that did nothing, or ran with the
    scalar of an earlier one, cannot pass."""
    key = ("sequence", n, _key(plan), buff)
    if key not in _cache:
        inputs = sequence_inputs(n)
        out = [expected(inputs, I32, op, arg, plan, buff) for op, arg in SEQUENCE]
        for i in range(1, len(out)):
            assert differing(I32, out[i], out[i - 1]) >= 0.5, ("sequence", i)
        assert differing(I32, out[1], out[4]) >= 0.5  # the two PreMulSum scalars
        _cache[key] = out
    return _cache[key]
