"""CPU: what tests/refdrv_worker.py's mode "avg" launches can fail.

The cases of tests/refdrv_avg_cases.py are pure functions of the world size
and the plan.  For both configurations the worker runs (the reference ring and
the two-channel override), at the plans vnode.Planner(2, rings).select gives,
the conditions the worker asserts before each launch are asserted here without
a GPU: an edge-value expectation that is mostly non-NaN and far from the plain
Sum's, a rounding case in which a fused multiply-add would show, batched tasks
whose scalars cannot be swapped unnoticed, and a launch sequence in which no
launch can be skipped.  The case functions raise where a condition is missed;
the tests below call them and check what they return.
"""
import numpy as np
import pytest

import avg_ref as A
import elem_ref as E
import refdrv_avg_cases as K
import test_gpu_avg_rounding as R
from mccs_amd import refdrive


def _plans(n, nbytes):
    return {name: K.plan_of(rings, nbytes) for name, rings in K.variant_rings(n).items()}


def test_variants_are_the_workers():
    import refdrv_worker

    assert (K.OVERRIDE8, K.NTHR_OF_BUCKET) == (refdrv_worker.OVERRIDE8, refdrv_worker.NTHR_OF_BUCKET)
    for n in (2, 3):
        v = K.variant_rings(n)
        assert list(v) == ["ref_sender", "override_receiver"]
        assert v["ref_sender"] == refdrive.reference_rings(n, 2)
        assert all(sorted(r) == list(range(n)) for r in v["override_receiver"])
    assert K.variant_rings(3)["override_receiver"] == [[0, 1, 2], [2, 1, 0]]


@pytest.mark.parametrize("n", [2, 3])
def test_edge_sweep_covers_the_sixteen_pairs_and_can_fail(n):
    cases = K.edge_cases(n)
    assert {(c, o) for c, o, _ in cases} == set(A.PAIRS) and len(A.PAIRS) == 16 and len(cases) == 32
    assert not any(o == A.SUMPOSTDIV and A.divisor(a) == 0 for _, o, a in cases)
    for code, op, arg in cases:
        inputs = K.edge_inputs(n, code)
        count = inputs[0].size
        assert count % (16 // K.ESIZE[code]) != 0  # the last chunk ends in a typed tail
        assert rs_size(n, code) - count in (0, 1)
        for name, plan in _plans(n, count * K.ESIZE[code]).items():
            exp = K.edge_expected(n, code, op, arg, plan)  # asserts >= 75 % non-NaN, >= half unlike the Sum
            assert len(exp) == n and all(e.size == count for e in exp), (name, code, op)


def rs_size(n, code):
    import rs_ref

    return rs_ref.edge_inputs(n, code, E.SUM)[0].size


@pytest.mark.parametrize("code", K.ROUNDING_CODES, ids=["fp16", "bf16", "fp32", "fp64"])
def test_rounding_case_tells_a_fused_multiply_add_apart(code):
    """The sanity check that the rounding case can fail: at the reference plan
    of each variant the single-rounding alternative differs from the contract
    in at least 10 % of every rank's elements."""
    assert (R.N, R.N * R.CNT) == (3, 3009)
    inputs = K.rounding_inputs(code)
    assert len(inputs) == 3 and all(x.size == 3009 for x in inputs)
    for name, plan in _plans(3, 3009 * K.ESIZE[code]).items():
        exp, told_apart = K.rounding_expected(code, plan)
        print(f"dtype {code} {name} {plan[:2]}: a fused multiply-add changes {[round(t, 3) for t in told_apart]}")
        assert len(told_apart) == 3 and min(told_apart) >= 0.10, (name, told_apart)
        assert E.same_bits(code, exp[0], exp[1])[0] and E.same_bits(code, exp[0], exp[2])[0]


@pytest.mark.parametrize("n", [2, 3])
def test_buckets_take_every_block_size(n):
    seen = set()
    for code, op, arg, nbytes, inputs in K.bucket_cases(n):
        assert inputs[0].nbytes == nbytes <= 40000
        for plan in _plans(n, nbytes).values():
            K.bucket_expected(n, code, op, arg, nbytes, inputs, plan)
            seen.add((code, op, plan[1]))
    assert seen == {(c, o, t) for c, o in ((K.BF16, A.PREMULSUM), (K.I32, A.SUMPOSTDIV)) for t in (96, 160, 288, 544)}


@pytest.mark.parametrize("code,op", list(K.BATCH_ARGS), ids=["fp32-premulsum", "int32-sumpostdiv"])
@pytest.mark.parametrize("n", [2, 3])
def test_batched_plan_puts_scalars_where_the_case_says(n, code, op):
    tasks = K.batch_tasks(n, code, op)
    assert tasks[1][1] != tasks[2][1] and all(a.tobytes() == b.tobytes() for a, b in zip(tasks[1][2], tasks[2][2]))
    if code == K.F32:
        assert tasks[2][1] == 0  # the all-zero redOpArg the reference host uploads today
    else:
        assert {arg for _, arg, _ in tasks} == {2, 3, 7}
    host = [(0x100000 * (t + 1), 0x100000 * (t + 1) + 0x80000, count, code, arg)
            for t, (count, arg, _) in enumerate(tasks)]
    p = refdrive.build_plan(host, 2, 0)
    assert (p.chans, p.nworks, p.block, p.grid) == ([0, 1], [1, 2], 544, 2)
    first, chained = p.works[1][1], p.works[2][1]
    assert [p.works[i][0] for i in range(3)] == [0, 1, 2] and first.header.workNext == 2 and chained.header.isLast
    assert [(first.elems[i].isUsed, first.elems[i].redOpArg) for i in range(3)] == \
        [(1, tasks[1][1]), (1, tasks[2][1]), (0, 0)]
    assert (chained.elems[0].redOpArg, chained.elems[0].nWarps, chained.elems[1].isUsed) == (tasks[3][1], 5, 0)
    for name, rings in K.variant_rings(n).items():
        plans = K.batch_plans(rings, code, op)
        assert [(k, nthr) for k, nthr, _ in plans] == [(1, 544), (1, 96), (1, 96), (1, 160)]
        assert [pl[2] for pl in plans] == [[rings[c] for c in sel] for _, _, sel in p.tasks], name
        exp = K.batch_expected(n, code, op, plans)  # asserts that no two scalars can be swapped unnoticed
        assert K.differing(code, exp[1], exp[2]) >= 0.5
        if code == K.F32:  # scalar 0 on finite inputs: nothing but signed zeros, and both of them
            bits = np.concatenate([E.bits_of(code, e) for e in exp[2]])
            assert set(np.unique(bits).tolist()) == {0, 0x80000000}


@pytest.mark.parametrize("n", [2, 3])
def test_odd_and_sequence_cases_can_fail(n):
    for code, op, arg, inputs in K.odd_cases(n):
        assert inputs[0].size == K.ODD_COUNT == 4097
        for plan in _plans(n, 4097 * K.ESIZE[code]).values():
            K.odd_expected(n, code, op, arg, inputs, plan)
    assert [op for op, _ in K.SEQUENCE] == [E.SUM, A.PREMULSUM, E.MAX, A.SUMPOSTDIV, A.PREMULSUM, E.SUM]
    assert K.SEQUENCE[1][1] != K.SEQUENCE[4][1]
    for plan in _plans(n, K.SEQ_COUNT * 4).values():
        exp = K.sequence_expected(n, plan)  # asserts that consecutive launches differ in >= half the elements
        assert len(exp) == 6 and all(E.same_bits(K.I32, a, b)[0] for a, b in zip(exp[0], exp[5]))
