"""CPU: what the guarded mixed-alignment sweeps of
tests/test_gpu_footprint_collectives.py cover, and their cases on the
host-thread ring.

1. For every GPU sweep the union of footprint_cases.slice_paths over its cases
   contains the paths the sweep is meant to reach: the typed loop, whole wave
   units, remainder packs, a typed tail, no pack, an empty part, and the
   alternation units -> typed -> units on one parity counter (both parities)
   wherever the schedule has three slices of a parity.  It has none at n = 2
   (two calls per loop on one block base each) and none on a one-hop AllToAll
   (every send of an element reads one block, every recv writes one), which
   the model shows too.  Broadcast and Reduce make one call per loop at one
   offset: they need the ranks of one chain on different paths instead.
2. Every case can fail: its expectation differs from the NOT prefill in every
   byte and from every single input.
3. The same cases run on the host-thread ring on footprint.Guarded CPU
   buffers, built and checked by the code the GPU tests use
   (footprint_cases.Buffers): results bit for bit, pads intact, sources
   unchanged.
"""
import numpy as np
import pytest

import footprint_cases as K
from footprint_cases import ROOTED_PATHS, SWEEP_PATHS

NO_ALT = SWEEP_PATHS - {"alternation", "alternation by block base"}
RS_PATHS = {2: NO_ALT, 3: SWEEP_PATHS, 8: SWEEP_PATHS}
# n = 2: four channels cut the 24 KiB + 8 block into 8 KiB parts and 8 bytes, no part has packs and a tail
A2A_PATHS = {"n2": NO_ALT - {"tail"}, "n4": NO_ALT, "n8": NO_ALT, "n6": SWEEP_PATHS, "n3-relay": SWEEP_PATHS}
ROOTED = [(n, root) for n in (2, 3, 8) for root in K.roots(n)]
ROOTED_IDS = [f"n{n}-root{root}" for n, root in ROOTED]


# ---- 1. coverage ------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 3, 8])
def test_reduce_scatter_sweep_reaches_its_paths(n):
    assert K.reached(K.rs_cases(n)) >= RS_PATHS[n]


def test_sweeps_reach_the_alternation_as_a_whole():
    assert K.reached([c for n in (2, 3, 8) for c in K.rs_cases(n)]) >= SWEEP_PATHS
    assert K.reached([c for s in K.A2A_SHAPES for c in K.a2a_cases(s)]) >= SWEEP_PATHS


@pytest.mark.parametrize("func", ["bc", "rd"])
@pytest.mark.parametrize("n,root", ROOTED, ids=ROOTED_IDS)
def test_rooted_sweeps_reach_their_paths(func, n, root):
    cases = K.rooted_cases(func, n, root)
    assert K.reached(cases) >= ROOTED_PATHS
    assert all(not K.alternation_parities(K.slice_paths(c)) for c in cases[-3:])  # one call per loop at one offset
    names = {c.name for c in cases}
    assert {"only the root", "only the chain's last rank", "in place, per rank"} <= names


@pytest.mark.parametrize("shape", list(K.A2A_SHAPES))
def test_all_to_all_sweep_reaches_its_paths(shape):
    cases = K.a2a_cases(shape)
    assert K.reached(cases) >= A2A_PATHS[shape]
    n, relay, cc, _, _ = K.A2A_SHAPES[shape]
    route = K.elements(cases[0])[1]
    want = {"n2": (1, 4), "n4": (1, 2), "n8": (1, 1), "n6": (5, 0), "n3-relay": (2, 0)}
    assert (route["hops"], route["m"]) == want[shape]
    assert all(len({o for pair in c.offs for o in pair}) > 1 for c in cases if c.name == "per rank")


def test_allgather_alternation_cases_reach_it():
    cases = K.ag_alternation_cases()
    assert K.reached(cases) >= {"alternation", "units", "typed", "tail"}
    assert K.reached([c for c in cases if c.inplace]) >= {"alternation by block base"}
    assert K.reached([c for c in cases if not c.inplace]) >= {"alternation by block base"}


@pytest.mark.parametrize("func", ["rs", "a2a"])
@pytest.mark.parametrize("n", [2, 3, 8])
def test_several_loops_cases(func, n):
    cases = K.loops_cases(func, n)
    walk = K.C.ring_walk(K.FUNCS[func], n, 1, 1 if func == "a2a" else 2, K.elements(cases[0])[0], K.LOOPS_BUFF,
                         cases[0].count)
    assert [nelem for _, _, _, nelem in walk][:2] == [walk[0][1]] * 2 and len(walk) == 3  # two whole loops, a third
    assert 0 < walk[2][3] < walk[0][1] and cases[0].count * cases[0].es % 16 == 8
    # the GPU test runs them in two halves: aligned buffers first, then the rest
    assert len(cases) == (4 if func == "rs" else 3) and cases[0].name == "send+0 recv+0"
    assert K.reached(cases[:2]) >= {"units", "typed", "tail"} | ({"alternation by block base"} if n > 2 else set())
    assert K.reached(cases[2:]) >= {"units", "typed", "tail"} | ({"alternation"} if n > 2 else set())


@pytest.mark.parametrize("func", ["rs", "a2a"])
@pytest.mark.parametrize("shape", list(K.LAUNCH_SHAPES))
def test_launch_shape_cases(func, shape):
    assert K.reached(K.launch_shape_cases(func, shape)) >= {"typed", "packs", "tail"}


def test_two_element_cases():
    """One launch, two elements: the first typed throughout, the second with
    whole units, in one work (equal thread counts)."""
    typed, units = K.two_element_cases()
    assert K.reached([typed]) == {"typed"}
    assert K.reached([units]) >= {"units", "tail"}
    assert K.elements(typed)[0] == K.elements(units)[0]


def test_a_multiple_of_the_pack_loses_the_alternation():
    """The model decides the counts: with blocks of whole packs every block
    base is aligned and no slice of an aligned call is typed."""
    for n, (code, count, buff) in K.ALT_RS.items():
        if n == 2:  # two slices per loop, one block base each: nothing to lose
            continue
        pack = 16 // K.ESIZE[code]
        cases = [c for c in K.rs_cases(n) if c.count == count]
        assert "alternation by block base" in K.reached(cases)
        assert "alternation by block base" not in K.reached([K.with_count(c, count // pack * pack) for c in cases])


def test_path_model_on_cases_worked_by_hand():
    """ReduceScatter, n = 3, identity ring, aligned buffers, three loops of
    blocks of 8 bytes modulo 16: rank 1's calls of a loop work on blocks 0, 2
    and 1, so slices 2, 5 and 8 are typed; both lanes hold whole units."""
    case = [c for c in K.rs_cases(3) if c.count == K.ALT_RS[3][1] and c.name == "send+0 recv+0"][0]
    paths = K.slice_paths(case)
    assert set(paths) == {(r, 0, lane) for r in range(3) for lane in range(2)}
    seq = paths[(1, 0, 1)]
    assert [p.split("+")[0] for p in seq] == ["units", "units", "typed"] * 3
    assert seq[6] == "units+tail" and paths[(1, 0, 0)][0] == "units"
    assert K.alternation_parities({0: seq}) == {0, 1}
    # blocks of one fp16 element: only block 0 is aligned (rank 0 receives it), and the second lane has nothing
    one = [c for c in K.rs_cases(3) if c.count == 1 and c.name == "send+0 recv+0"][0]
    assert K.slice_paths(one)[(0, 0, 0)] == ["typed", "typed", "no pack"]
    assert K.slice_paths(one)[(0, 0, 1)] == ["empty"] * 3
    assert K.part_path(64 * 8 * 8, 2, True) == "units" and K.part_path(64 * 8 * 8 - 8, 2, True) == "packs"
    assert K.part_path(64 * 4 * 16, 1, True) == "units" and K.part_path(64 * 4 * 16 - 1, 1, True) == "packs+tail"


# ---- 2. and 3. every case can fail, and passes on the host ring ----------------------------
def host_sweep(orc, cases):
    bad = {}
    for case in cases:
        xs, exp = K.inputs(case), K.expected(orc, case)
        msg = K.can_fail_message(case, exp)
        assert not msg, (case.tag(), msg)
        b = K.Buffers(case, xs, exp)
        for r, d in enumerate(b.recvs):  # the prefill differs from the expectation in every byte
            if d is not None and exp[r] is not None and not (case.func == "bc" and case.inplace and r == case.root):
                assert np.all(d.read() ^ np.ascontiguousarray(exp[r]).view(np.uint8).reshape(-1) == 0xFF), case.tag()
        K.host_run(case, b)
        for r, m in b.check().items():
            bad[case.tag() + (r,)] = m
    assert not bad, K.F.brief(bad)


@pytest.mark.parametrize("n", [2, 3, 8])
def test_host_ring_reduce_scatter_cases(orc, n):
    host_sweep(orc, K.rs_cases(n))


@pytest.mark.parametrize("func", ["bc", "rd"])
@pytest.mark.parametrize("n,root", ROOTED, ids=ROOTED_IDS)
def test_host_ring_rooted_cases(orc, func, n, root):
    host_sweep(orc, K.rooted_cases(func, n, root))


@pytest.mark.parametrize("shape", list(K.A2A_SHAPES))
def test_host_ring_all_to_all_cases(orc, shape):
    host_sweep(orc, K.a2a_cases(shape))


@pytest.mark.parametrize("func", ["rs", "a2a"])
def test_host_ring_loops_shapes_and_two_elements(orc, func):
    cases = [c for n in (2, 3, 8) for c in K.loops_cases(func, n)]
    cases += [c for s in K.LAUNCH_SHAPES for c in K.launch_shape_cases(func, s)]
    host_sweep(orc, cases + (list(K.two_element_cases()) if func == "rs" else []))


def test_allgather_cases_can_fail_and_their_buffers_are_what_they_say(orc):
    """The host ring has no AllGather: the cases' buffers are checked by
    doing the gather with numpy through the pointers the ranks would pass."""
    import ctypes

    for case in K.ag_alternation_cases():
        xs, exp = K.inputs(case), K.expected(orc, case)
        assert not K.can_fail_message(case, exp)
        b = K.Buffers(case, xs, exp)
        B = case.count
        assert b.check()  # nothing gathered yet: every rank fails
        blocks = [bytes((ctypes.c_ubyte * B).from_address(b.send[r])) for r in range(case.n)]
        for r in range(case.n):
            assert b.send[r] % 16 == K.bases(case, r)[0] % 16 and b.recv[r] % 16 == K.bases(case, r)[1] % 16
            for s in range(case.n):
                ctypes.memmove(b.recv[r] + s * B, blocks[s], B)
        assert not b.check(), case.tag()
        past = (ctypes.c_ubyte * 1).from_address(b.recv[0] + case.n * B)
        past[0] ^= 0xFF  # one byte too many is seen
        assert "wrote outside" in b.check()[0]
