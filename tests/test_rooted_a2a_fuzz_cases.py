"""CPU: what the case lists and overrides of tests/test_gpu_rooted_a2a_fuzz.py
cover, that every case can fail, and that the expected values the GPU tests
use agree with the host ring.

The lists are pure functions of their seeds.  DEFAULT_CASES there is, per list,
the smallest count from its seed base for which everything in
`coverage_gaps` and `sensitivity_gaps` below holds: test_default_cases_are_the_smallest
counts up from one to check that.
"""
import functools

import numpy as np
import pytest

import a2a_ref
import avg_ref
from mccs_amd import comm as C
import rooted_ref
import rs_ref
import test_gpu_all_to_all_sequences as A
import test_gpu_rooted_a2a_fuzz as F
import test_gpu_rooted_sequences as S
import vnode

LISTS = ("bc", "rd", "a2a")


# ---- the plan of a case ---------------------------------------------------------------------------
def plan(which, case):
    """(channels a buffer or block is split over, threads, size in the walk's
    units, dtype code of the walk).  bc / rd: the planner's selection for the
    buffer's bytes.  a2a, one hop: a block over the m channels of its pair,
    only the thread count from the schema; relayed: the schema's channels for
    n * B bytes (plan.cpp a2a_enqueue)."""
    if which == "a2a":
        rings = F.case_rings(case)
        nch, nthr = C.task_schema(case["n"] * case["size"], len(rings))
        m = F.a2a_route(case)["m"]
        return (m or nch), nthr, case["size"], 0
    nch, nthr, _ = F.rooted_plan(case)
    return (nch, nthr, case["size"], 0) if which == "bc" else (nch, nthr, case["count"], case["code"])


def loops(which, case):
    nch, _, size, code = plan(which, case)
    chunk = F.buffer_size(case) // 8 // vnode.ESIZE[code] * 4
    return -(-size // (nch * chunk))


def last_channel_runs_empty(which, case):
    """The last channel has no piece in some loop and makes an empty call that
    still takes and posts its steps.  Up to six channels a rooted call keeps a
    channel only while the buffer has 32 KiB for it, more than a granule, so
    its last channel never goes without any piece
    (test_gpu_rooted.test_empty_trailing_channels needs ten): it goes empty in
    the last loop of a several-loop call whose tail fits the earlier
    channels.  A one-hop AllToAll keeps all m channels of a pair at every
    size, so a block of a few bytes leaves the last one without any piece."""
    nch, nthr, size, code = plan(which, case)
    pieces = rs_ref.pieces(size, code, nch, nthr, F.buffer_size(case))
    return sum(bid == nch - 1 for bid, _, _ in pieces) < loops(which, case)


def relayed_by_rings(case):
    return a2a_ref.route(case["n"], F.case_rings(case))["hops"] != 1


# ---- coverage ---------------------------------------------------------------------------------------
def coverage_gaps(which, cases):
    """What the list still lacks: names of the requirements not met."""
    gaps = []

    def need(ok, name):
        if not ok:
            gaps.append(name)

    ns = {c["n"] for c in cases}
    need(2 in ns and 8 in ns and ns & {3, 5, 7}, "n = 2, 8 and an odd one")
    for key, vals in (("block_threads", {128, 256, 544, 576}), ("buffer_size", {1 << 16, 1 << 20, 1 << 21}),
                      ("fifo_slots", {8, 16, 32}), ("lanes", {1, 2, 3})):
        need({c["cfg"][key] for c in cases if key in c["cfg"]} == vals, key)
    need(sum(c["cfg"].get("lanes", 0) > 1 and c["cfg"].get("fifo_slots") == 8 for c in cases) >= 3, "lanes x 8 slots")
    need(sum(c["slice2"] for c in cases) >= 2, "slice2")
    need(any(c["slice2"] and c["cfg"].get("fifo_slots") == 8 for c in cases), "slice2 x 8 slots")
    need(any(c["cfg"].get("fifo_memory") == C.FIFO_DEVICE for c in cases), "FIFO_DEVICE")
    need(any(c["cfg"].get("locality") == C.LOCALITY_SENDER for c in cases), "LOCALITY_SENDER")
    need(any("rings" in c["cfg"] for c in cases), "permuted rings")
    need(any(c["fifo_works"] for c in cases), "fifo_works")
    need({c["kind"] for c in cases} == set(F.KINDS), "size kinds")
    need(sum(c["kind"] == "loops" and loops(which, c) == 3 for c in cases) >= 3, "three loops")
    need(sum(last_channel_runs_empty(which, c) for c in cases) >= 2, "empty last channel")
    if which == "rd":
        need({c["code"] for c in cases} == set(range(10)), "dtypes")
        need({c["op"] for c in cases} == set(range(6)), "ops")
        need(sum(c["inplace"] for c in cases) >= 3, "in place")
        need(any(c["root"] == 0 for c in cases) and any(c["root"] == c["n"] - 1 for c in cases)
             and any(0 < c["root"] < c["n"] - 1 for c in cases), "roots")
        need(any("rings" in c["cfg"] and len({list(r).index(c["root"]) for r in c["cfg"]["rings"]}) > 1
                 for c in cases), "root at different positions")
    if which == "bc":
        need(any(c["inplace"] for c in cases) and any(not c["inplace"] for c in cases), "in and out of place")
        offs = {o for c in cases for o in c["recv_off"]}
        need(0 in offs and any(o % 16 for o in offs), "receive offsets")
    if which == "a2a":
        routes = [F.a2a_route(c) for c in cases]
        need(sum(r["hops"] == 1 for r in routes) >= 3, "one hop")
        need(sum(not c["relay"] and relayed_by_rings(c) for c in cases) >= 3, "relayed by the ring set")
        need(sum(c["relay"] and not relayed_by_rings(c) for c in cases) >= 2, "relayed by the variable")
        relays = [c for c, r in zip(cases, routes) if r["hops"] != 1]
        need(any(c["cfg"].get("fifo_memory") == C.FIFO_DEVICE for c in relays), "relay x FIFO_DEVICE")
        need(any(c["cfg"].get("fifo_slots") == 8 and c["slice2"] for c in relays), "relay x 8 slots x slice2")
    return gaps


# ---- every case can fail ------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _rd_facts(seed):
    """Per rd case (by seed): (differs from every single input, ring order
    visible, differs from the plain Sum)."""
    from oracle import oracle as orc

    c = F.rd_case(seed)
    inputs = F.rd_inputs(c)
    exp = F.rd_expected(orc, c, inputs)
    code, op = c["code"], c["op"]
    not_an_input = all(exp.tobytes() != x.tobytes() for x in inputs)
    nch, nthr, rings = F.rooted_plan(c)
    order = None
    if code in F.FP and c["n"] >= 3 and op != avg_ref.SUMPOSTDIV:
        srcs = [avg_ref.pre(code, x, c["op_arg"]) for x in inputs] if op == avg_ref.PREMULSUM else inputs
        order = exp.tobytes() != rooted_ref.rank_order(orc, srcs, code, 0 if op == avg_ref.PREMULSUM else op).tobytes()
    not_sum = None
    if op >= avg_ref.PREMULSUM:
        plain = rooted_ref.reduce_expected(orc, inputs, code, 0, c["root"], nch, nthr, rings, F.buffer_size(c))
        not_sum = exp.tobytes() != plain.tobytes()
    return not_an_input, order, not_sum


def sensitivity_gaps(which, cases):
    gaps = []
    if which == "bc":
        for c in cases:
            words = c["size"] // 4
            datas = [F.bc_data(r, c["size"])[:4 * words].view(np.int32) for r in range(c["n"])]
            for a in range(c["n"]):
                for b in range(a):
                    if words and not (datas[a] != datas[b]).all():
                        gaps.append(("two roots share a word", c["seed"]))
    if which == "rd":
        facts = [(c, _rd_facts(c["seed"])) for c in cases]
        gaps += [("the result is one rank's input", c["seed"]) for c, f in facts if c["count"] >= 2 and not f[0]]
        gaps += [("the new op gives the plain Sum", c["seed"]) for c, f in facts if f[2] is False]
        if sum(f[1] is True for _, f in facts) < 5:
            gaps.append(("ring order visible in fewer than 5 cases",))
    if which == "a2a":
        for c in cases:
            n, B = c["n"], min(c["size"], 64)
            if B >= 4:  # block (s, t) is a ramp from 31 s + 7 t + salt: its first 64 bytes at any B
                xs = a2a_ref.make_inputs(n, B, salt=c["seed"] % 7)
                blocks = {xs[s][t * B:(t + 1) * B].tobytes() for s in range(n) for t in range(n)}
                if len(blocks) != n * n:
                    gaps.append(("two blocks are equal", c["seed"]))
    return gaps


@pytest.mark.parametrize("which", LISTS)
def test_fuzz_cases_cover_the_list(which):
    cases = F.cases(which)
    assert F.MAKE[which](F.SEED_BASE[which]) == cases[0]  # pure functions of the seed
    assert not coverage_gaps(which, cases)
    assert not sensitivity_gaps(which, cases)


@pytest.mark.parametrize("which", LISTS)
def test_default_cases_are_the_smallest(which):
    """One case fewer leaves a gap.  Every coverage requirement is "at least k
    cases", which a shorter list meets no better, and a per-case sensitivity
    failure stays in every longer list: so no smaller count is free of gaps."""
    fewer = F.cases(which, F.DEFAULT_CASES[which] - 1)
    assert coverage_gaps(which, fewer) or sensitivity_gaps(which, fewer)


def test_a2a_block_prefix_is_size_independent():
    """sensitivity_gaps looks at the first 64 bytes of every block: they do not depend on B."""
    n = 5
    small, large = a2a_ref.make_inputs(n, 64, 3), a2a_ref.make_inputs(n, 4099, 3)
    for s in range(n):
        for t in range(n):
            assert small[s][t * 64:(t + 1) * 64].tobytes() == large[s][t * 4099:t * 4099 + 64].tobytes()


def test_no_configuration_is_excluded():
    """The generators exclude nothing the value sets allow but SumPostDiv on a
    floating type (mccs_hip.h: defined for the integer types), which becomes
    PreMulSum."""
    for c in F.cases("rd", 200):
        assert not (c["op"] == avg_ref.SUMPOSTDIV and c["code"] in F.FP)
        assert (c["op_arg"] is None) == (c["op"] < avg_ref.PREMULSUM)
    for which in LISTS:
        for c in F.cases(which, 200):
            assert 2 <= c["n"] <= 8 and len(F.case_rings(c)) >= 1
            assert all(sorted(r) == list(range(c["n"])) for r in F.case_rings(c))
            if c["kind"] == "loops":
                assert F.buffer_size(c) == F.LOOP_BUFFER and loops(which, c) == 3, c


# ---- the expected values against the host ring ------------------------------------------------------------
def test_reduce_expected_values_match_the_host_ring(orc):
    """n <= 4: mccs_host_ring_reduce with the planner's channels, threads,
    rings and the case's buffer size gives the value the GPU test expects."""
    seen = set()
    for c in F.cases("rd"):
        if c["n"] > 4:
            continue
        inputs = F.rd_inputs(c)
        exp = F.rd_expected(orc, c, inputs)
        nch, nthr, rings = F.rooted_plan(c)
        recvs = [np.zeros_like(x) if r == c["root"] else None for r, x in enumerate(inputs)]
        C.host_ring_reduce([x.copy() for x in inputs], recvs, c["count"], c["code"], c["op"], c["root"], channels=nch,
                           nthreads=nthr, buffer_size=F.buffer_size(c), rings=rings, op_arg=c["op_arg"])
        assert recvs[c["root"]].tobytes() == exp.tobytes(), c
        seen.add(c["op"] >= avg_ref.PREMULSUM)
    assert seen == {False, True}


def test_scaled_route_matches_avg_ref(orc):
    """rd_expected folds bf16 PreMulSum cases above 4099 elements under the
    oracle's Sum: on every PreMulSum case small enough for avg_ref's exact
    rationals that route gives avg_ref.reduce_expected's bits."""
    checked, bf16 = 0, 0
    for c in F.cases("rd", 4 * F.DEFAULT_CASES["rd"]):
        if c["op"] != avg_ref.PREMULSUM or c["count"] > (4099 if c["code"] == F.BF16 else 1 << 16):
            continue
        inputs = F.rd_inputs(c)
        nch, nthr, rings = F.rooted_plan(c)
        ref = avg_ref.reduce_expected(inputs, c["code"], c["op"], c["op_arg"], c["root"], nch, nthr, rings,
                                      F.buffer_size(c))
        assert F.rd_expected_scaled(orc, c, inputs).tobytes() == ref.tobytes(), c
        checked += 1
        bf16 += c["code"] == F.BF16
    assert checked >= 8 and bf16 >= 1, (checked, bf16)


def test_broadcast_expected_values_match_the_host_ring():
    for c in F.cases("bc"):
        if c["n"] > 4:
            continue
        n, root, size = c["n"], c["root"], c["size"]
        nch, nthr, rings = F.rooted_plan(c)
        data = F.bc_data(root, size)
        recvs = [np.zeros(size, np.uint8) for _ in range(n)]
        C.host_ring_broadcast([data if r == root else None for r in range(n)], recvs, size, root, channels=nch,
                              nthreads=nthr, buffer_size=F.buffer_size(c), rings=rings)
        want = rooted_ref.broadcast_expected([F.bc_data(r, size) for r in range(n)], root)
        for r in range(n):
            assert recvs[r].tobytes() == want.tobytes(), (c, r)


def test_all_to_all_expected_values_match_the_host_ring_on_permuted_rings():
    """tests/test_all_to_all_host.py holds a2a_ref.expected to the host ring on
    the default rings; here one case of the list with permuted rings."""
    c = next(c for c in F.cases("a2a") if "rings" in c["cfg"] and c["size"] >= 127)
    n, B = c["n"], min(c["size"], 70001)
    rings = F.case_rings(c)
    inputs = a2a_ref.make_inputs(n, B, salt=c["seed"] % 7)
    recvs = [np.zeros(n * B, np.uint8) for _ in range(n)]
    nch, nthr = C.task_schema(n * B, len(rings))
    C.host_ring_all_to_all([x.copy() for x in inputs], recvs, B, channels=len(rings), nthreads=nthr,
                           buffer_size=F.buffer_size(c), rings=rings, force_relay=c["relay"])
    for r, want in enumerate(a2a_ref.expected(inputs, B)):
        assert recvs[r].tobytes() == want.tobytes(), (c, r)


# ---- part two's overrides ---------------------------------------------------------------------------------
def test_overrides_name_every_setting():
    kws = [kw for kw, _ in F.OVERRIDES.values()]
    envs = [env for _, env in F.OVERRIDES.values()]
    both = list(zip(kws, envs))
    assert any(kw.get("fifo_slots") == 8 and kw.get("lanes") == 3 for kw in kws)
    assert any(kw.get("fifo_slots") == 32 and kw.get("lanes") == 1 for kw in kws)
    assert any(kw.get("fifo_slots") == 8 and env.get("MCCS_SLICE_STEPS") == "2" for kw, env in both)
    assert any(kw.get("fifo_memory") == C.FIFO_DEVICE and kw.get("fifo_slots") == 8 for kw in kws)
    assert any(kw.get("locality") == C.LOCALITY_SENDER and env.get("MCCS_INLINE_WORKS") == "0" for kw, env in both)
    assert any("rings" in kw for kw in kws)
    for n in F.SEQ_NS:
        rings = F.permuted_rings(n)
        assert len(rings) == 2 and all(sorted(r) == list(range(n)) for r in rings)
        assert rings != C.default_rings(n, 2) and rings[0] != rings[1]


@pytest.mark.parametrize("name", list(F.OVERRIDES))
@pytest.mark.parametrize("n", F.SEQ_NS)
def test_sequences_keep_their_properties_under_every_override(n, name):
    """Among the rooted calls at least three distinct roots and two calls of
    more than one loop on the override's channels: a guard against an edit of
    S.CFG or of the overrides' buffer size."""
    cfg, env, rings = F.override(name, n)
    assert cfg["buffer_size"] == S.BUFF and all(cfg[k] == v for k, v in S.CFG.items())
    loop = len(rings) * (S.BUFF // 2)
    for seq in (S.sequence(S.SEED, n), A.sequence(n)):
        rooted = [c for c in seq if c["kind"] in ("bc", "rd")]
        assert len({c["root"] for c in rooted}) >= 3
        assert sum(c["count"] * vnode.ESIZE[c["code"]] > loop for c in rooted) >= 2
        for c in seq:
            want = "ring" if c["kind"] != "ard" else "oneshot" if cfg.get("fifo_memory") == C.FIFO_DEVICE else "ll"
            assert F.seq_algo(c, cfg) == want
