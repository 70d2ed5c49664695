"""CPU: what the seeded cases of tests/test_gpu_direct_collectives_fuzz.py
cover, that each plans as it says, and that each can fail.

The cases and sequences are pure functions of their seeds
(tests/direct_fuzz_cases.py).  Here, with no GPU:

  * the default part-one list meets the coverage list (REQUIRED), it is the
    smallest list from its seed base that does, and one case fewer leaves a
    named gap;
  * every default case, and every call of every default sequence, goes
    through the planner on the recording fake device runtime
    (tests/test_rooted_direct_plan.py): the recorded mode is the case's `algo`
    -- a case that would silently fall back to the ring never reaches the GPU
    --, and the record's workgroups, pieces, channels and threads are the
    model's (`geometry`, `select`), so the coverage entries derived from the
    model are the planner's.  Those are: "more pieces than workgroups" and
    "deal wraps at G=2 / 3 / 5", counted on the count-based bodies only, where
    MCCS_DIRECT_BLOCKS holds the launch to that G, a loop that deals has more
    pieces than G and one of its groups starts at base != 0 (the LL bodies are
    thread-linear: their analogue, more rounds of words than workgroups, is an
    entry of its own); one such wrap per loop that deals (ReduceScatter's two
    phases, Reduce's fold, Broadcast's copies); a workgroup on the wrapped
    branch that gets a piece; and the fold's early return from the walk;
  * every case can fail: its expected output differs from a zero buffer and
    from its inputs, and for fp32 Sum from four ranks on from the rank-order
    fold (but for a Reduce at n = 4 to root 3, where the two folds are one:
    direct_fuzz_cases.needs_order_control); a ReduceScatter and a Reduce of the
    default list carry that control;
  * the default sequences cover every call kind, every ordered adjacency of
    {rs-direct, rd-direct, bc-direct, other direct kernel, ring}, a root change
    between consecutive rooted calls and one slot parity reused by two
    functions.
"""
import ctypes

import pytest

import direct_fuzz_cases as K
import test_gpu_rooted_direct_sequences as RDS
import vnode
from mccs_amd import _lib
from mccs_amd import comm as C

ENV = ("MCCS_BC_DIRECT_BYTES", "MCCS_BC_LL_BYTES", "MCCS_RD_DIRECT_BYTES", "MCCS_RD_LL_BYTES", "MCCS_RS_DIRECT_BYTES",
       "MCCS_RS_LL_BYTES", "MCCS_A2A_LL_BYTES", "MCCS_A2AV_LL_BYTES", "MCCS_DIRECT_BLOCKS", "MCCS_DIRECT_WG_BYTES",
       "MCCS_ONESHOT_BYTES", "MCCS_DIRECT_BYTES", "MCCS_LL_BYTES")


# ---- coverage -------------------------------------------------------------------
def test_the_default_cases_meet_the_list_and_one_fewer_leave_a_gap():
    cases = K.default_cases(K.DEFAULT_CASES)
    assert K.gaps(cases) == set()
    gap = K.gaps(cases[:-1])
    assert gap, "the last default case adds nothing"
    print(f"{K.DEFAULT_CASES} cases from seed {K.SEED_BASE}; without the last one nothing covers {sorted(gap)}")
    for k in range(1, K.DEFAULT_CASES):  # no shorter list from this base
        assert K.gaps(cases[:k]), k


def test_the_list_is_what_the_issue_names():
    need = K.REQUIRED
    assert {f"{f}-{v}" for f in ("rs", "rd", "bc") for v in ("oneshot", "ll")} <= need
    assert {f"n{n}" for n in range(2, 9)} <= need
    assert {f"dtype{d}" for d in range(10)} | {f"op{o}" for o in range(4)} <= need
    assert {f"blocks-{b}" for b in (None, 1, 2, 3, 5)} <= need
    assert {"count 1", "cap-oneshot", "cap-ll", "three loops", "partial LL tail word", "in place", "send misaligned",
            "recv misaligned", "both misaligned", "permuted rings", "FIFO_DEVICE", "more pieces than workgroups",
            "root 0", "root n-1", "deal wraps at G=2", "deal wraps at G=3", "deal wraps at G=5",
            "early return of the walk"} <= need
    assert {f"{d} deal wraps" for d in ("rs phase 1", "rs phase 2", "rd phase 2", "bc phase 1")} <= need


def test_a_deal_wraps_only_on_a_count_based_launch_held_to_that_g():
    """The deal `j = bx >= base ? bx - base : bx + G - base` exists in the
    count-based bodies only: no LL case is credited with a wrap, a credited
    case has MCCS_DIRECT_BLOCKS == G in {2, 3, 5}, and the model of the deal
    agrees with dealing the pieces out one by one."""
    for case in K.default_cases(K.DEFAULT_CASES) + [K.case(s) for s in range(300)]:
        wraps = {f for f in K.case_features(case) if "wrap" in f}
        call = K.calls(case)[0]
        if case["variant"] == "ll":
            assert not wraps and K.deals(case, call) == {}, case["seed"]
        if any(f.startswith("deal wraps at G=") for f in wraps):
            g = K.geometry(case, call)[0]
            assert case["variant"] == "oneshot" and case["blocks"] == g and g in (2, 3, 5), case["seed"]
    for g, groups in ((2, [1, 1, 1]), (2, [2, 2]), (3, [4, 4, 4]), (5, [3, 3]), (5, [5, 5]), (3, [1, 3]), (1, [4, 2])):
        # piece p (numbered through the groups) belongs to workgroup p % G; the kernel's start for workgroup bx
        base, p, wraps, lands = 0, 0, False, False
        for np_ in groups:
            for bx in range(g):
                j = bx - base if bx >= base else bx + g - base
                assert [q for q in range(np_) if (p + q) % g == bx] == list(range(j, np_, g))
                if bx < base:
                    wraps, lands = True, lands or j < np_
            p += np_
            base = p % g
        assert K.deal_wraps(g, groups) == (wraps, lands), (g, groups)


def test_case_fields_stay_within_what_the_kernels_take():
    for case in K.default_cases(K.DEFAULT_CASES) + [K.case(s) for s in range(300)]:
        n, es = case["n"], K.ESIZE[case["code"]]
        cap = case["slots"][0 if case["variant"] == "oneshot" else 1]
        assert 2 <= n <= 8 and 0 <= case["root"] < n and 1 <= case["count"] and case["count"] * es <= cap
        assert case["soff"] % es == 0 and case["roff"] % es == 0 and 0 <= case["soff"] < 16 and 0 <= case["roff"] < 16
        assert 1 <= len(case["rings"]) <= 6 and all(sorted(r) == list(range(n)) for r in case["rings"])
        assert not (case["fifo_device"] and case["variant"] == "ll")
        for call in K.calls(case):
            assert K.nbytes_of(call) <= cap and call["algo"] == case["variant"]
        assert K.calls(case)[2]["kind"] != case["func"]


# ---- through the planner ----------------------------------------------------------
@pytest.fixture
def fake(monkeypatch):
    lib = _lib.load()
    monkeypatch.setenv("MCCS_TEST_HOOKS", "1")
    monkeypatch.setenv("MCCS_GATE", "0")
    for v in ENV:
        monkeypatch.delenv(v, raising=False)

    def install(ndev):
        assert lib.mccs_test_fake_runtime(ndev) == 0

    yield install
    lib.mccs_test_fake_runtime(0)


def _launches():
    lib = _lib.load()
    n = lib.mccs_test_fake_log(None, 0, 0)
    assert n >= 0, "fake runtime not installed"
    buf = ctypes.create_string_buffer(n + 1)
    lib.mccs_test_fake_log(buf, n + 1, 1)
    out = []
    for line in buf.value.decode().splitlines():
        kind, *kv = line.split()
        if kind == "launch":
            out.append(dict(x.split("=", 1) for x in kv))
    return out


def _fake_buffers(case, call):
    """Addresses the fake never touches, at the call's misalignments."""
    n = case["n"]
    send = [0x10000000 * (r + 1) + call["soff"] for r in range(n)]
    recv = [0x10000000 * (r + 1) + 0x8000000 + call["roff"] for r in range(n)]
    return K.pointers(case, call, send, recv)


def test_every_default_case_plans_as_its_algo_with_the_models_geometry(fake, monkeypatch):
    seen_g, seen_loops = 0, 0
    for case in K.default_cases(K.DEFAULT_CASES):
        if case["blocks"] is None:
            monkeypatch.delenv("MCCS_DIRECT_BLOCKS", raising=False)
        else:
            monkeypatch.setenv("MCCS_DIRECT_BLOCKS", str(case["blocks"]))
        fake(1)
        comms = C.init_all([0] * case["n"], C.CommConfig(**case["cfg"]))
        try:
            assert comms[0].rings() == case["rings"]
            assert (comms[0].fifo_memory == C.FIFO_DEVICE) == case["fifo_device"]
            K.opt_in(comms, case)
            _launches()
            for call in K.calls(case):
                send, recv = _fake_buffers(case, call)
                K.issue(comms, call, send, recv, stream=0)
                (kv,) = _launches()
                tag = (case["seed"], call["index"], kv)
                assert kv["kind"] == "direct" and kv["mode"] == f"{call['kind']}-{call['algo']}", tag
                assert [c.last_algo() for c in comms] == [call["algo"]] * case["n"], tag
                nch, nthr, _ = K.select(case, call)
                assert (int(kv["nch"]), int(kv["nthr"])) == (nch, nthr), tag
                g, piece, piece2, _ = K.geometry(case, call)
                assert (int(kv["gx"]), int(kv["piece"]), int(kv["piece2"])) == (g, piece, piece2), tag
                assert kv["grid"] == f"{g}x{case['n']}", tag
                if case["fifo_device"]:
                    assert kv["fence"] == "0", tag  # MCCS_FENCE_SYSTEM: the count-based body fences
                if call["kind"] != "rs":
                    assert kv["root"] == str(call["root"]), tag
                slots = [s.split(":") for s in kv["slots"].split("/")]
                assert [(int(s[1], 16), int(s[2], 16)) for s in slots] == list(zip(send, recv)), tag
                seen_g, seen_loops = max(seen_g, g), max(seen_loops, K.loops(case, call))
        finally:
            for c in comms:
                c.destroy()
    print(f"largest G {seen_g}, most loops of the walk {seen_loops}")
    assert seen_g >= 32 and seen_loops >= 3


ALL_RUNS = K.ONE_STREAM + K.TWO_STREAMS + K.GRAPH


@pytest.mark.parametrize("seed,n", ALL_RUNS)
def test_every_sequence_call_plans_as_its_algo(fake, seed, n):
    assert RDS.CFG == dict(buffer_size=K.SEQ_BUFF, oneshot_bytes=K.ONESHOT, ll_bytes=K.LL_BYTES, direct_bytes=K.TWOSHOT)
    assert RDS.ROOTED_LL == K.SMALL_LL
    fake(1)
    comms = C.init_all([0] * n, C.CommConfig(**RDS.CFG))
    try:
        for c in comms:
            RDS.opt_in(c)
        assert comms[0].all_to_all_ll_max() >= K.A2A_LL
        took = []
        for call in K.sequence(seed, n):
            es = 1 if call["kind"] in ("bc", "ag", "a2a") else vnode.ESIZE[call["code"]]
            mult = n if call["kind"] in ("rs", "a2a") else 1
            send = [0x10000000 * (r + 1) for r in range(n)]
            recv = [s + 0x8000000 for s in send]
            assert 0 < mult * call["count"] * es < 0x8000000
            if call["kind"] in ("rs", "rd", "bc"):
                one = dict(call, null_other=False)
                s, d = K.pointers(dict(n=n), one, send, recv)
                K.issue(comms, one, s, d, stream=0)
            else:
                with C.group():
                    for r, c in enumerate(comms):
                        if call["kind"] == "ar":
                            C.all_reduce(c, send[r], recv[r], call["count"], call["code"], call["op"], stream=0)
                        elif call["kind"] == "ag":
                            C.all_gather(c, send[r], recv[r], call["count"], stream=0)
                        else:
                            C.all_to_all(c, send[r], recv[r], call["count"], stream=0)
            took.append((call["name"], comms[0].last_algo()))
            assert [c.last_algo() for c in comms] == [call["algo"]] * n, (seed, n, call, took[-8:])
    finally:
        for c in comms:
            c.destroy()


# ---- every case can fail -------------------------------------------------------------
def test_every_default_case_can_fail(orc):
    salts = []
    for case in K.default_cases(K.DEFAULT_CASES):
        for call in K.calls(case):
            xs, exp, salt = K.call_payload(orc, case, call)  # raises when no salt gives one
            assert not K.can_fail_message(orc, case, call, xs, exp)
            salts.append(salt)
            if call["index"] == 0:  # the second run's payload is a fresh one
                ys = K.call_inputs(case, dict(call, index=1), salt)
                assert any(x is not None and x.tobytes() != y.tobytes() for x, y in zip(xs, ys))
    controls = sorted(c["func"] for c in K.default_cases(K.DEFAULT_CASES) if K.needs_order_control(c, K.calls(c)[0]))
    print(f"salts used: {sorted(set(salts))}; cases that carry the rank-order control: {controls}")
    assert {"rs", "rd"} <= set(controls)


# ---- sequences ---------------------------------------------------------------------
def test_the_default_sequences_cover_every_kind_adjacency_root_change_and_parity_reuse():
    assert K.sequence_gaps(ALL_RUNS) == set()
    assert len({(a, b) for a in K.CLASSES for b in K.CLASSES}) == 25
    assert sorted({n for _, n in K.ONE_STREAM}) == [2, 3, 4, 8]
    for seed, n in ALL_RUNS:
        seq = K.sequence(seed, n)
        assert len(seq) == K.SEQ_OPS + 1 and seq[-1]["name"] == "a2a-ring" and seq[-1]["algo"] == "ring"
        assert seq == K.sequence(seed, n)  # a pure function of (seed, n)
        for call in seq:
            es = 1 if call["kind"] in ("bc", "ag", "a2a") else vnode.ESIZE[call["code"]]
            assert K.predicted_algo(call["kind"], call["count"] * es) == call["algo"], call
            assert call["root"] is None or 0 <= call["root"] < n
        rooted = [c["root"] for c in seq if c["root"] is not None]
        assert len(set(rooted)) > 1 or n == 1
