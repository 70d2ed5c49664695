"""CPU: what the seeded Send/Recv groups of tests/test_gpu_send_recv_fuzz.py and
the chained groups of tests/test_gpu_send_recv_chained.py cover, that every
case can fail, that the host-thread ring completes every case with the expected
bytes, and that the planner queues every case's elements as the model of
tests/sr_ref.py pairs them (on the recording fake runtime).

The case list is a pure function of its seeds.  NCASES there is the smallest
count from SEED_BASE for which `coverage_gaps` below is empty:
test_ncases_is_the_smallest checks that one case fewer leaves a gap.
"""
import functools

import pytest

import a2a_ref
import a2av_ref as V
import sr_ref as SR
from mccs_amd import abi
from mccs_amd import comm as C
import test_gpu_send_recv_chained as H
import test_gpu_send_recv_fuzz as F
from test_all_to_all_v_plan import _log, fake  # noqa: F401  (the fixture)
from test_send_recv_plan import _addr, _elems, _launches
import vnode


@functools.lru_cache(maxsize=None)
def case(k):
    return SR.random_group(F.SEED_BASE + k)


def cases(count):
    return [case(k) for k in range(count)]


# ---- coverage ---------------------------------------------------------------------------------------
def group_facts(n, m, rings, ops) -> set:
    """Names of what one group reaches."""
    out = set()
    ranks = SR.ranks_of(ops)
    if len(ranks) < n:
        out.add("absent rank")
    for r in ranks:
        els = SR.elements(ops, r, rings)
        nworks = SR.works(ops, r, rings)
        idle = any(len(es) == 1 and es[0]["send"] is None and es[0]["recv"] is None for es in els)
        if len(set(nworks)) > 1:
            out.add("unequal works on a rank")
        if idle and max(nworks) > 1:
            out.add("idle beside chained")
        for es in els:
            if len(es) > 10:
                out.add("more than 10 elements")
            if len(es) > 20:
                out.add("more than 20 elements")
            for e in es[:-1]:
                if e["S"] > 0 and e["R"] == 0:
                    out.add("S only, not last")
                if e["S"] == 0 and e["R"] > 0:
                    out.add("R only, not last")
        peers = [o.peer for o in ops if o.rank == r]
        runs = 1 + sum(a != b for a, b in zip(peers, peers[1:]))
        if runs > len(set(peers)):
            out.add("issue order not grouped by peer")
    for q in SR.queues(ops).values():
        if any(ops[i].nbytes == 0 for i in q[1:-1]):
            out.add("zero bytes inside a queue")
    for ls, lr in SR.loop_cases(ops, rings, m):
        for name, hit in (("(0, >=2)", ls == 0 and lr >= 2), ("(>=2, 0)", ls >= 2 and lr == 0),
                          ("(1, 3)", (ls, lr) == (1, 3)), ("(3, 1)", (ls, lr) == (3, 1)),
                          ("(3, 3)", (ls, lr) == (3, 3))):
            if hit:
                out.add("loops " + name)
    return out


GROUP_FACTS = {"absent rank", "unequal works on a rank", "idle beside chained", "more than 10 elements",
               "more than 20 elements", "S only, not last", "R only, not last", "issue order not grouped by peer",
               "zero bytes inside a queue", "loops (0, >=2)", "loops (>=2, 0)", "loops (1, 3)", "loops (3, 1)",
               "loops (3, 3)"}


def coverage_gaps(cs) -> list:
    """What the list still lacks: names of the requirements not met."""
    gaps = []

    def need(ok, name):
        if not ok:
            gaps.append(name)

    need({c["n"] for c in cs} == set(F.NS), "every n")
    for key, vals in (("lanes", {None, 1, 2, 3}), ("fifo_slots", {None, 8, 16, 32}),
                      ("block_threads", {None, 128, 256, 544, 576}), ("fifo_memory", {None, C.FIFO_DEVICE}),
                      ("locality", {None, C.LOCALITY_SENDER})):
        need({c["cfg"].get(key) for c in cs} == vals, key)
    for key in ("slice2", "fifo_works", "relabelled"):
        need({c[key] for c in cs} == {False, True}, key)
    need(any(c["relabelled"] and c["rings"] != C.default_rings(c["n"]) for c in cs), "rings that differ")
    seen = set()
    for c in cs:
        seen |= group_facts(c["n"], c["m"], c["rings"], c["ops"])
    gaps += sorted(GROUP_FACTS - seen)
    live = [o for c in cs for o in c["ops"] if o.nbytes]
    for kind in ("send", "recv"):
        need({o.off for o in live if o.kind == kind} == set(range(16)), f"every offset on a {kind}")
    need(any(set(V.boundary_values(m)) <= {o.nbytes for c in cs if c["m"] == m for o in c["ops"]} for m in (1, 2, 4)),
         "every boundary value of one m")
    need(len({o.code for o in live}) >= 6, "six element types")
    return gaps


def test_the_case_list_covers_what_it_claims():
    cs = cases(F.NCASES)
    assert SR.random_group(F.SEED_BASE) == cs[0] == F.cases(1)[0]  # a pure function of the seed
    assert not coverage_gaps(cs)


def test_ncases_is_the_smallest():
    """One case fewer leaves a gap.  Every requirement is "some case has it",
    which a shorter list meets no better: so no smaller count is free of gaps."""
    assert coverage_gaps(cases(F.NCASES - 1))


def test_every_group_is_legal_and_within_its_caps():
    assert SR.ESIZE == tuple(vnode.ESIZE[k] for k in range(10)) and SR.MAX_WORK_ELEMENTS == abi.MCCS_MAX_WORK_ELEMENTS
    for c in cases(F.NCASES):
        n, m, ops = c["n"], c["m"], c["ops"]
        route = a2a_ref.route(n, c["rings"])
        assert route["hops"] == 1 and route["m"] == m, c["seed"]  # relabelling keeps the one-hop route
        SR.matches(ops)  # every send has its receive, of its size
        assert all(o.peer != o.rank and 0 <= o.peer < n and 0 <= o.rank < n and 0 <= o.off < 16 for o in ops)
        assert all(o.nbytes % SR.ESIZE[o.code] == 0 and o.nbytes in SR.sizes(m) for o in ops)
        assert len(ops) <= SR.MAX_OPS and any(o.nbytes for o in ops)
        assert sum(o.nbytes for o in ops if o.kind == "send") <= SR.MAX_SENT
        if c["heavy"]:
            q = SR.queues(ops)[(c["heavy"][0], "send", c["heavy"][1])]
            assert len(q) in SR.HEAVY and all(ops[i].nbytes <= V.loop_bytes(m) for i in q)
        for si, ri in SR.matches(ops):
            assert ops[si].code == ops[ri].code


def test_the_chained_groups_are_what_they_claim():
    for n in (2, 4):
        rings = C.default_rings(n)
        m = a2a_ref.route(n, rings)["m"]
        ops = SR.chained(n, m)
        SR.matches(ops)
        Cb = V.loop_bytes(m)
        q = SR.queues(ops)
        if n == 2:  # every channel joins the pair: three works one way, two the other
            assert len(q[(0, "send", 1)]) == 23 and len(q[(1, "send", 0)]) == 12 and m == len(rings)
            assert SR.works(ops, 0, rings) == SR.works(ops, 1, rings) == [3] * len(rings)
            for r, (ks, kr) in ((0, (23, 12)), (1, (12, 23))):
                for es in SR.elements(ops, r, rings):
                    assert sum(e["send"] is not None for e in es) == ks and sum(e["recv"] is not None for e in es) == kr
        else:  # rank 0: chained channels beside idle ones; rank 1: its send after its 12 receives, in element 0
            assert sorted(SR.works(ops, 0, rings)) == [1] * (len(rings) - m) + [2] * m
            idle = [es for es in SR.elements(ops, 0, rings) if es[0]["send"] is None and es[0]["recv"] is None]
            assert len(idle) == len(rings) - m and all(len(es) == 1 for es in idle)
            assert [o.kind for o in ops if o.rank == 1] == ["recv"] * 12 + ["send"]
            both = [es for es in SR.elements(ops, 1, rings) if es[0]["S"] and es[0]["recv"] is not None]
            assert both and all(len(es) == 12 for es in both)
            assert 3 * Cb in {o.nbytes for o in ops if o.rank == 2}
        for key in ((0, "send", 1), (1, "send", 0)) if n == 2 else ((0, "send", 1),):
            sz = [ops[i].nbytes for i in q[key]]
            assert [j for j, v in enumerate(sz) if v == 0] == [0, 9, 10, len(sz) - 1]
            assert sz[len(sz) // 2] == 2 * Cb + 999 and max(sz[:len(sz) // 2] + sz[len(sz) // 2 + 1:]) <= Cb
            assert set(sz) - {0, 2 * Cb + 999} <= set(V.boundary_values(m)) and len(set(sz)) >= 7
        assert "idle beside chained" in group_facts(n, m, rings, ops) or n == 2


# ---- every case can fail ------------------------------------------------------------------------------
def _can_fail(ops, tag):
    """Shifting one message by a byte changes the expected bytes, and any two
    messages differ at every byte, so swapping two of one pair does too."""
    sent = SR.payloads(ops)
    live = [i for i in sent if ops[i].nbytes > 0]
    assert live, tag
    want = SR.expected(ops, sent)
    for i in live:
        shifted = dict(sent)
        shifted[i] = V.make_send(0, ops[i].nbytes + 1, salt=1 + i)[1:]
        got = SR.expected(ops, shifted)
        assert any((got[k] != want[k]).any() for k in want), (tag, i)
    for x, i in enumerate(live):
        for j in live[x + 1:]:
            k = min(ops[i].nbytes, ops[j].nbytes)
            assert (sent[i][:k] != sent[j][:k]).all(), (tag, i, j)


@pytest.mark.parametrize("k", range(F.NCASES))
def test_every_case_can_fail(k):
    _can_fail(case(k)["ops"], case(k)["seed"])


def test_the_chained_groups_can_fail():
    for n, m in ((2, 4), (4, 2)):
        _can_fail(SR.chained(n, m), n)


# ---- the host-thread ring ---------------------------------------------------------------------------------
def _host_ring(n, ops, rings):
    bufs = SR.frames(ops)
    hops = [(o.rank, o.kind, o.peer, a.ctypes.data + sl.start, o.nbytes) for o, (a, sl) in zip(ops, bufs)]
    C.host_ring_send_recv(n, hops, len(rings), 544, SR.BUFF, rings)
    SR.check(ops, bufs)


@pytest.mark.parametrize("k", range(F.NCASES))
def test_the_host_ring_completes_every_case(k):
    c = case(k)
    _host_ring(c["n"], c["ops"], c["rings"])


@pytest.mark.parametrize("n", [2, 4])
def test_the_host_ring_completes_the_chained_groups(n):
    rings = C.default_rings(n)
    _host_ring(n, SR.chained(n, a2a_ref.route(n, rings)["m"]), rings)


# ---- the planner, on the fake runtime ---------------------------------------------------------------------
def _planned(monkeypatch, n, ops, cfg, slice2, fifo_works, tag):
    """Issues the group with typed calls; the launch's elements equal the model."""
    F.set_env(monkeypatch, slice2, fifo_works)
    comms = C.init_all([0] * n, C.CommConfig(buffer_size=SR.BUFF, **cfg))
    try:
        _log()
        rings = comms[0].rings()
        assert comms[0].all_to_all_route()["hops"] == 1
        addr = lambda i: _addr(i, ops[i].off)
        with C.group():
            for i, o in enumerate(ops):
                (C.send if o.kind == "send" else C.recv)(comms[o.rank], addr(i), o.nbytes // SR.ESIZE[o.code], o.code,
                                                         o.peer, stream=0)
        launches = _launches()
        assert len(launches) == 1 and launches[0]["kind"] == "ring", (tag, launches)
        ranks = SR.ranks_of(ops)
        gx, gy = (int(v) for v in launches[0]["grid"].split("x"))
        assert gy == len(ranks) and gx == comms[0].nchannels * comms[0].lanes, tag
        got = _elems(launches[0])
        for slot, r in enumerate(ranks):
            assert got[slot] == SR.work_elements(ops, r, rings, addr), (tag, r)
        single = all(len(ch) == 1 for slot in got for ch in slot)
        inline = launches[0]["inline_works"] != "0"
        assert inline == (single and not fifo_works and len(ranks) * len(rings) <= 8), tag
        assert all(comms[r].last_algo() == "ring" for r in ranks)
        return rings
    finally:
        for c in comms:
            c.destroy()


@pytest.mark.parametrize("k", range(F.NCASES))
def test_queued_elements_equal_the_model_on_every_case(fake, monkeypatch, k):  # noqa: F811
    fake(1)
    c = case(k)
    rings = _planned(monkeypatch, c["n"], c["ops"], c["cfg"], c["slice2"], c["fifo_works"], c["seed"])
    assert rings == [list(r) for r in c["rings"]]


@pytest.mark.parametrize("name", list(H.CONFIGS))
@pytest.mark.parametrize("n", [2, 4])
def test_queued_elements_equal_the_model_on_the_chained_groups(fake, monkeypatch, n, name):  # noqa: F811
    fake(1)
    cfg, slice2 = H.CONFIGS[name]
    m = a2a_ref.route(n, C.default_rings(n))["m"]
    _planned(monkeypatch, n, SR.chained(n, m), cfg, slice2, False, (n, name))
