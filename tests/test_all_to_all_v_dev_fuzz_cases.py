"""CPU: what the seeded AllToAllvDev sweep of
tests/test_gpu_all_to_all_v_dev_fuzz.py covers, the route words its relabelled
cases need from the planner, and that the host-thread ring that resolves the
tables gives every case's expected bytes."""
import a2a_ref
import a2av_ref as V
import a2avd_ref as D
from mccs_amd import comm as C
import test_gpu_all_to_all_v_dev_fuzz as F
import test_gpu_all_to_all_v_fuzz as H


def test_the_sweep_covers_the_engine_overrides_the_cursor_cases_and_the_boundary_values():
    cs = F.cases()
    assert len(cs) == 24 and F.SEED_BASE != H.SEED_BASE
    assert not set(range(F.SEED_BASE, F.SEED_BASE + 24)) & set(range(H.SEED_BASE, H.SEED_BASE + 24))
    assert {c["n"] for c in cs} == set(F.NS)
    assert {c["cfg"].get("lanes") for c in cs} >= {None, 1, 2, 3}
    assert {c["cfg"].get("fifo_slots") for c in cs} >= {None, 8, 16, 32}
    assert len({c["cfg"].get("block_threads") for c in cs}) >= 3
    for key, val in (("fifo_memory", C.FIFO_DEVICE), ("locality", C.LOCALITY_SENDER)):
        hit = [c for c in cs if c["cfg"].get(key) == val]
        assert 2 <= len(hit) < len(cs), key
    for key in ("slice2", "fifo_works", "relabelled"):
        assert 2 <= sum(c[key] for c in cs) < len(cs), key
    assert {c["layout"] for c in cs} == set(V.LAYOUTS)
    seen, boundary = set(), set()
    for c in cs:
        n, m = c["n"], c["m"]
        route = a2a_ref.route(n, c["rings"])
        assert route["hops"] == 1 and route["m"] == m, c["seed"]  # relabelling keeps the one-hop route
        seen |= V.loop_cases(c["cnt"], c["rings"], m)
        pool = set(V.values(m)) | set(V.boundary_values(m))
        off = {c["cnt"][s][t] for s in range(n) for t in range(n) if s != t}
        assert off <= pool, c["seed"]
        # which boundary value it is, by its place in the list (the values scale with m)
        boundary |= {V.boundary_values(m).index(v) for v in off if v not in V.values(m)}
        lay = V.layout(c["cnt"], c["layout"])
        assert max(lay["send_len"] + lay["recv_len"]) < 1 << 20, c["seed"]
    assert {(3, 0), (0, 3), (1, 3), (1, 1), (3, 3), (2, 0), (0, 2)} <= seen, seen
    assert len(boundary) >= 10, boundary
    assert any(c["relabelled"] and c["rings"] != C.default_rings(c["n"]) for c in cs)


def test_a_relabelled_case_needs_other_successors_and_predecessors_in_the_route_word():
    """The kernel indexes the table by the successor and the predecessor of the
    route word: on some (rank, channel) of every relabelled case with other
    rings they are not the default rings'."""
    hit = 0
    for c in F.cases():
        n, default = c["n"], C.default_rings(c["n"])
        if not c["relabelled"] or c["rings"] == default:
            continue
        differ = 0
        for r in range(n):
            mine = [e for e in D.want_elements(n, c["rings"], r, 0x1000, 0x2000, 0x3000) if e["hops"] == 1]
            base = [e for e in D.want_elements(n, default, r, 0x1000, 0x2000, 0x3000) if e["hops"] == 1]
            assert len(mine) == len(base) == len(default)
            for e in mine:
                assert e["part"] != r and e["parts"] != r and e["count"] == 0x3000 and e["nch"] == c["m"]
            differ += sum((a["part"], a["parts"]) != (b["part"], b["parts"]) for a, b in zip(mine, base))
        assert differ > 0, c["seed"]
        hit += 1
    assert hit >= 2


def test_the_host_ring_that_reads_tables_agrees_on_every_case():
    for c in F.cases():
        n, cnt = c["n"], c["cnt"]
        lay = V.layout(cnt, c["layout"])
        sends = [V.make_send(s, lay["send_len"][s], c["seed"] % 7) for s in range(n)]
        rf = [V.frame(lay["recv_len"][r]) for r in range(n)]
        C.host_ring_all_to_all_v_tables([s.ctypes.data for s in sends], [a.ctypes.data + sl.start for a, sl in rf],
                                        D.tables(cnt, lay), len(c["rings"]), 544, V.BUFF, c["rings"])
        for r, w in enumerate(V.expected(sends, cnt, lay)):
            a, sl = rf[r]
            assert (a[sl] == w).all() and (a[:sl.start] == V.SENTINEL).all() and (a[sl.stop:] == V.SENTINEL).all(), \
                (c["seed"], r)
