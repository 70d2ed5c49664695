"""CPU: what the seeded AllToAllv sweep of tests/test_gpu_all_to_all_v_fuzz.py
covers, and that the host-thread ring gives every case's expected bytes."""
import numpy as np

import a2a_ref
import a2av_ref as V
from mccs_amd import comm as C
import test_gpu_all_to_all_v_fuzz as F


def test_the_sweep_covers_the_engine_overrides_and_the_cursor_cases():
    cs = F.cases()
    assert len(cs) == 24
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
    seen, vals_ix = set(), set()
    for c in cs:
        route = a2a_ref.route(c["n"], c["rings"])
        assert route["hops"] == 1 and route["m"] == c["m"], c["seed"]  # relabelling keeps the one-hop route
        seen |= V.loop_cases(c["cnt"], c["rings"], c["m"])
        vals = V.values(c["m"])
        vals_ix |= {vals.index(c["cnt"][s][t]) for s in range(c["n"]) for t in range(c["n"]) if s != t}
    assert {(3, 0), (0, 3), (1, 3), (1, 1), (3, 3), (2, 0), (0, 2)} <= seen, seen
    assert vals_ix == set(range(8))
    assert any(c["relabelled"] and c["rings"] != C.default_rings(c["n"]) for c in cs)


def test_the_host_ring_agrees_on_every_case():
    for c in F.cases():
        n, cnt = c["n"], c["cnt"]
        lay = V.layout(cnt, c["layout"])
        sends = [V.make_send(s, lay["send_len"][s], c["seed"] % 7) for s in range(n)]
        rf = [V.frame(lay["recv_len"][r]) for r in range(n)]
        C.host_ring_all_to_all_v([s.ctypes.data for s in sends], [a.ctypes.data + sl.start for a, sl in rf], cnt,
                                 lay["sdispls"], lay["rdispls"], len(c["rings"]), 544, V.BUFF, c["rings"])
        for r, w in enumerate(V.expected(sends, cnt, lay)):
            a, sl = rf[r]
            assert (a[sl] == w).all() and (a[:sl.start] == V.SENTINEL).all() and (a[sl.stop:] == V.SENTINEL).all()
