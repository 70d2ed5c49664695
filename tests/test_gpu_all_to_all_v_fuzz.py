"""GPU: AllToAllv under random engine configurations.

Per seed: a rank count with a one-hop default ring set, lanes, 8 / 16 / 32 FIFO
slots, two-step slicing, block size, sender-side placement, the cached arena,
the work list through the work FIFO, the default rings relabelled by a random
permutation of the ranks (which keeps every arc count, so the route stays one
hop), a random count matrix over the value set of tests/a2av_ref.py and a
layout.  One grouped call on a virtual node, every byte of every frame compared.
The case list is a pure function of the seeds;
tests/test_all_to_all_v_fuzz_cases.py asserts on the CPU what it covers.
"""
import numpy as np
import pytest

import a2a_ref
import a2av_ref as V
from mccs_amd import comm as C
import test_gpu_all_to_all_v as G
import vnode

pytestmark = pytest.mark.gpu
DIRECT_DEFAULTS = True  # RING_ONLY is passed explicitly

SEED_BASE = 51200
NCASES = 24
NS = (2, 3, 4, 5, 7, 8)
ENV = ("MCCS_SLICE_STEPS", "MCCS_INLINE_WORKS", "MCCS_ALLTOALL_HOPS")


def engine_case(rng):
    """The engine draws of one case from rng: n, cfg (CommConfig keywords),
    slice2, fifo_works, relabelled, rings, m.  (tests/sr_ref.random_group
    takes the same draws.)"""
    n = int(rng.choice(NS))
    cfg = {}
    if rng.random() < 0.5:
        cfg["lanes"] = int(rng.choice([1, 2, 3]))
    if rng.random() < 0.6:
        cfg["fifo_slots"] = int(rng.choice([8, 16, 32]))
    if rng.random() < 0.3:
        cfg["block_threads"] = int(rng.choice([128, 256, 544, 576]))
    if rng.random() < 0.3:
        cfg["fifo_memory"] = C.FIFO_DEVICE
    if rng.random() < 0.3:
        cfg["locality"] = C.LOCALITY_SENDER
    slice2 = bool(rng.random() < 0.3)
    fifo_works = bool(rng.random() < 0.3)
    rings = C.default_rings(n)
    relabelled = bool(rng.random() < 0.4)
    if relabelled:
        pi = [int(v) for v in rng.permutation(n)]
        rings = [[pi[x] for x in ring] for ring in rings]
        cfg["rings"] = rings
        cfg["channel_count"] = len(rings)
    m = a2a_ref.route(n, rings)["m"]
    return dict(n=n, cfg=cfg, slice2=slice2, fifo_works=fifo_works, relabelled=relabelled, rings=rings, m=m)


def v_case(seed):
    """A dict: the keys of engine_case, then cnt (the matrix) and layout."""
    rng = np.random.default_rng(seed)
    e = engine_case(rng)
    n, m = e["n"], e["m"]
    vals = V.values(m)
    cnt = [[int(vals[int(rng.integers(0, len(vals)))]) for _ in range(n)] for _ in range(n)]
    for r in range(n):
        cnt[r][r] = int(rng.choice([0, 1, 15, 4099, V.loop_bytes(m) + 1]))
    layout = V.LAYOUTS[int(rng.integers(0, len(V.LAYOUTS)))]
    return dict(seed=seed, **e, cnt=cnt, layout=layout)


def cases(count=NCASES):
    return [v_case(SEED_BASE + k) for k in range(count)]


@pytest.mark.parametrize("k", range(NCASES))
def test_random_all_to_all_v_case(k, monkeypatch):
    case = v_case(SEED_BASE + k)
    for e in ENV:
        monkeypatch.delenv(e, raising=False)
    if case["slice2"]:
        monkeypatch.setenv("MCCS_SLICE_STEPS", "2")
    if case["fifo_works"]:
        monkeypatch.setenv("MCCS_INLINE_WORKS", "0")
    cfg = case["cfg"]
    comms = G._comms(case["n"], **cfg)
    try:
        assert comms[0].rings() == [list(r) for r in case["rings"]]
        assert comms[0].all_to_all_route() == {"hops": 1, "m": case["m"]}
        for c in comms:
            assert c.lanes == cfg.get("lanes", c.lanes) and c.block_threads == cfg.get("block_threads", c.block_threads)
            assert (c.fifo_memory == C.FIFO_DEVICE) == (cfg.get("fifo_memory") == C.FIFO_DEVICE)
        G.run(comms, case["cnt"], case["layout"], salt=case["seed"] % 7, tag=case["seed"])
        assert all(c.last_algo() == "ring" for c in comms)
    finally:
        vnode.destroy(comms)
