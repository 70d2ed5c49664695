"""GPU: AllToAllvDev under random engine configurations.

The draws of tests/test_gpu_all_to_all_v_fuzz.py v_case (rank count, lanes,
FIFO slots, two-step slicing, block size, sender-side placement, the cached
arena, the work FIFO switch, relabelled rings, layout) under seeds of its own,
with the off-diagonal counts redrawn from a2av_ref.values(m) and
a2av_ref.boundary_values(m), half from each.  The call differs from its
host-count sibling where the configuration matters: it is never an inline work,
its route word carries the successor and the predecessor the kernel indexes
the table by (relabelled rings change them), and every lane's workgroup
resolves its own copy of the element.

Each rank's table is a view that starts at an odd 64-bit word of a larger
tensor: 8-byte but not 16-byte aligned.  Every other word of that tensor holds
7, so a misread neighbour gives a small in-bounds size: wrong bytes or the
watchdog, never an access outside the frames.  After the call the table and
its neighbours are unchanged.  The case list is a pure function of the seeds;
tests/test_all_to_all_v_dev_fuzz_cases.py asserts on the CPU what it covers.
"""
import numpy as np
import pytest

import a2av_ref as V
import a2avd_ref as D
from mccs_amd import comm as C
import test_gpu_all_to_all_v as G
import test_gpu_all_to_all_v_fuzz as F
from test_gpu_all_to_all_v_dev import DStaged
import vnode

pytestmark = pytest.mark.gpu
DIRECT_DEFAULTS = True  # RING_ONLY is passed explicitly

SEED_BASE = 78400
NCASES = 24
NS = F.NS
NEIGHBOUR = 7  # what the words around a table hold
PAD = 2  # words of the larger tensor after the table; one word before it


def dev_case(seed):
    """F.v_case(seed) with its off-diagonal counts redrawn (a generator of their own, so the
    other draws stay v_case's): half from V.values(m), half from V.boundary_values(m)."""
    case = F.v_case(seed)
    n, m = case["n"], case["m"]
    rng = np.random.default_rng([seed, 1])
    old, new = V.values(m), V.boundary_values(m)
    for s in range(n):
        for t in range(n):
            if s != t:
                pool = old if rng.random() < 0.5 else new
                case["cnt"][s][t] = int(pool[int(rng.integers(0, len(pool)))])
    return case


def cases(count=NCASES):
    return [dev_case(SEED_BASE + k) for k in range(count)]


class OddTableStaged(DStaged):
    """DStaged whose tables sit at word 1 of tensors filled with NEIGHBOUR."""

    def __init__(self, n, cnt, kind, salt=0):
        import torch

        super().__init__(n, cnt, kind, salt)
        self.big = [torch.full((1 + 4 * n + PAD,), NEIGHBOUR, dtype=torch.int64, device="cuda") for _ in range(n)]
        for r in range(n):
            view = self.big[r][1:1 + 4 * n]
            view.copy_(self.tab[r])
            self.tab[r] = view
            assert view.is_contiguous() and view.data_ptr() % 16 == 8

    def check_tables(self, tag):
        for r in range(self.n):
            want = [NEIGHBOUR] + D.table(self.cnt, self.lay, r).astype(np.int64).tolist() + [NEIGHBOUR] * PAD
            assert self.big[r].cpu().tolist() == want, (tag, r, "the table or a neighbouring word changed")


@pytest.mark.parametrize("k", range(NCASES))
def test_random_all_to_all_v_dev_case(k, monkeypatch):
    import torch

    case = dev_case(SEED_BASE + k)
    for e in F.ENV:
        monkeypatch.delenv(e, raising=False)
    if case["slice2"]:
        monkeypatch.setenv("MCCS_SLICE_STEPS", "2")
    if case["fifo_works"]:
        monkeypatch.setenv("MCCS_INLINE_WORKS", "0")
    cfg, n = case["cfg"], case["n"]
    comms = G._comms(n, **cfg)
    try:
        assert comms[0].rings() == [list(r) for r in case["rings"]]
        assert comms[0].all_to_all_route() == {"hops": 1, "m": case["m"]}
        for c in comms:
            assert c.lanes == cfg.get("lanes", c.lanes) and c.block_threads == cfg.get("block_threads", c.block_threads)
            assert (c.fifo_memory == C.FIFO_DEVICE) == (cfg.get("fifo_memory") == C.FIFO_DEVICE)
        st = OddTableStaged(n, case["cnt"], case["layout"], salt=case["seed"] % 7)
        torch.cuda.synchronize()
        st.issue(comms)
        torch.cuda.synchronize()
        for c in comms:
            c.sync()
        st.check(None, comms[0], ("seed", case["seed"]))
        st.check_tables(("seed", case["seed"]))
        assert all(c.last_algo() == "ring" for c in comms)
    finally:
        vnode.destroy(comms)
