"""GPU, virtual node: mccsAllToAllv and mccsAllToAllvDev on counts that sit on
the edges of the byte cut (tests/a2av_ref.py boundary_matrices: granule,
channel, loop and slice edges; tests/test_all_to_all_v_boundary_cases.py
asserts on the CPU which situations they reach).

n = 2 (m = 4), 4 (m = 2) and 8 (m = 1).  Every matrix goes through both calls
on the same payload, the layouts cycling over packed, misaligned and
overlap_send: every byte of every 0xA5 frame compared, the send frames
unchanged, the two calls' receive frames equal.  Configurations: the default;
three lanes (the lane split of a slice has edges of its own on small slices);
at n = 4 two-step slices (MCCS_SLICE_STEPS=2) on 8 FIFO slots.  One
communicator set per (n, configuration).  buffer_size = 1 << 16 and an 8 s
watchdog.
"""
import pytest

import a2av_ref as V
import test_gpu_all_to_all_v as G
from test_gpu_all_to_all_v_dev import DStaged
import vnode

pytestmark = pytest.mark.gpu
DIRECT_DEFAULTS = True  # RING_ONLY is passed explicitly

KINDS = ("packed", "misaligned", "overlap_send")
M = {2: 4, 4: 2, 8: 1}
CONFIGS = [(n, name) for n in (2, 4, 8) for name in ("default", "lanes3")] + [(4, "slice2")]


@pytest.mark.parametrize("n,config", CONFIGS)
def test_boundary_matrices_on_both_calls(monkeypatch, n, config):
    import torch

    monkeypatch.delenv("MCCS_SLICE_STEPS", raising=False)
    cfg = {}
    if config == "lanes3":
        cfg = dict(lanes=3)
    elif config == "slice2":
        monkeypatch.setenv("MCCS_SLICE_STEPS", "2")
        cfg = dict(fifo_slots=8)
    comms = G._comms(n, monkeypatch, **cfg)
    try:
        assert comms[0].all_to_all_route() == {"hops": 1, "m": M[n]}
        assert all(c.lanes == cfg.get("lanes", c.lanes) for c in comms)
        mats = V.boundary_matrices(n, M[n], comms[0].rings())
        for i, cnt in enumerate(mats):
            kind = KINDS[i % len(KINDS)]
            host, dev = G.VStaged(n, cnt, kind, salt=i), DStaged(n, cnt, kind, salt=i)
            torch.cuda.synchronize()
            host.issue(comms)
            dev.issue(comms)
            torch.cuda.synchronize()
            for c in comms:
                c.sync()
            assert all(c.last_algo() == "ring" for c in comms)
            host.check(None, comms[0], (n, config, "matrix", i, kind, "AllToAllv"))
            dev.check(None, comms[0], (n, config, "matrix", i, kind, "AllToAllvDev"))
            for r in range(n):
                assert dev.recv[r].cpu().numpy().tobytes() == host.recv[r].cpu().numpy().tobytes(), (n, config, i, r)
    finally:
        vnode.destroy(comms)
