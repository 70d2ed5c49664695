"""GPU: Send/Recv groups drawn from a seed, under random engine configurations.

Per seed (tests/sr_ref.random_group): the engine draws of the AllToAllv fuzz
(rank count, lanes, 8 / 16 / 32 FIFO slots, two-step slicing, block size,
sender-side placement, the cached arena, the work list through the work FIFO,
relabelled rings), then a group: 0-3 messages on every ordered pair, sometimes a
pair with 11-23 (two or three works on its channels), sometimes an absent
rank, sizes from the value set and the cut edges, zero-byte messages anywhere,
buffers 0-15 bytes off alignment, typed counts, and each rank's calls in a
random interleaving of its per-(peer, direction) queues.

Each case runs the group twice on one communicator set (other payloads the
second time), every byte of every frame compared, and then one uniform
AllToAll over all ranks, absent ones included: a group advances each connection
by its own pair's loops alone, the uniform call uses every connection, so it
fails if the group left any end out of step.  All under the 8 s watchdog.
The case list is a pure function of the seeds;
tests/test_send_recv_fuzz_cases.py asserts on the CPU what it covers.
"""
import pytest

import a2a_ref
import sr_ref as SR
from mccs_amd import comm as C
import test_gpu_all_to_all_v as G
import test_gpu_all_to_all_v_fuzz as F
import test_gpu_send_recv as P
import vnode

pytestmark = pytest.mark.gpu
DIRECT_DEFAULTS = True  # RING_ONLY is passed explicitly

SEED_BASE = 64800
NCASES = 26  # tests/test_send_recv_fuzz_cases.py: the smallest count from SEED_BASE that meets the coverage list
NS = F.NS
STEP_BYTES = 4099


def cases(count=NCASES):
    return [SR.random_group(SEED_BASE + k) for k in range(count)]


def set_env(monkeypatch, slice2, fifo_works):
    for e in F.ENV:
        monkeypatch.delenv(e, raising=False)
    if slice2:
        monkeypatch.setenv("MCCS_SLICE_STEPS", "2")
    if fifo_works:
        monkeypatch.setenv("MCCS_INLINE_WORKS", "0")


def run_staged(comms, st, tag):
    import torch

    torch.cuda.synchronize()
    st.issue(comms)
    torch.cuda.synchronize()
    for c in comms:
        c.sync()
    st.check(None, comms[0], tag)
    assert all(comms[r].last_algo() == "ring" for r in SR.ranks_of(st.ops)), tag


def step_check(comms, tag):
    """One uniform AllToAll of STEP_BYTES over every rank of the set."""
    import torch

    n = len(comms)
    inputs = a2a_ref.make_inputs(n, STEP_BYTES, salt=n)
    send = [vnode.to_dev(x) for x in inputs]
    recv = [torch.zeros(n * STEP_BYTES, dtype=torch.uint8, device="cuda") for _ in range(n)]
    torch.cuda.synchronize()
    with C.group():
        for r in range(n):
            C.all_to_all(comms[r], send[r], recv[r], STEP_BYTES)
    torch.cuda.synchronize()
    for c in comms:
        c.sync()
    for r, w in enumerate(a2a_ref.expected(inputs, STEP_BYTES)):
        assert recv[r].cpu().numpy().tobytes() == w.tobytes(), (tag, "the uniform call after the group", r)


@pytest.mark.parametrize("k", range(NCASES))
def test_random_send_recv_group(k, monkeypatch):
    case = SR.random_group(SEED_BASE + k)
    set_env(monkeypatch, case["slice2"], case["fifo_works"])
    cfg, n, tag = case["cfg"], case["n"], ("seed", case["seed"])
    comms = G._comms(n, **cfg)
    try:
        assert comms[0].rings() == [list(r) for r in case["rings"]]
        assert comms[0].all_to_all_route() == {"hops": 1, "m": case["m"]}
        for c in comms:
            assert c.lanes == cfg.get("lanes", c.lanes) and c.block_threads == cfg.get("block_threads", c.block_threads)
            assert (c.fifo_memory == C.FIFO_DEVICE) == (cfg.get("fifo_memory") == C.FIFO_DEVICE)
        st = P.SRStaged(n, case["ops"], salt=case["seed"] % 7)
        run_staged(comms, st, tag + ("first run",))
        st.refill(100 + case["seed"] % 11)
        run_staged(comms, st, tag + ("second run",))
        step_check(comms, tag)
    finally:
        vnode.destroy(comms)
