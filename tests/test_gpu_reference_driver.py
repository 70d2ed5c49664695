"""GPU: the reference-named kernels driven the way the reference host drives them.

The Rust service builds every device structure itself and calls the kernel
through collectives-sys; tests/refdrv_worker.py restates
that host side (comm/device.rs, the SHM connector's SendBufMeta/RecvBufMeta
layout, plan.rs work upload and launch_plan) with no communicator of this
library involved, and launches through mccs_hip_launch_coll with the
reference's grid (#channels) and 544-thread blocks.  One rank per process on
the one-GPU box (kernels of one process on one GPU need not run concurrently;
the reference gives each rank its own GPU), FIFO memory shared over IPC.
Results are bit-exact against the oracle, three launches in a row on the same
structures (conn->step persistence), with workFifoDone = doneAcks.

test_reference_driven_modes runs the worker's further modes: the AllGather
kernel, batched plans (several tasks per launch, chained works, a negative
workNext), buckets smaller than the ring, misaligned guarded buffers, edge
values, and the sixteen PreMulSum / SumPostDiv kernels with the scalar in each
work element's redOpArg.  Each asserts that the path it is for was reached.
"""
import json
import os
import socket
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def _free_port() -> int:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _run_worker(world, **extra):
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.join(HERE, "refdrv_worker.py")]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", **extra)
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env, cwd=os.path.dirname(HERE))
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert r.returncode == 0 and lines, r.stdout[-3000:] + r.stderr[-3000:]
    return json.loads(lines[-1])


@pytest.mark.parametrize("world,big", [(2, False), (3, False), (3, True)], ids=["2", "3", "3-configs2-bucket"])
def test_reference_driven_launch_matches_oracle(world, big):
    """big: configs[2]'s 128 MiB fp32 bucket, random inputs, 2 and 32
    channels (grid = channels, 544 threads), bit-exact at n = 3 where the
    ring order matters (a rank-order sum differs: checked)."""
    res = _run_worker(world, REFDRV_BIG="1" if big else "0")
    assert res["all_ok"], res
    assert res["world"] == world


VARIANTS = ("ref_sender", "override_receiver")
# what each mode is for: the worker reports it as reached only if it saw it
# on every rank (tests/refdrv_worker.py Modes)
REACHES = {
    # func 2 went to mccs_hip_launch_coll for every AllGather, in place and on two channels too
    "allgather": ["allgather_symbol_launched"],
    # a second chained work in a 544-thread block with 96-thread elements, selections
    # that are not 0..k-1, ten elements per work, a negative workNext uploaded, and
    # (oracle alone) a channel order that decides the values under the override
    "batched": [f"{v}/{what}" for v in VARIANTS for what in
                ("chained_work_mixed_block", "selection_not_identity", "ten_elements_per_work", "negative_workNext")]
    + ["override_order_decides_values"],
    "small": ["nthr_96_160_288_544"],
    # the guarded control saw exactly the extra element's bytes
    "odd": [f"{v}/control_reports_extra_bytes/dtype{code}" for v in VARIANTS for code in (6, 7)],
    "edge": ["all_40_kernels"],
    # every PreMulSum / SumPostDiv symbol went to mccs_hip_launch_coll on every rank, each
    # block size too, and one plan uploaded two scalars in one work and one in a chained work
    "avg": ["all_16_avg_kernels", "avg_nthr_96_160_288_544", "two_scalars_in_one_work", "scalar_in_chained_work"],
}
# n = 3 only: with the scalar 1/3 a fused multiply-add would show (at n = 2 every product is exact)
REACHES_AT = {("avg", 3): ["rounding_fp16_bf16_fp32_fp64"]}


@pytest.mark.parametrize("mode,world", [("allgather", 2), ("allgather", 3), ("allgather", 4), ("batched", 3),
                                        ("batched", 4), ("small", 3), ("odd", 3), ("edge", 2), ("avg", 2),
                                        ("avg", 3)])
def test_reference_driven_modes(mode, world):
    """The rest of plan.rs's host side on the reference-named kernels: the
    AllGather kernel, batched plans with chained works, buckets smaller than
    the ring, misaligned guarded buffers and edge values; "avg": the sixteen
    PreMulSum / SumPostDiv kernels against tests/avg_ref.py (the cases are
    tests/refdrv_avg_cases.py's).  Exact comparisons only; one worker launch
    per case."""
    res = _run_worker(world, REFDRV_MODE=mode)
    assert res["all_ok"], {k: v for k, v in res.items() if k != "cases"} | {
        "failed": [k for k, ok in res["cases"].items() if not ok][:20]}
    assert res["world"] == world and res["mode"] == mode and res["launches"] > 0
    keys = REACHES[mode] + REACHES_AT.get((mode, world), [])
    for key in keys:
        assert res["reached"].get(key) is True, (key, res["reached"])
    if mode == "avg":
        # per variant 32 edge launches, 4 rounding ones at n = 3, 16 bucket ones, 2 plans,
        # 4 misaligned launches and the sequence's 6: every one of them was checked
        assert len(res["cases"]) == 2 * (60 + (4 if world == 3 else 0)) + len(keys), len(res["cases"])
