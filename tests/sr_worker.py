#!/usr/bin/env python3
"""One rank per process: the sequence of tests/test_gpu_send_recv_sequences.py
(Send/Recv groups between Broadcasts, ring AllReduces, an AllToAllv and an
AllToAllvDev) through IPC-mapped FIFO arenas.

  python -m torch.distributed.run --nproc-per-node 2 --master-addr 127.0.0.1 \
      --master-port 29515 tests/sr_worker.py

Driven by tests/test_gpu_send_recv_sequences.py (a worker, not a test module).
Each process groups only its own sends and receives of a pattern; after the
sequence rank 0 sends 3C bytes to rank 1 with an ungrouped call that an
ungrouped receive matches (the FIFO holds two of its three loops, so the send
ends only once the receive runs).  Every rank issues everything without a sync
in between, syncs once and checks its own buffers byte for byte; rank 0 prints
the merged verdicts.
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import torch
    import torch.distributed as dist

    from mccs_amd import comm as C
    from oracle import oracle as orc
    import a2av_ref as V
    import sr_ref as SR
    import test_gpu_all_to_all_v as G
    import test_gpu_rooted_sequences as S
    import test_gpu_send_recv as P
    import test_gpu_send_recv_sequences as Q

    rank = int(os.environ["RANK"])
    world = int(os.environ["WORLD_SIZE"])
    dev = int(os.environ.get("LOCAL_RANK", rank)) % torch.cuda.device_count()
    torch.cuda.set_device(dev)
    dist.init_process_group("gloo", rank=rank, world_size=world)

    def exchange(b):
        out = [None] * world
        dist.all_gather_object(out, b)
        return out

    comm = C.init_communicator_rank(rank, world, dev, exchange,
                                    C.CommConfig(timeout_ms=G.TIMEOUT_MS, buffer_size=V.BUFF, **G.RING_ONLY))
    rings, m = comm.rings(), comm.all_to_all_route()["m"]
    rng = np.random.default_rng(900 + rank)
    calls = Q.sequence(world) + [dict(kind="sr1", pat="ungrouped_3C", salt=11, root=None, count=0)]
    staged = []
    for call in calls:
        if call["kind"] == "sr1":
            ops = [SR.S(0, 1, 3 * V.loop_bytes(m)), SR.R(1, 0, 3 * V.loop_bytes(m))]
            staged.append((call, P.SRStaged(world, ops, call["salt"], call=call), None))
        elif call["kind"] in ("sr", "a2av", "a2avd"):
            # every rank builds the whole case (the data is a function of the op) and issues its own part
            staged.append((call, Q.stage_call(call, world, rings, m, rng), None))
        else:
            x = S.call_input(call, world, rng)
            xs = [None] * world
            dist.all_gather_object(xs, x)
            staged.append((call, xs, S.rank_buffers(call, world, rank, x)))
    torch.cuda.synchronize()
    algos = []
    for call, xs, bufs in staged:
        if call["kind"] == "sr":
            with C.group():  # this rank's calls only
                xs.issue_rank(comm, rank)
        elif call["kind"] in ("sr1", "a2av", "a2avd"):
            xs.issue_rank(comm, rank)  # sr1: one ungrouped call (none on a third rank)
        else:
            S.issue_rank(comm, call, bufs[0], bufs[1])
        algos.append(comm.last_algo())
    torch.cuda.synchronize()
    comm.sync()
    checks = {}
    for i, (call, xs, bufs) in enumerate(staged):
        if bufs is None:
            try:
                xs.check_rank(rank, i)
                ok = True
            except AssertionError as e:
                print(f"rank {rank}: {e}", file=sys.stderr, flush=True)
                ok = False
        else:
            send, recv, out = bufs
            exp = S.call_expected(orc, call, xs, comm.nchannels, comm.rings())[rank]
            ok = (out is None) == (exp is None) and (out is None or out.cpu().numpy().tobytes() == exp.tobytes())
        ok = ok and algos[i] == "ring"
        checks[f"{i}/{call['kind']}/{call.get('pat', call.get('mat', ''))}/root{call['root']}/{algos[i]}"] = bool(ok)
    route = comm.all_to_all_route()
    dist.barrier()  # every rank's last kernel is done before any arena returns to the pool
    comm.destroy()
    allres = [None] * world
    dist.all_gather_object(allres, checks)
    if rank == 0:
        merged = {k: all(r.get(k, False) for r in allres) for k in checks}
        print(json.dumps({"world": world, "route": route, "checks": merged, "all_ok": all(merged.values())}),
              flush=True)
    dist.barrier()
    dist.destroy_process_group()
    sys.exit(0 if all(checks.values()) else 1)


if __name__ == "__main__":
    main()
