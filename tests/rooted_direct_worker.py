#!/usr/bin/env python3
"""One rank per process: the sequence of
tests/test_gpu_rooted_direct_sequences.py (direct and LL Broadcasts and Reduces
with a rotating root among direct ReduceScatters, one-shot, two-shot and LL
AllReduces, AllGathers, an LL AllToAll, ring rooted calls and a closing ring
AllToAll) through IPC-mapped FIFO arenas.  Every process opts in with the same
limits.

  python -m torch.distributed.run --nproc-per-node 2 --master-addr 127.0.0.1 \
      --master-port 29518 tests/rooted_direct_worker.py

Driven by tests/test_gpu_rooted_direct_sequences.py (a worker, not a test
module).  Every rank issues the whole sequence without a sync in between,
syncs once and checks its own outputs byte for byte; rank 0 prints the merged
verdicts.
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
    import a2a_ref
    import test_gpu_rooted_direct_sequences as T
    import test_gpu_rooted_sequences as S
    import vnode

    rank = int(os.environ["RANK"])
    world = int(os.environ["WORLD_SIZE"])
    dev = int(os.environ.get("LOCAL_RANK", rank)) % torch.cuda.device_count()
    torch.cuda.set_device(dev)
    dist.init_process_group("gloo", rank=rank, world_size=world)

    def exchange(b):
        out = [None] * world
        dist.all_gather_object(out, b)
        return out

    comm = C.init_communicator_rank(rank, world, dev, exchange, C.CommConfig(timeout_ms=S.TIMEOUT_MS, **T.CFG))
    T.opt_in(comm)
    rng = np.random.default_rng(900 + rank)
    staged = []
    for call in T.sequence(world):
        if call["kind"] == "a2a":
            xs = a2a_ref.make_inputs(world, call["count"], call["salt"])
            send = vnode.to_dev(xs[rank])
            recv = vnode.to_dev(np.full(world * call["count"], a2a_ref.SENTINEL, np.uint8))
            staged.append((call, xs, (send, recv, recv)))
        else:
            x = S.call_input(call, world, rng)
            xs = [None] * world
            dist.all_gather_object(xs, x)
            staged.append((call, xs, S.rank_buffers(call, world, rank, x)))
    torch.cuda.synchronize()
    algos = []
    for call, xs, bufs in staged:
        if call["kind"] == "a2a":
            C.all_to_all(comm, bufs[0], bufs[1], call["count"])
        else:
            S.issue_rank(comm, call, bufs[0], bufs[1])
        algos.append(comm.last_algo())
    torch.cuda.synchronize()
    comm.sync()
    checks = {}
    for i, (call, xs, bufs) in enumerate(staged):
        send, recv, out = bufs
        if call["kind"] == "a2a":
            exp = a2a_ref.expected(xs, call["count"])[rank]
        else:
            exp = S.call_expected(orc, call, xs, comm.nchannels, comm.rings())[rank]
        ok = algos[i] == call["algo"] and (out is None) == (exp is None)
        if ok and out is not None:
            ok = out.cpu().numpy().tobytes() == exp.tobytes()
        if ok and send is not None and send is not out:  # out of place the input stays as it was
            ok = send.cpu().numpy().tobytes() == np.ascontiguousarray(xs[rank]).tobytes()
        checks[f"{i}/{call['kind']}/n{call['count']}/{algos[i]}"] = bool(ok)
    dist.barrier()  # every rank's last kernel is done before any arena returns to the pool
    comm.destroy()
    allres = [None] * world
    dist.all_gather_object(allres, checks)
    if rank == 0:
        merged = {k: all(r.get(k, False) for r in allres) for k in checks}
        print(json.dumps({"world": world, "checks": merged, "all_ok": all(merged.values())}), flush=True)
    dist.barrier()
    dist.destroy_process_group()
    sys.exit(0 if all(checks.values()) else 1)


if __name__ == "__main__":
    main()
