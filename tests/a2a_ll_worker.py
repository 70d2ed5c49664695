#!/usr/bin/env python3
"""One rank per process: the sequence of tests/test_gpu_all_to_all_ll_sequences.py
(LL AllToAll / AllToAllv / AllToAllvDev launches among LL, one-shot and ring
AllReduces, an LL AllGather, a ring AllToAll, a Broadcast and a Send/Recv
group) through IPC-mapped FIFO arenas.  Every process opts in with the same two
limits and holds its size tables in its own device memory.

  python -m torch.distributed.run --nproc-per-node 2 --master-addr 127.0.0.1 \
      --master-port 29517 tests/a2a_ll_worker.py

Driven by tests/test_gpu_all_to_all_ll_sequences.py (a worker, not a test
module).  Every rank issues the whole sequence without a sync in between, syncs
once and checks its own outputs byte for byte; rank 0 prints the merged verdicts.
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
    import test_gpu_all_to_all_ll_sequences as T
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
    cap = comm.all_to_all_ll_max()
    comm.set_all_to_all_ll(bytes_per_peer=cap, v_bytes_per_peer=cap)
    rings, m = comm.rings(), comm.all_to_all_route()["m"]
    rng = np.random.default_rng(900 + rank)
    staged = []
    for call in T.sequence(world):
        kind = call["kind"]
        if kind in ("a2av", "a2avd", "xdev", "sr"):
            # every rank builds the whole case (the data is a function of the rank) and issues its own part
            staged.append((call, T.stage_call(call, world, rings, m, rng), None))
        elif kind == "a2a":
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
        kind = call["kind"]
        if kind == "xdev":
            xs.issue_rank(comm, rank, part=0)
            first = comm.last_algo()
            xs.issue_rank(comm, rank, part=1)
            algos.append(comm.last_algo() if first == "ll" else "exchange_counts:" + str(first))
            continue
        if kind in ("a2av", "a2avd"):
            xs.issue_rank(comm, rank)
        elif kind == "sr":
            with C.group():
                xs.issue_rank(comm, rank)
        elif kind == "a2a":
            C.all_to_all(comm, bufs[0], bufs[1], call["count"])
        else:
            S.issue_rank(comm, call, bufs[0], bufs[1])
        algos.append(comm.last_algo())
    torch.cuda.synchronize()
    comm.sync()
    checks = {}
    for i, (call, xs, bufs) in enumerate(staged):
        kind = call["kind"]
        if bufs is None:
            try:
                xs.check_rank(rank, i)
                ok = True
            except AssertionError as e:
                print(f"rank {rank}: {e}", file=sys.stderr, flush=True)
                ok = False
        else:
            send, recv, out = bufs
            if kind == "a2a":
                exp = a2a_ref.expected(xs, call["count"])[rank]
                ok = send.cpu().numpy().tobytes() == xs[rank].tobytes()
            else:
                exp = S.call_expected(orc, call, xs, comm.nchannels, comm.rings())[rank]
                ok = True
            ok = ok and (out is None) == (exp is None) and (out is None or
                                                            out.cpu().numpy().tobytes() == exp.tobytes())
        ok = ok and algos[i] == T.expected_algo(call)
        checks[f"{i}/{kind}/root{call['root']}/n{call['count']}/{algos[i]}"] = bool(ok)
    dist.barrier()  # every rank's last kernel is done before any arena returns to the pool
    comm.destroy()
    allres = [None] * world
    dist.all_gather_object(allres, checks)
    if rank == 0:
        merged = {k: all(r.get(k, False) for r in allres) for k in checks}
        print(json.dumps({"world": world, "cap": cap, "checks": merged, "all_ok": all(merged.values())}), flush=True)
    dist.barrier()
    dist.destroy_process_group()
    sys.exit(0 if all(checks.values()) else 1)


if __name__ == "__main__":
    main()
