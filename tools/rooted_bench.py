#!/usr/bin/env python3
"""Per-call time of ring Broadcast and Reduce on the one-GPU virtual node,
beside AllGather and ReduceScatter calls that put the same bytes on each link.

A Broadcast or Reduce of S bytes moves S bytes over every link of the chain.
An AllGather of s bytes per rank, or a ReduceScatter of blocks of s bytes,
moves (n - 1) * s over every link, so the siblings run with s = S / (n - 1).
The table exists to show a chain that fails to pipeline across loops (a rooted
call taking a multiple of its sibling's time); it sets no pass mark.  Not the
xGMI number: all ranks share one GPU's HBM (tools/vnode_bench.py).

  python tools/rooted_bench.py [--n 2 8] [--sizes-kib 64 1024 65536] [--out FILE.jsonl]

Every (n, size) step runs in a fresh child process under its own time limit;
the first step that fails or runs out of time ends the run.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def step(n, kib, iters):
    """One (n, size) step: four collectives on one communicator set, the ring at every size."""
    import torch

    from mccs_amd import comm as C

    F32 = C.AllReduceDataType.Float32
    comms = C.init_all([0] * n, C.CommConfig(direct_bytes=-1, oneshot_bytes=-1, ll_bytes=-1))
    cnt = (kib << 10) // 4                 # fp32 elements of the rooted buffer
    part = max(1, cnt // (n - 1))          # elements per rank / per block of the siblings
    xs = [torch.randn(max(cnt, n * part), device="cuda") for _ in range(n)]
    ys = [torch.empty(max(cnt, n * part), device="cuda") for _ in range(n)]
    calls = {
        "broadcast": lambda r: C.broadcast(comms[r], xs[r] if r == 0 else None, ys[r], cnt * 4, 0),
        "reduce": lambda r: C.reduce(comms[r], xs[r], ys[r] if r == 0 else None, cnt, F32, root=0),
        "allgather": lambda r: C.all_gather(comms[r], xs[r], ys[r], part * 4),
        "reduce_scatter": lambda r: C.reduce_scatter(comms[r], xs[r], ys[r], part, F32),
    }
    out = {"n": n, "KiB": kib, "link_KiB": kib, "lanes": comms[0].lanes, "channels": comms[0].nchannels, "iters": iters}

    def run(call, k):
        for _ in range(k):
            with C.group():
                for r in range(n):
                    call(r)
        for c in comms:
            c.sync()
        torch.cuda.synchronize()

    for name, call in calls.items():
        run(call, 2)  # warm-up: code object load, steady FIFO state
        t0 = time.perf_counter()
        run(call, iters)
        out[name + "_us"] = round((time.perf_counter() - t0) / iters * 1e6, 1)
    out["broadcast_over_allgather"] = round(out["broadcast_us"] / out["allgather_us"], 2)
    out["reduce_over_reduce_scatter"] = round(out["reduce_us"] / out["reduce_scatter_us"], 2)
    torch.cuda.synchronize()
    for c in comms:
        c.destroy()
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[2, 8])
    ap.add_argument("--sizes-kib", type=int, nargs="+", default=[64, 1024, 65536])
    ap.add_argument("--iters", type=int, default=0, help="timed calls per collective (0: by size)")
    ap.add_argument("--step-timeout", type=int, default=120, help="seconds per (n, size) step")
    ap.add_argument("--out", default=None, help="also append the result lines to this file")
    ap.add_argument("--step", type=int, nargs=2, default=None, help=argparse.SUPPRESS)  # child: n KiB
    args = ap.parse_args()
    if args.step:
        n, kib = args.step
        step(n, kib, args.iters or (200 if kib <= 1024 else 20))
        return 0
    for n in args.n:
        for kib in args.sizes_kib:
            cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--step",
                   str(n), str(kib), "--iters", str(args.iters)]
            r = subprocess.run(cmd, capture_output=True, text=True)
            lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
            if r.returncode != 0 or not lines:
                print(f"step n={n} KiB={kib} failed (exit {r.returncode}); stopping\n{r.stdout[-2000:]}{r.stderr[-2000:]}",
                      file=sys.stderr)
                return 1
            print(lines[-1], flush=True)
            if args.out:
                with open(args.out, "a") as f:
                    f.write(lines[-1] + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
