#!/usr/bin/env python3
"""Virtual-node ring allreduce timing on ONE GPU (all ranks share its HBM).

Not the xGMI number: every rank's FIFO traffic lands in the same HBM, so this
measures protocol overhead and per-lane streaming, not link bandwidth.
  python tools/vnode_bench.py [--sizes-mib 128] [--n 2 4 8]
Cost of an op against Sum in one run (Avg = PreMulSum by 1/n for floating
types, SumPostDiv by n for integer ones), the ops interleaved per repeat:
  python tools/vnode_bench.py --n 4 --sizes-mib 128 --dtype bfloat16 --op sum avg --repeats 5
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    import torch

    from mccs_amd import comm as C

    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[2, 4, 8])
    ap.add_argument("--sizes-mib", type=int, nargs="+", default=[1, 16, 128])
    ap.add_argument("--sizes-kib", type=int, nargs="+", default=None, help="bucket sizes in KiB (override MiB)")
    ap.add_argument("--lanes", type=int, nargs="+", default=[0])
    ap.add_argument("--block", type=int, default=0)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--bridge", type=int, default=0, help="CommConfig.bridge_streams (0 = library default)")
    ap.add_argument("--profile", action="store_true", help="per-slice wait/stream timing (MCCS_RING_PROFILE)")
    ap.add_argument("--graph", action="store_true", help="also time the same calls captured in one HIP graph")
    ap.add_argument("--allgather", action="store_true", help="time AllGather (size = bytes per rank) instead")
    ap.add_argument("--reduce-scatter", action="store_true",
                    help="time ReduceScatter (size = bytes per rank of input; each rank receives size / n) instead")
    ap.add_argument("--op", nargs="+", default=["sum"], choices=["sum", "avg"],
                    help="reduction op(s) of AllReduce / ReduceScatter, timed one after the other in each repeat")
    ap.add_argument("--dtype", default="float32", choices=["float32", "bfloat16", "float16", "int32", "int64"])
    ap.add_argument("--repeats", type=int, default=1, help="timed repeats of every (size, op), one JSON line each")
    args = ap.parse_args()
    if args.allgather and args.reduce_scatter:
        ap.error("--allgather and --reduce-scatter are exclusive")
    tdt = getattr(torch, args.dtype)
    dt_code = getattr(C.AllReduceDataType, args.dtype.capitalize())
    es = torch.empty(0, dtype=tdt).element_size()
    coll = "allgather" if args.allgather else "reduce_scatter" if args.reduce_scatter else "allreduce"
    if args.profile:
        os.environ["MCCS_RING_PROFILE"] = "1"
    for n in args.n:
        for lanes in args.lanes:
            # the ring at every size (the direct kernel has tools/direct_bench.py)
            comms = C.init_all([0] * n, C.CommConfig(lanes=lanes, block_threads=args.block,
                                                          bridge_streams=args.bridge or None,
                                                          direct_bytes=-1, oneshot_bytes=-1, ll_bytes=-1))
            for kib in (args.sizes_kib or [m << 10 for m in args.sizes_mib]):
                cnt = (kib << 10) // es
                if tdt.is_floating_point:
                    xs = [torch.randn(cnt, device="cuda").to(tdt) for _ in range(n)]
                else:
                    xs = [torch.randint(-1000, 1000, (cnt,), device="cuda", dtype=tdt) for _ in range(n)]
                ys = [torch.empty(n * cnt if args.allgather else cnt // n if args.reduce_scatter else cnt,
                                  device="cuda", dtype=tdt) for _ in xs]
                op_name = "sum"

                def call(r, st=None):
                    op, op_arg = (C.AllReduceOpType.Sum, None) if op_name == "sum" else C.avg_op(dt_code, n)
                    if args.allgather:
                        C.all_gather(comms[r], xs[r], ys[r], cnt * es, stream=st)
                    elif args.reduce_scatter:  # the first n * (cnt // n) elements of the input
                        C.reduce_scatter(comms[r], xs[r], ys[r], cnt // n, dt_code, op, stream=st, op_arg=op_arg)
                    else:
                        C.all_reduce(comms[r], xs[r], ys[r], cnt, dt_code, op, stream=st, op_arg=op_arg)

                def once():
                    with C.group():
                        for r in range(n):
                            call(r)

                for repeat in range(args.repeats):
                    for op_name in args.op:
                        once()
                        for c in comms:
                            c.sync()
                        torch.cuda.synchronize()
                        if args.profile:
                            C.ring_profile(0, reset=True)
                        t0 = time.perf_counter()
                        for _ in range(args.iters):
                            once()
                        for c in comms:
                            c.sync()
                        torch.cuda.synchronize()
                        dt = (time.perf_counter() - t0) / args.iters
                        prof = C.ring_profile(0, reset=True) if args.profile else None
                        graph_ms = None
                        if args.graph:  # the same iters calls as one graph replay (no host path per call)
                            st = torch.cuda.Stream()
                            g = torch.cuda.CUDAGraph()
                            torch.cuda.synchronize()
                            with torch.cuda.graph(g, stream=st):
                                for _ in range(args.iters):
                                    with C.group():
                                        for r in range(n):
                                            call(r, st)
                            g.replay()
                            torch.cuda.synchronize()
                            t0 = time.perf_counter()
                            g.replay()
                            torch.cuda.synchronize()
                            graph_ms = (time.perf_counter() - t0) / args.iters * 1e3
                            del g
                        print(json.dumps({"coll": coll, "n": n, "lanes": comms[0].lanes, "channels": comms[0].nchannels,
                                          "op": op_name, "dtype": args.dtype, "repeat": repeat,
                                          "block": comms[0].block_threads, "bridge": args.bridge, "KiB": kib,
                                          "ms": round(dt * 1e3, 4),
                                          "algbw_GBps": round((kib << 10) / dt / 1e9, 2), "slice_profile": prof,
                                          "graph_ms": round(graph_ms, 4) if graph_ms else None,
                                          "graph_algbw_GBps": round((kib << 10) / graph_ms / 1e6, 2) if graph_ms else None}),
                              flush=True)
                del xs, ys
            torch.cuda.synchronize()
            for c in comms:
                c.destroy()


if __name__ == "__main__":
    main()
