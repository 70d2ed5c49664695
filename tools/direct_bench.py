#!/usr/bin/env python3
"""Direct (two-shot, one-shot) vs ring AllReduce per call on the virtual node (all
ranks on ONE GPU, one fused launch per call).

Not the xGMI number: every rank's traffic lands in one GPU's HBM.  What it
shows is the protocol's fixed cost per call -- flag round trips, launch,
workgroup count -- which is what decides the threshold below which the
direct kernel should take a bucket.
  python tools/direct_bench.py [--n 2 4 8] [--sizes-kib 32 128 ...] [--blocks 32 128]
Per (n, size): ring / direct us per call, eager (back-to-back calls, one
sync) and graph-replayed (20 calls per graph).
  python tools/direct_bench.py --reduce-scatter [--n 2 4 8] [--sizes-kib 1 4 ...]
ReduceScatter per block size (1 KiB to the caps by default): the ring (limits
0), the direct and the LL variant (mccsCommSetReduceScatterDirect) and the
one-shot AllGather of the same bytes per rank beside them.
  python tools/direct_bench.py --rooted [--n 2 4 8] [--sizes-kib 1 4 ...] [--regions 5]
Broadcast and Reduce per buffer size: the ring (limits 0) against the
count-based and the LL variant (mccsCommSetRootedDirect at the caps), the root
rotating on every call.  Every variant is warmed up, then timed in --regions
regions of --calls calls each, the variants alternating region by region; a
row holds the median and the min / max of the regions' us per call.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _time_call(torch, once, st, calls):
    """us per call: eager (back-to-back, one sync) and graph-replayed (20 calls per graph)."""
    for _ in range(5):
        once()
    st.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        once()
    st.synchronize()
    eager = (time.perf_counter() - t0) / calls
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=st):
        for _ in range(20):
            once()
    g.replay()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(5):
        g.replay()
    torch.cuda.synchronize()
    graph = (time.perf_counter() - t0) / 100
    del g
    return round(eager * 1e6, 2), round(graph * 1e6, 2)


def reduce_scatter_mode(args, torch, C, st, dt, code, es):
    """--reduce-scatter: per block size (bytes per block = bytes per rank of the
    AllGather beside it) the ring ReduceScatter (limits 0), the direct and the
    LL ReduceScatter (mccsCommSetReduceScatterDirect at the caps) and the
    one-shot AllGather, its partner in a sharded-optimizer step."""
    top = 1 << 20
    sizes = args.sizes_kib if args.sizes_kib != DEFAULT_SIZES_KIB else [1, 4, 16, 64, 256, 1024]
    rows = []
    for n in args.n:
        cfg = C.CommConfig(direct_bytes=-1, oneshot_bytes=top, ll_bytes=top)
        sets = {"rs_ring": C.init_all([0] * n, cfg), "rs_direct": C.init_all([0] * n, cfg),
                "rs_ll": C.init_all([0] * n, cfg),
                "ag_oneshot": C.init_all([0] * n, C.CommConfig(direct_bytes=-1, oneshot_bytes=top, ll_bytes=-1))}
        cap, ll_cap = sets["rs_direct"][0].reduce_scatter_direct_max()
        for c in sets["rs_direct"]:
            c.set_reduce_scatter_direct(block_bytes=cap)
        for c in sets["rs_ll"]:
            c.set_reduce_scatter_direct(ll_block_bytes=ll_cap)
        want = {"rs_ring": "ring", "rs_direct": "oneshot", "rs_ll": "ll", "ag_oneshot": "oneshot"}
        for kib in sizes:
            nbytes = kib << 10
            cnt = nbytes // es
            xs = [torch.randn(n * cnt, device="cuda").to(dt) for _ in range(n)]
            ys = [torch.empty(n * cnt, dtype=dt, device="cuda") for _ in xs]
            row = {"n": n, "block_bytes": nbytes, "cap": cap, "ll_cap": ll_cap}
            for name, comms in sets.items():
                if (name == "rs_direct" and nbytes > cap) or (name == "rs_ll" and nbytes > ll_cap) or \
                        (name == "ag_oneshot" and nbytes > top):
                    continue

                def once():
                    with C.group():
                        for r in range(n):
                            if name == "ag_oneshot":
                                C.all_gather(comms[r], xs[r], ys[r], nbytes, stream=st)
                            else:
                                C.reduce_scatter(comms[r], xs[r], ys[r], cnt, code, 0, stream=st)

                row[name + "_eager_us"], row[name + "_graph_us"] = _time_call(torch, once, st, args.calls)
                assert comms[0].last_algo() == want[name], (name, comms[0].last_algo())
                for c in comms:
                    c.sync()
            rows.append(row)
            print(json.dumps(row), flush=True)
            del xs, ys
        torch.cuda.synchronize()
        for comms in sets.values():
            for c in comms:
                c.destroy()
    print(json.dumps({"tool": "direct_bench", "collective": "reducescatter", "dtype": args.dtype, "rows": rows}),
          flush=True)


def rooted_mode(args, torch, C, st, dt, code, es):
    """--rooted: Broadcast and Reduce of one buffer size, ring / count-based / LL."""
    import statistics

    top = 1 << 20
    sizes = args.sizes_kib if args.sizes_kib != DEFAULT_SIZES_KIB else [1, 4, 16, 64, 256, 1024]
    rows = []
    for n in args.n:
        cfg = C.CommConfig(direct_bytes=-1, oneshot_bytes=top, ll_bytes=top)
        sets = {"ring": C.init_all([0] * n, cfg), "direct": C.init_all([0] * n, cfg), "ll": C.init_all([0] * n, cfg)}
        cap, ll_cap = sets["direct"][0].rooted_direct_max()
        for c in sets["direct"]:
            c.set_rooted_direct(bcast_bytes=cap, reduce_bytes=cap)
        for c in sets["ll"]:
            c.set_rooted_direct(bcast_ll_bytes=ll_cap, reduce_ll_bytes=ll_cap)
        want = {"ring": "ring", "direct": "oneshot", "ll": "ll"}
        for kib in sizes:
            nbytes = kib << 10
            cnt = nbytes // es
            xs = [torch.randn(cnt, device="cuda").to(dt) for _ in range(n)]
            ys = [torch.empty(cnt, dtype=dt, device="cuda") for _ in xs]
            for func in ("broadcast", "reduce"):
                row = {"n": n, "func": func, "bytes": nbytes, "cap": cap, "ll_cap": ll_cap}
                live = [a for a in sets if not (a == "direct" and nbytes > cap) and not (a == "ll" and nbytes > ll_cap)]
                turn = {a: 0 for a in live}

                def once(algo):
                    root = turn[algo] % n  # the root rotates on every call
                    turn[algo] += 1
                    with C.group():
                        for r, c in enumerate(sets[algo]):
                            if func == "broadcast":
                                C.broadcast(c, xs[r] if r == root else None, ys[r], nbytes, root, stream=st)
                            else:
                                C.reduce(c, xs[r], ys[r] if r == root else None, cnt, code, 0, root, stream=st)

                for a in live:  # warm-up: every kernel's code object, every root
                    for _ in range(max(5, n)):
                        once(a)
                    st.synchronize()
                    assert sets[a][0].last_algo() == want[a], (a, sets[a][0].last_algo())
                us = {a: [] for a in live}
                for _ in range(args.regions):
                    for a in live:  # the variants alternate region by region
                        t0 = time.perf_counter()
                        for _ in range(args.calls):
                            once(a)
                        st.synchronize()
                        us[a].append((time.perf_counter() - t0) / args.calls * 1e6)
                for a in live:
                    row[a + "_us"] = round(statistics.median(us[a]), 2)
                    row[a + "_min_us"], row[a + "_max_us"] = round(min(us[a]), 2), round(max(us[a]), 2)
                    for c in sets[a]:
                        c.sync()
                rows.append(row)
                print(json.dumps(row), flush=True)
            del xs, ys
        torch.cuda.synchronize()
        for comms in sets.values():
            for c in comms:
                c.destroy()
    print(json.dumps({"tool": "direct_bench", "collective": "rooted", "dtype": args.dtype, "calls": args.calls,
                      "regions": args.regions, "rows": rows}), flush=True)


DEFAULT_SIZES_KIB = [32, 128, 512, 2048, 8192, 32768]


def main():
    import torch

    from mccs_amd import comm as C
    from mccs_amd._streams import side_stream

    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[2, 4, 8])
    ap.add_argument("--sizes-kib", type=int, nargs="+", default=DEFAULT_SIZES_KIB)
    ap.add_argument("--blocks", type=int, nargs="+", default=[128])
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--dtype", default="float16")
    ap.add_argument("--oneshot-max-kib", type=int, default=2048)
    ap.add_argument("--algos", nargs="+", default=["ring", "direct", "oneshot", "ll"],
                    help="variants to time (rocprof passes isolate one kernel mode each)")
    ap.add_argument("--allgather", action="store_true", help="time AllGather (size = bytes per rank): ring vs one-shot")
    ap.add_argument("--reduce-scatter", action="store_true",
                    help="time ReduceScatter (size = bytes per block, 1 KiB to the caps): ring vs direct vs LL, and "
                         "the one-shot AllGather of the same bytes per rank")
    ap.add_argument("--rooted", action="store_true",
                    help="time Broadcast and Reduce (size = the buffer, 1 KiB to the caps): ring vs count-based vs LL")
    ap.add_argument("--regions", type=int, default=5, help="--rooted: timed regions of --calls calls per variant")
    args = ap.parse_args()
    dt = getattr(torch, args.dtype)
    code = {torch.float16: 6, torch.float32: 7, torch.bfloat16: 9}[dt]
    es = torch.empty(0, dtype=dt).element_size()
    rows = []
    st = side_stream(torch, 0, slot=1)
    if args.reduce_scatter:
        reduce_scatter_mode(args, torch, C, st, dt, code, es)
        return
    if args.rooted:
        rooted_mode(args, torch, C, st, dt, code, es)
        return
    for n in args.n:
        top = max(args.sizes_kib) << 10
        cfgs = {"ring": C.CommConfig(direct_bytes=-1, oneshot_bytes=-1, ll_bytes=-1),
                "direct": C.CommConfig(direct_bytes=top, oneshot_bytes=-1, ll_bytes=-1),
                "oneshot": C.CommConfig(direct_bytes=-1, ll_bytes=-1, oneshot_bytes=min(top, args.oneshot_max_kib << 10)),
                "ll": C.CommConfig(direct_bytes=-1, oneshot_bytes=-1, ll_bytes=1 << 20)}
        if len(args.blocks) == 1:
            os.environ["MCCS_DIRECT_BLOCKS"] = str(args.blocks[0])
        sets = {a: C.init_all([0] * n, cfg) for a, cfg in cfgs.items()}
        for a in [a for a in sets if a not in args.algos]:
            for c in sets.pop(a):
                c.destroy()
        for kib in args.sizes_kib:
            cnt = (kib << 10) // es
            xs = [torch.randn(cnt, device="cuda").to(dt) for _ in range(n)]
            ys = [torch.empty(n * cnt if args.allgather else cnt, dtype=dt, device="cuda") for _ in xs]
            row = {"n": n, "bytes": kib << 10}
            for algo, comms in sets.items():
                if algo == "oneshot" and kib > args.oneshot_max_kib or algo == "ll" and kib > 1024:
                    continue
                if args.allgather and algo == "direct":
                    continue
                for blocks in (args.blocks if algo != "ring" else [0]):
                    if blocks and len(args.blocks) > 1:
                        # MCCS_DIRECT_BLOCKS is read when a communicator is created
                        os.environ["MCCS_DIRECT_BLOCKS"] = str(blocks)
                        for c in comms:
                            c.destroy()
                        comms = sets[algo] = C.init_all([0] * n, cfgs[algo])

                    def once():
                        with C.group():
                            for r in range(n):
                                if args.allgather:
                                    C.all_gather(comms[r], xs[r], ys[r], cnt * es, stream=st)
                                else:
                                    C.all_reduce(comms[r], xs[r], ys[r], cnt, code, 0, stream=st)

                    for _ in range(5):
                        once()
                    st.synchronize()
                    assert comms[0].last_algo() == algo, (algo, comms[0].last_algo())
                    t0 = time.perf_counter()
                    for _ in range(args.calls):
                        once()
                    st.synchronize()
                    eager = (time.perf_counter() - t0) / args.calls
                    g = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(g, stream=st):
                        for _ in range(20):
                            once()
                    g.replay()
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(5):
                        g.replay()
                    torch.cuda.synchronize()
                    graph = (time.perf_counter() - t0) / 100
                    del g
                    for c in comms:
                        c.sync()
                    key = algo if not blocks else f"{algo}_g{blocks}"
                    row[key + "_eager_us"] = round(eager * 1e6, 2)
                    row[key + "_graph_us"] = round(graph * 1e6, 2)
            rows.append(row)
            print(json.dumps(row), flush=True)
            del xs, ys
        torch.cuda.synchronize()
        for comms in sets.values():
            for c in comms:
                c.destroy()
    print(json.dumps({"tool": "direct_bench", "collective": "allgather" if args.allgather else "allreduce",
                      "dtype": args.dtype, "rows": rows}), flush=True)


if __name__ == "__main__":
    main()
