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
  python tools/direct_bench.py --algos direct wide-direct quant --dtype bfloat16 [--n 4 8] [--sizes-kib 1024 4096 8192]
The two opt-in two-shots beside the ring-order one at the same sizes, each on
the two-shot's arena: the wide-accumulate one (mccsCommSetAllReduceWide) and the
block-scaled FP8 one (mccsCommSetAllReduceQuant); float16 / bfloat16 only.
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
  python tools/direct_bench.py --wide --dtype bfloat16 [--n 2 4 8] [--sizes-kib 8 32 ...] [--regions 5]
The wide-accumulate AllReduce (mccsCommSetAllReduceWide) against the ring-order
LL / one-shot / two-shot body the same size takes, timed like --rooted, plus
us per call of a 20-call graph replay.
  python tools/direct_bench.py --wide --reduce-scatter | --wide --rooted --dtype bfloat16 [--n 2 4 8] [--sizes-kib ...]
The wide-accumulate ReduceScatter (size = bytes per block) or Reduce (the
buffer, the root rotating; mccsCommSetReduceScatterWide / mccsCommSetReduceWide)
timed the same way: Sum beside the ring-order direct body of the same size,
the average (PreMulSum) beside the ring, its only other path.
  python tools/direct_bench.py --wide --reduce-scatter --stream --dtype bfloat16 [--n 2 4 8] [--sizes-kib 1024 4096 16384]
The wide streamed ReduceScatter (mccsCommSetReduceScatterWideStream, whole-slot
rounds of 1 MiB) at blocks of 1x, 4x and 16x the slot, timed the same way
beside the ring of the same size and the same bytes as a host-issued sequence
of slot-sized wide one-shot launches.
  python tools/direct_bench.py --wide --stream --dtype bfloat16 [--n 2 4 8] [--sizes-kib 4096 16384 65536]
The wide streamed AllReduce (mccsCommSetAllReduceWideStream, largest rounds) at
buffers of 2x, 8x and 32x the 2 MiB two-shot slot, per graph-replayed call,
beside the ring of the same size and the same bytes as a host-issued sequence
of slot-sized wide two-shot launches; the three alternate region by region.
  python tools/direct_bench.py --wide --reduce-scatter --stream --quant --dtype bfloat16 [--n 4 8] [--sizes-kib 1024 ... 32768]
The block-scaled FP8 streamed ReduceScatter (mccsCommSetReduceScatterQuant,
largest rounds of a 1 MiB slot) at blocks of 1 to 32 MiB, per graph-replayed
call, beside the ring and the wide streamed kernel of the same size; the three
alternate region by region.
  python tools/direct_bench.py --wide --stream --quant --dtype bfloat16 [--n 4 8] [--sizes-kib 4096 16384 65536]
The block-scaled FP8 streamed AllReduce (mccsCommSetAllReduceQuantStream,
largest rounds of a 1 MiB one-shot slot and half a 2 MiB two-shot slot) at
buffers of 4 to 64 MiB, likewise beside the ring and the wide streamed
AllReduce.
  python tools/direct_bench.py --allgather --quant --dtype bfloat16 [--n 4 8] [--sizes-kib 1024 4096 16384 65536]
The explicit block-scaled FP8 streamed AllGather (mccsAllGatherQuant, largest
rounds of a 1 MiB slot) at 1 to 64 MiB per rank, per graph-replayed call,
beside the ring AllGather and, where a rank's bytes fit the slot, the one-shot
AllGather, at equal input bytes.
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


def wide_mode(args, torch, C, st, dt, code, es):
    """--wide: the wide-accumulate AllReduce against the ring-order body that
    the same size takes (LL to 64 KiB, one-shot to 1 MiB, two-shot to 8 MiB),
    per call: eager regions that alternate between the two, and 20 calls per
    graph replay."""
    import statistics

    assert es == 2, "--wide times float16 / bfloat16"
    ll_top, one_top, two_top = 64 << 10, 1 << 20, 8 << 20
    sizes = args.sizes_kib if args.sizes_kib != DEFAULT_SIZES_KIB else [8, 32, 128, 512, 2048, 8192]
    rows = []
    for n in args.n:
        cfg = C.CommConfig(ll_bytes=ll_top, oneshot_bytes=one_top, direct_bytes=two_top)
        sets = {"order": C.init_all([0] * n, cfg), "wide": C.init_all([0] * n, cfg)}
        assert sets["wide"][0].all_reduce_wide_max() == (ll_top, one_top, two_top)
        for c in sets["wide"]:
            c.set_all_reduce_wide(ll_top, one_top, two_top)
        for kib in sizes:
            nbytes = kib << 10
            cnt = nbytes // es
            body = "ll" if nbytes <= ll_top else "oneshot" if nbytes <= one_top else "direct"
            want = {"order": body, "wide": "wide-" + body}
            xs = [torch.randn(cnt, device="cuda").to(dt) for _ in range(n)]
            ys = [torch.empty(cnt, dtype=dt, device="cuda") for _ in xs]
            row = {"n": n, "bytes": nbytes, "body": body}

            def once(a):
                with C.group():
                    for r, c in enumerate(sets[a]):
                        C.all_reduce(c, xs[r], ys[r], cnt, code, 0, stream=st)

            for a in sets:  # warm-up: every kernel's code object
                for _ in range(5):
                    once(a)
                st.synchronize()
                assert sets[a][0].last_algo() == want[a], (a, sets[a][0].last_algo())
            us = {a: [] for a in sets}
            for _ in range(args.regions):
                for a in sets:  # the variants alternate region by region
                    t0 = time.perf_counter()
                    for _ in range(args.calls):
                        once(a)
                    st.synchronize()
                    us[a].append((time.perf_counter() - t0) / args.calls * 1e6)
            for a in sets:
                row[a + "_us"] = round(statistics.median(us[a]), 2)
                row[a + "_min_us"], row[a + "_max_us"] = round(min(us[a]), 2), round(max(us[a]), 2)
                row[a + "_graph_us"] = _time_call(torch, lambda: once(a), st, 5)[1]
                for c in sets[a]:
                    c.sync()
            rows.append(row)
            print(json.dumps(row), flush=True)
            del xs, ys
        torch.cuda.synchronize()
        for comms in sets.values():
            for c in comms:
                c.destroy()
    print(json.dumps({"tool": "direct_bench", "collective": "allreduce-wide", "dtype": args.dtype, "calls": args.calls,
                      "regions": args.regions, "rows": rows}), flush=True)


def wide_rs_mode(args, torch, C, st, dt, code, es, rooted):
    """--wide --reduce-scatter / --wide --rooted: the wide ReduceScatter (per
    block) or Reduce (per buffer, the root rotating on every call), LL to
    64 KiB and one-shot to 1 MiB.  Sum: beside the ring-order direct body of
    the same size ("order"); the average: beside the ring ("ring").  Eager
    regions alternate between the two; 20 calls per graph replay."""
    import statistics

    assert es == 2, "--wide times float16 / bfloat16"
    ll_top, one_top = 64 << 10, 1 << 20
    sizes = args.sizes_kib if args.sizes_kib != DEFAULT_SIZES_KIB else [1, 8, 64, 256, 1024]
    rows = []
    for n in args.n:
        cfg = C.CommConfig(ll_bytes=ll_top, oneshot_bytes=one_top, direct_bytes=-1)
        sets = {a: C.init_all([0] * n, cfg) for a in ("ring", "order", "wide")}
        for c in sets["order"]:
            if rooted:
                c.set_rooted_direct(reduce_bytes=one_top, reduce_ll_bytes=ll_top)
            else:
                c.set_reduce_scatter_direct(one_top, ll_top)
        for c in sets["wide"]:
            assert (c.reduce_wide_max() if rooted else c.reduce_scatter_wide_max()) == (ll_top, one_top)
            (c.set_reduce_wide if rooted else c.set_reduce_scatter_wide)(ll_top, one_top)
        turn = [0]
        for kib in sizes:
            nbytes = kib << 10
            cnt = nbytes // es
            body = "ll" if nbytes <= ll_top else "oneshot"
            xs = [torch.randn(cnt * (1 if rooted else n), device="cuda").to(dt) for _ in range(n)]
            ys = [torch.empty(cnt, dtype=dt, device="cuda") for _ in xs]
            for op, base in (("sum", "order"), ("avg", "ring")):
                want = {base: body if base == "order" else "ring", "wide": "wide-" + body}
                row = {"n": n, "func": "reduce" if rooted else "reducescatter", "bytes": nbytes, "body": body, "op": op}

                def once(a):
                    turn[0] += 1
                    root = turn[0] % n
                    with C.group():
                        for r, c in enumerate(sets[a]):
                            if rooted and op == "avg":
                                C.reduce_avg(c, xs[r], ys[r] if r == root else None, cnt, code, root, stream=st)
                            elif rooted:
                                C.reduce(c, xs[r], ys[r] if r == root else None, cnt, code, 0, root, stream=st)
                            elif op == "avg":
                                C.reduce_scatter_avg(c, xs[r], ys[r], cnt, code, stream=st)
                            else:
                                C.reduce_scatter(c, xs[r], ys[r], cnt, code, 0, stream=st)

                for a in want:  # warm-up: every kernel's code object, every root
                    for _ in range(max(5, n)):
                        once(a)
                    st.synchronize()
                    assert sets[a][0].last_algo() == want[a], (a, sets[a][0].last_algo())
                us = {a: [] for a in want}
                for _ in range(args.regions):
                    for a in want:  # the variants alternate region by region
                        t0 = time.perf_counter()
                        for _ in range(args.calls):
                            once(a)
                        st.synchronize()
                        us[a].append((time.perf_counter() - t0) / args.calls * 1e6)
                for a in want:
                    row[a + "_us"] = round(statistics.median(us[a]), 2)
                    row[a + "_min_us"], row[a + "_max_us"] = round(min(us[a]), 2), round(max(us[a]), 2)
                    row[a + "_graph_us"] = _time_call(torch, lambda: once(a), st, 5)[1]
                    for c in sets[a]:
                        c.sync()
                rows.append(row)
                print(json.dumps(row), flush=True)
            del xs, ys
        torch.cuda.synchronize()
        for comms in sets.values():
            for c in comms:
                c.destroy()
    print(json.dumps({"tool": "direct_bench", "collective": "reduce-wide" if rooted else "reducescatter-wide",
                      "dtype": args.dtype, "calls": args.calls, "regions": args.regions, "rows": rows}), flush=True)


def wide_stream_mode(args, torch, C, st, dt, code, es):
    """--wide --reduce-scatter --stream: per block size (1x, 4x, 16x the 1 MiB
    one-shot slot) the ring ReduceScatter ("ring": where such a block goes
    without the opt-in), the streamed kernel ("stream", rounds of one slot) and
    the same bytes as K host-issued wide one-shot launches of one slot each
    ("split": launch j reduces n blocks of one slot lying one after another, so
    the layout differs and the bytes do not).  Eager regions alternate between
    the three."""
    import statistics

    assert es == 2, "--wide times float16 / bfloat16"
    slot = 1 << 20
    sizes = args.sizes_kib if args.sizes_kib != DEFAULT_SIZES_KIB else [1024, 4096, 16384]
    rows = []
    for n in args.n:
        cfg = C.CommConfig(ll_bytes=-1, oneshot_bytes=slot, direct_bytes=-1)
        sets = {a: C.init_all([0] * n, cfg) for a in ("ring", "stream", "split")}
        for c in sets["stream"]:
            assert c.reduce_scatter_wide_stream_max() == slot
            c.set_reduce_scatter_wide_stream(max(sizes) << 10, 0)
        for c in sets["split"]:
            c.set_reduce_scatter_wide(0, slot)
        want = {"ring": "ring", "stream": "wide-stream", "split": "wide-oneshot"}
        for kib in sizes:
            nbytes = kib << 10
            cnt, part, k = nbytes // es, slot // es, nbytes // slot
            assert k * slot == nbytes, "--stream block sizes are multiples of the 1 MiB slot"
            xs = [torch.randn(cnt * n, device="cuda").to(dt) for _ in range(n)]
            ys = [torch.empty(cnt, dtype=dt, device="cuda") for _ in xs]
            row = {"n": n, "func": "reducescatter", "block_bytes": nbytes, "slot_bytes": slot, "rounds": k}

            def once(a):
                for j in range(k if a == "split" else 1):
                    with C.group():
                        for r, c in enumerate(sets[a]):
                            if a == "split":
                                C.reduce_scatter(c, xs[r][j * n * part:], ys[r][j * part:], part, code, 0, stream=st)
                            else:
                                C.reduce_scatter(c, xs[r], ys[r], cnt, code, 0, stream=st)

            for a in sets:  # warm-up: every kernel's code object
                for _ in range(5):
                    once(a)
                st.synchronize()
                assert sets[a][0].last_algo() == want[a], (a, sets[a][0].last_algo())
            us = {a: [] for a in sets}
            for _ in range(args.regions):
                for a in sets:  # the variants alternate region by region
                    t0 = time.perf_counter()
                    for _ in range(args.calls):
                        once(a)
                    st.synchronize()
                    us[a].append((time.perf_counter() - t0) / args.calls * 1e6)
            for a in sets:
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
    print(json.dumps({"tool": "direct_bench", "collective": "reducescatter-wide-stream", "dtype": args.dtype,
                      "calls": args.calls, "regions": args.regions, "rows": rows}), flush=True)


def wide_ar_stream_mode(args, torch, C, st, dt, code, es):
    """--wide --stream: per buffer size (2x, 8x, 32x the 2 MiB two-shot slot)
    the ring AllReduce ("ring": where such a buffer goes without the opt-in),
    the streamed kernel ("stream", rounds of 1 MiB per share) and the same
    bytes as K host-issued wide two-shot launches of one slot each ("split":
    what keeps the bits today).  Each variant is captured as a graph of
    --graph-calls calls after an eager warm-up; a region replays it until
    --calls calls ran, and the regions alternate between the three."""
    import statistics

    assert es == 2, "--wide times float16 / bfloat16"
    slot = 2 << 20
    sizes = args.sizes_kib if args.sizes_kib != DEFAULT_SIZES_KIB else [4096, 16384, 65536]
    per, rows = args.graph_calls, []
    for n in args.n:
        cfg = C.CommConfig(ll_bytes=-1, oneshot_bytes=slot // 2, direct_bytes=slot)
        sets = {a: C.init_all([0] * n, cfg) for a in ("ring", "stream", "split")}
        for c in sets["stream"]:
            assert c.all_reduce_wide_stream_max() == slot // 2
            c.set_all_reduce_wide_stream(max(sizes) << 10, 0)
        for c in sets["split"]:
            c.set_all_reduce_wide(0, 0, slot)
        want = {"ring": "ring", "stream": "wide-stream", "split": "wide-direct"}
        for kib in sizes:
            nbytes = kib << 10
            cnt, part, k = nbytes // es, slot // es, nbytes // slot
            assert k * slot == nbytes, "--stream buffer sizes are multiples of the 2 MiB slot"
            xs = [torch.randn(cnt, device="cuda").to(dt) for _ in range(n)]
            ys = [torch.empty(cnt, dtype=dt, device="cuda") for _ in xs]
            rounds = -(-((-(-cnt // n) + 7) // 8 * 8) // (slot // 2 // es))
            row = {"n": n, "func": "allreduce", "bytes": nbytes, "slot_bytes": slot, "launches_split": k, "rounds": rounds}

            def once(a):
                for j in range(k if a == "split" else 1):
                    with C.group():
                        for r, c in enumerate(sets[a]):
                            if a == "split":
                                C.all_reduce(c, xs[r][j * part:], ys[r][j * part:], part, code, 0, stream=st)
                            else:
                                C.all_reduce(c, xs[r], ys[r], cnt, code, 0, stream=st)

            graphs = {}
            for a in sets:  # warm-up (every kernel's code object), then one graph of `per` calls per variant
                for _ in range(3):
                    once(a)
                st.synchronize()
                assert sets[a][0].last_algo() == want[a], (a, sets[a][0].last_algo())
                graphs[a] = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graphs[a], stream=st):
                    for _ in range(per):
                        once(a)
                graphs[a].replay()
                torch.cuda.synchronize()
            us = {a: [] for a in sets}
            for _ in range(args.regions):
                for a in sets:  # the variants alternate region by region
                    t0 = time.perf_counter()
                    for _ in range(max(1, args.calls // per)):
                        graphs[a].replay()
                    torch.cuda.synchronize()
                    us[a].append((time.perf_counter() - t0) / (max(1, args.calls // per) * per) * 1e6)
            for a in sets:
                row[a + "_us"] = round(statistics.median(us[a]), 2)
                row[a + "_min_us"], row[a + "_max_us"] = round(min(us[a]), 2), round(max(us[a]), 2)
                for c in sets[a]:
                    c.sync()
            rows.append(row)
            print(json.dumps(row), flush=True)
            del graphs, xs, ys
        torch.cuda.synchronize()
        for comms in sets.values():
            for c in comms:
                c.destroy()
    print(json.dumps({"tool": "direct_bench", "collective": "allreduce-wide-stream", "dtype": args.dtype, "timed": "graph",
                      "calls": args.calls, "graph_calls": per, "regions": args.regions, "rows": rows}), flush=True)


def quant_rs_mode(args, torch, C, st, dt, code, es):
    """--wide --reduce-scatter --stream --quant: per block size (1 to 32 MiB)
    the ring ReduceScatter ("ring": where such a block goes without an
    opt-in), the wide streamed kernel ("stream", 16-bit rounds of one 1 MiB
    slot) and the block-scaled FP8 streamed kernel ("quant", the largest
    rounds of the same slot).  Each variant is captured as a graph of
    --graph-calls calls after an eager warm-up; a region replays it until
    --calls calls ran, and the regions alternate between the three."""
    import statistics

    assert es == 2, "--quant times float16 / bfloat16"
    slot = 1 << 20
    sizes = args.sizes_kib if args.sizes_kib != DEFAULT_SIZES_KIB else [1024, 4096, 16384, 32768]
    per, rows = args.graph_calls, []
    for n in args.n:
        cfg = C.CommConfig(ll_bytes=-1, oneshot_bytes=slot, direct_bytes=-1)
        sets = {a: C.init_all([0] * n, cfg) for a in ("ring", "stream", "quant")}
        for c in sets["stream"]:
            c.set_reduce_scatter_wide_stream(max(sizes) << 10, 0)
        for c in sets["quant"]:
            c.set_reduce_scatter_quant(max(sizes) << 10, 0, 0)
        round_q = sets["quant"][0].reduce_scatter_quant_max()
        want = {"ring": "ring", "stream": "wide-stream", "quant": "quant-stream"}
        for kib in sizes:
            nbytes = kib << 10
            cnt = nbytes // es
            xs = [torch.randn(cnt * n, device="cuda").to(dt) for _ in range(n)]
            ys = [torch.empty(cnt, dtype=dt, device="cuda") for _ in xs]
            row = {"n": n, "func": "reducescatter", "block_bytes": nbytes, "slot_bytes": slot,
                   "rounds_stream": -(-nbytes // slot), "rounds_quant": -(-nbytes // round_q)}

            def once(a):
                with C.group():
                    for r, c in enumerate(sets[a]):
                        C.reduce_scatter(c, xs[r], ys[r], cnt, code, 0, stream=st)

            graphs = {}
            for a in sets:  # warm-up (every kernel's code object), then one graph of `per` calls per variant
                for _ in range(3):
                    once(a)
                st.synchronize()
                assert sets[a][0].last_algo() == want[a], (a, sets[a][0].last_algo())
                graphs[a] = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graphs[a], stream=st):
                    for _ in range(per):
                        once(a)
                graphs[a].replay()
                torch.cuda.synchronize()
            us = {a: [] for a in sets}
            for _ in range(args.regions):
                for a in sets:  # the variants alternate region by region
                    t0 = time.perf_counter()
                    for _ in range(max(1, args.calls // per)):
                        graphs[a].replay()
                    torch.cuda.synchronize()
                    us[a].append((time.perf_counter() - t0) / (max(1, args.calls // per) * per) * 1e6)
            for a in sets:
                row[a + "_us"] = round(statistics.median(us[a]), 2)
                row[a + "_min_us"], row[a + "_max_us"] = round(min(us[a]), 2), round(max(us[a]), 2)
                for c in sets[a]:
                    c.sync()
            rows.append(row)
            print(json.dumps(row), flush=True)
            del graphs, xs, ys
        torch.cuda.synchronize()
        for comms in sets.values():
            for c in comms:
                c.destroy()
    print(json.dumps({"tool": "direct_bench", "collective": "reducescatter-quant-stream", "dtype": args.dtype, "timed": "graph",
                      "calls": args.calls, "graph_calls": per, "regions": args.regions, "rows": rows}), flush=True)


def quant_ag_mode(args, torch, C, st, dt, code, es):
    """--allgather --quant: per input size per rank (1 to 64 MiB) the ring
    AllGather ("ring": where the byte-typed call goes above the one-shot
    limit), the one-shot AllGather ("oneshot", only where a rank's bytes fit
    the 1 MiB slot) and the explicit block-scaled FP8 streamed AllGather
    ("quant", the largest rounds of the same slot), at equal input bytes.
    Captured, replayed and alternated as quant_rs_mode does."""
    import statistics

    assert es == 2, "--quant times float16 / bfloat16"
    slot = 1 << 20
    sizes = args.sizes_kib if args.sizes_kib != DEFAULT_SIZES_KIB else [1024, 4096, 16384, 65536]
    per, rows = args.graph_calls, []
    for n in args.n:
        sets = {"ring": C.init_all([0] * n, C.CommConfig(ll_bytes=-1, oneshot_bytes=-1, direct_bytes=-1))}
        for a in ("oneshot", "quant"):
            sets[a] = C.init_all([0] * n, C.CommConfig(ll_bytes=-1, oneshot_bytes=slot, direct_bytes=-1))
        for c in sets["quant"]:
            c.set_all_gather_quant(0)
        round_q = sets["quant"][0].all_gather_quant_max()
        want = {"ring": "ring", "oneshot": "oneshot", "quant": "quant-stream"}
        for kib in sizes:
            nbytes = kib << 10
            cnt = nbytes // es
            xs = [torch.randn(cnt, device="cuda").to(dt) for _ in range(n)]
            ys = [torch.empty(cnt * n, dtype=dt, device="cuda") for _ in xs]
            row = {"n": n, "func": "allgather", "bytes_per_rank": nbytes, "slot_bytes": slot,
                   "rounds_quant": -(-nbytes // round_q)}
            algos = [a for a in sets if a != "oneshot" or nbytes <= slot]

            def once(a):
                with C.group():
                    for r, c in enumerate(sets[a]):
                        if a == "quant":
                            C.all_gather_quant(c, xs[r], ys[r], cnt, code, stream=st)
                        else:
                            C.all_gather(c, xs[r], ys[r], nbytes, stream=st)

            graphs = {}
            for a in algos:  # warm-up (every kernel's code object), then one graph of `per` calls per variant
                for _ in range(3):
                    once(a)
                st.synchronize()
                assert sets[a][0].last_algo() == want[a], (a, sets[a][0].last_algo())
                graphs[a] = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graphs[a], stream=st):
                    for _ in range(per):
                        once(a)
                graphs[a].replay()
                torch.cuda.synchronize()
            us = {a: [] for a in algos}
            for _ in range(args.regions):
                for a in algos:  # the variants alternate region by region
                    t0 = time.perf_counter()
                    for _ in range(max(1, args.calls // per)):
                        graphs[a].replay()
                    torch.cuda.synchronize()
                    us[a].append((time.perf_counter() - t0) / (max(1, args.calls // per) * per) * 1e6)
            for a in algos:
                row[a + "_us"] = round(statistics.median(us[a]), 2)
                row[a + "_min_us"], row[a + "_max_us"] = round(min(us[a]), 2), round(max(us[a]), 2)
                for c in sets[a]:
                    c.sync()
            rows.append(row)
            print(json.dumps(row), flush=True)
            del graphs, xs, ys
        torch.cuda.synchronize()
        for comms in sets.values():
            for c in comms:
                c.destroy()
    print(json.dumps({"tool": "direct_bench", "collective": "allgather-quant-stream", "dtype": args.dtype, "timed": "graph",
                      "calls": args.calls, "graph_calls": per, "regions": args.regions, "rows": rows}), flush=True)


def quant_ar_mode(args, torch, C, st, dt, code, es):
    """--wide --stream --quant: per buffer size (4 to 64 MiB) the ring AllReduce
    ("ring": where such a buffer goes without an opt-in), the wide streamed
    kernel ("stream", 16-bit rounds of 1 MiB per share) and the block-scaled FP8
    streamed kernel ("quant", the largest rounds of the same slots).  Each
    variant is captured as a graph of --graph-calls calls after an eager
    warm-up; a region replays it until --calls calls ran, and the regions
    alternate between the three."""
    import statistics

    assert es == 2, "--quant times float16 / bfloat16"
    slot = 2 << 20
    sizes = args.sizes_kib if args.sizes_kib != DEFAULT_SIZES_KIB else [4096, 16384, 65536]
    per, rows = args.graph_calls, []
    for n in args.n:
        cfg = C.CommConfig(ll_bytes=-1, oneshot_bytes=slot // 2, direct_bytes=slot)
        sets = {a: C.init_all([0] * n, cfg) for a in ("ring", "stream", "quant")}
        for c in sets["stream"]:
            c.set_all_reduce_wide_stream(max(sizes) << 10, 0)
        for c in sets["quant"]:
            c.set_all_reduce_quant_stream(max(sizes) << 10, 0, 0)
        round_q = sets["quant"][0].all_reduce_quant_stream_max() // es
        want = {"ring": "ring", "stream": "wide-stream", "quant": "quant-stream"}
        for kib in sizes:
            nbytes = kib << 10
            cnt = nbytes // es
            xs = [torch.randn(cnt, device="cuda").to(dt) for _ in range(n)]
            ys = [torch.empty(cnt, dtype=dt, device="cuda") for _ in xs]
            row = {"n": n, "func": "allreduce", "bytes": nbytes, "slot_bytes": slot,
                   "rounds_stream": -(-((-(-cnt // n) + 7) // 8 * 8) // (slot // 2 // es)),
                   "rounds_quant": -(-((-(-cnt // n) + 511) // 512 * 512) // round_q)}

            def once(a):
                with C.group():
                    for r, c in enumerate(sets[a]):
                        C.all_reduce(c, xs[r], ys[r], cnt, code, 0, stream=st)

            graphs = {}
            for a in sets:  # warm-up (every kernel's code object), then one graph of `per` calls per variant
                for _ in range(3):
                    once(a)
                st.synchronize()
                assert sets[a][0].last_algo() == want[a], (a, sets[a][0].last_algo())
                graphs[a] = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graphs[a], stream=st):
                    for _ in range(per):
                        once(a)
                graphs[a].replay()
                torch.cuda.synchronize()
            us = {a: [] for a in sets}
            for _ in range(args.regions):
                for a in sets:  # the variants alternate region by region
                    t0 = time.perf_counter()
                    for _ in range(max(1, args.calls // per)):
                        graphs[a].replay()
                    torch.cuda.synchronize()
                    us[a].append((time.perf_counter() - t0) / (max(1, args.calls // per) * per) * 1e6)
            for a in sets:
                row[a + "_us"] = round(statistics.median(us[a]), 2)
                row[a + "_min_us"], row[a + "_max_us"] = round(min(us[a]), 2), round(max(us[a]), 2)
                for c in sets[a]:
                    c.sync()
            rows.append(row)
            print(json.dumps(row), flush=True)
            del graphs, xs, ys
        torch.cuda.synchronize()
        for comms in sets.values():
            for c in comms:
                c.destroy()
    print(json.dumps({"tool": "direct_bench", "collective": "allreduce-quant-stream", "dtype": args.dtype, "timed": "graph",
                      "calls": args.calls, "graph_calls": per, "regions": args.regions, "rows": rows}), flush=True)


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
                    help="variants to time, among ring direct oneshot ll wide-direct quant (rocprof passes isolate one "
                         "kernel mode each)")
    ap.add_argument("--allgather", action="store_true", help="time AllGather (size = bytes per rank): ring vs one-shot")
    ap.add_argument("--reduce-scatter", action="store_true",
                    help="time ReduceScatter (size = bytes per block, 1 KiB to the caps): ring vs direct vs LL, and "
                         "the one-shot AllGather of the same bytes per rank")
    ap.add_argument("--rooted", action="store_true",
                    help="time Broadcast and Reduce (size = the buffer, 1 KiB to the caps): ring vs count-based vs LL")
    ap.add_argument("--wide", action="store_true",
                    help="time the wide-accumulate AllReduce (--dtype float16 / bfloat16; 8 KiB to 8 MiB) against the "
                         "ring-order LL / one-shot / two-shot body of the same size; with --reduce-scatter or --rooted: "
                         "the wide ReduceScatter / Reduce (1 KiB to 1 MiB) against the ring-order direct body, and its "
                         "average against the ring")
    ap.add_argument("--stream", action="store_true",
                    help="with --wide --reduce-scatter: the wide streamed ReduceScatter at 1x, 4x and 16x the one-shot "
                         "slot against the ring and a host-issued sequence of slot-sized wide one-shot launches; with "
                         "--wide alone: the wide streamed AllReduce at 2x, 8x and 32x the two-shot slot, graph-replayed, "
                         "against the ring and a host-issued sequence of slot-sized wide two-shot launches")
    ap.add_argument("--quant", action="store_true",
                    help="with --wide --reduce-scatter --stream: a quant row, the block-scaled FP8 streamed ReduceScatter "
                         "at 1 to 32 MiB per block, graph-replayed, against the ring and the wide streamed kernel; "
                         "with --wide --stream: the block-scaled FP8 streamed AllReduce at 4 to 64 MiB likewise; with "
                         "--allgather: the explicit block-scaled FP8 AllGather at 1 to 64 MiB per rank against the ring "
                         "and, where a rank's bytes fit a slot, the one-shot AllGather")
    ap.add_argument("--graph-calls", type=int, default=4, help="--wide --stream: calls captured into each replayed graph")
    ap.add_argument("--regions", type=int, default=5, help="--rooted, --wide: timed regions of --calls calls per variant")
    args = ap.parse_args()
    args.algos = [a for word in args.algos for a in word.split(",") if a]  # "direct,quant" or "direct quant"
    dt = getattr(torch, args.dtype)
    code = {torch.float16: 6, torch.float32: 7, torch.bfloat16: 9}[dt]
    es = torch.empty(0, dtype=dt).element_size()
    rows = []
    st = side_stream(torch, 0, slot=1)
    if args.allgather and args.quant:
        quant_ag_mode(args, torch, C, st, dt, code, es)
        return
    if args.wide and args.reduce_scatter and args.stream and args.quant:
        quant_rs_mode(args, torch, C, st, dt, code, es)
        return
    if args.wide and args.stream and args.quant:
        quant_ar_mode(args, torch, C, st, dt, code, es)
        return
    if args.wide and args.reduce_scatter and args.stream:
        wide_stream_mode(args, torch, C, st, dt, code, es)
        return
    if args.wide and args.stream and not args.rooted:
        wide_ar_stream_mode(args, torch, C, st, dt, code, es)
        return
    if args.wide and (args.reduce_scatter or args.rooted):
        wide_rs_mode(args, torch, C, st, dt, code, es, args.rooted)
        return
    if args.reduce_scatter:
        reduce_scatter_mode(args, torch, C, st, dt, code, es)
        return
    if args.rooted:
        rooted_mode(args, torch, C, st, dt, code, es)
        return
    if args.wide:
        wide_mode(args, torch, C, st, dt, code, es)
        return
    for n in args.n:
        top = max(args.sizes_kib) << 10
        cfgs = {"ring": C.CommConfig(direct_bytes=-1, oneshot_bytes=-1, ll_bytes=-1),
                "direct": C.CommConfig(direct_bytes=top, oneshot_bytes=-1, ll_bytes=-1),
                "oneshot": C.CommConfig(direct_bytes=-1, ll_bytes=-1, oneshot_bytes=min(top, args.oneshot_max_kib << 10)),
                "ll": C.CommConfig(direct_bytes=-1, oneshot_bytes=-1, ll_bytes=1 << 20),
                # the two opt-in two-shots on the two-shot's own arena (float16 / bfloat16 only)
                "wide-direct": C.CommConfig(direct_bytes=top, oneshot_bytes=-1, ll_bytes=-1),
                "quant": C.CommConfig(direct_bytes=top, oneshot_bytes=-1, ll_bytes=-1)}
        cfgs = {a: cfg for a, cfg in cfgs.items() if a in args.algos}
        assert es == 2 or not {"wide-direct", "quant"} & set(cfgs), "wide-direct and quant time float16 / bfloat16"

        def opt_in(algo, comms):
            for c in comms:
                if algo == "wide-direct":
                    c.set_all_reduce_wide(twoshot_bytes=top)
                if algo == "quant":
                    c.set_all_reduce_quant(top)
            return comms
        if len(args.blocks) == 1:
            os.environ["MCCS_DIRECT_BLOCKS"] = str(args.blocks[0])
        sets = {a: opt_in(a, C.init_all([0] * n, cfg)) for a, cfg in cfgs.items()}
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
                        comms = sets[algo] = opt_in(algo, C.init_all([0] * n, cfgs[algo]))

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
                    assert comms[0].last_algo() == {"quant": "quant-direct"}.get(algo, algo), (algo, comms[0].last_algo())
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
