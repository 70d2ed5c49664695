#!/usr/bin/env python3
"""Per-call time of AllToAll on the one-GPU virtual node: one hop, the relay
(MCCS_ALLTOALL_HOPS=relay) and an AllGather of the same bytes per rank.

An AllToAll of B bytes per peer moves n * B bytes out of and into every rank; an
AllGather of B bytes per rank writes as many per rank.  A number for the record
(DESIGN.md §3.2); it sets no pass mark.  Not the xGMI number: all ranks share
one GPU's HBM (tools/vnode_bench.py), so the relay's extra link traffic costs
here only its extra FIFO copies.

  python tools/a2a_bench.py [--n 8] [--sizes-kib 64 1024] [--out FILE.jsonl]
  python tools/a2a_bench.py --v [--out FILE.jsonl]
  python tools/a2a_bench.py --v --dev [--out FILE.jsonl]
  python tools/a2a_bench.py --p2p [--out FILE.jsonl]
  python tools/a2a_bench.py --ll [--n 4 6 8] [--sizes-kib 1 8 64] [--out FILE.jsonl]

--v: AllToAllv beside AllToAll.  Per size one process alternates a
uniform-count AllToAllv with an AllToAll of the same bytes, five repeats of
each, and reports both ranges, the ratio of the medians and AllToAll's own
spread (max / min: the margin the ratio is read against); then a skewed matrix
of the same total bytes per rank (a circulant of weights 1 3 0 1 0 2 0 1 ...
times the size, zeros included), and the uniform matrix without the self
block, whose works have one element and ride in the launch arguments.

--v --dev: AllToAllvDev (the sizes in a table on the device) beside the
host-count AllToAllv with a self block, the yardstick: both queue two elements
per channel and take the work FIFO, so the difference is the table reads.
Uniform counts; per size one process alternates the yardstick, the eager Dev
call and a replayed graph holding exchange_counts and the Dev call, five
repeats of each, and reports the three ranges, the ratios of the medians and the
yardstick's own spread (max / min), the margin the ratios are read against.

--p2p: Send/Recv beside AllToAllv.  The pattern is a ring shift: every rank
sends one message to rank + 1 and receives one from rank - 1, as one group per
call.  The yardstick is mccsAllToAllv with the same sparse matrix (what a
caller had to use before).  Per message size one process alternates the two,
five repeats of each, and reports both ranges, the ratio of the medians and the
yardstick's own spread (max / min), the margin the ratio is read against.

--ll: the LL all-to-all (mccsCommSetAllToAllLL) beside the ring.  Per size one
process alternates the ring AllToAll (the yardstick) and the LL AllToAll on the
same communicators, eagerly and as replayed one-launch graphs, and then a
skewed AllToAllvDev (a circulant of weights 1 3 0 1 0 2 0 1 ... times a third
of the size, zeros included) as a replayed graph, ring beside LL (6 ranks have
no one-hop route: LL only); five repeats of each.  It reports every range, the
ratios of the medians and the ring AllToAll's own spread (max / min), the
margin the ratios are read against.

Every (n, size, mode) step runs in a fresh child process under its own time
limit; the first step that fails or runs out of time ends the run.
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def step(n, kib, iters):
    """One step: AllToAll (the route the environment selects) and AllGather, the ring at every size."""
    import torch

    from mccs_amd import comm as C

    comms = C.init_all([0] * n, C.CommConfig(direct_bytes=-1, oneshot_bytes=-1, ll_bytes=-1))
    B = kib << 10
    xs = [torch.randint(0, 255, (n * B,), dtype=torch.uint8, device="cuda") for _ in range(n)]
    ys = [torch.empty(n * B, dtype=torch.uint8, device="cuda") for _ in range(n)]
    calls = {
        "alltoall": lambda r: C.all_to_all(comms[r], xs[r], ys[r], B),
        "allgather": lambda r: C.all_gather(comms[r], xs[r], ys[r], B),
    }
    out = {"n": n, "KiB_per_peer": kib, "lanes": comms[0].lanes, "channels": comms[0].nchannels, "iters": iters,
           **comms[0].all_to_all_route()}

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
    out["alltoall_over_allgather"] = round(out["alltoall_us"] / out["allgather_us"], 2)
    torch.cuda.synchronize()
    for c in comms:
        c.destroy()
    print(json.dumps(out), flush=True)


def step_v(n, kib, iters, repeats=5):
    """One --v step: uniform AllToAllv and AllToAll alternating, then the skewed matrix."""
    import statistics

    import torch

    from mccs_amd import comm as C

    comms = C.init_all([0] * n, C.CommConfig(direct_bytes=-1, oneshot_bytes=-1, ll_bytes=-1))
    B = kib << 10
    xs = [torch.randint(0, 255, (n * B,), dtype=torch.uint8, device="cuda") for _ in range(n)]
    ys = [torch.empty(n * B, dtype=torch.uint8, device="cuda") for _ in range(n)]
    weights = ([1, 3, 0, 1, 0, 2, 0, 1] * n)[:n]
    weights[0] += n - sum(weights)  # every row and column still sums to n * B
    skew = [[B * weights[(t - s) % n] for t in range(n)] for s in range(n)]
    packed = lambda c: [sum(c[:i]) for i in range(n)]
    uni = [B] * n

    sz = lambda v: (ctypes.c_size_t * n)(*v)  # marshalled once: the loop times the library, not the wrapper

    def v_call(cnt):
        cols = [[cnt[s][r] for s in range(n)] for r in range(n)]
        a = [(sz(cnt[r]), sz(packed(cnt[r])), sz(cols[r]), sz(packed(cols[r]))) for r in range(n)]
        return lambda r: C.all_to_all_v(comms[r], xs[r], a[r][0], a[r][1], ys[r], a[r][2], a[r][3])

    # no self block: one element per work, which rides in the launch arguments like the uniform call's
    noself = [[0 if s == t else B for t in range(n)] for s in range(n)]
    calls = {"alltoall": lambda r: C.all_to_all(comms[r], xs[r], ys[r], B),
             "alltoallv_uniform": v_call([uni] * n), "alltoallv_skewed": v_call(skew),
             "alltoallv_noself": v_call(noself)}

    def run(call, k):
        for _ in range(k):
            with C.group():
                for r in range(n):
                    call(r)
        for c in comms:
            c.sync()
        torch.cuda.synchronize()

    times = {k: [] for k in calls}
    for call in calls.values():
        run(call, 2)
    for _ in range(repeats):
        for name, call in calls.items():  # alternating, in one process
            t0 = time.perf_counter()
            run(call, iters)
            times[name].append(round((time.perf_counter() - t0) / iters * 1e6, 1))
    med = {k: statistics.median(v) for k, v in times.items()}
    out = {"bench": "a2av", "n": n, "KiB_per_peer": kib, "lanes": comms[0].lanes, "channels": comms[0].nchannels,
           "iters": iters, "repeats": repeats, **comms[0].all_to_all_route()}
    for k, v in times.items():
        out[k + "_us"] = [min(v), med[k], max(v)]  # min, median, max of the repeats
    out["v_uniform_over_alltoall"] = round(med["alltoallv_uniform"] / med["alltoall"], 3)
    out["v_skewed_over_alltoall"] = round(med["alltoallv_skewed"] / med["alltoall"], 3)
    out["v_noself_over_alltoall"] = round(med["alltoallv_noself"] / med["alltoall"], 3)
    out["alltoall_spread"] = round(max(times["alltoall"]) / min(times["alltoall"]), 3)
    torch.cuda.synchronize()
    for c in comms:
        c.destroy()
    print(json.dumps(out), flush=True)


def step_dev(n, kib, iters, repeats=5):
    """One --v --dev step: host-count AllToAllv (self block), AllToAllvDev eager, and
    exchange_counts + AllToAllvDev in a replayed graph, alternating."""
    import statistics

    import torch

    from mccs_amd import comm as C

    comms = C.init_all([0] * n, C.CommConfig(direct_bytes=-1, oneshot_bytes=-1, ll_bytes=-1))
    B = kib << 10
    xs = [torch.randint(0, 255, (n * B,), dtype=torch.uint8, device="cuda") for _ in range(n)]
    ys = [torch.empty(n * B, dtype=torch.uint8, device="cuda") for _ in range(n)]
    disp = [t * B for t in range(n)]
    sz = lambda v: (ctypes.c_size_t * n)(*v)  # marshalled once: the loop times the library, not the wrapper
    a = (sz([B] * n), sz(disp))
    tabs = [torch.tensor([B] * n + disp + [B] * n + disp, dtype=torch.int64, device="cuda") for _ in range(n)]
    tptr = [t.data_ptr() for t in tabs]
    torch.cuda.synchronize()

    def grouped(call):
        with C.group():
            for r in range(n):
                call(r)

    host = lambda r: C.all_to_all_v(comms[r], xs[r], a[0], a[1], ys[r], a[0], a[1])
    dev = lambda r: C.all_to_all_v_dev(comms[r], xs[r], ys[r], tptr[r])
    grouped(host)
    grouped(dev)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        grouped(lambda r: C.exchange_counts(comms[r], tptr[r]))
        grouped(dev)
    calls = {"alltoallv_host_self": lambda: grouped(host), "alltoallv_dev": lambda: grouped(dev),
             "alltoallv_dev_graph_with_exchange": g.replay}

    def run(call, k):
        for _ in range(k):
            call()
        for c in comms:
            c.sync()
        torch.cuda.synchronize()

    times = {k: [] for k in calls}
    for call in calls.values():
        run(call, 2)
    for _ in range(repeats):
        for name, call in calls.items():  # alternating, in one process
            t0 = time.perf_counter()
            run(call, iters)
            times[name].append(round((time.perf_counter() - t0) / iters * 1e6, 1))
    med = {k: statistics.median(v) for k, v in times.items()}
    out = {"bench": "a2avd", "n": n, "KiB_per_peer": kib, "lanes": comms[0].lanes, "channels": comms[0].nchannels,
           "iters": iters, "repeats": repeats, **comms[0].all_to_all_route()}
    for k, v in times.items():
        out[k + "_us"] = [min(v), med[k], max(v)]  # min, median, max of the repeats
    out["dev_over_host"] = round(med["alltoallv_dev"] / med["alltoallv_host_self"], 3)
    out["dev_graph_over_host"] = round(med["alltoallv_dev_graph_with_exchange"] / med["alltoallv_host_self"], 3)
    out["host_spread"] = round(max(times["alltoallv_host_self"]) / min(times["alltoallv_host_self"]), 3)
    for r in range(n):  # the exchanged row 2 is still the uniform count
        assert tabs[r].tolist() == [B] * n + disp + [B] * n + disp, r
    del g
    torch.cuda.synchronize()
    for c in comms:
        c.destroy()
    print(json.dumps(out), flush=True)


def step_p2p(n, kib, iters, repeats=5):
    """One --p2p step: a ring shift as one Send/Recv group per call, and the
    AllToAllv of the same sparse matrix (the yardstick), alternating."""
    import statistics

    import torch

    from mccs_amd import comm as C

    comms = C.init_all([0] * n, C.CommConfig(direct_bytes=-1, oneshot_bytes=-1, ll_bytes=-1))
    B = kib << 10
    xs = [torch.randint(0, 255, (B,), dtype=torch.uint8, device="cuda") for _ in range(n)]
    ys = [torch.empty(B, dtype=torch.uint8, device="cuda") for _ in range(n)]
    xp, yp = [x.data_ptr() for x in xs], [y.data_ptr() for y in ys]
    sz = lambda v: (ctypes.c_size_t * n)(*v)  # marshalled once: the loop times the library, not the wrapper
    zero = sz([0] * n)
    sc = [sz([B if t == (r + 1) % n else 0 for t in range(n)]) for r in range(n)]
    rc = [sz([B if s == (r - 1) % n else 0 for s in range(n)]) for r in range(n)]
    u8 = int(C.AllReduceDataType.Uint8)
    # looked up once, like the sizes: the wrapper's default-stream lookup costs as much per call as the library
    # does, and the shift makes two calls per rank where the yardstick makes one
    st = torch.cuda.current_stream().cuda_stream
    torch.cuda.synchronize()

    def shift(r):
        C.send(comms[r], xp[r], B, u8, (r + 1) % n, stream=st)
        C.recv(comms[r], yp[r], B, u8, (r - 1) % n, stream=st)

    calls = {"alltoallv_sparse": lambda r: C.all_to_all_v(comms[r], xp[r], sc[r], zero, yp[r], rc[r], zero, stream=st),
             "sendrecv_shift": shift}

    def run(call, k):
        for _ in range(k):
            with C.group():
                for r in range(n):
                    call(r)
        for c in comms:
            c.sync()
        torch.cuda.synchronize()

    for call in calls.values():
        run(call, 2)
        for r in range(n):
            assert torch.equal(ys[r], xs[(r - 1) % n]), r
            ys[r].zero_()
    times = {k: [] for k in calls}
    for _ in range(repeats):
        for name, call in calls.items():  # alternating, in one process
            t0 = time.perf_counter()
            run(call, iters)
            times[name].append(round((time.perf_counter() - t0) / iters * 1e6, 1))
    med = {k: statistics.median(v) for k, v in times.items()}
    out = {"bench": "sendrecv", "pattern": "ring shift", "n": n, "KiB_per_message": kib, "lanes": comms[0].lanes,
           "channels": comms[0].nchannels, "iters": iters, "repeats": repeats, **comms[0].all_to_all_route()}
    for k, v in times.items():
        out[k + "_us"] = [min(v), med[k], max(v)]  # min, median, max of the repeats
    out["sendrecv_over_alltoallv"] = round(med["sendrecv_shift"] / med["alltoallv_sparse"], 3)
    out["alltoallv_spread"] = round(max(times["alltoallv_sparse"]) / min(times["alltoallv_sparse"]), 3)
    torch.cuda.synchronize()
    for c in comms:
        c.destroy()
    print(json.dumps(out), flush=True)


def step_ll(n, kib, iters, repeats=5):
    """One --ll step: ring and LL AllToAll, eager and replayed, and the skewed Dev replay, alternating."""
    import statistics

    import torch

    from mccs_amd import comm as C

    comms = C.init_all([0] * n, C.CommConfig(direct_bytes=-1, oneshot_bytes=-1))  # ll_bytes: the default
    B = kib << 10
    cap = comms[0].all_to_all_ll_max()
    assert B <= cap, (B, cap)
    one_hop = comms[0].all_to_all_route()["hops"] == 1
    xs = [torch.randint(0, 255, (n * B,), dtype=torch.uint8, device="cuda") for _ in range(n)]
    ys = [torch.empty(n * B, dtype=torch.uint8, device="cuda") for _ in range(n)]
    xp, yp = [x.data_ptr() for x in xs], [y.data_ptr() for y in ys]
    weights = ([1, 3, 0, 1, 0, 2, 0, 1] * n)[:n]
    skew = [[B // 3 * weights[(t - s) % n] for t in range(n)] for s in range(n)]
    packed = lambda c: [sum(c[:i]) for i in range(n)]
    tabs = []
    for r in range(n):
        col = [skew[s][r] for s in range(n)]
        tabs.append(torch.tensor(skew[r] + packed(skew[r]) + col + packed(col), dtype=torch.int64, device="cuda"))
    tptr = [t.data_ptr() for t in tabs]
    torch.cuda.synchronize()

    def limits(uniform, v):
        for c in comms:
            c.set_all_to_all_ll(bytes_per_peer=uniform, v_bytes_per_peer=v)

    def grouped(call):
        with C.group():
            for r in range(n):
                call(r)

    # (the current stream is looked up per call: inside a capture it is the capturing one)
    a2a = lambda r: C.all_to_all(comms[r], xp[r], yp[r], B)
    dev = lambda r: C.all_to_all_v_dev(comms[r], xp[r], yp[r], tptr[r])

    def capture(call, uniform, v, algo):
        limits(uniform, v)
        grouped(call)  # once eagerly
        assert comms[0].last_algo() == algo, (comms[0].last_algo(), algo)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            grouped(call)
        return g

    def eager(uniform, algo):
        def run_one():
            grouped(a2a)
        return (uniform, algo, run_one)

    graphs = {"alltoall_ring_graph": capture(a2a, 0, 0, "ring"), "alltoall_ll_graph": capture(a2a, cap, 0, "ll"),
              "a2avd_skewed_ll_graph": capture(dev, 0, cap, "ll")}
    if one_hop:
        graphs["a2avd_skewed_ring_graph"] = capture(dev, 0, 0, "ring")
    want = [y.clone() for y in ys]  # the skewed ring (or LL) result, to hold the LL replay to
    calls = {"alltoall_ring": eager(0, "ring"), "alltoall_ll": eager(cap, "ll")}
    calls.update({k: (None, None, g.replay) for k, g in graphs.items()})

    def run(name, k):
        uniform, algo, call = calls[name]
        if uniform is not None:
            limits(uniform, 0)
        for _ in range(k):
            call()
        if algo is not None:
            assert comms[0].last_algo() == algo, (name, comms[0].last_algo())
        for c in comms:
            c.sync()
        torch.cuda.synchronize()

    for name in calls:
        run(name, 2)
    run("a2avd_skewed_ll_graph", 1)
    for r in range(n):
        assert torch.equal(ys[r], want[r]), r
    times = {k: [] for k in calls}
    for _ in range(repeats):
        for name in calls:  # alternating, in one process
            t0 = time.perf_counter()
            run(name, iters)
            times[name].append(round((time.perf_counter() - t0) / iters * 1e6, 1))
    med = {k: statistics.median(v) for k, v in times.items()}
    out = {"bench": "a2a_ll", "n": n, "KiB_per_peer": kib, "ll_cap": cap, "lanes": comms[0].lanes,
           "channels": comms[0].nchannels, "iters": iters, "repeats": repeats, **comms[0].all_to_all_route()}
    for k, v in times.items():
        out[k + "_us"] = [min(v), med[k], max(v)]  # min, median, max of the repeats
    out["ll_over_ring"] = round(med["alltoall_ll"] / med["alltoall_ring"], 3)
    out["ll_graph_over_ring_graph"] = round(med["alltoall_ll_graph"] / med["alltoall_ring_graph"], 3)
    if one_hop:
        out["dev_ll_graph_over_ring_graph"] = round(med["a2avd_skewed_ll_graph"] / med["a2avd_skewed_ring_graph"], 3)
    out["ring_spread"] = round(max(times["alltoall_ring"]) / min(times["alltoall_ring"]), 3)
    out["ring_graph_spread"] = round(max(times["alltoall_ring_graph"]) / min(times["alltoall_ring_graph"]), 3)
    graphs.clear()
    calls.clear()
    torch.cuda.synchronize()
    for c in comms:
        c.destroy()
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[8])
    ap.add_argument("--sizes-kib", type=int, nargs="+", default=[64, 1024])
    ap.add_argument("--iters", type=int, default=200, help="timed calls per collective")
    ap.add_argument("--step-timeout", type=int, default=120, help="seconds per step")
    ap.add_argument("--out", default=None, help="also append the result lines to this file")
    ap.add_argument("--v", action="store_true", help="AllToAllv beside AllToAll (one hop only)")
    ap.add_argument("--dev", action="store_true", help="with --v: AllToAllvDev beside the host-count AllToAllv")
    ap.add_argument("--p2p", action="store_true", help="a Send/Recv ring shift beside the sparse AllToAllv")
    ap.add_argument("--ll", action="store_true", help="the LL all-to-all beside the ring (n 4 6 8, 1 8 64 KiB)")
    ap.add_argument("--step", type=int, nargs=2, default=None, help=argparse.SUPPRESS)  # child: n KiB
    args = ap.parse_args()
    if args.dev and not args.v:
        ap.error("--dev goes with --v")
    if (args.p2p or args.ll) and args.v or args.p2p and args.ll:
        ap.error("--p2p and --ll are modes of their own")
    if args.ll and not args.step:
        if args.n == [8]:
            args.n = [4, 6, 8]
        if args.sizes_kib == [64, 1024]:
            args.sizes_kib = [1, 8, 64]
    if args.step:
        (step_ll if args.ll else step_p2p if args.p2p else step_dev if args.v and args.dev else step_v if args.v else step)(
            args.step[0], args.step[1], args.iters)
        return 0
    for n in args.n:
        for kib in args.sizes_kib:
            for relay in ((False,) if args.v or args.p2p or args.ll else (False, True)):
                env = dict(os.environ)
                env.pop("MCCS_ALLTOALL_HOPS", None)
                if relay:
                    env["MCCS_ALLTOALL_HOPS"] = "relay"
                cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__),
                       "--step", str(n), str(kib), "--iters", str(args.iters)] + (["--v"] if args.v else []) + \
                      (["--dev"] if args.v and args.dev else []) + (["--p2p"] if args.p2p else []) + (["--ll"] if args.ll else [])
                r = subprocess.run(cmd, capture_output=True, text=True, env=env)
                lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
                if r.returncode != 0 or not lines:
                    print(f"step n={n} KiB={kib} relay={relay} failed (exit {r.returncode}); stopping\n"
                          f"{r.stdout[-2000:]}{r.stderr[-2000:]}", file=sys.stderr)
                    return 1
                print(lines[-1], flush=True)
                if args.out:
                    with open(args.out, "a") as f:
                        f.write(lines[-1] + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
