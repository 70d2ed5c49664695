#!/usr/bin/env python3
"""The reference-named kernels driven the way the reference host drives them,
one rank per process (a worker of tests/test_gpu_reference_driver.py).

  python -m torch.distributed.run --nproc-per-node 2 --master-addr 127.0.0.1 \
      --master-port 29513 tests/refdrv_worker.py

No communicator of this library is involved: mccs_amd/refdrive.py restates
the Rust service's host side (the SHM connector's SendBufMeta/RecvBufMeta +
FIFO layout, comm/device.rs, plan.rs's host-mapped work ring with rolling
acks, get_task_schema and launch_plan: grid = #channels, 544-thread blocks).

Each variant (reference ring with the FIFO at the sender, the reference
default; a rotated ring override with the FIFO at the receiver; both again
with every SendBufMeta / RecvBufMeta / FIFO in the reference's own SHM
memory: mlock'ed host pages registered mapped, transport/shm/buffer.rs:17-26,
cuda/alloc.rs:59-99) runs four
cases three times each on the same structures (conn->step persists across
launches, prims_simple.h:318-319,461) and then 1100 back-to-back launches,
so the 1024-entry work ring wraps and flow-controls on workFifoDone
(plan.rs:380-541).  Results are compared bit for bit with the oracle,
workFifoDone with doneAcks, and conn->step across ranks.

REFDRV_MODE selects one of the further modes instead (class Modes below):
allgather, batched, small, odd, edge, avg.  Unset: the run described above.
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

    from mccs_amd import refdrive
    from oracle import oracle as orc
    import vnode

    rank, n = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dev = int(os.environ.get("LOCAL_RANK", rank)) % torch.cuda.device_count()
    torch.cuda.set_device(dev)
    dist.init_process_group("gloo", rank=rank, world_size=n)

    def allgather(obj):
        out = [None] * n
        dist.all_gather_object(out, obj)
        return out

    if os.environ.get("REFDRV_BIG") == "1":
        return big_case(torch, dist, refdrive, orc, rank, n, dev, allgather)
    if os.environ.get("REFDRV_MODE"):
        return Modes(torch, dist, refdrive, orc, rank, n, dev, allgather).run(os.environ["REFDRV_MODE"])
    rot = list(range(1, n)) + [0]
    variants = [("ref_sender", 2, None, "sender", "device"),
                ("rotated_receiver", 2, [rot, rot[::-1]], "receiver", "device"),
                ("ref_sender_hostfifo", 2, None, "sender", "host"),
                ("rotated_receiver_hostfifo", 2, [rot, rot[::-1]], "receiver", "host")]
    results = {}
    stream = torch.cuda.Stream()
    for vname, nch, rings, loc, fifo in variants:
        rr = refdrive.RefDrivenRank(rank, n, dev, allgather, nch=nch, rings=rings, locality=loc, fifo=fifo)
        for code, count in ((6, 1 << 20), (7, (1 << 21) + 3), (2, 300007), (6, 777777)):
            rng = np.random.default_rng(count + rank)
            for rep in range(3):
                x = np.full(count, 2042 + rank, np.int32) if code == 2 else vnode.gen(code, count, rng)
                xs = allgather(x)
                send, recv = vnode.to_dev(x), vnode.to_dev(np.zeros_like(x))
                torch.cuda.synchronize()
                dist.barrier()
                rr.all_reduce(send.data_ptr(), recv.data_ptr(), count, code, 0, stream.cuda_stream)
                stream.synchronize()
                k, nthr, ring_used = rr.last_plan
                exp = orc.ring_allreduce(code, 0, xs, nchannels=k, nthreads=nthr, buff_size=rr.buff,
                                         ring_orders=ring_used)
                got = vnode.from_dev(recv, code)
                ok = bool(np.array_equal(got.view(np.uint8), exp.view(np.uint8))) and not rr.aborted()
                ok = ok and nthr == 544 and all(a == rr.ring.chan_next[c] for c, a in enumerate(rr.done_acks()))
                if code == 2:
                    ok = ok and int(exp[0]) == 2042 * n + n * (n - 1) // 2
                results[f"{vname}/dtype{code}/n{count}/rep{rep}"] = {"ok": ok, "steps": rr.steps()}
                del send, recv
        if vname == "ref_sender":
            # every (dtype, op) kernel the reference names, at a ragged count
            # that takes several passes and a tail per slice (the reference-
            # named kernels stream 16 packs per source, bf16 12, bytes 4:
            # a code path of their own, ring_kernel.h kRefUnroll)
            for code in range(10):
                for op in range(4):
                    count = 150001 + 17 * code + op
                    rng = np.random.default_rng(1000 * code + 10 * op + rank)
                    x = vnode.gen(code, count, rng)
                    xs = allgather(x)
                    send, recv = vnode.to_dev(x), vnode.to_dev(np.zeros_like(x))
                    torch.cuda.synchronize()
                    dist.barrier()
                    rr.all_reduce(send.data_ptr(), recv.data_ptr(), count, code, op, stream.cuda_stream)
                    stream.synchronize()
                    k, nthr, ring_used = rr.last_plan
                    exp = orc.ring_allreduce(code, op, xs, nchannels=k, nthreads=nthr, buff_size=rr.buff,
                                             ring_orders=ring_used)
                    got = vnode.from_dev(recv, code)
                    ok = bool(np.array_equal(got.view(np.uint8), exp.view(np.uint8))) and not rr.aborted()
                    results[f"{vname}/all_kernels/dtype{code}/op{op}"] = {"ok": ok, "steps": rr.steps()}
                    del send, recv
        # 1100 back-to-back 4 KiB launches (one channel, one work entry each):
        # the 1024-entry work ring wraps and the host waits on workFifoDone
        count = 1024
        x = np.full(count, 2042 + rank, np.int32)
        send, recv = vnode.to_dev(x), vnode.to_dev(np.zeros_like(x))
        torch.cuda.synchronize()
        dist.barrier()
        for _ in range(1100):
            rr.all_reduce(send.data_ptr(), recv.data_ptr(), count, 2, 0, stream.cuda_stream)
        stream.synchronize()
        got = vnode.from_dev(recv, 2)
        ok = bool(np.all(got == 2042 * n + n * (n - 1) // 2)) and not rr.aborted() and rr.ring.next_available > 1024
        results[f"{vname}/wrap1100"] = {"ok": ok, "steps": rr.steps()}
        rr.close(dist.barrier)
    allres = allgather(results)
    if rank == 0:
        merged = {}
        for k in results:
            steps = [r[k]["steps"] for r in allres]
            merged[k] = all(r[k]["ok"] for r in allres) and all(s == steps[0] for s in steps)
        print(json.dumps({"world": n, "cases": merged, "all_ok": all(merged.values()),
                          "final_steps": allres[0][k]["steps"]}), flush=True)
    dist.barrier()
    dist.destroy_process_group()


# comm_patterns_override: tests/test_gpu_ring.py's two channels whose orders do
# not start at rank 0 and are no rotations of each other, cut down to the world
OVERRIDE8 = [[3, 0, 6, 1, 7, 2, 5, 4], [4, 5, 2, 7, 1, 6, 0, 3]]
F16, F32, I32, I8 = 6, 7, 2, 0
NTHR_OF_BUCKET = {5000: 96, 10000: 160, 20000: 288, 40000: 544}  # get_task_schema, plan.rs:602-635


class Modes:
    """REFDRV_MODE = allgather | batched | small | odd | edge | avg: what plan.rs's
    host side does beyond one aligned AllReduce per plan (see each method).
    Every mode runs on the reference ring with the FIFO at the sender and on a
    two-channel ring override with the FIFO at the receiver.  After every
    stream.synchronize() the abort flag is read (set: exit 3, nothing more is
    issued) and workFifoDone is compared with the host's expectation on every
    channel; conn->step is compared across ranks at the end.  Nothing is
    retried."""

    def __init__(self, torch, dist, refdrive, orc, rank, n, dev, allgather):
        self.torch, self.dist, self.refdrive, self.orc = torch, dist, refdrive, orc
        self.rank, self.n, self.dev, self.allgather = rank, n, dev, allgather
        self.stream = torch.cuda.Stream()
        self.results, self.reached, self.calls = {}, {}, []

    # -- scaffolding ----------------------------------------------------------------
    def variants(self, host=False):
        ov = [[r for r in ring if r < self.n] for ring in OVERRIDE8]
        vs = [("ref_sender", None, "sender", "device"), ("override_receiver", ov, "receiver", "device")]
        if host:
            vs += [(name + "_hostfifo", rings, loc, "host") for name, rings, loc, _ in vs]
        return vs

    def open(self, variant, **kw):
        _, rings, loc, fifo = variant
        rr = self.refdrive.RefDrivenRank(self.rank, self.n, self.dev, self.allgather, nch=2, rings=rings,
                                         locality=loc, fifo=fifo, **kw)
        if not getattr(rr.lib.mccs_hip_launch_coll, "spied", False):  # record every launch by symbol
            real, calls = rr.lib.mccs_hip_launch_coll, self.calls

            def spy(func, dtype, op, comm, mask, work, grid, block, stream):
                calls.append((func, dtype, op, grid, block))
                return real(func, dtype, op, comm, mask, work, grid, block, stream)

            spy.spied = True
            rr.lib.mccs_hip_launch_coll = spy
        return rr

    def barrier(self):
        self.torch.cuda.synchronize()
        self.dist.barrier()

    def dev_bytes(self, x):
        return self.torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).copy()).cuda()

    def fill(self, nbytes):
        return self.torch.full((nbytes,), 0xA5, dtype=self.torch.uint8, device="cuda")

    def finish(self, rr, key, check):
        """Synchronize, stop on an abort, then run check() -> '' or what is wrong."""
        self.stream.synchronize()
        if rr.aborted():
            print(f"rank {self.rank}: abortFlag is set after {key}; stopping", flush=True)
            sys.exit(3)
        why = check() or ""
        done = rr.done_acks()
        if any(done[c] != rr.ring.chan_next[c] for c in range(rr.nch)):
            why += f" workFifoDone {done} != expected {rr.ring.chan_next}"
        self.results[key] = {"ok": not why, "why": why[:400], "steps": rr.steps()}

    def reach(self, key, ok):
        self.reached[key] = bool(ok)

    def run(self, mode):
        getattr(self, "mode_" + mode)()
        for k, ok in self.reached.items():
            self.results["reached/" + k] = {"ok": ok, "why": "" if ok else "not reached", "steps": []}
        allres = self.allgather(self.results)
        if self.rank == 0:
            merged, why = {}, {}
            for k in self.results:
                steps = [r[k]["steps"] for r in allres]
                merged[k] = all(r[k]["ok"] for r in allres) and all(s == steps[0] for s in steps)
                if not merged[k]:
                    why[k] = [r[k]["why"] for r in allres] + [str(steps)]
            print(json.dumps({"world": self.n, "mode": mode, "cases": merged, "all_ok": all(merged.values()),
                              "why": dict(list(why.items())[:6]), "reached": self.reached,
                              "launches": len(self.calls)}), flush=True)
        self.dist.barrier()
        self.dist.destroy_process_group()

    def oracle(self, code, op, xs, plan, rr):
        k, nthr, rings = plan
        return self.orc.ring_allreduce(code, op, xs, nchannels=k, nthreads=nthr, buff_size=rr.buff, ring_orders=rings)

    @staticmethod
    def same(got, exp):
        return "" if np.array_equal(np.ascontiguousarray(got).view(np.uint8),
                                    np.ascontiguousarray(exp).view(np.uint8)) else "result differs "

    # -- allgather --------------------------------------------------------------------
    def mode_allgather(self):
        """mccsKernel_AllGather_RING_SIMPLE_Sum_int8_t (all_gather.h:7-79): sizes
        from one byte to several loops, out of place and in place (send = recv +
        rank * nbytes: directSend), against the concatenation by rank index."""
        import vnode
        from mccs_amd import comm as C

        n, rank, rd = self.n, self.rank, self.refdrive
        inplace_seen = two_channels = 0
        for v in self.variants(host=True):
            rr, host = self.open(v), v[3] == "host"
            for nbytes in (1000, 65539) if host else (1, 13, 1000, 4096, 65539, 1 << 20, (5 << 20) + 3):
                xs = [np.random.default_rng([nbytes, r]).integers(0, 256, nbytes, dtype=np.uint8) for r in range(n)]
                exp = np.concatenate(xs)
                for inplace in (False, True):
                    # every byte of the output differs from the expectation before the call
                    recv = self.dev_bytes(~exp)
                    send = None
                    if inplace:
                        recv[rank * nbytes:(rank + 1) * nbytes].copy_(self.torch.from_numpy(xs[rank]))
                    else:
                        send = self.dev_bytes(xs[rank])
                    send_ptr = recv.data_ptr() + rank * nbytes if inplace else send.data_ptr()
                    self.barrier()
                    p = rr.all_gather(send_ptr, recv.data_ptr(), nbytes, self.stream.cuda_stream)

                    def check():
                        why = self.same(recv.cpu().numpy(), exp)
                        if send is not None and not np.array_equal(send.cpu().numpy(), xs[rank]):
                            why += "source modified "
                        k, nthr = C.task_schema(nbytes * n, 2)
                        if p.tasks != [(k, nthr, list(range(k)))] or self.calls[-1] != (rd.FUNC_ALLGATHER, 0, 0, k, nthr):
                            why += f"plan {p.tasks} launch {self.calls[-1]} "
                        return why

                    self.finish(rr, f"{v[0]}/ag/{nbytes}/{'in' if inplace else 'out'}", check)
                    inplace_seen += inplace
                    two_channels += p.grid == 2
            if host:
                rr.close(self.dist.barrier)
                continue
            # the reference's own check (allgather_proto): int32 2042 + r, 1 MiB per rank
            cnt = (1 << 20) // 4
            send, recv = self.dev_bytes(np.full(cnt, 2042 + rank, np.int32)), self.fill(n << 20)
            self.barrier()
            rr.all_gather(send.data_ptr(), recv.data_ptr(), 1 << 20, self.stream.cuda_stream)
            self.finish(rr, f"{v[0]}/ag/int32_fill", lambda: self.same(
                recv.cpu().numpy().view(np.int32), np.repeat(np.arange(2042, 2042 + n, dtype=np.int32), cnt)))
            # AllGathers and AllReduces alternating on the same structures: steps persist
            for rnd in range(3):
                nbytes, count = 65539, 70001
                gs = [np.random.default_rng([rnd, nbytes, r]).integers(0, 256, nbytes, dtype=np.uint8)
                      for r in range(n)]
                send, recv = self.dev_bytes(gs[rank]), self.fill(n * nbytes)
                self.barrier()
                rr.all_gather(send.data_ptr(), recv.data_ptr(), nbytes, self.stream.cuda_stream)
                self.finish(rr, f"{v[0]}/alternate{rnd}/ag", lambda: self.same(recv.cpu().numpy(), np.concatenate(gs)))
                xs = [vnode.gen(F32, count, np.random.default_rng([rnd, count, r])) * np.float32(0.7) for r in range(n)]
                send, recv = self.dev_bytes(xs[rank]), self.fill(4 * count)
                self.barrier()
                rr.all_reduce(send.data_ptr(), recv.data_ptr(), count, F32, 0, self.stream.cuda_stream)
                self.finish(rr, f"{v[0]}/alternate{rnd}/ar",
                            lambda: self.same(recv.cpu().numpy(), self.oracle(F32, 0, xs, rr.last_plan, rr)))
            rr.close(self.dist.barrier)
        # per device variant 7 sizes twice, the fill and 3 alternating; per host variant 2 sizes twice
        launched = sum(1 for c in self.calls if c[:3] == (rd.FUNC_ALLGATHER, 0, 0))
        self.reach("allgather_symbol_launched", launched == 2 * (14 + 1 + 3) + 2 * 4 and inplace_seen and two_channels)

    # -- batched ----------------------------------------------------------------------
    def mode_batched(self):
        """pre_launch_schedule's batch (plan.rs:111-169) through RefDrivenRank.plan:
        several AllReduce tasks in one launch, channels by running load, chained
        works, block = the largest nthreads."""
        import vnode

        n, rank = self.n, self.rank
        st = self.stream.cuda_stream
        for v in self.variants():
            rr = self.open(v, work_depth=64)  # step (c) walks to the ring's end with single launches
            override = v[1] is not None
            # (a) 12 fp32 Sum tasks of mixed sizes, 1000 + 7919 i, the two
            # one-channel tasks larger first: channel 0 then carries more
            # bytes than channel 1 and every two-channel task is selected
            # [1, 0] (in ascending order of i all of them get [0, 1])
            counts = [1000 + 7919 * i for i in (1, 0) + tuple(range(2, 12))]
            # vnode.gen's fp32 values are multiples of 2^-23 in [-1, 1): no sum
            # of two of them rounds, so every three-term sum is one rounding of
            # the exact value whatever the order.  Scaled by 0.7 the values
            # fill the mantissa and the summation order shows.
            xs = [[vnode.gen(F32, c, np.random.default_rng([c, r])) * np.float32(0.7) for r in range(n)]
                  for c in counts]
            send, recv = [self.dev_bytes(x[rank]) for x in xs], [self.fill(4 * c) for c in counts]
            self.barrier()
            p = rr.plan([(send[t].data_ptr(), recv[t].data_ptr(), counts[t], F32, 0) for t in range(12)], st)
            order_matters = []

            def check_fp():
                why = ""
                for t in range(12):
                    exp = self.oracle(F32, 0, xs[t], rr.last_tasks[t], rr)
                    if self.same(recv[t].cpu().numpy(), exp):
                        why += f"task {t} differs "
                    k, nthr, sel = p.tasks[t]
                    asc = self.oracle(F32, 0, xs[t], (k, nthr, [rr.rings[c] for c in sorted(sel)]), rr)
                    order_matters.append(not np.array_equal(asc, exp))
                if override and not any(order_matters):
                    why += "vacuous: ascending channel order gives the same values "
                return why

            self.finish(rr, f"{v[0]}/fp32x12", check_fp)
            nthrs = {nthr for _, nthr, _ in p.tasks}
            self.reach(f"{v[0]}/chained_work_mixed_block",
                       max(p.nworks) > 1 and {96, 544} <= nthrs and p.block == 544 and self.calls[-1][3:] == (2, 544))
            self.reach(f"{v[0]}/selection_not_identity", any(k == 2 and sel == [1, 0] for k, _, sel in p.tasks))
            if override:
                self.reach("override_order_decides_values", any(order_matters))
            # (b) 21 int32 tasks, two channels each: three works per channel
            counts = [16384 + 3 * t for t in range(21)]
            send = [self.dev_bytes(np.full(c, 2042 + rank + t, np.int32)) for t, c in enumerate(counts)]

            def int_plan(key):
                recv = [self.fill(4 * c) for c in counts]
                p = rr.plan([(send[t].data_ptr(), recv[t].data_ptr(), counts[t], I32, 0) for t in range(21)], st)

                def check():
                    bad = [t for t in range(21) if not np.all(
                        recv[t].cpu().numpy().view(np.int32) == n * (2042 + t) + n * (n - 1) // 2)]
                    return f"tasks {bad} differ " if bad else ""

                self.finish(rr, key, check)
                return p

            self.barrier()
            p = int_plan(f"{v[0]}/int32x21")
            self.reach(f"{v[0]}/ten_elements_per_work", p.nworks == [3, 3] and all(k == 2 for k, _, _ in p.tasks))
            # (c) single 4 KiB launches until the next plan's two first works are
            # the last but two entries of the ring: its four later works cross
            # the ring's end
            depth = rr.ring.depth
            x = self.dev_bytes(np.full(1024, 2042 + rank, np.int32))
            out = self.fill(4096)
            self.barrier()
            singles = 0
            while rr.ring.next_available % depth != depth - 4 and singles < 2 * depth:
                rr.all_reduce(x.data_ptr(), out.data_ptr(), 1024, I32, 0, st)
                singles += 1
            self.finish(rr, f"{v[0]}/singles", lambda: "" if np.all(
                out.cpu().numpy().view(np.int32) == 2042 * n + n * (n - 1) // 2) else "result differs")
            self.barrier()
            p = int_plan(f"{v[0]}/int32x21_across_ring_end")
            nexts = [w.header.workNext for _, w in p.works if not w.header.isLast]
            self.reach(f"{v[0]}/negative_workNext", p.start % depth == depth - 4 and min(nexts) < 0 < max(nexts))
            rr.close(self.dist.barrier)

    # -- small ------------------------------------------------------------------------
    def mode_small(self):
        """Buckets below nChannels * nranks elements (empty chunks) and the 96-,
        160-, 288- and 544-thread blocks of get_task_schema, in and out of place."""
        import vnode

        n, rank = self.n, self.rank
        planned = set()
        for v in self.variants():
            rr = self.open(v)
            for code in (F16, I32):
                es = vnode.ESIZE[code]
                for count in (1, n - 1, 7, 255) + tuple(b // es for b in NTHR_OF_BUCKET):
                    xs = [vnode.gen(code, count, np.random.default_rng([code, count, r])) for r in range(n)]
                    for inplace in (False, True):
                        send = self.dev_bytes(xs[rank])
                        recv = send if inplace else self.fill(count * es)
                        self.barrier()
                        rr.all_reduce(send.data_ptr(), recv.data_ptr(), count, code, 0, self.stream.cuda_stream)

                        def check():
                            k, nthr, _ = rr.last_plan
                            why = self.same(recv.cpu().numpy(), self.oracle(code, 0, xs, rr.last_plan, rr))
                            if k != 1 or nthr != NTHR_OF_BUCKET.get(count * es, 96) or self.calls[-1][3:] != (1, nthr):
                                why += f"plan {rr.last_plan} launch {self.calls[-1]} "
                            if not inplace and not np.array_equal(send.cpu().numpy(), xs[rank].view(np.uint8)):
                                why += "source modified "
                            return why

                        self.finish(rr, f"{v[0]}/dtype{code}/n{count}/{'in' if inplace else 'out'}", check)
                        planned.add(self.calls[-1][4])
            rr.close(self.dist.barrier)
        self.reach("nthr_96_160_288_544", planned == {96, 160, 288, 544})

    # -- odd --------------------------------------------------------------------------
    def mode_odd(self):
        """Misaligned user buffers (the typed fallback) between guard bands: the
        oracle bit for bit, the pads intact, the sources unchanged."""
        import footprint as F
        import vnode
        from footprint import Guarded
        from mccs_amd import comm as C
        from test_gpu_footprint import extra_element

        n, rank = self.n, self.rank
        st = self.stream.cuda_stream

        def plan_of(rr, nbytes):  # one task per plan: channels 0..k-1
            k, nthr = C.task_schema(nbytes, 2)
            return k, nthr, [rr.rings[c] for c in range(k)]

        for v in self.variants():
            rr = self.open(v)
            for code in (F16, F32, I8):
                es = vnode.ESIZE[code]
                offs = [0, es, 8, 16 - es]
                for count in (n * (16 // es) + 1, 4097):
                    xs = [vnode.gen(code, count, np.random.default_rng([code, count, r])) for r in range(n)]
                    plan = plan_of(rr, count * es)
                    exp = self.oracle(code, 0, xs, plan, rr)
                    for pattern in ("mixed", "one_rank", "inplace"):
                        if pattern == "mixed":  # every rank differently, send and receive differently
                            soff, roff = offs[(rank + 1) % 4], offs[(rank + 2) % 4]
                        elif pattern == "one_rank":
                            soff = roff = es if rank == 1 else 0
                        else:
                            soff = roff = offs[1 + rank % 3]
                        send = Guarded(count * es, soff, "cuda")
                        send.write(xs[rank])
                        recv = send
                        if pattern != "inplace":
                            recv = Guarded(count * es, roff, "cuda")
                            recv.prefill_not(exp)
                        self.barrier()
                        rr.all_reduce(send.ptr, recv.ptr, count, code, 0, st)

                        def check():
                            why = F.diff_message(recv.read(), exp) + recv.pads_message()
                            if recv is not send:
                                why += send.source_message()
                            if rr.last_plan != plan:
                                why += f" plan {rr.last_plan} != {plan}"
                            return why

                        self.finish(rr, f"{v[0]}/dtype{code}/n{count}/{pattern}", check)
            # control: one element more than the buffers are guarded for
            for code, count, off in ((F16, 4097, 0), (F32, 4097, 4)):
                es = vnode.ESIZE[code]
                xs = [vnode.gen(code, count + 1, np.random.default_rng([code, count, r, 1])) for r in range(n)]
                exp = self.oracle(code, 0, xs, plan_of(rr, (count + 1) * es), rr)
                send, recv = Guarded(xs[rank].nbytes, off, "cuda"), Guarded(count * es, off, "cuda")
                planted, where = extra_element(exp, count, es)
                send.write(xs[rank])
                recv.prefill_not(exp[:count])
                recv.poke(count * es, planted)
                self.barrier()
                rr.all_reduce(send.ptr, recv.ptr, count + 1, code, 0, st)
                seen = []

                def check():
                    seen.append(recv.check().tolist())
                    why = "" if seen[0] == where else f"control reports {seen[0][:8]}, not {where} "
                    return why + F.diff_message(recv.read(), exp[:count]) + send.source_message()

                self.finish(rr, f"{v[0]}/control/dtype{code}", check)
                self.reach(f"{v[0]}/control_reports_extra_bytes/dtype{code}", seen[0] == where and len(where) == es)
            rr.close(self.dist.barrier)

    # -- edge -------------------------------------------------------------------------
    def mode_edge(self):
        """All 40 AllReduce kernels on each type's edge values (signed zeros,
        subnormals, ties, overflow, NaNs, integer wrap): rank 0 holds x, rank 1
        holds y; expected from the FIFO simulation under the independent functor."""
        import types

        import elem_ref as E
        import vnode
        from test_gpu_edge_values import expected_ring, pair_case

        assert self.n == 2
        kernels = set()
        for v in self.variants():
            rr = self.open(v)
            shim = types.SimpleNamespace(nchannels=rr.nch, rings=lambda rr=rr: rr.rings)
            for code in range(10):
                for op in (E.SUM, E.PROD, E.MAX, E.MIN):
                    x, y, _ = pair_case(code, op)  # asserts >= 75 % non-NaN and the required result classes
                    inputs = [x, y]
                    send, recv = self.dev_bytes(inputs[self.rank]), self.fill(x.nbytes)
                    self.barrier()
                    rr.all_reduce(send.data_ptr(), recv.data_ptr(), x.size, code, op, self.stream.cuda_stream)

                    def check():
                        planned = vnode.Planner(rr.nch, rr.rings).select(x.nbytes, x.nbytes)
                        if tuple(planned) != tuple(rr.last_plan):
                            return f"plan {rr.last_plan} != {planned}"
                        exp = expected_ring(shim, inputs, code, op, v[0])[self.rank]
                        ok, live = E.same_bits(code, vnode.from_dev(recv, code), exp)
                        if ok and live >= 0.75:
                            return ""
                        bad = E.mismatches(code, vnode.from_dev(recv, code), exp)
                        return f"{bad.size} of {exp.size} differ, first at {bad[:5].tolist()}, live {live:.2f}"

                    self.finish(rr, f"{v[0]}/dtype{code}/op{op}", check)
                    kernels.add(self.calls[-1][:3])
            rr.close(self.dist.barrier)
        self.reach("all_40_kernels", kernels == {(4, code, op) for code in range(10) for op in range(4)})

    # -- avg --------------------------------------------------------------------------
    def mode_avg(self):
        """The sixteen reference-named PreMulSum / SumPostDiv kernels, launched by
        symbol with the scalar in each element's redOpArg, bit for bit against
        tests/avg_ref.py: (a) edge values under both arguments of every pair,
        (b) at n = 3 the inputs on which a fused multiply-add would show, (c) the
        96-, 160-, 288- and 544-thread blocks in and out of place, (d) one plan
        whose elements carry different scalars, two in one work and one in a
        chained work, (e) misaligned buffers between guard bands, (f) six
        launches of alternating ops on the same buffers.  The cases and what
        makes each able to fail are tests/refdrv_avg_cases.py's, asserted there
        before anything is launched (and on the CPU by
        tests/test_refdrive_avg_cases.py)."""
        import avg_ref as A
        import refdrv_avg_cases as K
        import vnode
        from footprint import Guarded
        from mccs_amd import _lib
        from test_gpu_avg_values import diff

        n, rank, st = self.n, self.rank, self.stream.cuda_stream
        assert (K.OVERRIDE8, K.NTHR_OF_BUCKET) == (OVERRIDE8, NTHR_OF_BUCKET)
        lib = _lib.load()
        for code, op in A.PAIRS:
            assert lib.mccs_hip_coll_kernel(4, code, op), (code, op)
        for code in (6, 7, 8, 9):  # SumPostDiv is defined for the integer types only
            assert not lib.mccs_hip_coll_kernel(4, code, A.SUMPOSTDIV), code

        def one(rr, key, inputs, code, op, arg, exp, plan, inplace=False):
            """One AllReduce alone in its plan; the output starts as NOT(expected)."""
            x = inputs[rank]
            send = self.dev_bytes(x)
            recv = send if inplace else self.dev_bytes(~np.ascontiguousarray(exp[rank]).view(np.uint8))
            self.barrier()
            rr.all_reduce(send.data_ptr(), recv.data_ptr(), x.size, code, op, st, op_arg=arg)

            def check():
                why = ""
                if tuple(rr.last_plan) != tuple(plan) or self.calls[-1] != (4, code, op, plan[0], plan[1]):
                    why += f"plan {rr.last_plan} != {plan}, launch {self.calls[-1]} "
                why += diff(code, vnode.from_dev(recv, code), exp[rank])
                if not inplace and not np.array_equal(send.cpu().numpy(), np.ascontiguousarray(x).view(np.uint8)):
                    why += " source modified"
                return why

            self.finish(rr, key, check)

        swept, rounded, blocks, two_scalars, chained_scalar = [], [], set(), [], []
        for v in self.variants():
            rr = self.open(v)
            assert rr.buff == K.BUFF
            # (a) edge values, all sixteen pairs under both arguments
            kernels = set()
            for code, op, arg in K.edge_cases(n):
                inputs = K.edge_inputs(n, code)
                if n == 2:  # the last chunk ends in a typed tail
                    assert inputs[0].size % (16 // vnode.ESIZE[code]) != 0
                plan = K.plan_of(rr.rings, inputs[0].nbytes)
                exp = K.edge_expected(n, code, op, arg, plan, rr.buff)
                one(rr, f"{v[0]}/edge/dtype{code}/op{op}/{arg:x}", inputs, code, op, arg, exp, plan)
                kernels.add(self.calls[-1][:3])
            swept.append(kernels == {(4, code, op) for code, op in A.PAIRS})
            # (b) product and sum round separately
            if n == 3:
                for code in K.ROUNDING_CODES:
                    inputs = K.rounding_inputs(code)
                    plan = K.plan_of(rr.rings, inputs[0].nbytes)
                    exp, told_apart = K.rounding_expected(code, plan, rr.buff)
                    op, arg = A.avg_op(code, 3)
                    one(rr, f"{v[0]}/rounding/dtype{code}", inputs, code, op, arg, exp, plan)
                    rounded.append(self.calls[-1][:3] == (4, code, A.PREMULSUM) and min(told_apart) >= 0.10)
            # (c) every block size, out of place and in place
            for code, op, arg, nbytes, inputs in K.bucket_cases(n):
                plan = K.plan_of(rr.rings, nbytes)
                exp = K.bucket_expected(n, code, op, arg, nbytes, inputs, plan, rr.buff)
                for inplace in (False, True):
                    one(rr, f"{v[0]}/bucket/dtype{code}/{nbytes}/{'in' if inplace else 'out'}", inputs, code, op, arg,
                        exp, plan, inplace)
                    blocks.add((self.calls[-1][1], self.calls[-1][2], self.calls[-1][4], inplace))
            # (d) one plan, a scalar per element
            for code, op in K.BATCH_ARGS:
                tasks = K.batch_tasks(n, code, op)
                plans = K.batch_plans(rr.rings, code, op)
                exp = K.batch_expected(n, code, op, plans, rr.buff)
                send = [self.dev_bytes(inputs[rank]) for _, _, inputs in tasks]
                recv = [self.dev_bytes(~np.ascontiguousarray(e[rank]).view(np.uint8)) for e in exp]
                self.barrier()
                p = rr.plan([(send[t].data_ptr(), recv[t].data_ptr(), tasks[t][0], code, op, tasks[t][1])
                             for t in range(len(tasks))], st)

                def check():
                    why = ""
                    if [tuple(t) for t in rr.last_tasks] != [tuple(pl) for pl in plans] or \
                            self.calls[-1] != (4, code, op, 2, 544):
                        why += f"plan {rr.last_tasks} != {plans}, launch {self.calls[-1]} "
                    for t, (_, _, inputs) in enumerate(tasks):
                        d = diff(code, vnode.from_dev(recv[t], code), exp[t][rank])
                        if d:
                            why += f"task {t}: {d} "
                        if not np.array_equal(send[t].cpu().numpy(), np.ascontiguousarray(inputs[rank]).view(np.uint8)):
                            why += f"task {t}: source modified "
                    return why

                self.finish(rr, f"{v[0]}/batched/dtype{code}/op{op}", check)
                first, later = p.works[1][1], p.works[2][1]  # channel 1's works: (at, work) in upload order
                args = [arg for _, arg, _ in tasks]
                two_scalars.append(p.nworks == [1, 2] and not first.header.isLast and first.elems[2].isUsed == 0
                                   and [first.elems[i].redOpArg for i in range(2)] == args[1:3] and args[1] != args[2])
                chained_scalar.append(p.works[2][0] == p.start + 2 and p.works[1][1].header.workNext == 2
                                      and later.header.isLast and later.elems[0].redOpArg == args[3] != 0
                                      and later.elems[0].nWarps * 32 == 160 and self.calls[-1][4] == 544)
            # (e) both buffers one element past a 16-byte boundary, between guard bands
            for code, op, arg, inputs in K.odd_cases(n):
                es = vnode.ESIZE[code]
                plan = K.plan_of(rr.rings, K.ODD_COUNT * es)
                exp = K.odd_expected(n, code, op, arg, inputs, plan, rr.buff)
                for inplace in (False, True):
                    send = Guarded(K.ODD_COUNT * es, es, "cuda")
                    send.write(inputs[rank])
                    recv = send
                    if not inplace:
                        recv = Guarded(K.ODD_COUNT * es, es, "cuda")
                        recv.prefill_not(exp[rank])
                    assert send.ptr % 16 == es and recv.ptr % 16 == es
                    self.barrier()
                    rr.all_reduce(send.ptr, recv.ptr, K.ODD_COUNT, code, op, st, op_arg=arg)

                    def check():
                        why = diff(code, recv.read(vnode.NPDT[code]), exp[rank]) + " " + recv.pads_message()
                        if recv is not send:
                            why += send.source_message()
                        if tuple(rr.last_plan) != tuple(plan):
                            why += f" plan {rr.last_plan} != {plan}"
                        return why.strip()

                    self.finish(rr, f"{v[0]}/odd/dtype{code}/{'in' if inplace else 'out'}", check)
            # (f) six launches of four translation units' kernels on the same buffers
            inputs = K.sequence_inputs(n)
            plan = K.plan_of(rr.rings, inputs[0].nbytes)
            exps = K.sequence_expected(n, plan, rr.buff)
            send, recv = self.dev_bytes(inputs[rank]), self.fill(inputs[0].nbytes)
            for i, ((op, arg), exp) in enumerate(zip(K.SEQUENCE, exps)):
                self.barrier()
                rr.all_reduce(send.data_ptr(), recv.data_ptr(), K.SEQ_COUNT, K.I32, op, st, op_arg=arg)

                def check():
                    why = diff(K.I32, vnode.from_dev(recv, K.I32), exp[rank])
                    if tuple(rr.last_plan) != tuple(plan) or self.calls[-1] != (4, K.I32, op, plan[0], plan[1]):
                        why += f" plan {rr.last_plan} != {plan}, launch {self.calls[-1]}"
                    if not np.array_equal(send.cpu().numpy(), inputs[rank].view(np.uint8)):
                        why += " source modified"
                    return why

                self.finish(rr, f"{v[0]}/sequence/{i}/op{op}", check)
            rr.close(self.dist.barrier)
        self.reach("all_16_avg_kernels", len(swept) == 2 and all(swept))
        if n == 3:
            self.reach("rounding_fp16_bf16_fp32_fp64", len(rounded) == 8 and all(rounded))
        self.reach("avg_nthr_96_160_288_544",
                   blocks == {(code, op, nthr, inplace) for code, op in ((K.BF16, A.PREMULSUM), (K.I32, A.SUMPOSTDIV))
                              for nthr in NTHR_OF_BUCKET.values() for inplace in (False, True)})
        self.reach("two_scalars_in_one_work", len(two_scalars) == 4 and all(two_scalars))
        self.reach("scalar_in_chained_work", len(chained_scalar) == 4 and all(chained_scalar))


def big_case(torch, dist, refdrive, orc, rank, n, dev, allgather):
    """configs[2]'s bucket (128 MiB fp32 per rank), random uniform [-1, 1)
    inputs, reference-driven at the mccs.toml default (2 channels, ring
    0..n-1), at 32 channels, and at 2 channels on host-memory FIFOs (the
    reference SHM transport's own memory): every rank's output bit for bit against the
    oracle's ring order.  Each process regenerates every rank's inputs from
    the same seeds (no bulk exchange)."""
    import numpy as np

    count = (128 << 20) // 4
    g = torch.Generator(device="cuda")

    def inputs_of(r):
        g.manual_seed(9100 + r)
        return torch.rand(count, device="cuda", generator=g) * 2 - 1

    mine = inputs_of(rank)
    host = [inputs_of(r).cpu().numpy() for r in range(n)]
    stream = torch.cuda.Stream()
    results = {}
    for nch, fifo in ((2, "device"), (32, "device"), (2, "host")):
        rr = refdrive.RefDrivenRank(rank, n, dev, allgather, nch=nch, fifo=fifo)
        recv = torch.empty_like(mine)
        torch.cuda.synchronize()
        dist.barrier()
        rr.all_reduce(mine.data_ptr(), recv.data_ptr(), count, 7, 0, stream.cuda_stream)
        stream.synchronize()
        k, nthr, rings = rr.last_plan
        want = orc.ring_allreduce_mt(7, 0, host, nchannels=k, nthreads=nthr, buff_size=rr.buff, ring_orders=rings,
                                     workers=min(16, os.cpu_count() or 1))
        got = recv.cpu().numpy()
        naive = host[0].copy()
        for r in range(1, n):
            naive += host[r]
        results[f"big/ch{nch}/{fifo}"] = {"ok": bool(np.array_equal(got.view(np.uint32), want.view(np.uint32)))
                                   and not rr.aborted() and (n < 3 or not np.array_equal(naive, want)),
                                   "steps": rr.steps(), "grid": k, "block": nthr}
        rr.close(dist.barrier)
    allres = allgather(results)
    if rank == 0:
        merged = {k: all(r[k]["ok"] for r in allres) for k in results}
        print(json.dumps({"world": n, "cases": merged, "all_ok": all(merged.values()),
                          "plans": {k: [results[k]["grid"], results[k]["block"]] for k in results}}), flush=True)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
