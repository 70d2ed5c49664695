"""GPU: the opt-in wide-accumulate direct ReduceScatter and Reduce (csrc/direct_wide_rs.h) on the virtual node, bit for
bit (NaN payloads aside) against tests/wide_ref.py's AllReduce, sliced: block t on rank t, the whole array on the root.
Every run asserts last_algo().  LL slots for 32 KiB, one-shot slots of 256 KiB; pieces are 4 KiB (2048 elements) and up.
"""
import numpy as np
import pytest

from mccs_amd import comm as C
from mccs_amd._lib import MccsError
import test_gpu_all_reduce_wide_sequence as A
import test_gpu_rooted_sequences as S
import vnode
import wide_ref

pytestmark = pytest.mark.gpu
DIRECT_DEFAULTS = True  # the configurations below set every threshold

I32, F16, F32, BF16 = 2, 6, 7, 9
SUM, MAX, PREMULSUM, SUMPOSTDIV = 0, 2, 4, 5
CAPS = (32 << 10, 256 << 10)
BODIES = ["wide-ll", "wide-oneshot"]
WRAP = [8197, 131059]  # more words / pieces than 3 workgroups hold at once


def cases(f):
    for name, values in (("code", [F16, BF16]), ("body", BODIES), ("fn", ["rs", "rd"])):
        f = pytest.mark.parametrize(name, values)(f)
    return f


def _opt_in(comms, fn, limits):
    for c in comms:
        (c.set_reduce_scatter_wide if fn == "rs" else c.set_reduce_wide)(*limits)


def _comms(n, fn, body, **kw):
    comms = C.init_all([0] * n, C.CommConfig(ll_bytes=CAPS[0], oneshot_bytes=CAPS[1], direct_bytes=1 << 20,
                                             timeout_ms=8000, **kw))
    assert comms[0].reduce_scatter_wide_max() == CAPS and comms[0].reduce_wide_max() == CAPS
    _opt_in(comms, fn, [cap if body == b else 0 for b, cap in zip(BODIES, CAPS)])
    return comms


def _scalar(code, arg):
    return None if arg is None else np.array([arg], np.uint16).view(vnode.NPDT[code])[0]


def _run(comms, fn, xs, code, algo, wide=True, inplace=False, op=SUM, op_arg=None, root=0, avg=False):
    """One grouped call; xs[r] holds n blocks (rs) or the buffer (rd).  Returns rank 0's / the root's output."""
    n = len(comms)
    cnt = xs[0].size // n if fn == "rs" else xs[0].size
    send = [vnode.to_dev(x) for x in xs]
    owner = [fn == "rs" or r == root for r in range(n)]
    recv = [None if not owner[r] else vnode.to_dev(np.zeros(cnt, xs[0].dtype)) if not inplace
            else send[r][r * cnt * 2:(r + 1) * cnt * 2] if fn == "rs" else send[r] for r in range(n)]
    with C.group():
        for r in range(n):
            a = (comms[r], send[r], recv[r], cnt, code)
            if avg:
                C.reduce_scatter_avg(*a) if fn == "rs" else C.reduce_avg(*a, root)
            elif fn == "rs":
                C.reduce_scatter(*a, op, op_arg=op_arg)
            else:
                C.reduce(*a, op, root, op_arg=op_arg)
    assert [c.last_algo() for c in comms] == [algo] * n
    for c in comms:
        c.sync()
    want = wide_ref.all_reduce(xs, code, _scalar(code, C.avg_op(code, n)[1] if avg else op_arg)) if wide else None
    for r in range(n):
        assert inplace or vnode.from_dev(send[r], code).tobytes() == xs[r].tobytes(), ("send buffer written", r)
        if owner[r] and wide:
            lo = r * cnt if fn == "rs" else 0
            assert wide_ref.same(vnode.from_dev(recv[r], code), want[lo:lo + cnt], code), (fn, algo, cnt, inplace, op_arg, r)
    return vnode.from_dev(recv[0 if fn == "rs" else root], code).copy()


@pytest.mark.parametrize("n", [2, 3, 5, 8])
@cases
def test_counts_in_place_and_out_of_place(monkeypatch, fn, body, code, n):
    """The LL word (1, 3, 4, 5), the pack (7, 8, 9: odd blocks misalign every foreign block), one piece +- 1, the
    cap; the root moves with the case; then a deal that wraps, on communicators held to three workgroups."""
    top = CAPS[BODIES.index(body)] // 2
    for counts, blocks in (([1, 3, 4, 5, 7, 8, 9, 2047, 2049, top], None), ([WRAP[BODIES.index(body)]], "3")):
        if blocks:
            monkeypatch.setenv("MCCS_DIRECT_BLOCKS", blocks)
        comms = _comms(n, fn, body)
        try:
            rng = np.random.default_rng(n)
            for k, cnt in enumerate(counts):
                xs = [vnode.gen(code, cnt * (n if fn == "rs" else 1), rng) for _ in range(n)]
                for inplace in (False, True):
                    _run(comms, fn, xs, code, body, inplace=inplace, root=(n - 1 - k - inplace) % n)
            xs = [vnode.gen(code, (top + 1) * (n if fn == "rs" else 1), rng) for _ in range(n)]
            _run(comms, fn, xs, code, "ring", wide=False)  # one element above the cap: the ring, as before
        finally:
            vnode.destroy(comms)


@cases
def test_misaligned_send_and_recv_inside_sentinel_bands(fn, body, code):
    import torch

    n, cnt, band = 3, 4099, 32
    scnt = cnt * (n if fn == "rs" else 1)
    comms = _comms(n, fn, body)
    try:
        xs = [vnode.gen(code, scnt, np.random.default_rng(19)) for _ in range(n)]
        want = wide_ref.all_reduce(xs, code)
        send, recv = [[torch.empty(band + 16 + c * 2 + band, dtype=torch.uint8, device="cuda") for _ in range(n)]
                      for c in (scnt, cnt)]
        for a, b in [(a, b) for a in (2, 6, 14) for b in (2, 6, 14)]:
            root = (a + b) // 4 % n
            for r in range(n):
                send[r].fill_(0xA5)
                send[r][band + a:band + a + scnt * 2] = vnode.to_dev(xs[r])
                recv[r].fill_(0xA5)
            keep = [f.clone() for f in send]
            with C.group():
                for r in range(n):
                    ps, pr = send[r].data_ptr() + band + a, recv[r].data_ptr() + band + b
                    if fn == "rs":
                        C.reduce_scatter(comms[r], ps, pr, cnt, code, SUM)
                    else:  # one non-root passes its frame, the other NULL
                        C.reduce(comms[r], ps, None if r == (root + 2) % n else pr, cnt, code, SUM, root)
            assert comms[0].last_algo() == body
            for c in comms:
                c.sync()
            for r in range(n):
                lo, hi = band + b, band + b + cnt * 2
                if fn == "rs" or r == root:
                    w = want[r * cnt:(r + 1) * cnt] if fn == "rs" else want
                    assert torch.equal(recv[r][lo:hi], vnode.to_dev(w)), (a, b, r, "payload")
                else:
                    lo = hi  # a non-root's frame is untouched
                assert bool((recv[r][:lo] == 0xA5).all() and (recv[r][hi:] == 0xA5).all()), (a, b, r, "band")
                assert torch.equal(send[r], keep[r]), (a, b, r, "send buffer written")
    finally:
        vnode.destroy(comms)


@pytest.mark.parametrize("n", [3, 8])
@cases
def test_value_rows_sum_and_premulsum(fn, body, code, n):
    """tests/test_gpu_all_reduce_wide.py's eight value rows (exact in T) at the head of every block."""
    from test_gpu_all_reduce_wide import _bits

    tiny = 2.0 ** -24 if code == F16 else 2.0 ** -133  # the smallest subnormal of T
    over = [60000.0, 8000.0] if code == F16 else [(2 - 2.0 ** -7) * 2.0 ** 127, 1.5 * 2.0 ** 119]  # overflows T only
    rows = np.array([[256.0] + [1.0] * (n - 1), [np.inf, -np.inf] + [1.0] * (n - 2), [np.inf] + [1.0] * (n - 1),
                     [-0.0] * n, [-0.0, 0.0] + [-0.0] * (n - 2), [tiny] * n, [tiny, -tiny] + [tiny * 3] * (n - 2),
                     over + [0.0] * (n - 2)], np.float32)
    rng = np.random.default_rng(31)
    xs = [np.tile(np.concatenate([_bits(code, rows[:, r]), vnode.gen(code, 1000, rng)]), n if fn == "rs" else 1)
          for r in range(n)]
    comms = _comms(n, fn, body)
    try:
        w = wide_ref.widen(_run(comms, fn, xs, code, body, root=n - 1)[:8], code)
        assert np.isnan(w[1]) and np.isposinf(w[2]) and np.signbit(w[3]) and w[3] == 0 and not np.signbit(w[4])
        assert w[5] != 0 and np.isposinf(w[7]) and (code == F16 or w[0] == {3: 258.0, 8: 264.0}[n])
        # PreMulSum: 1/n (also through the _avg entry points), 0, and a bf16 scalar whose product underflows binary32
        for s in [C.avg_op(code, n)[1], 0] + ([int(_bits(BF16, [2.0 ** -120])[0])] if code == BF16 else []):
            _run(comms, fn, xs, code, body, op=PREMULSUM, op_arg=s, root=1)
        _run(comms, fn, xs, code, body, avg=True, root=2)
    finally:
        vnode.destroy(comms)


@pytest.mark.parametrize("fn", ["rs", "rd"])
def test_controls_and_refusals(fn):
    """Element e of each block holds 256 on rank e and 1 elsewhere: 264 wide, while the ring keeps 256 where that rank
    comes first.  Twisted rings, opted in to both kinds: the same wide bits; other dtypes and ops stay ring-order."""
    from test_gpu_all_reduce_wide import _bits

    n = 8
    xs = [np.tile(_bits(BF16, [256.0 if r == e else 1.0 for e in range(n)]), n if fn == "rs" else 1) for r in range(n)]
    rings = C.default_rings(8, 0)
    plain = _comms(n, fn, None)
    twisted = _comms(n, fn, None, rings=rings + [list(reversed(r)) for r in rings])
    try:
        assert twisted[0].nchannels == 14
        assert np.any(wide_ref.widen(_run(plain, fn, xs, BF16, "ring", wide=False, root=3), BF16) == 256.0)
        for c in twisted:
            c.set_reduce_scatter_direct(*reversed(CAPS))
            c.set_rooted_direct(0, 0, *reversed(CAPS))
        rng = np.random.default_rng(17)
        for k, (body, cnt) in enumerate(zip(BODIES, (5003, 28749))):
            with pytest.raises(MccsError):
                _opt_in(plain[:1], fn, [CAPS[j] + (j == k) for j in range(2)])
            _opt_in(twisted, fn, [cap if body == b else 0 for b, cap in zip(BODIES, CAPS)])
            assert np.all(wide_ref.widen(_run(twisted, fn, xs, BF16, body, root=3), BF16) == 264.0)
            for code in (F16, BF16):
                _run(twisted, fn, [vnode.gen(code, cnt * (n if fn == "rs" else 1), rng) for _ in range(n)], code, body, root=n - 1)
        _opt_in(twisted, fn, CAPS)
        for code, op, arg, algo in ((F32, SUM, None, "ll"), (BF16, MAX, None, "ll"), (I32, SUMPOSTDIV, n, "ring")):
            xs = [vnode.gen(code, 1000 * (n if fn == "rs" else 1), rng) for _ in range(n)]
            _run(twisted, fn, xs, code, algo, wide=False, op=op, op_arg=arg)
    finally:
        vnode.destroy(plain)
        vnode.destroy(twisted)


def sequence(n):
    """2n wide Reduces, root and body changing with every call; then wide ReduceScatters among the other launches."""
    def call(kind, count, algo, code=F32, root=None, avg=False):
        return dict(kind=kind, code=code, op=4 if avg else 0, root=root, inplace=False, count=count, algo=algo,
                    op_arg=C.avg_op(code, n)[1] if avg else None)

    return [call("rd", (777, 30011)[k % 2], BODIES[k % 2], (BF16, F16)[k % 2], root=k % n, avg=k % 3 == 0)
            for k in range(2 * n)] + [
        call("rs", 1000, "wide-ll", BF16), call("ar", 30000, "oneshot"), call("rs", 30011, "wide-oneshot", F16, avg=True),
        call("rd", 3000, "oneshot", root=0), call("ar", 20000, "wide-oneshot", BF16), call("ar", 200000, "direct"),
        call("rs", 5, "wide-ll", F16, avg=True), call("ar", 2000, "ll"), call("rs", 20000, "oneshot"),
        call("rd", 9, "wide-ll", BF16, root=n - 1), call("ag", 5000, "ll", 0), call("rd", 3000, "oneshot", root=1),
        call("ar", 600000, "ring"), call("rs", 131072 // n, "wide-oneshot", BF16), call("rs", 4097, "wide-ll", BF16),
        call("rd", 131072, "wide-oneshot", F16, root=0), call("rd", 3000, "oneshot", root=n - 1)]


class Staged(A.Staged):
    """A.Staged with the wide ReduceScatter / Reduce (Sum, or PreMulSum through op_arg) against the sliced definition."""

    def issue(self, comms, stream=None):
        c = self.call
        if c["kind"] == "ar" or c["op_arg"] is None:
            return (A.Staged if c["kind"] == "ar" else S.Staged).issue(self, comms, stream)
        with C.group():
            for r in range(self.n):
                a = (comms[r], self.bufs[r][0], self.bufs[r][1], c["count"], c["code"], c["op"])
                (C.reduce_scatter(*a, stream=stream, op_arg=c["op_arg"]) if c["kind"] == "rs" else
                 C.reduce(*a, c["root"], stream=stream, op_arg=c["op_arg"]))

    def check(self, orc, comm0, tag):
        c = self.call
        if c["kind"] == "ar" or not c["algo"].startswith("wide"):
            return super().check(orc, comm0, tag)
        want = wide_ref.all_reduce(self.xs, c["code"], _scalar(c["code"], c["op_arg"]))
        for r in [c["root"]] if c["kind"] == "rd" else range(self.n):
            lo = r * c["count"] if c["kind"] == "rs" else 0
            assert wide_ref.same(vnode.from_dev(self.bufs[r][2], c["code"]), want[lo:lo + c["count"]], c["code"]), (tag, c, r)


@pytest.mark.parametrize("setting", ["one stream", "two streams", "graph"])
@pytest.mark.parametrize("n", [2, 3])
def test_sequence(orc, n, setting):
    import torch

    comms = C.init_all([0] * n, C.CommConfig(timeout_ms=S.TIMEOUT_MS, **A.CFG))
    try:
        for c in comms:
            c.set_all_reduce_wide(oneshot_bytes=A.ONESHOT), c.set_reduce_wide(16 << 10, A.ONESHOT)
            c.set_reduce_scatter_wide(16 << 10, A.ONESHOT), c.set_reduce_scatter_direct(block_bytes=A.ONESHOT)
            c.set_rooted_direct(reduce_bytes=A.ONESHOT)
        rng = np.random.default_rng(n)
        items = [Staged(call, n, [S.call_input(call, n, rng) for _ in range(n)]) for call in sequence(n)]
        torch.cuda.synchronize()
        streams = (torch.cuda.current_stream(), torch.cuda.Stream()) if setting == "two streams" else (None,)
        A._issue_all(items, comms, streams)
        S._finish(orc, comms, items, (setting, n))
        if setting == "graph":
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                A._issue_all(items, comms)
            for rep in range(3):
                for s in items:
                    s.refill([S.call_input(s.call, n, rng) for _ in range(n)])
                torch.cuda.synchronize()
                g.replay()
                S._finish(orc, comms, items, (setting, n, rep))
            del g
    finally:
        vnode.destroy(comms)
