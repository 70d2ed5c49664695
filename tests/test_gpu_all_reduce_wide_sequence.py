"""GPU: the wide-accumulate AllReduce between the launches that share its slots,
E_IN, E_OUT, E_SELF, the parity and the launch count, on one set of
communicators at n = 2 and 3; every output is checked (wide calls:
tests/wide_ref.py; the others: tests/test_gpu_rooted_sequences.py's call_expected).
Wide LL, one-shot and two-shot calls with the average among them, each body
twice back to back, alternate with an fp32 one-shot, two-shot and LL AllReduce,
a direct ReduceScatter, an LL AllGather, direct Reduces with a moving root and
an oversized ring call, no sync in between: on one stream, on two streams, and
in a graph replayed three times with the inputs rewritten between replays.
"""
import numpy as np
import pytest

from mccs_amd import comm as C
import test_gpu_rooted_sequences as S
import vnode
import wide_ref

pytestmark = pytest.mark.gpu
DIRECT_DEFAULTS = True  # CFG sets every threshold

ONESHOT, LL_BYTES, TWOSHOT = 256 << 10, 32 << 10, 2 << 20
CFG = dict(buffer_size=S.BUFF, oneshot_bytes=ONESHOT, ll_bytes=LL_BYTES, direct_bytes=TWOSHOT)
F16, F32, BF16 = 6, 7, 9


def sequence(n):
    """S's call dicts plus `algo`, the kernel the call must take; avg: a wide PreMulSum with 1/n."""
    def call(kind, count, algo, code=F32, root=None, avg=False):
        return dict(kind=kind, code=code, op=4 if avg else 0, root=root, inplace=False, count=count, algo=algo,
                    op_arg=C.avg_op(code, n)[1] if avg else None)

    return [call("ar", 1000, "wide-ll", BF16), call("ar", 30000, "oneshot"), call("ar", 30011, "wide-oneshot", F16),
            call("rd", 3000, "oneshot", root=0), call("ar", 200001, "wide-direct", BF16), call("ar", 200000, "direct"),
            call("ar", 777, "wide-ll", BF16, avg=True), call("ar", 2000, "ll"),
            call("ar", 20000, "wide-oneshot", F16, avg=True), call("rs", 20000, "oneshot"),
            call("ar", 150000, "wide-direct", F16, avg=True), call("ag", 5000, "ll", 0),
            call("rd", 3000, "oneshot", root=1), call("ar", 600000, "ring"),
            call("ar", 5, "wide-ll", F16), call("ar", 8191, "wide-ll", BF16),
            call("ar", 131072, "wide-oneshot", BF16), call("ar", 9000, "wide-oneshot", BF16),
            call("rd", 3000, "oneshot", root=n - 1),
            call("ar", 1 << 20, "wide-direct", F16), call("ar", 131073, "wide-direct", F16)]


class Staged(S.Staged):
    """S.Staged with the call's op_arg, and the wide definition for the wide calls."""

    def issue(self, comms, stream=None):
        if not self.call["algo"].startswith("wide"):
            return super().issue(comms, stream)
        with C.group():
            for r in range(self.n):
                C.all_reduce(comms[r], self.bufs[r][0], self.bufs[r][1], self.call["count"], self.call["code"],
                             self.call["op"], stream=stream, op_arg=self.call["op_arg"])

    def check(self, orc, comm0, tag):
        if not self.call["algo"].startswith("wide"):
            return super().check(orc, comm0, tag)
        code, arg = self.call["code"], self.call["op_arg"]
        scalar = None if arg is None else np.array([arg], np.uint16).view(vnode.NPDT[code])[0]
        want = wide_ref.all_reduce(self.xs, code, scalar)
        for r in range(self.n):
            assert wide_ref.same(vnode.from_dev(self.bufs[r][2], code), want, code), (tag, self.call, r)


def _issue_all(items, comms, streams=(None,)):
    for i, s in enumerate(items):
        s.issue(comms, streams[i % len(streams)])
        assert comms[0].last_algo() == s.call["algo"], (i, s.call, comms[0].last_algo())


@pytest.mark.parametrize("setting", ["one stream", "two streams", "graph"])
@pytest.mark.parametrize("n", [2, 3])
def test_sequence(orc, n, setting):
    import torch

    comms = C.init_all([0] * n, C.CommConfig(timeout_ms=S.TIMEOUT_MS, **CFG))
    try:
        for c in comms:
            c.set_all_reduce_wide(ll_bytes=16 << 10, oneshot_bytes=ONESHOT, twoshot_bytes=TWOSHOT)
            c.set_reduce_scatter_direct(block_bytes=ONESHOT)
            c.set_rooted_direct(reduce_bytes=ONESHOT)
        rng = np.random.default_rng(n)
        items = [Staged(call, n, [S.call_input(call, n, rng) for _ in range(n)]) for call in sequence(n)]
        torch.cuda.synchronize()
        streams = (torch.cuda.current_stream(), torch.cuda.Stream()) if setting == "two streams" else (None,)
        # (the graph case too: a kernel's first launch loads its code object, which a capture cannot)
        _issue_all(items, comms, streams)
        S._finish(orc, comms, items, (setting, n))
        if setting == "graph":
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                _issue_all(items, comms)
            for rep in range(3):
                for s in items:
                    s.refill([S.call_input(s.call, n, rng) for _ in range(n)])
                torch.cuda.synchronize()
                g.replay()
                S._finish(orc, comms, items, (setting, n, rep))
            del g
    finally:
        vnode.destroy(comms)
