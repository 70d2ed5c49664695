"""GPU: the opt-in block-scaled FP8 AllReduce (csrc/direct_quant.h) on the
virtual node, bit for bit (NaN payloads aside) against tests/quant_ref.py on
every rank: fp16 and bf16, Sum and PreMulSum.  Every run asserts last_algo().
A wave moves units of 512 elements and shares start on units; two-shot slots of
64 KiB hold PAY = 63488 codes, pieces are 2048 elements to 64 KiB of input.
"""
import numpy as np
import pytest

from mccs_amd import comm as C
from mccs_amd._lib import MccsError
import quant_ref
import test_gpu_all_reduce_wide_sequence as W
import test_gpu_rooted_sequences as S
import vnode

pytestmark = pytest.mark.gpu
DIRECT_DEFAULTS = True  # the configs below set every threshold

F16, F32, BF16 = 6, 7, 9
SUM, PREMULSUM = 0, 4
PAY = (64 << 10) * 32 // 33 // 512 * 512
each_dtype = pytest.mark.parametrize("code", [F16, BF16])


def _comms(n, direct_bytes=64 << 10, quant=True):
    comms = C.init_all([0] * n, C.CommConfig(ll_bytes=4 << 10, oneshot_bytes=16 << 10, direct_bytes=direct_bytes,
                                             timeout_ms=8000))
    cap = comms[0].all_reduce_quant_max()
    assert cap == 2 * (direct_bytes * 32 // 33 // 512 * 512)
    for c in comms:
        c.set_all_reduce_quant(cap if quant else 0)
    return comms


def _run(comms, inputs, code, algo="quant-direct", want=None, inplace=False, op=SUM, op_arg=None):
    """One grouped all_reduce, checked on every rank; out of place the send buffers must stay as they were."""
    n, cnt = len(comms), inputs[0].size
    send = [vnode.to_dev(x) for x in inputs]
    recv = send if inplace else [vnode.to_dev(np.zeros_like(x)) for x in inputs]
    with C.group():
        for r in range(n):
            C.all_reduce(comms[r], send[r], recv[r], cnt, code, op, op_arg=op_arg)
    assert [c.last_algo() for c in comms] == [algo] * n
    for c in comms:
        c.sync()
    got = [vnode.from_dev(t, code).copy() for t in recv]
    for r in range(n):
        assert inplace or vnode.from_dev(send[r], code).tobytes() == inputs[r].tobytes(), ("send buffer written", r)
        assert want is None or quant_ref.same(got[r], want, code), (algo, cnt, inplace, op_arg, r)
    return got


def _bits(code, values):
    """float values as T (fp16 arrays, bf16 raw bits; exact for the values used here)."""
    f = np.asarray(values, np.float32)
    return f.astype(np.float16) if code == F16 else (f.view(np.uint32) >> 16).astype(np.uint16)


@pytest.mark.parametrize("n", [2, 3, 8])
@each_dtype
def test_counts_in_place_and_out_of_place(monkeypatch, code, n):
    """The block (31, 32, 33), the unit (511, 512, 513), 512 n +- 1 (ranks that own nothing or one unit), a piece
    +- 1, the cap; then a deal that wraps, on communicators held to three workgroups (1 MiB slots)."""
    for counts, blocks, slot in (({1, 31, 32, 33, 511, 512, 513, 512 * n - 1, 512 * n + 1, 4095, 4097, PAY}, None, 64 << 10),
                                 ({500003}, "3", 1 << 20)):
        if blocks:
            monkeypatch.setenv("MCCS_DIRECT_BLOCKS", blocks)
        comms = _comms(n, slot)
        try:
            rng = np.random.default_rng(n)
            for cnt in sorted(counts):
                xs = [vnode.gen(code, cnt, rng) for _ in range(n)]
                for inplace in (False, True):
                    _run(comms, xs, code, want=quant_ref.all_reduce(xs, code), inplace=inplace)
            if not blocks:  # one element above the cap is above every threshold here: the ring, as without quant
                _run(comms, [vnode.gen(code, PAY + 1, rng) for _ in range(n)], code, "ring")
        finally:
            vnode.destroy(comms)


@each_dtype
def test_misaligned_send_and_recv_inside_sentinel_bands(code):
    import torch

    n, cnt, band = 3, 4099, 32
    comms = _comms(n)
    try:
        xs = [vnode.gen(code, cnt, np.random.default_rng(19)) for _ in range(n)]
        want = vnode.to_dev(quant_ref.all_reduce(xs, code))
        frames = [[torch.empty(band + 16 + cnt * 2 + band, dtype=torch.uint8, device="cuda") for _ in range(n)]
                  for _ in range(2)]
        for a, b in ((a, b) for a in (2, 6, 14) for b in (2, 6, 14)):
            for r in range(n):
                frames[0][r].fill_(0xA5)
                frames[0][r][band + a:band + a + cnt * 2] = vnode.to_dev(xs[r])
                frames[1][r].fill_(0xA5)
            keep = [f.clone() for f in frames[0]]
            with C.group():
                for r in range(n):
                    C.all_reduce(comms[r], frames[0][r].data_ptr() + band + a, frames[1][r].data_ptr() + band + b, cnt,
                                 code, SUM)
            assert comms[0].last_algo() == "quant-direct"
            for c in comms:
                c.sync()
            for r in range(n):
                lo, hi = band + b, band + b + cnt * 2
                assert torch.equal(frames[1][r][lo:hi], want), (a, b, r, "payload")
                assert bool((frames[1][r][:lo] == 0xA5).all() and (frames[1][r][hi:] == 0xA5).all()), (a, b, r, "band")
                assert torch.equal(frames[0][r], keep[r]), (a, b, r, "send buffer written")
    finally:
        vnode.destroy(comms)


@pytest.mark.parametrize("n", [2, 3, 8])
@each_dtype
def test_value_rows_sum_and_premulsum(code, n):
    """Rows of one block each (exact in T), the same on every rank unless said, with seeded data behind them."""
    tiny = 2.0 ** -24 if code == F16 else 2.0 ** -133  # the smallest subnormal of T (bf16: b clamps to 1)
    ramp = np.arange(32, dtype=np.float32)
    rows = np.zeros((9, n, 32), np.float32)
    rows[0] = np.where(ramp % 2 == 0, -0.0, 0.0)             # zeros: -0 on every rank stays -0 ...
    rows[0, 0] = np.where((ramp % 2 == 0) | (ramp % 3 == 0), -0.0, 0.0)  # ... -0 on one rank alone gives +0
    rows[1] = np.where(ramp == 7, 4.0, (ramp - 16) / 8)      # amax an exact power of two
    rows[2] = np.array([136.0, 152.0, 240.0, 17.0, 19.0, -136.0, -152.0, 34.0] * 4)  # ties: 17 -> 16, 19 -> 20
    rows[3] = 128.0 * np.array([1.0, 2.0 ** -17, 1.5 * 2.0 ** -17, -2.0 ** -16, 3 * 2.0 ** -16, -2.0 ** -17, 0.0, 2.0 ** -14] * 4)
    rows[4] = tiny * np.where(ramp % 2 == 0, ramp % 7, -(ramp % 5))  # a subnormal amax
    rows[5] = ramp - 11
    rows[5, 1 % n, 5] = np.inf                                # one Inf: 32 NaN ...
    rows[6] = ramp - 20                                       # ... and the block behind it untouched
    rows[7, :2, 3] = [61440.0, 8192.0]                        # the sum leaves fp16 only
    rows[8, :2, 9] = 1.5 * 2.0 ** 127 if code == BF16 else 60000.0  # bf16: the sum leaves binary32
    rng = np.random.default_rng(31)
    xs = [np.concatenate([_bits(code, rows[:, r].reshape(-1)), vnode.gen(code, 1000, rng)]) for r in range(n)]
    comms = _comms(n)
    try:
        w = quant_ref.widen(_run(comms, xs, code, want=quant_ref.all_reduce(xs, code))[0][:9 * 32], code).reshape(9, 32)
        assert np.all(w[0] == 0) and np.any(np.signbit(w[0])) and not np.all(np.signbit(w[0]))
        assert np.all(np.isnan(w[5])) and np.all(np.isfinite(w[6])) and np.any(w[4] != 0)
        assert np.isinf(w[7, 3]) == (code == F16) and np.all(np.isnan(w[8])) == (code == BF16)
        # PreMulSum: 1/n (the average) and 0
        assert C.avg_op(code, n)[0] == PREMULSUM
        for s in (C.avg_op(code, n)[1], 0):
            scalar = np.array([s], np.uint16).view(vnode.NPDT[code])[0]
            _run(comms, xs, code, want=quant_ref.all_reduce(xs, code, scalar), op=PREMULSUM, op_arg=s)
    finally:
        vnode.destroy(comms)


def test_a_communicator_that_never_opted_in_gives_other_bits():
    n, cnt = 4, 4096
    rng = np.random.default_rng(5)
    xs = [_bits(BF16, rng.standard_normal(cnt)) for _ in range(n)]
    plain = _comms(n, quant=False)
    try:
        got = _run(plain, xs, BF16, "oneshot")
        assert not quant_ref.same(got[0], quant_ref.all_reduce(xs, BF16), BF16)  # the comparisons above are live
        with pytest.raises(MccsError):
            plain[0].set_all_reduce_quant(2 * PAY + 1)
    finally:
        vnode.destroy(plain)


class Staged(W.Staged):
    """W.Staged with the quant definition for the quant calls."""

    def issue(self, comms, stream=None):
        if self.call["algo"] != "quant-direct":
            return super().issue(comms, stream)
        with C.group():
            for r in range(self.n):
                C.all_reduce(comms[r], self.bufs[r][0], self.bufs[r][1], self.call["count"], self.call["code"],
                             self.call["op"], stream=stream, op_arg=self.call["op_arg"])

    def check(self, orc, comm0, tag):
        if self.call["algo"] != "quant-direct":
            return super().check(orc, comm0, tag)
        code, arg = self.call["code"], self.call["op_arg"]
        scalar = None if arg is None else np.array([arg], np.uint16).view(vnode.NPDT[code])[0]
        want = quant_ref.all_reduce(self.xs, code, scalar)
        for r in range(self.n):
            assert quant_ref.same(vnode.from_dev(self.bufs[r][2], code), want, code), (tag, self.call, r)


@pytest.mark.parametrize("setting", ["one stream", "graph"])
@pytest.mark.parametrize("n", [2, 3])
def test_sequence_between_the_other_direct_launches(orc, n, setting):
    """Quant calls (window 300 .. 600 KiB) between a wide two-shot, a two-shot, a one-shot, an LL call and a ring
    call on one set of communicators, no sync in between; the graph is replayed three times on fresh inputs."""
    import torch

    def call(count, algo, code=F32, avg=False):
        return dict(kind="ar", code=code, op=4 if avg else 0, root=None, inplace=False, count=count, algo=algo,
                    op_arg=C.avg_op(code, n)[1] if avg else None)

    seq = [call(200001, "quant-direct", BF16), call(200000, "direct"), call(160000, "quant-direct", F16, avg=True),
           call(30000, "oneshot"), call(100000, "wide-direct", BF16), call(153601, "quant-direct", F16),
           call(2000, "ll"), call(600000, "ring"), call(299999, "quant-direct", BF16, avg=True),
           call(200001, "quant-direct", BF16)]
    comms = C.init_all([0] * n, C.CommConfig(timeout_ms=S.TIMEOUT_MS, **W.CFG))
    try:
        for c in comms:
            c.set_all_reduce_wide(twoshot_bytes=W.TWOSHOT)
            c.set_all_reduce_quant(600 << 10, 300 << 10)
        rng = np.random.default_rng(n)
        items = [Staged(c, n, [S.call_input(c, n, rng) for _ in range(n)]) for c in seq]
        torch.cuda.synchronize()
        W._issue_all(items, comms)
        S._finish(orc, comms, items, (setting, n))
        if setting == "graph":
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                W._issue_all(items, comms)
            for rep in range(3):
                for s in items:
                    s.refill([S.call_input(s.call, n, rng) for _ in range(n)])
                torch.cuda.synchronize()
                g.replay()
                S._finish(orc, comms, items, (setting, n, rep))
            del g
    finally:
        vnode.destroy(comms)
