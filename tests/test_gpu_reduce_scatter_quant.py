"""GPU: the opt-in block-scaled FP8 streamed ReduceScatter (csrc/direct_quant_stream.h) on the virtual node, bit for bit
(NaN payloads aside) against tests/quant_rs_ref.py, whatever the rounds.  Every run asserts last_algo() == "quant-stream".
Helpers: tests/test_gpu_reduce_wide.py.
"""
import numpy as np
import pytest

from mccs_amd import comm as C
import quant_ref
import quant_rs_ref
import test_gpu_all_reduce_wide_sequence as A
import test_gpu_reduce_wide as W
import test_gpu_rooted_sequences as S
import vnode
import wide_ref

pytestmark = pytest.mark.gpu
DIRECT_DEFAULTS = True  # the configurations below set every threshold

F16, F32, BF16 = 6, 7, 9
SUM, PREMULSUM = 0, 4
BAND = 64
COUNTS = [1, 31, 33, 511, 512, 513, 1025, 3 * 512 + 37, 5 * 512]  # K = 1 (five times), 2, 3, 4, 5 at 512 elements a round


def _comms(n, max_block, round_bytes, oneshot=256 << 10):
    comms = C.init_all([0] * n, C.CommConfig(ll_bytes=32 << 10, oneshot_bytes=oneshot, direct_bytes=1 << 20, timeout_ms=8000))
    assert all(c.reduce_scatter_quant_max() == 2 * (oneshot * 32 // 33 // 512 * 512) for c in comms)
    for c in comms if max_block is not None else []:
        c.set_reduce_scatter_quant(max_block, 0, round_bytes)
    return comms


def _banded(comms, xs, code, inplace, op=SUM, op_arg=None):
    """One grouped call; out of place into a frame of 0xA5 bytes, in place inside the send buffer, whose other blocks
    are the band.  Every rank's block against the definition, every other byte untouched.  Returns the blocks."""
    import torch

    n, cnt = len(comms), xs[0].size // len(comms)
    send = [vnode.to_dev(x) for x in xs]
    frame = [torch.full((BAND + cnt * 2 + BAND,), 0xA5, dtype=torch.uint8, device="cuda") for _ in range(n)]
    recv = [send[r][r * cnt * 2:(r + 1) * cnt * 2] if inplace else frame[r][BAND:BAND + cnt * 2] for r in range(n)]
    with C.group():
        for r in range(n):
            C.reduce_scatter(comms[r], send[r], recv[r], cnt, code, op, op_arg=op_arg)
    assert [c.last_algo() for c in comms] == ["quant-stream"] * n
    for c in comms:
        c.sync()
    want = quant_rs_ref.reduce_scatter(xs, code, W._scalar(code, op_arg))
    out = [vnode.from_dev(recv[r], code).copy() for r in range(n)]
    for r in range(n):
        tag = (n, code, cnt, inplace, op_arg, r)
        assert wide_ref.same(out[r], want[r], code), tag
        got = vnode.from_dev(send[r], code)
        if inplace:
            got[r * cnt:(r + 1) * cnt] = xs[r][r * cnt:(r + 1) * cnt]
        assert got.tobytes() == xs[r].tobytes(), ("send buffer written", tag)
        assert bool((frame[r][:BAND] == 0xA5).all() and (frame[r][-BAND:] == 0xA5).all()), ("band", tag)
        assert not inplace or bool((frame[r] == 0xA5).all()), ("frame", tag)
    return out


@pytest.mark.parametrize("code", [F16, BF16])
@pytest.mark.parametrize("n", [2, 3, 8])
def test_bits_across_the_round_structure(code, n):
    """Rounds of one unit: one to five rounds, partial quantisation blocks and units, odd counts (blocks off a pack);
    then two units a round."""
    comms = _comms(n, 1 << 20, 1024)
    try:
        rng = np.random.default_rng(n)
        for cnt in COUNTS + [2 * 1024 + 5]:
            if cnt == 2 * 1024 + 5:
                for c in comms:
                    c.set_reduce_scatter_quant(1 << 20, 0, 2048)
            xs = [vnode.gen(code, cnt * n, rng) for _ in range(n)]
            for inplace in (False, True):
                _banded(comms, xs, code, inplace)
                _banded(comms, xs, code, inplace, PREMULSUM, C.avg_op(code, n)[1])
    finally:
        vnode.destroy(comms)


@pytest.mark.parametrize("blocks", ["1", "3"])
def test_bits_with_idle_workgroups(monkeypatch, blocks):
    """Communicators held to one and three workgroups; rounds of 8 KiB at n = 3 ask for four, so some workgroups hold
    no send or no fold piece in some rounds: the case the per-round acknowledgement exists for."""
    monkeypatch.setenv("MCCS_DIRECT_BLOCKS", blocks)
    rng = np.random.default_rng(7)
    comms = _comms(3, 1 << 20, 8192)
    try:
        for code in (F16, BF16):
            for cnt in (4097, 2 * 4096 + 5, 5 * 4096):
                xs = [vnode.gen(code, cnt * 3, rng) for _ in range(3)]
                _banded(comms, xs, code, False)
                _banded(comms, xs, code, True, PREMULSUM, C.avg_op(code, 3)[1])
    finally:
        vnode.destroy(comms)


def test_past_the_old_reach_and_the_control():
    """One-shot slots of 64 KiB and whole-slot rounds: a block of 150 Ki + 1 elements takes three rounds and is more
    than the wide one-shot's slot.  A communicator that never opted in takes the ring and returns other bits."""
    from test_gpu_all_reduce_wide import _bits

    n, cnt = 8, (150 << 10) + 1
    rng = np.random.default_rng(5)
    xs = [_bits(BF16, rng.standard_normal(cnt * n)) for _ in range(n)]
    plain, comms = _comms(n, None, 0, 64 << 10), _comms(n, 1 << 30, 0, 64 << 10)
    try:
        assert comms[0].reduce_scatter_wide_max()[1] == 64 << 10 < cnt * 2 and -(-cnt // (comms[0].reduce_scatter_quant_max() // 2)) == 3
        ring = W._run(plain, "rs", xs, BF16, "ring", wide=False)
        assert not wide_ref.same(ring, quant_rs_ref.reduce_scatter(xs, BF16)[0], BF16)  # the comparisons here are live
        _banded(comms, xs, BF16, False)
        _banded(comms, [vnode.gen(F16, cnt * n, rng) for _ in range(n)], F16, True, PREMULSUM, C.avg_op(F16, n)[1])
    finally:
        vnode.destroy(plain + comms)


@pytest.mark.parametrize("code", [F16, BF16])
def test_value_rows(code):
    """Rows of one quantisation block each (exact in T) at the head of every block, the same in every block of a rank:
    what is a foreign input for two owners is the own input of the third."""
    from test_gpu_all_reduce_wide import _bits

    n, ramp = 3, np.arange(32, dtype=np.float32)
    tiny = 2.0 ** -24 if code == F16 else 2.0 ** -133  # the smallest subnormal of T (bf16: b clamps to 1)
    rows = np.zeros((7, n, 32), np.float32)
    rows[0] = np.where(ramp % 2 == 0, -0.0, 0.0)             # zeros: -0 on every rank stays -0 ...
    rows[0, 0] = np.where((ramp % 2 == 0) | (ramp % 3 == 0), -0.0, 0.0)  # ... -0 on one rank alone gives +0
    rows[1] = ramp - 11
    rows[1, 1, 5] = np.inf                                    # rank 1's Inf: 32 NaN on owners 0 and 2, one Inf on 1
    rows[2] = ramp - 20
    rows[2, 0, 3] = np.nan                                    # rank 0's NaN: one NaN on owner 0, 32 on 1 and 2
    rows[3] = tiny * np.where(ramp % 2 == 0, ramp % 7, -(ramp % 5))  # an all-subnormal block
    rows[4, 2, 9] = 65504.0 if code == F16 else 65280.0       # the largest fp16; v = 255.875 rounds to 256
    rows[5, :2, 3] = [61440.0, 8192.0] if code == F16 else [(2 - 2.0 ** -7) * 2.0 ** 127, 1.5 * 2.0 ** 119]  # leaves T only
    rows[6] = (ramp - 16) / 8                                 # finite behind them
    rng = np.random.default_rng(31)
    xs = [np.tile(np.concatenate([_bits(code, rows[:, r].reshape(-1)), vnode.gen(code, 1000, rng)]), n) for r in range(n)]
    comms = _comms(n, 1 << 20, 1024)
    try:
        w = [wide_ref.widen(o[:7 * 32], code).reshape(7, 32) for o in _banded(comms, xs, code, False)]
        assert all(np.all(x[0] == 0) and np.any(np.signbit(x[0])) and not np.all(np.signbit(x[0])) for x in w)
        assert [int(np.isnan(x[1]).sum()) for x in w] == [32, 0, 32] and np.isposinf(w[1][1, 5]) and np.isfinite(w[1][1]).sum() == 31
        assert [int(np.isnan(x[2]).sum()) for x in w] == [1, 32, 32] and np.isnan(w[0][2, 3])
        assert all(np.any(x[3] != 0) and np.all(np.isfinite(x[6])) for x in w) and np.isposinf(w[0][5, 3])
        assert w[2][4, 9] == rows[4, 2, 9] and (code == BF16 or np.isposinf(w[0][4, 9]))  # exact on its owner
        for s in (C.avg_op(code, n)[1], 0):  # PreMulSum: 1/n (the average) and 0
            _banded(comms, xs, code, True, PREMULSUM, s)
    finally:
        vnode.destroy(comms)


class Staged(W.Staged):
    """W.Staged with the two FP8 definitions for the quant calls."""

    def check(self, orc, comm0, tag):
        c = self.call
        if not c["algo"].startswith("quant"):
            return super().check(orc, comm0, tag)
        s = W._scalar(c["code"], c["op_arg"])
        want = (quant_rs_ref.reduce_scatter(self.xs, c["code"], s) if c["kind"] == "rs"
                else [quant_ref.all_reduce(self.xs, c["code"], s)] * self.n)
        for r in range(self.n):
            assert wide_ref.same(vnode.from_dev(self.bufs[r][2], c["code"]), want[r], c["code"]), (tag, c, r)


def sequence(n):
    """FP8 ReduceScatters of K = 3, 2, 1, 4 (rounds of 8 KiB), back to back and between every other kind of launch."""
    def call(kind, count, algo, code=F32, root=None, avg=False):
        return dict(kind=kind, code=code, op=4 if avg else 0, root=root, inplace=False, count=count, algo=algo,
                    op_arg=C.avg_op(code, n)[1] if avg else None)

    def q(k, code=BF16, avg=False):
        return call("rs", {1: 4000, 2: 4097, 3: 2 * 4096 + 77, 4: 3 * 4096 + 1}[k], "quant-stream", code, avg=avg)

    return [q(3), q(2), q(1), q(4), call("ar", 30000, "oneshot"), q(3, F16, True), call("rs", 20000, "wide-stream", BF16),
            q(2), call("rs", 1000, "wide-oneshot", BF16), q(1, F16), call("ar", 2000, "ll"), q(4, BF16, True),
            call("ar", 200000, "direct"), q(3), call("ar", 200001, "quant-direct", BF16), q(2, F16),
            call("rd", 3000, "oneshot", root=n - 1), q(1), call("ar", 600000, "ring"), q(4, F16)]


@pytest.mark.parametrize("setting", ["one stream", "two streams", "graph"])
@pytest.mark.parametrize("n", [2, 3])
def test_sequence(orc, n, setting):
    import torch

    comms = C.init_all([0] * n, C.CommConfig(timeout_ms=S.TIMEOUT_MS, **A.CFG))
    try:
        for c in comms:
            c.set_reduce_scatter_wide(0, 2048), c.set_reduce_scatter_wide_stream(1 << 20, 8192)
            c.set_reduce_scatter_quant(25000, 8000, 8192), c.set_all_reduce_quant(600 << 10, 300 << 10)
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
