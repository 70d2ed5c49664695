"""GPU: the opt-in wide streamed ReduceScatter (csrc/direct_wide_stream.h) on the virtual node, bit for bit (NaN payloads
aside) against tests/wide_ref.py's AllReduce, sliced: block t on rank t, whatever the rounds.  Every run asserts
last_algo() == "wide-stream".  Helpers: tests/test_gpu_reduce_wide.py.
"""
import ctypes

import numpy as np
import pytest

from mccs_amd import _lib
from mccs_amd import comm as C
from mccs_amd._lib import MccsError
import test_gpu_all_reduce_wide_sequence as A
import test_gpu_reduce_wide as W
import test_gpu_rooted_sequences as S
import vnode
import wide_ref

pytestmark = pytest.mark.gpu
DIRECT_DEFAULTS = True  # the configurations below set every threshold

I32, F16, F32, BF16 = 2, 6, 7, 9
SUM, MAX, PREMULSUM = 0, 2, 4
BAND = 64
COUNTS = [1, 127, 128, 129, 256, 257, 3 * 128 + 5, 5 * 128]  # K = 1, 1, 1, 2, 2, 3, 4, 5 at 128 elements a round


def _comms(n, max_block, round_bytes, oneshot=256 << 10):
    comms = C.init_all([0] * n, C.CommConfig(ll_bytes=32 << 10, oneshot_bytes=oneshot, direct_bytes=1 << 20, timeout_ms=8000))
    assert all(c.reduce_scatter_wide_stream_max() == oneshot for c in comms)
    for c in comms if max_block is not None else []:
        c.set_reduce_scatter_wide_stream(max_block, round_bytes)
    return comms


def _banded(comms, xs, code, inplace, op=SUM, op_arg=None):
    """One grouped call; out of place into a frame of 0xA5 bytes, in place inside the send buffer, whose other blocks
    are the band.  Every rank's block against the definition, every other byte untouched."""
    import torch

    n, cnt = len(comms), xs[0].size // len(comms)
    send = [vnode.to_dev(x) for x in xs]
    frame = [torch.full((BAND + cnt * 2 + BAND,), 0xA5, dtype=torch.uint8, device="cuda") for _ in range(n)]
    recv = [send[r][r * cnt * 2:(r + 1) * cnt * 2] if inplace else frame[r][BAND:BAND + cnt * 2] for r in range(n)]
    with C.group():
        for r in range(n):
            C.reduce_scatter(comms[r], send[r], recv[r], cnt, code, op, op_arg=op_arg)
    assert [c.last_algo() for c in comms] == ["wide-stream"] * n
    for c in comms:
        c.sync()
    want = wide_ref.all_reduce(xs, code, W._scalar(code, op_arg))
    for r in range(n):
        tag = (n, code, cnt, inplace, op_arg, r)
        assert wide_ref.same(vnode.from_dev(recv[r], code), want[r * cnt:(r + 1) * cnt], code), tag
        got = vnode.from_dev(send[r], code)
        if inplace:
            got[r * cnt:(r + 1) * cnt] = xs[r][r * cnt:(r + 1) * cnt]
        assert got.tobytes() == xs[r].tobytes(), ("send buffer written", tag)
        assert bool((frame[r][:BAND] == 0xA5).all() and (frame[r][-BAND:] == 0xA5).all()), ("band", tag)
        assert not inplace or bool((frame[r] == 0xA5).all()), ("frame", tag)


@pytest.mark.parametrize("code", [F16, BF16])
@pytest.mark.parametrize("n", [2, 3, 8])
def test_bits_across_the_round_structure(code, n):
    """Rounds of 256 bytes: one to five rounds, a full and a partial last one, odd counts (blocks off a pack)."""
    comms = _comms(n, 1 << 20, 256)
    try:
        rng = np.random.default_rng(n)
        for cnt in COUNTS:
            xs = [vnode.gen(code, cnt * n, rng) for _ in range(n)]
            for inplace in (False, True):
                _banded(comms, xs, code, inplace)
                _banded(comms, xs, code, inplace, PREMULSUM, C.avg_op(code, n)[1])
    finally:
        vnode.destroy(comms)


@pytest.mark.parametrize("code", [F16, BF16])
@pytest.mark.parametrize("blocks", ["1", "3"])
def test_bits_with_idle_workgroups(monkeypatch, code, blocks):
    """Communicators held to one and three workgroups.  Rounds of 256 bytes run on one workgroup either way (G comes
    from one round's bytes); rounds of 8 KiB at n = 3 ask for four, so with three some workgroups hold no send or no
    fold piece in some rounds: the case the per-round acknowledgement exists for."""
    monkeypatch.setenv("MCCS_DIRECT_BLOCKS", blocks)
    rng = np.random.default_rng(7)
    for round_bytes, counts in ((256, [129, 3 * 128 + 5, 5 * 128]), (8192, [4097, 2 * 4096 + 5, 5 * 4096])):
        comms = _comms(3, 1 << 20, round_bytes)
        try:
            for cnt in counts:
                xs = [vnode.gen(code, cnt * 3, rng) for _ in range(3)]
                _banded(comms, xs, code, False)
                _banded(comms, xs, code, True, PREMULSUM, C.avg_op(code, 3)[1])
        finally:
            vnode.destroy(comms)


def test_above_the_old_cap_and_the_control():
    """One-shot slots of 64 KiB, the smallest there are, and whole-slot rounds: a block of 200 KiB + 2 bytes takes four
    rounds.  Element e holds 256 on rank e and 1 elsewhere: 264 streamed, while a communicator that never opted in
    takes the ring, which keeps 256 where that rank comes first."""
    from test_gpu_all_reduce_wide import _bits

    n, cnt = 8, (200 << 10) // 2 + 1
    xs = [np.resize(_bits(BF16, [256.0 if r == e else 1.0 for e in range(n)]), cnt * n) for r in range(n)]
    plain, comms = _comms(n, None, 0, 64 << 10), _comms(n, 1 << 20, 0, 64 << 10)
    try:
        assert comms[0].reduce_scatter_wide_max()[1] == 64 << 10 < cnt * 2
        assert np.any(wide_ref.widen(W._run(plain, "rs", xs, BF16, "ring", wide=False), BF16) == 256.0)
        assert np.all(wide_ref.widen(W._run(comms, "rs", xs, BF16, "wide-stream"), BF16) == 264.0)
        rng = np.random.default_rng(5)
        for code in (F16, BF16):
            W._run(comms, "rs", [vnode.gen(code, cnt * n, rng) for _ in range(n)], code, "wide-stream", avg=code == F16)
    finally:
        vnode.destroy(plain + comms)


def sequence(n):
    """Streamed ReduceScatters of K = 3, 2, 1, 4 (rounds of 8 KiB) between every other kind of direct launch."""
    def call(kind, count, algo, code=F32, root=None, avg=False):
        return dict(kind=kind, code=code, op=4 if avg else 0, root=root, inplace=False, count=count, algo=algo,
                    op_arg=C.avg_op(code, n)[1] if avg else None)

    def rs(k, code=BF16, avg=False):
        return call("rs", {1: 4000, 2: 4097, 3: 2 * 4096 + 77, 4: 3 * 4096 + 1}[k], "wide-stream", code, avg=avg)

    return [rs(3), call("ar", 30000, "oneshot"), rs(2, F16, True), call("rs", 1000, "wide-oneshot", BF16), rs(1),
            call("ar", 2000, "ll"), rs(4, F16), call("ar", 200000, "direct"), call("rd", 3000, "oneshot", root=0),
            rs(3, BF16, True), rs(4), rs(1, F16), rs(2), call("rd", 3000, "oneshot", root=n - 1), call("ar", 600000, "ring"),
            rs(2, F16), call("rd", 3000, "oneshot", root=1), rs(4, BF16, True)]


@pytest.mark.parametrize("setting", ["one stream", "two streams", "graph"])
@pytest.mark.parametrize("n", [2, 3])
def test_sequence(orc, n, setting):
    import torch

    comms = C.init_all([0] * n, C.CommConfig(timeout_ms=S.TIMEOUT_MS, **A.CFG))
    try:
        for c in comms:
            c.set_reduce_scatter_wide(0, 2048), c.set_reduce_scatter_wide_stream(1 << 20, 8192)
            c.set_rooted_direct(reduce_bytes=A.ONESHOT)
        rng = np.random.default_rng(n)
        items = [W.Staged(call, n, [S.call_input(call, n, rng) for _ in range(n)]) for call in sequence(n)]
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


def test_refusals_and_calls_that_plan_as_before():
    n = 2
    comms = _comms(n, 1 << 20, 256)
    try:
        for bad in (24, (256 << 10) + 16):  # not a multiple of 16; above the slot
            with pytest.raises(MccsError):
                comms[0].set_reduce_scatter_wide_stream(1 << 20, bad)
        rng = np.random.default_rng(3)
        W._run(comms, "rs", [vnode.gen(BF16, 300 * n, rng) for _ in range(n)], BF16, "wide-stream")  # nothing changed
        for code, op in ((F32, SUM), (BF16, MAX)):  # not this opt-in's: the ring, as before
            W._run(comms, "rs", [vnode.gen(code, 300 * n, rng) for _ in range(n)], code, "ring", wide=False, op=op)
        lib, h, cfg = _lib.load(), ctypes.c_void_p(), C.CommConfig().to_c(n)
        mine = (ctypes.c_char * lib.mccsConnectHandleSize())()
        assert lib.mccsCommSetupRank(ctypes.byref(h), 0, n, 0, ctypes.byref(cfg[0]), mine) == 0
        loose = C.Communicator(h.value)  # set up, never connected
        try:
            with pytest.raises(MccsError):
                loose.set_reduce_scatter_wide_stream(1 << 20)
        finally:
            loose.destroy()
    finally:
        vnode.destroy(comms)
