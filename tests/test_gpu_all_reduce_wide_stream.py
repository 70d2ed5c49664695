"""GPU: the opt-in wide streamed AllReduce (csrc/direct_wide_stream_ar.h) on the virtual node, bit for bit (NaN payloads
aside) against tests/wide_ref.py's AllReduce on every rank, whatever the rounds.  Every run asserts last_algo() ==
"wide-stream".  Helpers: tests/test_gpu_all_reduce_wide.py, tests/test_gpu_reduce_wide.py.
"""
import ctypes

import numpy as np
import pytest

from mccs_amd import _lib
from mccs_amd import comm as C
from mccs_amd._lib import MccsError
import test_gpu_all_reduce_wide as AW
import test_gpu_all_reduce_wide_sequence as A
import test_gpu_reduce_wide as W
import test_gpu_rooted_sequences as S
import vnode
import wide_ref

pytestmark = pytest.mark.gpu
DIRECT_DEFAULTS = True  # the configurations below set every threshold

F16, F32, BF16, SUM, MAX, PREMULSUM, BAND = 6, 7, 9, 0, 2, 4, 64


def _comms(n, max_bytes, round_bytes, oneshot=256 << 10, twoshot=1 << 20):
    comms = C.init_all([0] * n, C.CommConfig(ll_bytes=32 << 10, oneshot_bytes=oneshot, direct_bytes=twoshot, timeout_ms=8000))
    assert all(c.all_reduce_wide_stream_max() == min(oneshot, twoshot // 2) for c in comms)
    for c in comms if max_bytes is not None else []:
        c.set_all_reduce_wide_stream(max_bytes, round_bytes)
    return comms


def _banded(comms, xs, code, inplace, op=SUM, op_arg=None):
    """One grouped call into a frame of 0xA5 bytes (in place: from it too): every rank's output, bands, send buffer."""
    import torch

    n, cnt = len(comms), xs[0].size
    frame = [torch.full((BAND + cnt * 2 + BAND,), 0xA5, dtype=torch.uint8, device="cuda") for _ in range(n)]
    recv = [f[BAND:BAND + cnt * 2] for f in frame]
    send = [vnode.to_dev(x) for x in xs]
    for r in range(n) if inplace else []:
        recv[r].copy_(send[r])
    with C.group():
        for r in range(n):
            C.all_reduce(comms[r], recv[r] if inplace else send[r], recv[r], cnt, code, op, op_arg=op_arg)
    assert [c.last_algo() for c in comms] == ["wide-stream"] * n
    for c in comms:
        c.sync()
    want = wide_ref.all_reduce(xs, code, W._scalar(code, op_arg))
    for r in range(n):
        tag = (n, code, cnt, inplace, op_arg, r)
        assert wide_ref.same(vnode.from_dev(recv[r], code), want, code), tag
        assert vnode.from_dev(send[r], code).tobytes() == xs[r].tobytes(), ("send buffer written", tag)
        assert bool((frame[r][:BAND] == 0xA5).all() and (frame[r][-BAND:] == 0xA5).all()), ("band", tag)


@pytest.mark.parametrize("code", [F16, BF16])
@pytest.mark.parametrize("n", [2, 3, 8])
def test_bits_across_the_round_structure(code, n):
    """Rounds of 256 bytes: the smallest count that streams; one full round; two rounds with the last share exhausted
    in the first (n = 3: 385 -> 136 / 136 / 113); four rounds of an odd count; five rounds (each parity reused)."""
    comms = _comms(n, 1 << 20, 256)
    try:
        rng = np.random.default_rng(n)
        for cnt in (8 * n * (n - 1) + 1, 128 * n, 128 * n + 1, 3 * 128 * n + 5, 5 * 128 * n):
            xs = [vnode.gen(code, cnt, rng) for _ in range(n)]
            for inplace in (False, True):
                _banded(comms, xs, code, inplace)
                _banded(comms, xs, code, inplace, PREMULSUM, C.avg_op(code, n)[1])
    finally:
        vnode.destroy(comms)


@pytest.mark.parametrize("code", [F16, BF16])
@pytest.mark.parametrize("blocks", ["1", "3"])
def test_bits_with_idle_workgroups(monkeypatch, code, blocks):
    """Rounds of 8 KiB at n = 3 ask for four workgroups; held to three or one, some hold no piece of some leg in some
    rounds and still have to count, arrive and acknowledge.  Two, three and five rounds."""
    monkeypatch.setenv("MCCS_DIRECT_BLOCKS", blocks)
    rng = np.random.default_rng(7)
    comms = _comms(3, 1 << 20, 8192)
    try:
        for cnt in (3 * 4096 + 1, 3 * (2 * 4096 + 5), 3 * 5 * 4096):
            xs = [vnode.gen(code, cnt, rng) for _ in range(3)]
            _banded(comms, xs, code, False)
            _banded(comms, xs, code, True, PREMULSUM, C.avg_op(code, 3)[1])
    finally:
        vnode.destroy(comms)


def test_above_the_two_shot_cap_and_the_control():
    """Slots of 64 KiB, the smallest there are: one element above the wide two-shot's cap, whole-cap rounds, n = 8.
    Element e holds 256 on rank e and 1 elsewhere: 264 everywhere when streamed; the ring keeps 256 somewhere."""
    n, small = 8, 64 << 10
    plain, comms = _comms(n, None, 0, small, small), _comms(n, 1 << 20, 0, small, small)
    try:
        cnt = comms[0].all_reduce_wide_max()[2] // 2 + 1
        xs = [np.resize(AW._bits(BF16, [256.0 if r == e else 1.0 for e in range(n)]), cnt) for r in range(n)]
        assert all(np.any(wide_ref.widen(g, BF16) == 256.0) for g in AW._run(plain, xs, BF16, "ring"))
        assert all(np.all(wide_ref.widen(g, BF16) == 264.0) for g in AW._run(comms, xs, BF16, "wide-stream"))
    finally:
        vnode.destroy(plain + comms)


def sequence(n):
    """Streamed AllReduces of K = 3, 2, 1, 4 (rounds of 8 KiB) back to back and between every other kind of launch; the
    ring-order two-shot refills the in slots the streamed gather just used."""
    def call(kind, count, algo, code=F32, root=None, avg=False):
        return dict(kind=kind, code=code, op=4 if avg else 0, root=root, inplace=False, count=count, algo=algo,
                    op_arg=C.avg_op(code, n)[1] if avg else None)

    def ar(k, code=BF16, avg=False):
        count = {1: 3000 * n, 2: 4097 * n, 3: (2 * 4096 + 77) * n + 1, 4: (3 * 4096 + 1) * n}[k]
        return call("ar", count, "wide-stream", code, avg=avg)

    return [ar(3), ar(2, F16, True), ar(1), ar(4, F16), call("ar", 4000, "wide-direct", BF16), ar(3, BF16, True),
            call("ar", 200000, "direct"), ar(2), call("ar", 30000, "oneshot"), ar(1, F16), call("ar", 2000, "ll"), ar(4),
            call("rs", 4097, "wide-stream", BF16), ar(2, F16), call("rd", 3000, "oneshot", root=0), ar(1, BF16, True),
            call("rd", 3000, "oneshot", root=n - 1), call("ar", 600000, "ring"), ar(4, BF16, True),
            call("ar", 200000, "direct"), call("ar", 4000, "wide-direct", F16, avg=True), ar(3, F16)]


@pytest.mark.parametrize("setting", ["one stream", "two streams", "graph"])
@pytest.mark.parametrize("n", [2, 3])
def test_sequence(orc, n, setting):
    import torch

    comms = C.init_all([0] * n, C.CommConfig(timeout_ms=S.TIMEOUT_MS, **A.CFG))
    try:
        for c in comms:
            c.set_all_reduce_wide(twoshot_bytes=8192), c.set_all_reduce_wide_stream(1 << 20, 8192)
            c.set_reduce_scatter_wide_stream(1 << 20, 8192), c.set_rooted_direct(reduce_bytes=A.ONESHOT)
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
        for bad in (24, (256 << 10) + 16):  # not a multiple of 16; above the cap
            with pytest.raises(MccsError):
                comms[0].set_all_reduce_wide_stream(1 << 20, bad)
        rng = np.random.default_rng(3)
        ys = [vnode.gen(BF16, 300, rng) for _ in range(n)]
        AW._run(comms, ys, BF16, "wide-stream", wide_ref.all_reduce(ys, BF16))  # the refused setters changed nothing
        for code, op, cnt, algo in ((F32, SUM, 300, "ll"), (BF16, MAX, 300, "ll"), (BF16, SUM, 8 * n * (n - 1), "ll")):
            AW._run(comms, [vnode.gen(code, cnt, rng) for _ in range(n)], code, algo, op=op)  # not this opt-in's: as before
        lib, h, cfg = _lib.load(), ctypes.c_void_p(), C.CommConfig().to_c(n)
        mine = (ctypes.c_char * lib.mccsConnectHandleSize())()
        assert lib.mccsCommSetupRank(ctypes.byref(h), 0, n, 0, ctypes.byref(cfg[0]), mine) == 0
        loose = C.Communicator(h.value)  # set up, never connected
        try:
            with pytest.raises(MccsError):
                loose.set_all_reduce_wide_stream(1 << 20)
        finally:
            loose.destroy()
    finally:
        vnode.destroy(comms)
