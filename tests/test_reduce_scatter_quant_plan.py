"""CPU: how the planner launches the opt-in block-scaled FP8 streamed ReduceScatter (csrc/direct_quant_stream.h), on the
recording fake device runtime (fixture and helpers: tests/test_reduce_scatter_direct_plan.py).  A held call's record is
kind=direct mode=quant-rs-stream with the count per block, pay= (the code bytes of a one-shot slot), rounds= and round=
(the elements of one round) and the scalar (op_arg, hex).
"""
import ctypes

import pytest

from mccs_amd import _lib
from mccs_amd import comm as C
from test_reduce_scatter_direct_plan import INVALID_ARGUMENT, _destroy, _launches, _recv, _refused, _send
from test_reduce_scatter_direct_plan import fake  # noqa: F401  (the fixture)
from test_reduce_wide_plan import BF16, CAP, F16, F32, HALF, LL_CAP, MAX, PREMULSUM, SUM, _call, _init

PAY = CAP * 32 // 33 // 512 * 512  # codes of one one-shot slot; the scale bytes lie behind them
QCAP = 2 * PAY                     # the largest round, in input bytes
ENV = ("MCCS_RS_QUANT_MIN_BYTES", "MCCS_RS_QUANT_BYTES", "MCCS_RS_QUANT_ROUND_BYTES")
PRE = "mccsCommSetReduceScatterQuant: "


def _set(comms, *limits):
    for c in comms:
        c.set_reduce_scatter_quant(*limits)


def _rounds(kv):
    return kv.get("mode"), int(kv.get("rounds", 0)), int(kv.get("round", 0))


@pytest.mark.parametrize("n", [2, 8])
def test_the_record_both_edges_and_the_precedence_over_the_wide_limits(fake, n):
    fake(1)
    comms = _init([0] * n)
    try:
        assert PAY + PAY // 32 <= CAP < QCAP and all(c.reduce_scatter_quant_max() == QCAP for c in comms)
        before = [_call("rs", comms, cnt) for cnt in (512, 5000)]
        assert before[0][0]["kind"] == "ring"  # not opted in
        _set(comms, 1 << 20, 64, 2048)
        for count, rounds in ((32, 1), (1024, 1), (1025, 2), (3 * 1024 + 5, 4), (1 << 19, 512)):
            for dtype, op, arg in ((BF16, SUM, None), (F16, PREMULSUM, 0x3800)):
                (kv,) = _call("rs", comms, count, dtype, op, arg)
                assert kv["kind"] == "direct" and _rounds(kv) == ("quant-rs-stream", rounds, 1024), kv
                assert kv["count"] == str(count) and kv["pay"] == str(PAY) and kv["op_arg"] == ("3800" if arg else "0")
                assert int(kv["piece"]) % 2048 == 0 and int(kv["piece2"]) % 2048 == 0 and kv["grid"] == f'{kv["gx"]}x{n}'
                assert all(c.last_algo() == "quant-stream" for c in comms)
        # one byte (so one element) outside either edge plans as before
        assert _call("rs", comms, 31)[0]["kind"] == "ring" and _call("rs", comms, (1 << 19) + 1)[0]["kind"] == "ring"
        _set(comms, 1 << 40)  # no cap on the block; round_bytes = 0 is the largest round
        assert _rounds(_call("rs", comms, PAY)[0]) == ("quant-rs-stream", 1, PAY)
        assert _rounds(_call("rs", comms, (1 << 32) + 1)[0]) == ("quant-rs-stream", (1 << 32) // PAY + 1, PAY)
        # inside its window the FP8 path wins over every wide limit; outside, the wide limits decide
        for c in comms:
            c.set_reduce_scatter_wide(LL_CAP, CAP), c.set_reduce_scatter_wide_stream(1 << 20)
        _set(comms, 8192, 4096)
        assert [_call("rs", comms, k)[0]["mode"] for k in (2047, 2048, 4096, 4097, CAP // 2 + 1)] == [
            "wide-rs-ll", "quant-rs-stream", "quant-rs-stream", "wide-rs-ll", "wide-rs-stream"]
        for c in comms:
            c.set_reduce_scatter_wide(0, 0), c.set_reduce_scatter_wide_stream(0)
        _set(comms, 0)  # off again: the records of before opting in
        assert [_call("rs", comms, cnt) for cnt in (512, 5000)] == before
    finally:
        _destroy(comms)


def test_other_calls_plan_as_before_and_a_grouped_pair_goes_to_the_ring_with_its_scalar(fake):
    fake(1)
    n = 4
    plain, comms = _init([0] * n), _init([0] * n)
    try:
        _set(comms, 1 << 30, 0, 4096)
        for fn, dtype, op in (("rs", F32, SUM), ("rs", BF16, MAX), ("rd", BF16, SUM)):  # not this opt-in's
            (want,), (kv,) = _call(fn, plain, 5000, dtype, op), _call(fn, comms, 5000, dtype, op)
            assert (kv["kind"], kv.get("mode"), kv["grid"]) == (want["kind"], want.get("mode"), want["grid"]) == \
                ("ring", None, want["grid"]) and comms[0].last_algo() == "ring"
        (want,) = _call("rs", plain, 5000, BF16, PREMULSUM, HALF, calls=2)
        (kv,) = _call("rs", comms, 5000, BF16, PREMULSUM, HALF, calls=2)
        assert kv["kind"] == "ring" and kv["redop_args"] == want["redop_args"] and "3f00" in kv["redop_args"]
        with C.group():  # the average of bf16 is PreMulSum with 1/n
            for r, c in enumerate(comms):
                C.reduce_scatter_avg(c, _send(r), _recv(r), 5000, BF16, stream=0)
        (kv,) = _launches()
        assert _rounds(kv) == ("quant-rs-stream", 3, 2048) and kv["op_arg"] == f"{C.avg_op(BF16, n)[1]:x}"
    finally:
        _destroy(plain + comms)
    comms = _init([0] * 9)  # outside 2..8 ranks there is no slot to stream through: the ring, and the opt-in is refused
    try:
        assert all(c.reduce_scatter_quant_max() == 0 for c in comms)
        _refused(INVALID_ARGUMENT, PRE + "max_block_bytes 64", lambda: _set(comms[:1], 64), ("closed here",))
        assert all(kv["kind"] == "ring" for kv in _call("rs", comms, 64))
    finally:
        _destroy(comms)


def test_the_environment_and_the_refusals(fake, monkeypatch):
    for name, v in zip(ENV, (2048, 1 << 30, (1 << 30) + 8)):  # read at creation; the round clamped to the cap
        monkeypatch.setenv(name, str(v))
    fake(1)
    comms = _init([0, 0])
    monkeypatch.setenv(ENV[2], "5000")  # cut to a multiple of 1024
    small = _init([0, 0])
    monkeypatch.setenv(ENV[2], "5")  # 1 .. 1023: the smallest round, not the largest
    small += _init([0, 0])
    for name in ENV:
        monkeypatch.delenv(name)
    others = _init([0, 0])
    c = others[0]
    try:
        assert _rounds(_call("rs", comms, PAY + 1)[0]) == ("quant-rs-stream", 2, PAY)
        assert _call("rs", comms, 1023)[0]["kind"] == "ring" and _call("rs", comms, (1 << 29) + 1)[0]["kind"] == "ring"
        assert _rounds(_call("rs", small[:2], 5000)[0]) == ("quant-rs-stream", 3, 2048)
        assert _rounds(_call("rs", small[2:], 1025)[0]) == ("quant-rs-stream", 3, 512)
        assert _call("rs", others, 4096)[0]["kind"] == "ring"  # created without the variables: off
        _refused(INVALID_ARGUMENT, PRE + "min_block_bytes 4097 is above max_block_bytes 4096", lambda: _set([c], 4096, 4097))
        _refused(INVALID_ARGUMENT, PRE + "round_bytes 1536 is not a multiple of 1024", lambda: _set([c], 4096, 0, 1536))
        _refused(INVALID_ARGUMENT, PRE + f"round_bytes {QCAP + 1024} is above the {QCAP} bytes",
                 lambda: _set([c], 4096, 0, QCAP + 1024))
        _set([c], 1 << 40, 1 << 40, QCAP), _set([c], 64, 64, 1024), _set([c], 0)  # the edges themselves are fine
        assert _call("rs", others, 4096)[0]["kind"] == "ring"  # the refused setters changed nothing
        lib, h, cfg = _lib.load(), ctypes.c_void_p(), C.CommConfig().to_c(2)
        mine = (ctypes.c_char * lib.mccsConnectHandleSize())()
        assert lib.mccsCommSetupRank(ctypes.byref(h), 0, 2, 0, ctypes.byref(cfg[0]), mine) == 0
        loose = C.Communicator(h.value)  # set up, never connected
        try:
            assert loose.reduce_scatter_quant_max() == 0
            _refused(INVALID_ARGUMENT, PRE + "the communicator is not connected", lambda: _set([loose], 64))
        finally:
            loose.destroy()
    finally:
        _destroy(comms + small + others)
