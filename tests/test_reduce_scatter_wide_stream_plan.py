"""CPU: how the planner launches the opt-in wide streamed ReduceScatter (csrc/direct_wide_stream.h), on the recording
fake device runtime (fixture and helpers: tests/test_reduce_scatter_direct_plan.py).  A held call's record is kind=direct
mode=wide-rs-stream with the count per block, rounds= and round= (the elements of one round) and the scalar (op_arg,
hex); the slot strings and launch wiring are held by tests/test_reduce_wide_plan.py for the same builder.
"""
import ctypes

import pytest

from mccs_amd import _lib
from mccs_amd import comm as C
from test_reduce_scatter_direct_plan import INVALID_ARGUMENT, INVALID_USAGE, _destroy, _launches, _recv, _refused, _send
from test_reduce_scatter_direct_plan import fake  # noqa: F401  (the fixture)
from test_reduce_wide_plan import BF16, CAP, F16, F32, HALF, I32, LL_CAP, MAX, PREMULSUM, SUM, SUMPOSTDIV, _call, _init

ENV = ("MCCS_RS_WIDE_STREAM_BYTES", "MCCS_RS_WIDE_STREAM_ROUND_BYTES")
PRE = "mccsCommSetReduceScatterWideStream: "


def _set(comms, *limits):
    for c in comms:
        c.set_reduce_scatter_wide_stream(*limits)


def _rounds(kv):
    return kv["mode"], int(kv["rounds"]), int(kv["round"])


@pytest.mark.parametrize("n", [2, 3, 8])
def test_the_record_the_edge_and_the_other_wide_limits_first(fake, n):
    fake(1)
    comms = _init([0] * n)
    try:
        assert all(c.reduce_scatter_wide_stream_max() == CAP for c in comms)
        assert _call("rs", comms, 512)[0]["kind"] == "ring"  # the limit is still 0
        _set(comms, 1 << 20, 256)
        for count, rounds in ((1, 1), (128, 1), (129, 2), (3 * 128 + 5, 4), (1 << 19, 4096)):
            for dtype, op, arg in ((BF16, SUM, None), (F16, PREMULSUM, 0x3800)):
                (kv,) = _call("rs", comms, count, dtype, op, arg)
                assert kv["kind"] == "direct" and _rounds(kv) == ("wide-rs-stream", rounds, 128), kv
                assert kv["count"] == str(count) and kv["op_arg"] == ("3800" if op == PREMULSUM else "0")
                assert all(c.last_algo() == "wide-stream" for c in comms) and kv["grid"] == f'{kv["gx"]}x{n}'
        assert _call("rs", comms, (1 << 19) + 1)[0]["kind"] == "ring"  # one element above the limit
        _set(comms, 1 << 40)  # no cap on the block; round_bytes = 0 is the whole slot
        assert _rounds(_call("rs", comms, CAP // 2)[0]) == ("wide-rs-stream", 1, CAP // 2)
        assert _rounds(_call("rs", comms, (1 << 32) + 1)[0]) == ("wide-rs-stream", (1 << 33) // CAP + 1, CAP // 2)
        for c in comms:  # LL wins, then the one-shot, within THEIR limits; the stream takes what they leave
            c.set_reduce_scatter_wide(1024, 4096)
        assert [_call("rs", comms, k)[0]["mode"] for k in (512, 513, 2048, 2049)] == [
            "wide-rs-ll", "wide-rs-oneshot", "wide-rs-oneshot", "wide-rs-stream"]
        assert _call("rd", comms, 4096)[0]["kind"] == "ring" and _call("rs", comms, 0) == []
    finally:
        _destroy(comms)


def test_other_calls_plan_as_before_and_a_grouped_pair_goes_to_the_ring_with_its_scalar(fake):
    fake(1)
    n = 4
    plain, comms = _init([0] * n), _init([0] * n)
    try:
        for c in plain + comms:  # both sets opted in to the ring-order direct ReduceScatter
            c.set_reduce_scatter_direct(CAP, LL_CAP)
        _set(comms, 1 << 30, 4096)
        for dtype, op, arg in ((F32, SUM, None), (BF16, MAX, None), (I32, SUMPOSTDIV, n), (F32, PREMULSUM, 0x3F000000)):
            for count in (300, 1 << 18):
                (want,) = _call("rs", plain, count, dtype, op, arg)
                (kv,) = _call("rs", comms, count, dtype, op, arg)
                assert (kv["kind"], kv.get("mode")) == (want["kind"], want.get("mode")) and "wide" not in kv.get("mode", "")
        (want,) = _call("rs", plain, 5000, BF16, PREMULSUM, HALF, calls=2)
        (kv,) = _call("rs", comms, 5000, BF16, PREMULSUM, HALF, calls=2)
        assert kv["kind"] == "ring" and kv["redop_args"] == want["redop_args"] and "3f00" in kv["redop_args"]
        (kv,) = _call("rs", comms, 5000, BF16, PREMULSUM, HALF)  # a single call afterwards streams again
        assert _rounds(kv) == ("wide-rs-stream", 3, 2048) and kv["op_arg"] == "3f00"
        with C.group():  # the average of bf16 is PreMulSum with 1/n
            for r, c in enumerate(comms):
                C.reduce_scatter_avg(c, _send(r), _recv(r), 5000, BF16, stream=0)
        assert _launches()[0]["op_arg"] == f"{C.avg_op(BF16, n)[1]:x}" and comms[0].last_algo() == "wide-stream"
    finally:
        _destroy(plain + comms)
    for n in (1, 9):  # outside 2..8 ranks there is no slot to stream through: the ring, and the opt-in is refused
        comms = _init([0] * n)
        try:
            assert all(c.reduce_scatter_wide_stream_max() == 0 for c in comms)
            _refused(INVALID_ARGUMENT, PRE + "max_block_bytes 64", lambda: _set(comms[:1], 64), ("closed here",))
            assert all(kv["kind"] == "ring" for kv in _call("rs", comms, 64))
        finally:
            _destroy(comms)


def test_captured_fused_launches_and_the_environment(fake, monkeypatch):
    for name, v in zip(ENV, (1 << 20, (1 << 30) + 8)):  # read at creation; the round clamped and cut to 16
        monkeypatch.setenv(name, str(v))
    fake(2)
    lib = _lib.load()
    comms = _init([0, 0, 1, 1])
    monkeypatch.setenv(ENV[1], "1000")
    small = _init([0, 0])
    for name in ENV:
        monkeypatch.delenv(name)
    others = _init([0, 0])
    try:
        assert lib.mccs_test_fake_capture(0x5000, 9) == 0
        got = _call("rs", comms, CAP, stream=0x5000)
        assert lib.mccs_test_fake_capture(0x5000, 0) == 0
        # two devices, two fused rank slots each; a captured launch has no stop event
        assert len(got) == 2 and all(kv["grid"].endswith("x2") and kv["stop_event"] == "0" for kv in got)
        assert [_rounds(kv) for kv in got] == [("wide-rs-stream", 2, CAP // 2)] * 2
        assert [kv["slots"].split(":")[0] for kv in got] == ["0", "2"]
        lib.mccs_test_fake_destroy_graph(9)
        assert all(kv["stop_event"] != "0" for kv in _call("rs", comms, 1 << 19))
        assert _call("rs", comms, (1 << 19) + 1)[0]["kind"] == "ring"
        assert _rounds(_call("rs", small, 1000)[0]) == ("wide-rs-stream", 3, 992 // 2)
        monkeypatch.setenv(ENV[0], "4096"), monkeypatch.setenv(ENV[1], "5")  # 1 .. 15: the smallest round, not the slot
        small += _init([0, 0])
        assert _rounds(_call("rs", small[2:], 20)[0]) == ("wide-rs-stream", 3, 8)
        monkeypatch.delenv(ENV[0]), monkeypatch.delenv(ENV[1])
        assert _call("rs", others, 256)[0]["kind"] == "ring"  # created without the variables: off
        _set(comms[:1], 1 << 20, 4096)  # fused comms that disagree on the round go to the ring together (device 0)
        assert [kv["kind"] for kv in _call("rs", comms, CAP)] == ["ring", "direct"]
    finally:
        _destroy(comms + small + others)


def test_refusals(fake):
    fake(1)
    comms = _init([0, 0])
    c = comms[0]
    try:
        _refused(INVALID_ARGUMENT, PRE + "round_bytes 24 is not a multiple of 16", lambda: _set([c], 64, 24))
        _refused(INVALID_ARGUMENT, PRE + "round_bytes 8 is not a multiple of 16", lambda: _set([c], 64, 8))
        _refused(INVALID_ARGUMENT, PRE + f"round_bytes {CAP + 16} is above the {CAP} bytes of a one-shot slot",
                 lambda: _set([c], 64, CAP + 16))
        _set([c], 1 << 40, CAP), _set([c], 64, 16), _set([c], 0, 0)  # the edges themselves are fine

        def in_group():
            with C.group():
                _set([c], 64, 64)

        _refused(INVALID_USAGE, PRE + "the communicator has a group open", in_group)
        assert _call("rs", comms, 16)[0]["kind"] == "ring"  # the refused setters changed nothing
        lib, h, cfg = _lib.load(), ctypes.c_void_p(), C.CommConfig().to_c(2)
        mine = (ctypes.c_char * lib.mccsConnectHandleSize())()
        assert lib.mccsCommSetupRank(ctypes.byref(h), 0, 2, 0, ctypes.byref(cfg[0]), mine) == 0
        loose = C.Communicator(h.value)  # set up, never connected
        try:
            assert loose.reduce_scatter_wide_stream_max() == 0
            _refused(INVALID_USAGE, PRE + "the communicator is not connected", lambda: _set([loose], 64))
        finally:
            loose.destroy()
    finally:
        _destroy(comms)
