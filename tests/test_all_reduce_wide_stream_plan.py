"""CPU: how the planner launches the opt-in wide streamed AllReduce (csrc/direct_wide_stream_ar.h), on the recording
fake device runtime (fixture: tests/test_reduce_scatter_direct_plan.py; helpers: tests/test_all_reduce_wide_plan.py).  A
held call's record is kind=direct mode=wide-ar-stream with the count, rounds= and round= (the elements of one round of a
share), the scalar (op_arg, hex) and the two-shot's share table (owned).
"""
import pytest

from mccs_amd import _lib
from mccs_amd import comm as C
from test_all_reduce_wide_plan import BF16, CAP, F16, F32, HALF, I32, MAX, PREMULSUM, SUM, SUMPOSTDIV, TWO_CAP, _ar, _init
from test_reduce_scatter_direct_plan import INVALID_ARGUMENT, _destroy, _launches, _recv, _refused, _send
from test_reduce_scatter_direct_plan import fake  # noqa: F401  (the fixture)

ENV = ("MCCS_AR_WIDE_STREAM_BYTES", "MCCS_AR_WIDE_STREAM_ROUND_BYTES")
PRE = "mccsCommSetAllReduceWideStream: "
RCAP = min(CAP, TWO_CAP // 2)  # a round fits one one-shot slot and half a two-shot in slot


def _set(comms, *limits):
    for c in comms:
        c.set_all_reduce_wide_stream(*limits)


def _rounds(kv):
    return kv.get("mode"), int(kv["rounds"]), int(kv["round"])


@pytest.mark.parametrize("n", [2, 3, 8])
def test_the_record_the_edges_and_the_other_wide_limits_first(fake, n):
    fake(1)
    plain, comms = _init([0] * n), _init([0] * n)
    low = 8 * n * (n - 1)  # up to here a trailing rank might own nothing: never streamed
    try:
        assert all(c.all_reduce_wide_stream_max() == RCAP for c in comms)
        _set(comms, 1 << 20, 256)
        for count in (low + 1, 128 * n, 128 * n + 1, 3 * 128 * n + 5, 1 << 19):
            for dtype, op, arg in ((BF16, SUM, None), (F16, PREMULSUM, 0x3800)):
                (kv,) = _ar(comms, count, dtype, op, arg)
                q = (-(-count // n) + 7) // 8 * 8  # the two-shot's contiguous shares
                shares = [str(min(q, count - t * q)) for t in range(n)]
                assert kv["kind"] == "direct" and _rounds(kv) == ("wide-ar-stream", -(-q // 128), 128), kv
                assert kv["count"] == str(count) and kv["op_arg"] == ("3800" if op == PREMULSUM else "0")
                assert kv["owned"].split(",") == shares and int(shares[-1]) >= 1
                assert all(c.last_algo() == "wide-stream" for c in comms) and kv["grid"] == f'{kv["gx"]}x{n}'
        for count in (low, (1 << 19) + 1):  # both edges: what a communicator that never opted in takes
            (want,), (kv,) = _ar(plain, count), _ar(comms, count)
            assert (kv["kind"], kv.get("mode")) == (want["kind"], want.get("mode")) and "rounds" not in kv
        _set(comms, 1 << 40)  # no cap on the buffer; round_bytes = 0 is the largest round
        assert _rounds(_ar(comms, RCAP * n)[0]) == ("wide-ar-stream", 2, RCAP // 2)
        for c in comms:  # LL, one-shot and two-shot win within THEIR limits; the stream takes what they leave
            c.set_all_reduce_wide(1024, 4096, 16384)
        assert [_ar(comms, k)[0]["mode"] for k in (512, 513, 2048, 2049, 8192, 8193)] == [
            "wide-ll", "wide-oneshot", "wide-oneshot", "wide-twoshot", "wide-twoshot", "wide-ar-stream"]
        _set(comms, 0)  # off again: every record equals the never-opted communicator's 
        for c in comms:
            c.set_all_reduce_wide()
        for count, dtype, op, arg in ((low + 1, BF16, SUM, None), (1 << 18, F16, PREMULSUM, HALF), (300, F32, SUM, None)):
            got, want = _ar(comms, count, dtype, op, arg), _ar(plain, count, dtype, op, arg)
            drop = dict(stop_event="", guard_order="")  # a communicator's own handles
            assert [dict(kv, **drop) for kv in got] == [dict(kv, **drop) for kv in want]
    finally:
        _destroy(plain + comms)


def test_other_calls_plan_as_before_and_a_grouped_pair_goes_to_the_ring_with_its_scalar(fake):
    fake(1)
    n = 4
    plain, comms = _init([0] * n), _init([0] * n)
    try:
        _refused(INVALID_ARGUMENT, PRE + "round_bytes 24 is not a multiple of 16", lambda: _set(comms[:1], 64, 24))
        _refused(INVALID_ARGUMENT, PRE + f"round_bytes {RCAP + 16} is above the {RCAP} bytes", lambda: _set(comms[:1], 64, RCAP + 16))
        _set(comms, 1 << 30, 4096)
        for dtype, op, arg in ((F32, SUM, None), (BF16, MAX, None), (I32, SUMPOSTDIV, n)):  # not this opt-in's
            (want,), (kv,) = _ar(plain, 1 << 18, dtype, op, arg), _ar(comms, 1 << 18, dtype, op, arg)
            assert (kv["kind"], kv.get("mode")) == (want["kind"], want.get("mode")) and "wide" not in kv.get("mode", "")
        (want,) = _ar(plain, 1 << 18, BF16, PREMULSUM, HALF, calls=2)
        (kv,) = _ar(comms, 1 << 18, BF16, PREMULSUM, HALF, calls=2)
        assert kv["kind"] == "ring" and kv["redop_args"] == want["redop_args"] and "3f00" in kv["redop_args"]
        (kv,) = _ar(comms, 20000, BF16, PREMULSUM, HALF)  # a single call afterwards streams again
        assert _rounds(kv) == ("wide-ar-stream", 3, 2048) and kv["op_arg"] == "3f00"
        with C.group():  # the average of bf16 is PreMulSum with 1/n
            for r, c in enumerate(comms):
                C.all_reduce_avg(c, _send(r), _recv(r), 20000, BF16, stream=0)
        assert _launches()[0]["op_arg"] == f"{C.avg_op(BF16, n)[1]:x}" and comms[0].last_algo() == "wide-stream"
    finally:
        _destroy(plain + comms)
    for n in (1, 9):  # outside 2..8 ranks there is no slot to stream through: the ring, and the opt-in is refused
        comms = _init([0] * n)
        try:
            assert all(c.all_reduce_wide_stream_max() == 0 for c in comms)
            _refused(INVALID_ARGUMENT, PRE + "max_bytes 64", lambda: _set(comms[:1], 64), ("closed here",))
            assert all(kv["kind"] == "ring" for kv in _ar(comms, 1 << 16))
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
    try:
        assert lib.mccs_test_fake_capture(0x5000, 9) == 0
        got = _ar(comms, RCAP * 4, stream=0x5000)
        assert lib.mccs_test_fake_capture(0x5000, 0) == 0
        # two devices, two fused rank slots each; a captured launch has no stop event
        assert len(got) == 2 and all(kv["grid"].endswith("x2") and kv["stop_event"] == "0" for kv in got)
        assert [_rounds(kv) for kv in got] == [("wide-ar-stream", 2, RCAP // 2)] * 2
        assert [kv["slots"].split(":")[0] for kv in got] == ["0", "2"]
        lib.mccs_test_fake_destroy_graph(9)
        assert all(kv["stop_event"] != "0" for kv in _ar(comms, 1 << 19)) and "rounds" not in _ar(comms, (1 << 19) + 1)[0]
        assert _rounds(_ar(small, 2000)[0]) == ("wide-ar-stream", 3, 992 // 2)
        _set(comms[:1], 1 << 20, 4096)  # fused comms that disagree on the round go to the ring together (device 0)
        assert [kv["kind"] for kv in _ar(comms, RCAP * 4)] == ["ring", "direct"]
    finally:
        _destroy(comms + small)
