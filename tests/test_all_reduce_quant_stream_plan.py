"""CPU: how the planner launches the opt-in block-scaled FP8 streamed AllReduce (csrc/direct_quant_stream_ar.h), on the
recording fake runtime.  Its record: kind=direct mode=quant-ar-stream, count, pay= (code bytes a round may have), rounds=,
round= (elements of one round), owned= and op_arg=."""
import ctypes

import pytest

from mccs_amd import _lib
from mccs_amd import comm as C
from test_all_reduce_wide_plan import BF16, CAP, F16, F32, LL_CAP, MAX, PREMULSUM, SUM, TWO_CAP, _ar, _init
from test_reduce_scatter_direct_plan import INVALID_ARGUMENT, _destroy, _launches, _recv, _refused, _send
from test_reduce_scatter_direct_plan import fake  # noqa: F401  (the fixture)
from test_reduce_wide_plan import _call

PAY = min(CAP, TWO_CAP // 2) * 32 // 33 // 512 * 512  # codes of one round; the scale bytes lie behind them
QCAP, MODE = 2 * PAY, "quant-ar-stream"               # the largest round, in input bytes
ENV = ("MCCS_AR_QUANT_STREAM_MIN_BYTES", "MCCS_AR_QUANT_STREAM_BYTES", "MCCS_AR_QUANT_STREAM_ROUND_BYTES")
PRE = "mccsCommSetAllReduceQuantStream: "


def _set(comms, *limits):
    for c in comms:
        c.set_all_reduce_quant_stream(*limits)


def _rounds(kvs):  # of a call's one launch; without rounds: its kind, mode and grid, to compare with a plain communicator's
    kv, = kvs
    return (kv["mode"], int(kv["rounds"]), int(kv["round"])) if "rounds" in kv else (kv["kind"], kv.get("mode"), kv["grid"])


@pytest.mark.parametrize("n", [2, 8])
def test_the_record_the_edges_the_rounds_and_the_precedence(fake, n):
    fake(1)
    plain, comms, three = _init([0] * n), _init([0] * n), _init([0] * 3)
    try:
        assert all(c.all_reduce_quant_stream_max() == QCAP for c in comms)
        before = [_ar(comms, k) for k in (600, 8192, 1 << 19)]  # not opted in
        _set(comms, 1 << 20, 8192, 1024)
        for count in (4096, 1 << 19):  # both edges of the window: q = count / n in rounds of 512 elements
            for dtype, op, arg in ((BF16, SUM, None), (F16, PREMULSUM, 0x3800)):
                (kv,) = _ar(comms, count, dtype, op, arg)
                assert kv["kind"] == "direct" and _rounds([kv]) == (MODE, count // n // 512, 512), kv
                assert kv["count"] == str(count) and kv["pay"] == str(PAY) and kv["op_arg"] == ("3800" if arg else "0")
                assert kv["owned"] == ",".join([str(count // n)] * n) and kv["grid"] == f'{kv["gx"]}x{n}'
                assert int(kv["piece"]) % 2048 == int(kv["piece2"]) % 2048 == 0 and comms[-1].last_algo() == "quant-stream"
        for count in (4095, (1 << 19) + 1):  # one element outside either edge plans as without the opt-in
            assert _rounds(_ar(comms, count)) == _rounds(_ar(plain, count))
        _set(comms, 1 << 40, 0, 1024)  # no cap on the buffer; K = 1 and 2; then round_bytes = 0, the largest round
        assert [_rounds(_ar(comms, 512 * n * k)) for k in (1, 2)] == [(MODE, k, 512) for k in (1, 2)]
        _set(comms, 1 << 40)
        assert _rounds(_ar(comms, PAY * n + 1)) == (MODE, 2, PAY)
        _set(three, 1 << 20, 0, 1024)  # the ownership boundary at n = 3: 1537 gives q = 1024 and the last rank nothing
        assert [_ar(three, k)[0].get("mode") for k in (1025, 2049)] == [MODE] * 2
        (kv,) = _ar(three, 1537)
        _set(three, 0)
        assert kv.get("mode") != MODE and [kv] == _ar(three, 1537)
        for c in comms:  # the two-shot quant window, this one, the wide limits (where a last rank without an element falls)
            c.set_all_reduce_quant(8192, 2048), c.set_all_reduce_wide(LL_CAP, CAP, TWO_CAP), _set([c], 32768, 0, 2048)
        assert [_ar(comms, k)[0]["mode"] for k in (4096, 8192, 16384, 20480, {2: 512, 8: 5000}[n])] == [
            "quant-twoshot", MODE, MODE, "wide-oneshot", "wide-ll"]
        for c in comms:
            c.set_all_reduce_quant(0), c.set_all_reduce_wide(), _set([c], 1 << 30)
        for dtype, op in ((F32, SUM), (BF16, MAX)):  # other dtypes and ops, and Reduce, plan as before
            assert _rounds(_ar(comms, 8192, dtype, op)) == _rounds(_ar(plain, 8192, dtype, op))
        assert _rounds(_call("rd", comms, 8192)) == _rounds(_call("rd", plain, 8192))
        with C.group():  # the average of bf16 is PreMulSum with 1/n
            for r, c in enumerate(comms):
                C.all_reduce_avg(c, _send(r), _recv(r), 8192, BF16, stream=0)
        (kv,) = _launches()
        assert kv["mode"] == MODE and kv["op_arg"] == f"{C.avg_op(BF16, n)[1]:x}"
        _set(comms, 0)  # off again: the records of before opting in
        assert [_ar(comms, k) for k in (600, 8192, 1 << 19)] == before
    finally:
        _destroy(plain + comms + three)


def test_the_environment_and_the_refusals(fake, monkeypatch):
    fake(1)
    made = []
    for rnd in ((1 << 30) + 8, 5000, 5, None):  # read at creation: the round clamped to the cap, cut to a multiple of
        for name, v in zip(ENV, (2048, 1 << 30, rnd)):  # 1024, and 1 .. 1023 the smallest round; then without them
            monkeypatch.setenv(name, str(v)) if rnd else monkeypatch.delenv(name)
        made.append(_init([0, 0]))
    nine, c = _init([0] * 9), made[3][0]
    try:
        assert [_rounds(_ar(made[k], cnt)) for k, cnt in enumerate((2 * PAY + 2, 10000, 2050))] == [
            (MODE, 2, PAY), (MODE, 3, 2048), (MODE, 3, 512)]
        assert _ar(made[0], 1023)[0].get("mode") == "ll" and _ar(made[0], (1 << 29) + 1)[0]["kind"] == "ring"  # the window
        _refused(INVALID_ARGUMENT, PRE + "min_bytes 4097 is above max_bytes 4096", lambda: _set([c], 4096, 4097))
        _refused(INVALID_ARGUMENT, PRE + "round_bytes 1536 is not a multiple of 1024", lambda: _set([c], 4096, 0, 1536))
        _refused(INVALID_ARGUMENT, PRE + f"round_bytes {QCAP + 1024} is above the {QCAP} bytes",
                 lambda: _set([c], 4096, 0, QCAP + 1024))
        _set([c], 1 << 40, 1 << 40, QCAP), _set([c], 64, 64, 1024), _set([c], 0)  # the edges themselves are fine
        assert _ar(made[3], 4096)[0].get("mode") != MODE  # created without the variables, and the refused setters: off
        _refused(INVALID_ARGUMENT, PRE + "max_bytes 64", lambda: _set(nine[:1], 64), ("closed here",))  # outside 2..8 ranks
        assert all(x.all_reduce_quant_stream_max() == 0 for x in nine) and all(kv["kind"] == "ring" for kv in _ar(nine, 8192))
        lib, h, cfg = _lib.load(), ctypes.c_void_p(), C.CommConfig().to_c(2)
        mine = (ctypes.c_char * lib.mccsConnectHandleSize())()
        assert lib.mccsCommSetupRank(ctypes.byref(h), 0, 2, 0, ctypes.byref(cfg[0]), mine) == 0
        loose = C.Communicator(h.value)  # set up, never connected
        try:
            assert loose.all_reduce_quant_stream_max() == 0
            _refused(INVALID_ARGUMENT, PRE + "the communicator is not connected", lambda: _set([loose], 64))
        finally:
            loose.destroy()
    finally:
        _destroy(sum(made, []) + nine)
