"""CPU: how the planner launches the explicit block-scaled FP8 streamed AllGather (csrc/direct_quant_ag.h), on the recording
fake runtime.  Its record: mode=quant-ag-stream, count (elements per rank), pay=, rounds=, round= (elements) and slots=."""
import ctypes

import pytest

from mccs_amd import _lib
from mccs_amd import comm as C
from test_all_reduce_wide_plan import BF16, CAP, F16, F32, _init
from test_reduce_scatter_direct_plan import INVALID_ARGUMENT, INVALID_USAGE, _destroy, _launches, _recv, _refused, _send
from test_reduce_scatter_direct_plan import fake  # noqa: F401  (the fixture)

PAY = CAP * 32 // 33 // 512 * 512    # codes of one round; the scale bytes lie behind them
QCAP, MODE = 2 * PAY, "quant-ag-stream"  # the largest round, in input bytes
PRE = "mccsCommSetAllGatherQuant: "


def _agq(comms, count, dtype=BF16, stream=0):  # dtype None: the byte-typed AllGather of `count` bytes
    with C.group():
        for r, c in enumerate(comms):
            if dtype is None:
                C.all_gather(c, _send(r), _recv(r), count, stream=stream)
            else:
                c.all_gather_quant(_send(r), _recv(r), count, dtype, stream=stream)
    return _launches()


@pytest.mark.parametrize("n", [2, 4, 8])
def test_the_record_the_rounds_and_the_byte_typed_call_untouched(fake, n):
    fake(1)
    comms = _init([0] * n)
    try:
        assert all(c.all_gather_quant_max() == QCAP == c.reduce_scatter_quant_max() for c in comms)
        plain = [_agq(comms, b, None) for b in (600, 8192, 1 << 19)]  # LL, one-shot, ring: before any quantised call
        (kv,) = _agq(comms, PAY + 1)  # the default round is the cap
        assert (kv["mode"], kv["rounds"], kv["round"]) == (MODE, "2", str(PAY)) and comms[-1].last_algo() == "quant-stream"
        [c.set_all_gather_quant(1024) for c in comms]
        for count, dtype in ((1, F16), (512, BF16), (513, F16), (4 * 512 + 511, BF16), (1 << 22, BF16)):  # any size
            (kv,) = _agq(comms, count, dtype)
            assert kv["kind"] == "direct" and kv["mode"] == MODE and kv["count"] == str(count) and kv["pay"] == str(PAY), kv
            assert (int(kv["rounds"]), kv["round"]) == (-(-count // 512), "512") and kv["grid"] == f'{kv["gx"]}x{n}'
            assert int(kv["piece"]) % 2048 == int(kv["piece2"]) % 2048 == 0 and kv["op_arg"] == "0"
            assert kv["slots"] == "/".join(f"{r}:{_send(r):x}:{_recv(r):x}" for r in range(n))
        assert [_agq(comms, b, None) for b in (600, 8192, 1 << 19)] == plain  # mccsAllGather never takes this path
        for c in comms:
            c.set_all_gather_quant(QCAP), c.set_all_gather_quant()  # the cap itself, and back to it
        assert _agq(comms, 3 * PAY)[0]["rounds"] == "3"
    finally:
        _destroy(comms)


def test_captured_fused_launches_and_the_environment(fake, monkeypatch):
    fake(2)
    lib, made = _lib.load(), []
    for rnd in ((1 << 30) + 8, 5000, 5, None):  # read at creation: clamped to the cap, cut to a multiple of 1024, and
        monkeypatch.setenv("MCCS_AG_QUANT_ROUND_BYTES", str(rnd)) if rnd else monkeypatch.delenv("MCCS_AG_QUANT_ROUND_BYTES")
        made.append(_init([0, 0, 1, 1] if rnd == 5000 else [0, 0]))  # 1 .. 1023 the smallest round; then without it
    try:
        assert [_agq(made[k], 5000)[0]["round"] for k in (0, 2, 3)] == [str(PAY), "512", str(PAY)]
        assert lib.mccs_test_fake_capture(0x5000, 9) == 0
        got = _agq(made[1], 5000, stream=0x5000)
        assert lib.mccs_test_fake_capture(0x5000, 0) == 0
        # two devices, two fused rank slots each; a captured launch has no stop event
        assert len(got) == 2 and all(kv["grid"].endswith("x2") and kv["stop_event"] == "0" for kv in got)
        assert [(kv["mode"], kv["rounds"], kv["round"], kv["slots"].split(":")[0]) for kv in got] == [
            (MODE, "3", "2048", "0"), (MODE, "3", "2048", "2")]
        lib.mccs_test_fake_destroy_graph(9)
        assert all(kv["stop_event"] != "0" for kv in _agq(made[1], 5000))  # eager: a stop event
    finally:
        _destroy(sum(made, []))


def test_refusals(fake):
    fake(1)
    comms, one, nine = _init([0, 0]), _init([0]), _init([0] * 9)
    noslot = C.init_all([0, 0], C.CommConfig(ll_bytes=-1, oneshot_bytes=-1, direct_bytes=-1, buffer_size=1 << 20))
    c, call = comms[0], "mccsAllGatherQuant: "
    try:
        for bad, words in ((one, "1 ranks are outside 2..8"), (nine, "9 ranks are outside 2..8"),
                           (noslot, "no one-shot slots in the direct region or no peer atomics")):
            assert bad[0].all_gather_quant_max() == 0
            _refused(INVALID_USAGE, call + words, lambda: _agq(bad, 4096), ("no ring fallback",))
        _refused(INVALID_USAGE, call + "dtype 7 is neither mccsFloat16 nor mccsBfloat16", lambda: _agq(comms, 4096, F32))

        def second(first):  # a second call of the communicator in the group, after it and before it
            with C.group():
                for k in (0, 1):
                    if (k == 0) == first:
                        c.all_gather_quant(_send(0), _recv(0), 4096, BF16, stream=0)
                    else:
                        C.all_gather(c, _send(0), _recv(0), 4096, stream=0)

        _refused(INVALID_USAGE, "mccsAllGather: a group mixes collectives", lambda: second(True))
        _refused(INVALID_USAGE, call + "the group holds a second call of this communicator", lambda: second(False))
        assert _launches() == [] and _agq(comms, 4096)[0]["mode"] == MODE  # nothing was launched, and the comm is usable
        _refused(INVALID_ARGUMENT, PRE + "round_bytes 1536 is not a multiple of 1024", lambda: c.set_all_gather_quant(1536))
        _refused(INVALID_ARGUMENT, PRE + f"round_bytes {QCAP + 1024} is above the {QCAP} bytes",
                 lambda: c.set_all_gather_quant(QCAP + 1024))
        _refused(INVALID_ARGUMENT, PRE + "round_bytes 1024 is above the 0 bytes", lambda: nine[0].set_all_gather_quant(1024),
                 ("closed here",))

        def in_group():
            with C.group():
                c.set_all_gather_quant(1024)

        _refused(INVALID_USAGE, PRE + "the communicator has a group open", in_group)
        assert _agq(comms, 4096)[0]["round"] == str(PAY)  # the refused setters changed nothing
        lib, h, cfg = _lib.load(), ctypes.c_void_p(), C.CommConfig().to_c(2)
        mine = (ctypes.c_char * lib.mccsConnectHandleSize())()
        assert lib.mccsCommSetupRank(ctypes.byref(h), 0, 2, 0, ctypes.byref(cfg[0]), mine) == 0
        loose = C.Communicator(h.value)  # set up, never connected
        try:
            assert loose.all_gather_quant_max() == 0
            _refused(INVALID_USAGE, call + "the communicator is not connected",
                     lambda: loose.all_gather_quant(_send(0), _recv(0), 64, BF16, stream=0))
            _refused(INVALID_ARGUMENT, PRE + "the communicator is not connected", lambda: loose.set_all_gather_quant(1024))
        finally:
            loose.destroy()
    finally:
        _destroy(comms + one + nine + noslot)
