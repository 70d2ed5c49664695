"""CPU: how the planner launches the opt-in block-scaled FP8 AllReduce
(csrc/direct_quant.h), on the recording fake device runtime (fixture and helpers:
tests/test_reduce_scatter_direct_plan.py).  A held call's record is kind=direct
mode=quant-twoshot with the count, the payload bytes of a slot (pay), the scalar
(op_arg, hex), the share table (owned) and, per rank slot, rank and buffers.
"""
import pytest

from mccs_amd import _lib
from mccs_amd import comm as C
from test_all_reduce_wide_plan import _ar, _init
from test_all_reduce_wide_plan import BF16, F16, F32, HALF, I32, LL_CAP, CAP, MAX, PREMULSUM, SUM, SUMPOSTDIV, TWO_CAP
from test_reduce_scatter_direct_plan import INVALID_ARGUMENT, INVALID_USAGE, _destroy, _launches, _recv, _refused, _send
from test_reduce_scatter_direct_plan import fake  # noqa: F401  (the fixture)

PAY = TWO_CAP * 32 // 33 // 512 * 512  # codes of one two-shot slot; the scale bytes lie behind them
QCAP = 2 * PAY


def _set(comms, max_bytes, min_bytes=0):
    for c in comms:
        c.set_all_reduce_quant(max_bytes, min_bytes)


@pytest.mark.parametrize("n", [2, 3, 8])
def test_the_record_both_edges_and_the_precedence_over_the_wide_limits(fake, n):
    fake(1)
    comms = _init([0] * n)
    try:
        assert PAY % 512 == 0 and PAY + PAY // 32 <= TWO_CAP < QCAP
        assert all(c.all_reduce_quant_max() == QCAP for c in comms)
        before = _ar(comms, 600)
        assert before[0]["mode"] == "ll"  # not opted in
        _set(comms, QCAP, 1024)
        for count, dtype, op, arg in ((512, BF16, SUM, None), (513, F16, PREMULSUM, 0x3800), (512 * n - 1, BF16, SUM, None),
                                      (512 * n + 1, BF16, SUM, None), (PAY, F16, SUM, None)):
            (kv,) = _ar(comms, count, dtype, op, arg)
            assert kv["kind"] == "direct" and kv["mode"] == "quant-twoshot" and kv["count"] == str(count), kv
            assert all(c.last_algo() == "quant-direct" for c in comms)
            assert kv["pay"] == str(PAY) and kv["op_arg"] == ("3800" if op == PREMULSUM else "0") and kv["nch"] == "0"
            assert kv["grid"] == f'{kv["gx"]}x{n}' and kv["block"] == "512" and int(kv["piece"]) % 512 == 0
            assert kv["slots"] == "/".join(f"{r}:{_send(r):x}:{_recv(r):x}" for r in range(n))
            q = (-(-count // n) + 511) // 512 * 512  # contiguous shares that start on wave units
            assert kv["owned"].split(",") == [str(max(0, min(q, count - t * q))) for t in range(n)]
        assert _ar(comms, 511)[0]["mode"] == "ll"          # below the window
        assert _ar(comms, PAY + 1)[0]["kind"] == "ring"    # above the cap
        # inside its window quant wins over every wide limit; outside the wide limits decide
        for c in comms:
            c.set_all_reduce_wide(LL_CAP, CAP, TWO_CAP)
        _set(comms, 8192, 4096)
        assert [_ar(comms, cnt)[0]["mode"] for cnt in (2047, 2048, 4096, 4097)] == \
            ["wide-ll", "quant-twoshot", "quant-twoshot", "wide-ll"]
        for c in comms:
            c.set_all_reduce_wide()
        _set(comms, 0)  # off again: the record of before opting in
        assert _ar(comms, 600) == before
    finally:
        _destroy(comms)


def test_other_calls_plan_as_before_and_a_grouped_pair_goes_to_the_ring_with_its_scalar(fake):
    fake(1)
    n = 4
    plain, comms = _init([0] * n), _init([0] * n)
    try:
        _set(comms, QCAP)
        for dtype, op, arg in ((F32, SUM, None), (BF16, MAX, None), (I32, SUMPOSTDIV, n), (F32, PREMULSUM, 0x3F000000)):
            (want,) = _ar(plain, 300, dtype, op, arg)
            (kv,) = _ar(comms, 300, dtype, op, arg)
            assert (kv["kind"], kv.get("mode")) == (want["kind"], want.get("mode")) and kv.get("mode") != "quant-twoshot"
            assert comms[0].last_algo() == plain[0].last_algo()
        (want,) = _ar(plain, 300, BF16, PREMULSUM, HALF, calls=2)
        (kv,) = _ar(comms, 300, BF16, PREMULSUM, HALF, calls=2)
        assert kv["kind"] == "ring" and kv["redop_args"] == want["redop_args"] and "3f00" in kv["redop_args"]
        with C.group():  # the average of bf16 is PreMulSum with 1/n
            for r, c in enumerate(comms):
                C.all_reduce_avg(c, _send(r), _recv(r), 300, BF16, stream=0)
        (kv,) = _launches()
        assert kv["mode"] == "quant-twoshot" and kv["op_arg"] == f"{C.avg_op(BF16, n)[1]:x}"
    finally:
        _destroy(plain + comms)
    for n in (1, 9):  # outside 2..8 ranks the cap is 0 and the ring runs
        comms = _init([0] * n)
        try:
            assert all(c.all_reduce_quant_max() == 0 for c in comms)
            assert all(kv["kind"] == "ring" for kv in _ar(comms, 64))
        finally:
            _destroy(comms)


def test_a_captured_fused_launch_the_environment_and_the_refusals(fake, monkeypatch):
    monkeypatch.setenv("MCCS_AR_QUANT_MIN_BYTES", "2048")
    monkeypatch.setenv("MCCS_AR_QUANT_BYTES", str(1 << 30))  # read at creation and clamped to the cap
    fake(2)
    lib = _lib.load()
    comms = _init([0, 0, 1, 1])
    monkeypatch.delenv("MCCS_AR_QUANT_MIN_BYTES")
    monkeypatch.delenv("MCCS_AR_QUANT_BYTES")
    others = _init([0, 0])
    c, pre = others[0], "mccsCommSetAllReduceQuant: "
    try:
        assert lib.mccs_test_fake_capture(0x5000, 9) == 0
        got = _ar(comms, 1024, stream=0x5000)
        assert lib.mccs_test_fake_capture(0x5000, 0) == 0
        # two devices, two fused rank slots each; a captured launch has no stop event
        assert len(got) == 2 and all(kv["grid"].endswith("x2") and kv["stop_event"] == "0" for kv in got)
        assert [kv["mode"] for kv in got] == ["quant-twoshot"] * 2 and [kv["slots"][0] for kv in got] == ["0", "2"]
        lib.mccs_test_fake_destroy_graph(9)
        assert all(kv["mode"] == "quant-twoshot" and kv["stop_event"] != "0" for kv in _ar(comms, PAY))  # clamped
        assert _ar(comms, 1023)[0]["mode"] == "ll" and _ar(comms, PAY + 1)[0]["kind"] == "ring"
        assert _ar(others, 1024)[0]["mode"] == "ll"  # created without the variables: off
        _refused(INVALID_ARGUMENT, pre + "max_bytes", lambda: c.set_all_reduce_quant(QCAP + 1), (str(QCAP + 1), str(QCAP)))
        _refused(INVALID_ARGUMENT, pre + "min_bytes", lambda: c.set_all_reduce_quant(4096, 4097), ("4097", "4096"))
        c.set_all_reduce_quant(QCAP, QCAP)  # the cap itself is fine
        c.set_all_reduce_quant(0)

        def in_group():
            with C.group():
                c.set_all_reduce_quant(64)

        _refused(INVALID_USAGE, pre + "the communicator has a group open", in_group)
        assert _ar(others, 1024)[0]["mode"] == "ll"  # the refused setters changed nothing
    finally:
        _destroy(comms + others)
