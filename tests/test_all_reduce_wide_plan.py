"""CPU: how the planner launches the opt-in wide-accumulate AllReduce
(csrc/direct_wide.h), on the recording fake device runtime (fixture and helpers:
tests/test_reduce_scatter_direct_plan.py).  A held call's record is kind=direct
mode=wide-ll / wide-oneshot / wide-twoshot with the count, the scalar (op_arg,
hex), the two-shot's share table (owned) and, per rank slot, rank and buffers.
"""
import pytest

from mccs_amd import _lib
from mccs_amd import comm as C
from test_reduce_scatter_direct_plan import INVALID_ARGUMENT, INVALID_USAGE, _destroy, _launches, _recv, _refused, _send
from test_reduce_scatter_direct_plan import fake  # noqa: F401  (the fixture)

I32, F16, F32, BF16 = 2, 6, 7, 9
SUM, MAX, PREMULSUM, SUMPOSTDIV = 0, 2, 4, 5
LL_CAP, CAP, TWO_CAP = 16 << 10, 64 << 10, 256 << 10
ENV = ("MCCS_AR_WIDE_LL_BYTES", "MCCS_AR_WIDE_ONESHOT_BYTES", "MCCS_AR_WIDE_BYTES")
HALF = 0x3F00  # 0.5 in bf16


def _init(devices, **kw):
    comms = C.init_all(devices, C.CommConfig(ll_bytes=LL_CAP, oneshot_bytes=CAP, direct_bytes=TWO_CAP,
                                             buffer_size=1 << 20, **kw))
    _launches()
    return comms


def _ar(comms, count, dtype=BF16, op=SUM, op_arg=None, stream=0, calls=1):
    with C.group():
        for k in range(calls):
            for r, c in enumerate(comms):
                C.all_reduce(c, _send(r) + k * 0x100000, _recv(r) + k * 0x100000, count, dtype, op, stream=stream,
                             op_arg=op_arg)
    return _launches()


def _set(comms, *limits):
    for c in comms:
        c.set_all_reduce_wide(*limits)


@pytest.mark.parametrize("n", [2, 3, 8])
def test_the_three_records_their_edges_and_the_precedence(fake, n):
    fake(1)
    comms = _init([0] * n)
    try:
        assert all(c.all_reduce_wide_max() == (LL_CAP, CAP, TWO_CAP) for c in comms)
        assert _ar(comms, 513)[0]["mode"] == "ll" and comms[0].last_algo() == "ll"  # limits still 0
        _set(comms, 1024, 4096, TWO_CAP)
        for count, mode, algo in ((512, "wide-ll", "wide-ll"), (513, "wide-oneshot", "wide-oneshot"),
                                  (2048, "wide-oneshot", "wide-oneshot"), (2049, "wide-twoshot", "wide-direct"),
                                  (n - 1, "wide-ll", "wide-ll"), (TWO_CAP // 2, "wide-twoshot", "wide-direct")):
            for dtype, op, arg in ((BF16, SUM, None), (F16, PREMULSUM, 0x3800)):
                (kv,) = _ar(comms, count, dtype, op, arg)
                assert kv["kind"] == "direct" and kv["mode"] == mode and kv["count"] == str(count), kv
                assert all(c.last_algo() == algo for c in comms)
                assert kv["op_arg"] == ("3800" if op == PREMULSUM else "0") and kv["nch"] == "0"
                assert kv["grid"] == f'{kv["gx"]}x{n}' and kv["block"] == "512" and kv["comms_on_dev"] == "1"
                assert kv["slots"] == "/".join(f"{r}:{_send(r):x}:{_recv(r):x}" for r in range(n))
                q = (-(-count // n) + 7) // 8 * 8  # contiguous shares that start on 16-byte packs
                shares = [max(0, min(q, count - t * q)) for t in range(n)]
                assert kv["owned"].split(",") == [str(x if mode == "wide-twoshot" else 0) for x in shares]
        (kv,) = _ar(comms, TWO_CAP // 2 + 1)  # above every limit: the ring
        assert kv["kind"] == "ring" and comms[0].last_algo() == "ring"
        _set(comms, 0, 0, TWO_CAP)  # trailing ranks own nothing: still one launch
        assert _ar(comms, n - 1)[0]["owned"] == ",".join([str(n - 1)] + ["0"] * (n - 1))
    finally:
        _destroy(comms)


def test_other_calls_plan_as_before_and_a_grouped_pair_goes_to_the_ring_with_its_scalar(fake):
    fake(1)
    n = 4
    plain, comms = _init([0] * n), _init([0] * n)
    try:
        _set(comms, LL_CAP, CAP, TWO_CAP)
        for dtype, op, arg in ((F32, SUM, None), (BF16, MAX, None), (I32, SUMPOSTDIV, n), (F32, PREMULSUM, 0x3F000000)):
            (want,) = _ar(plain, 300, dtype, op, arg)
            (kv,) = _ar(comms, 300, dtype, op, arg)
            assert (kv["kind"], kv.get("mode")) == (want["kind"], want.get("mode")) and "wide" not in kv.get("mode", "")
            assert comms[0].last_algo() == plain[0].last_algo()
        (want,) = _ar(plain, 300, BF16, PREMULSUM, HALF, calls=2)
        (kv,) = _ar(comms, 300, BF16, PREMULSUM, HALF, calls=2)
        assert kv["kind"] == "ring" and kv["redop_args"] == want["redop_args"] and "3f00" in kv["redop_args"]
        (kv,) = _ar(comms, 300, BF16, PREMULSUM, HALF)  # a single call afterwards is wide again
        assert kv["mode"] == "wide-ll" and kv["op_arg"] == "3f00"
        with C.group():  # the average of bf16 is PreMulSum with 1/n
            for r, c in enumerate(comms):
                C.all_reduce_avg(c, _send(r), _recv(r), 300, BF16, stream=0)
        assert _launches()[0]["op_arg"] == f"{C.avg_op(BF16, n)[1]:x}" and comms[0].last_algo() == "wide-ll"
    finally:
        _destroy(plain + comms)
    for n in (1, 9):  # outside 2..8 ranks the caps are 0 and the ring runs
        comms = _init([0] * n)
        try:
            assert all(c.all_reduce_wide_max() == (0, 0, 0) for c in comms)
            assert all(kv["kind"] == "ring" for kv in _ar(comms, 64))
        finally:
            _destroy(comms)


def test_captured_fused_launches_and_the_environment(fake, monkeypatch):
    for name, v in zip(ENV, (1024, 4096, 1 << 30)):  # read at creation and clamped to the caps
        monkeypatch.setenv(name, str(v))
    fake(2)
    lib = _lib.load()
    comms = _init([0, 0, 1, 1])
    for name in ENV:
        monkeypatch.delenv(name)
    others = _init([0, 0])
    try:
        assert lib.mccs_test_fake_capture(0x5000, 9) == 0
        got = _ar(comms, 512, stream=0x5000) + _ar(comms, 513, stream=0x5000)
        assert lib.mccs_test_fake_capture(0x5000, 0) == 0
        # two devices, two fused rank slots each; a captured launch has no stop event
        assert len(got) == 4 and all(kv["grid"].endswith("x2") and kv["stop_event"] == "0" for kv in got)
        assert [kv["mode"] for kv in got] == ["wide-ll", "wide-ll", "wide-oneshot", "wide-oneshot"]
        assert [kv["slots"].split(":")[0] for kv in got] == ["0", "2", "0", "2"]
        lib.mccs_test_fake_destroy_graph(9)
        for count, mode in ((2049, "wide-twoshot"), (TWO_CAP // 2, "wide-twoshot")):  # eager: a stop event
            assert all(kv["mode"] == mode and kv["stop_event"] != "0" for kv in _ar(comms, count))
        assert _ar(comms, TWO_CAP // 2 + 1)[0]["kind"] == "ring"
        assert _ar(others, 256)[0]["mode"] == "ll"  # created without the variables: off
    finally:
        _destroy(comms + others)


def test_refusals(fake):
    fake(1)
    comms, cached = _init([0, 0]), _init([0, 0], fifo_memory=C.FIFO_DEVICE)  # a cached arena has no LL lines
    c, pre = comms[0], "mccsCommSetAllReduceWide: "
    try:
        _refused(INVALID_ARGUMENT, pre + "ll_bytes", lambda: c.set_all_reduce_wide(LL_CAP + 8), (str(LL_CAP + 8), str(LL_CAP)))
        _refused(INVALID_ARGUMENT, pre + "oneshot_bytes", lambda: c.set_all_reduce_wide(0, CAP + 1), (str(CAP + 1), str(CAP)))
        _refused(INVALID_ARGUMENT, pre + "twoshot_bytes", lambda: c.set_all_reduce_wide(0, 0, TWO_CAP + 1), (str(TWO_CAP),))
        c.set_all_reduce_wide(LL_CAP, CAP, TWO_CAP)  # the capacities themselves are fine
        c.set_all_reduce_wide()

        def in_group():
            with C.group():
                c.set_all_reduce_wide(64, 64, 64)

        _refused(INVALID_USAGE, pre + "the communicator has a group open", in_group)
        assert _ar(comms, 16)[0]["mode"] == "ll"  # the refused setters changed nothing
        assert cached[0].all_reduce_wide_max() == (0, CAP, TWO_CAP)
        _refused(INVALID_ARGUMENT, pre + "ll_bytes 8 is above the 0 bytes", lambda: cached[0].set_all_reduce_wide(8),
                 ("the LL path is closed here",))
    finally:
        _destroy(comms + cached)
