"""CPU: how the planner launches the opt-in wide-accumulate ReduceScatter and Reduce (csrc/direct_wide_rs.h), on the
recording fake device runtime (fixture and helpers: tests/test_reduce_scatter_direct_plan.py).  A held call's record is
kind=direct mode=wide-rs-ll / wide-rs-oneshot / wide-rd-ll / wide-rd-oneshot with the count (per block / of the buffer),
the scalar (op_arg, hex), for Reduce the root, and per rank slot rank and buffers.
"""
import pytest

from mccs_amd import _lib
from mccs_amd import comm as C
from test_reduce_scatter_direct_plan import INVALID_ARGUMENT, INVALID_USAGE, _destroy, _launches, _recv, _refused, _send
from test_reduce_scatter_direct_plan import fake  # noqa: F401  (the fixture)

I32, F16, F32, BF16 = 2, 6, 7, 9
SUM, MAX, PREMULSUM, SUMPOSTDIV = 0, 2, 4, 5
LL_CAP, CAP = 16 << 10, 64 << 10
ENV = ("MCCS_RS_WIDE_LL_BYTES", "MCCS_RS_WIDE_BYTES", "MCCS_RD_WIDE_LL_BYTES", "MCCS_RD_WIDE_BYTES")
HALF = 0x3F00  # 0.5 in bf16
each_fn = pytest.mark.parametrize("fn", ["rs", "rd"])


def _init(devices, **kw):
    comms = C.init_all(devices, C.CommConfig(ll_bytes=LL_CAP, oneshot_bytes=CAP, direct_bytes=-1, buffer_size=1 << 20, **kw))
    _launches()
    return comms


def _call(fn, comms, count, dtype=BF16, op=SUM, op_arg=None, root=0, stream=0, calls=1):
    with C.group():
        for k in range(calls):
            for r, c in enumerate(comms):
                bufs = (_send(r) + k * 0x100000, _recv(r) + k * 0x100000, count, dtype, op)
                if fn == "rs":
                    C.reduce_scatter(c, *bufs, stream=stream, op_arg=op_arg)
                else:
                    C.reduce(c, *bufs, root, stream=stream, op_arg=op_arg)
    return _launches()


def _set(fn, comms, *limits):
    for c in comms:
        (c.set_reduce_scatter_wide if fn == "rs" else c.set_reduce_wide)(*limits)


def _max(fn, c):
    return c.reduce_scatter_wide_max() if fn == "rs" else c.reduce_wide_max()


@pytest.mark.parametrize("n", [2, 3, 8])
@each_fn
def test_the_records_the_edges_and_ll_over_oneshot(fake, fn, n):
    fake(1)
    comms = _init([0] * n)
    try:
        assert all(_max(fn, c) == (LL_CAP, CAP) for c in comms)
        assert _call(fn, comms, 512)[0]["kind"] == "ring"  # limits still 0
        _set(fn, comms, 1024, 4096)
        for count, body in ((1, "ll"), (512, "ll"), (513, "oneshot"), (2048, "oneshot")):
            for dtype, op, arg in ((BF16, SUM, None), (F16, PREMULSUM, 0x3800)):
                root = count % n
                (kv,) = _call(fn, comms, count, dtype, op, arg, root)
                assert kv["kind"] == "direct" and kv["mode"] == f"wide-{fn}-{body}" and kv["count"] == str(count), kv
                assert all(c.last_algo() == "wide-" + body for c in comms)
                assert kv["op_arg"] == ("3800" if op == PREMULSUM else "0") and kv["nch"] == "0"
                assert kv.get("root") == (str(root) if fn == "rd" else None)
                assert kv["grid"] == f'{kv["gx"]}x{n}' and kv["block"] == "512" and kv["comms_on_dev"] == "1"
                assert kv["slots"] == "/".join(f"{r}:{_send(r):x}:{_recv(r):x}" for r in range(n))
        (kv,) = _call(fn, comms, 2049)  # above both limits: the ring
        assert kv["kind"] == "ring" and comms[0].last_algo() == "ring"
        _set(fn, comms, LL_CAP, CAP)  # the caps themselves
        assert _call(fn, comms, LL_CAP // 2 + 1)[0]["mode"] == f"wide-{fn}-oneshot"
        assert _call(fn, comms, CAP // 2)[0]["mode"] == f"wide-{fn}-oneshot" and _call(fn, comms, CAP // 2 + 1)[0]["kind"] == "ring"
        assert _call(fn, comms, 0) == []
    finally:
        _destroy(comms)


@each_fn
def test_other_calls_plan_as_before_and_a_grouped_pair_goes_to_the_ring_with_its_scalar(fake, fn):
    fake(1)
    n = 4
    plain, comms = _init([0] * n), _init([0] * n)
    try:
        for c in plain + comms:  # both sets opted in to the ring-order direct variants
            c.set_reduce_scatter_direct(CAP, LL_CAP)
            c.set_rooted_direct(CAP, LL_CAP, CAP, LL_CAP)
        _set(fn, comms, LL_CAP, CAP)
        for dtype, op, arg in ((F32, SUM, None), (BF16, MAX, None), (I32, SUMPOSTDIV, n), (F32, PREMULSUM, 0x3F000000)):
            (want,) = _call(fn, plain, 300, dtype, op, arg, 1)
            (kv,) = _call(fn, comms, 300, dtype, op, arg, 1)
            assert (kv["kind"], kv.get("mode")) == (want["kind"], want.get("mode")) and "wide" not in kv.get("mode", "")
        assert _call(fn, plain, 300)[0]["mode"] == fn + "-ll" and _call(fn, comms, 300)[0]["mode"] == f"wide-{fn}-ll"
        other = "rd" if fn == "rs" else "rs"  # the other function is not this opt-in's
        assert _call(other, comms, 300)[0]["mode"] == other + "-ll"
        (want,) = _call(fn, plain, 300, BF16, PREMULSUM, HALF, 2, calls=2)
        (kv,) = _call(fn, comms, 300, BF16, PREMULSUM, HALF, 2, calls=2)
        assert kv["kind"] == "ring" and kv["redop_args"] == want["redop_args"] and "3f00" in kv["redop_args"]
        (kv,) = _call(fn, comms, 300, BF16, PREMULSUM, HALF, 2)  # a single call afterwards is wide again
        assert kv["mode"] == f"wide-{fn}-ll" and kv["op_arg"] == "3f00"
        with C.group():  # the average of bf16 is PreMulSum with 1/n
            for r, c in enumerate(comms):
                (C.reduce_scatter_avg if fn == "rs" else C.reduce_avg)(c, _send(r), _recv(r), 300, BF16, stream=0)
        assert _launches()[0]["op_arg"] == f"{C.avg_op(BF16, n)[1]:x}" and comms[0].last_algo() == "wide-ll"
    finally:
        _destroy(plain + comms)
    for n in (1, 9):  # outside 2..8 ranks the caps are 0 and the ring runs
        comms = _init([0] * n)
        try:
            assert all(_max(fn, c) == (0, 0) for c in comms)
            assert all(kv["kind"] == "ring" for kv in _call(fn, comms, 64))
        finally:
            _destroy(comms)


@each_fn
def test_captured_fused_launches_and_the_environment(fake, monkeypatch, fn):
    for name, v in zip(ENV, (1024, 1 << 30, 1024, 1 << 30)):  # read at creation and clamped to the caps
        monkeypatch.setenv(name, str(v))
    fake(2)
    lib = _lib.load()
    comms = _init([0, 0, 1, 1])
    for name in ENV:
        monkeypatch.delenv(name)
    others = _init([0, 0])
    try:
        assert lib.mccs_test_fake_capture(0x5000, 9) == 0
        got = _call(fn, comms, 512, stream=0x5000) + _call(fn, comms, 513, root=3, stream=0x5000)
        assert lib.mccs_test_fake_capture(0x5000, 0) == 0
        # two devices, two fused rank slots each; a captured launch has no stop event
        assert len(got) == 4 and all(kv["grid"].endswith("x2") and kv["stop_event"] == "0" for kv in got)
        assert [kv["mode"] for kv in got] == [f"wide-{fn}-ll"] * 2 + [f"wide-{fn}-oneshot"] * 2
        assert [kv["slots"].split(":")[0] for kv in got] == ["0", "2", "0", "2"]
        lib.mccs_test_fake_destroy_graph(9)
        assert all(kv["mode"] == f"wide-{fn}-oneshot" and kv["stop_event"] != "0" for kv in _call(fn, comms, CAP // 2))
        assert _call(fn, comms, CAP // 2 + 1)[0]["kind"] == "ring"
        assert _call(fn, others, 256)[0]["kind"] == "ring"  # created without the variables: off
    finally:
        _destroy(comms + others)


@each_fn
def test_refusals(fake, fn):
    fake(1)
    comms, cached = _init([0, 0]), _init([0, 0], fifo_memory=C.FIFO_DEVICE)  # a cached arena has no LL lines
    c = comms[0]
    pre = "mccsCommSetReduceScatterWide: " if fn == "rs" else "mccsCommSetReduceWide: "
    ll_name, name = ("ll_block_bytes", "block_bytes") if fn == "rs" else ("ll_bytes", "bytes")
    try:
        _refused(INVALID_ARGUMENT, pre + ll_name, lambda: _set(fn, [c], LL_CAP + 8), (str(LL_CAP + 8), str(LL_CAP)))
        _refused(INVALID_ARGUMENT, pre + name, lambda: _set(fn, [c], 0, CAP + 1), (str(CAP + 1), str(CAP)))
        _set(fn, [c], LL_CAP, CAP)  # the capacities themselves are fine
        _set(fn, [c], 0, 0)

        def in_group():
            with C.group():
                _set(fn, [c], 64, 64)

        _refused(INVALID_USAGE, pre + "the communicator has a group open", in_group)
        assert _call(fn, comms, 16)[0]["kind"] == "ring"  # the refused setters changed nothing
        assert _max(fn, cached[0]) == (0, CAP)
        _refused(INVALID_ARGUMENT, pre + ll_name + " 8 is above the 0 bytes", lambda: _set(fn, [cached[0]], 8),
                 ("the LL path is closed here",))
    finally:
        _destroy(comms + cached)
