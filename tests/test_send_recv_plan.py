"""CPU: how the planner launches a group of Send/Recv calls, on the recording
fake device runtime (see tests/test_all_to_all_plan.py).  The launch record's
sr= key lists, per rank slot and channel (';' between channels, ',' between a
channel's elements), each element's route word, bid, nChannels, count (S),
redOpArg (R), the two buffers and nWarps; they are held against the element
model of tests/sr_ref.py.  Then idle channels, inline and chained works,
captured and batched launches, and every refusal of the entry points.
"""
import subprocess

import pytest

import sr_ref as SR
from mccs_amd import _lib
from mccs_amd import abi
from mccs_amd import build
from mccs_amd import comm as C
from mccs_amd._lib import MccsError
from test_all_to_all_v_plan import _log, fake  # noqa: F401  (the fixture)

INVALID_ARGUMENT, INVALID_USAGE = 4, 5
U8 = C.AllReduceDataType.Uint8


def _addr(i, off=0):
    return 0x10000000 + 0x400000 * i + off  # the fake never touches "device" buffers


def _issue(comms, ops, addr=_addr, stream=0, ranks=None):
    """Every rank's calls in list order, all ranks in one group."""
    with C.group():
        for i, o in enumerate(ops):
            if ranks is not None and o.rank not in ranks:
                continue
            (C.send if o.kind == "send" else C.recv)(comms[o.rank], addr(i), o.nbytes, U8, o.peer, stream=stream)


def _elems(kv):
    """sr= of a launch: per rank slot, per channel, a list of dicts."""
    out = []
    for slot in kv["sr"].split("/"):
        chans = []
        for ch in slot.split(";"):
            es = []
            for e in ch.split(","):
                route, bid, nch, count, arg, send, recv, nwarps = e.split(":")
                route = int(route, 16)
                es.append({"hops": route & 0xff, "recv_bid": route >> 8 & 0xff, "part": route >> 16 & 0xff,
                           "parts": route >> 24, "bid": int(bid), "nch": int(nch), "count": int(count),
                           "arg": int(arg), "send": int(send, 16), "recv": int(recv, 16), "nwarps": int(nwarps)})
            chans.append(es)
        out.append(chans)
    return out


def _launches():
    return [kv for k, kv in _log() if k == "launch"]


@pytest.mark.parametrize("n", [2, 3, 4, 8])
def test_queued_elements_equal_the_model(fake, n):  # noqa: F811
    fake(1)
    comms = C.init_all([0] * n, C.CommConfig(buffer_size=SR.BUFF))
    try:
        _log()
        rings = comms[0].rings()
        route = comms[0].all_to_all_route()
        assert route["hops"] == 1
        for name, ops in SR.patterns(n, route["m"], rings).items():
            _issue(comms, ops)
            launches = _launches()
            assert len(launches) == 1 and launches[0]["kind"] == "ring", (name, launches)
            ranks = SR.ranks_of(ops)  # a rank without a call is not in the launch
            gx, gy = (int(v) for v in launches[0]["grid"].split("x"))
            assert gy == len(ranks) and gx == comms[0].nchannels * comms[0].lanes, name  # the mask is all channels
            got = _elems(launches[0])
            for slot, r in enumerate(ranks):
                want = SR.work_elements(ops, r, rings, _addr)
                assert got[slot] == want, (name, r)
                assert len(got[slot]) == len(rings)
            idle = [e for slot in got for ch in slot for e in ch if e["send"] == 0 and e["recv"] == 0]
            assert all(e["count"] == 0 and e["arg"] == 0 and e["hops"] == 1 and e["nwarps"] == SR.NWARPS for e in idle)
            single = all(len(ch) == 1 for slot in got for ch in slot)
            # one element per channel rides in the launch arguments, which hold 8 works (ring_cfg.h MCCS_INLINE_WORKS)
            assert (launches[0]["inline_works"] != "0") == (single and len(ranks) * len(rings) <= 8), name
            assert all(comms[r].last_algo() == "ring" for r in ranks)
            assert "a2av" not in launches[0] and "a2a" not in launches[0]
    finally:
        for c in comms:
            c.destroy()


def test_a_single_op_rides_inline_and_idle_channels_are_zero(fake):  # noqa: F811
    fake(1)
    n = 4
    comms = C.init_all([0] * n, C.CommConfig(buffer_size=SR.BUFF))
    try:
        _log()
        rings = comms[0].rings()
        ops = [SR.S(2, 0, 4099), SR.R(0, 2, 4099)]
        C.send(comms[2], _addr(0), 4099, U8, 0, stream=0)  # ungrouped: a launch of its own
        C.recv(comms[0], _addr(1), 4099, U8, 2, stream=0)
        launches = _launches()
        assert len(launches) == 2 and all(kv["inline_works"] == str(len(rings)) for kv in launches), launches
        for kv, r in zip(launches, (2, 0)):
            assert kv["grid"] == f"{comms[0].nchannels * comms[0].lanes}x1"
            got = _elems(kv)[0]
            assert got == SR.work_elements(ops, r, rings, _addr)
            live = [e for ch in got for e in ch if e["count"] or e["arg"]]
            assert len(live) == comms[0].all_to_all_route()["m"] and len(got) == len(rings)
        # typed counts scale the bytes
        C.send(comms[2], _addr(0), 10, C.AllReduceDataType.Float16, 0, stream=0)
        C.recv(comms[0], _addr(1), 10, C.AllReduceDataType.Int64, 2, stream=0)
        a, b = _launches()
        assert {e["count"] for ch in _elems(a)[0] for e in ch} == {0, 20}
        assert {e["arg"] for ch in _elems(b)[0] for e in ch} == {0, 80}
    finally:
        for c in comms:
            c.destroy()


def test_twelve_ops_on_one_channel_chain_a_second_work(fake):  # noqa: F811
    fake(1)
    n = 2
    comms = C.init_all([0] * n, C.CommConfig(buffer_size=SR.BUFF))
    try:
        _log()
        rings = comms[0].rings()
        assert abi.MCCS_MAX_WORK_ELEMENTS < 12 <= 2 * abi.MCCS_MAX_WORK_ELEMENTS
        ops = [SR.S(0, 1, 100 + k) for k in range(12)] + [SR.R(1, 0, 100 + k) for k in range(12)]
        ops += [SR.S(1, 0, 7), SR.R(0, 1, 7)]
        _issue(comms, ops)
        launches = _launches()
        assert len(launches) == 1 and launches[0]["inline_works"] == "0", launches
        got = _elems(launches[0])
        for r in range(n):
            assert got[r] == SR.work_elements(ops, r, rings, _addr), r
            assert all(len(ch) == 12 for ch in got[r])  # n = 2: every channel joins the pair
        assert [e["count"] for e in got[0][0]] == [100 + k for k in range(12)]
        assert [e["arg"] for e in got[0][0]] == [7] + [0] * 11
    finally:
        for c in comms:
            c.destroy()


def test_captured_and_batched_launches_carry_their_own_elements(fake):  # noqa: F811
    fake(1)
    lib = _lib.load()
    n = 4
    comms = C.init_all([0] * n, C.CommConfig(buffer_size=SR.BUFF))
    try:
        _log()
        rings, m = comms[0].rings(), comms[0].all_to_all_route()["m"]
        pats = SR.patterns(n, m, rings)
        a, b = pats["b_shift_3C"], pats["e_two_on_a_pair"]
        addr_b = lambda i: _addr(i, 0x40)
        stream = 0x5000
        assert lib.mccs_test_fake_capture(stream, 7) == 0
        _issue(comms, a, stream=stream)
        _issue(comms, b, addr=addr_b, stream=stream)
        assert lib.mccs_test_fake_capture(stream, 0) == 0
        launches = _launches()
        assert len(launches) == 2 and all(kv["inline_works"] == "0" for kv in launches), launches
        for kv, (ops, addr) in zip(launches, ((a, _addr), (b, addr_b))):
            assert _elems(kv) == [SR.work_elements(ops, r, rings, addr) for r in SR.ranks_of(ops)]
        assert lib.mccs_test_fake_destroy_graph(7) >= 1
        # one group, both lists: one launch, a rank's calls paired over the whole group in issue order
        both = list(a) + list(b)
        addr = lambda i: _addr(i) if i < len(a) else addr_b(i - len(a))
        _issue(comms, both, addr=addr)
        launches = _launches()
        assert len(launches) == 1 and launches[0]["grid"].endswith("x4")
        assert _elems(launches[0]) == [SR.work_elements(both, r, rings, addr) for r in range(n)]
        # batch_send_recv is one group of one comm
        C.batch_send_recv(comms[1], [("send", _addr(0), 5, None, 2), ("recv", _addr(1), 3, C.AllReduceDataType.Int32, 0),
                                     ("send", _addr(2), 9, U8, 2)], stream=0)
        (kv,) = _launches()
        ops = [SR.S(1, 2, 5), SR.R(1, 0, 12), SR.S(1, 2, 9)]
        assert _elems(kv)[0] == SR.work_elements(ops, 1, rings, _addr)
    finally:
        for c in comms:
            c.destroy()


def test_zero_byte_calls(fake):  # noqa: F811
    fake(1)
    comms = C.init_all([0] * 2, C.CommConfig(buffer_size=SR.BUFF))
    try:
        _log()
        C.send(comms[0], None, 0, U8, 1, stream=0)  # succeeds, launches nothing
        C.recv(comms[1], _addr(0), 0, U8, 0, stream=0)
        with C.group():
            C.send(comms[0], None, 0, U8, 1, stream=0)
            C.recv(comms[1], None, 0, U8, 0, stream=0)
        assert not _launches()
        with C.group():  # beside a live call the empty one keeps its place in the queue
            C.send(comms[0], None, 0, U8, 1, stream=0)
            C.send(comms[0], _addr(1), 64, U8, 1, stream=0)
        (kv,) = _launches()
        assert [[(e["count"], e["send"]) for e in ch] for ch in _elems(kv)[0]] == \
            [[(0, 0), (64, _addr(1))]] * comms[0].nchannels
    finally:
        for c in comms:
            c.destroy()


def _refused(code, start, call):
    with pytest.raises(MccsError) as ei:
        call()
    assert ei.value.code == code, (ei.value.code, _lib.last_error())
    assert _lib.last_error().startswith(start), _lib.last_error()


def test_argument_refusals(fake):  # noqa: F811
    fake(1)
    comms = C.init_all([0] * 3, C.CommConfig(buffer_size=SR.BUFF))
    one = C.init_all([0], C.CommConfig(buffer_size=SR.BUFF))
    c = comms[1]
    try:
        _log()
        for fn, name in ((C.send, "mccsSend"), (C.recv, "mccsRecv")):
            _refused(INVALID_ARGUMENT, f"{name}: peer 3 outside 0..2", lambda: fn(c, _addr(0), 8, U8, 3, stream=0))
            _refused(INVALID_ARGUMENT, f"{name}: peer -1 outside 0..2", lambda: fn(c, _addr(0), 8, U8, -1, stream=0))
            _refused(INVALID_ARGUMENT, f"{name}: peer is the calling rank", lambda: fn(c, _addr(0), 8, U8, 1, stream=0))
            _refused(INVALID_ARGUMENT, f"{name}: null buffer with a non-zero count",
                     lambda: fn(c, None, 8, U8, 0, stream=0))
            _refused(INVALID_ARGUMENT, f"{name}: unknown dtype", lambda: fn(c, _addr(0), 8, 99, 0, stream=0))
            _refused(INVALID_ARGUMENT, f"{name}: a communicator of one rank has no peer",
                     lambda: fn(one[0], _addr(0), 8, U8, 0, stream=0))
        assert not _launches()
        C.send(c, _addr(0), 8, U8, 0, stream=0)  # the comm stays usable
        assert len(_launches()) == 1
    finally:
        for x in comms + one:
            x.destroy()


def test_mixing_with_another_function_in_a_group_is_refused(fake):  # noqa: F811
    fake(2)
    comms = C.init_all([0, 1], C.CommConfig(buffer_size=SR.BUFF))
    lib = _lib.load()
    try:
        _log()
        assert lib.mccsGroupStart() == 0
        assert lib.mccsSend(_addr(0), 8, int(U8), 1, comms[0]._h, 0) == 0
        assert lib.mccsAllToAll(_addr(0), _addr(1), 4096, comms[0]._h, 0) == INVALID_USAGE
        assert _lib.last_error().startswith("mccsAllToAll"), _lib.last_error()
        assert lib.mccsGroupEnd() == INVALID_USAGE
        assert lib.mccsGroupStart() == 0
        assert lib.mccsAllReduce(_addr(0), _addr(1), 4096, 7, 0, comms[0]._h, 0) == 0
        assert lib.mccsRecv(_addr(0), 8, int(U8), 1, comms[0]._h, 0) == INVALID_USAGE
        assert _lib.last_error().startswith("mccsRecv") and "mixes collectives" in _lib.last_error(), _lib.last_error()
        assert lib.mccsGroupEnd() == INVALID_USAGE
        assert not _launches()
        with C.group():  # the comms stay usable, and nothing of the refused groups is left queued
            C.send(comms[0], _addr(0), 8, U8, 1, stream=0)
            C.recv(comms[1], _addr(1), 8, U8, 0, stream=0)
        launches = _launches()
        assert len(launches) == 2  # two devices
        assert all(len(ch) == 1 for kv in launches for ch in _elems(kv)[0])
    finally:
        for c in comms:
            c.destroy()


def test_a_group_keeps_its_first_error(fake):  # noqa: F811
    fake(2)
    comms = C.init_all([0, 1], C.CommConfig(buffer_size=SR.BUFF))
    lib = _lib.load()
    try:
        assert lib.mccsGroupStart() == 0
        assert lib.mccsSend(_addr(0), 8, int(U8), 0, comms[0]._h, 0) == INVALID_ARGUMENT
        assert lib.mccsRecv(0, 8, int(U8), 0, comms[1]._h, 0) == INVALID_ARGUMENT
        assert lib.mccsGroupEnd() == INVALID_ARGUMENT
        assert _lib.last_error().startswith("mccsSend: peer is the calling rank"), _lib.last_error()
    finally:
        for c in comms:
            c.destroy()


@pytest.mark.parametrize("how", ["six ranks", "env", "one channel", "user rings"])
def test_a_relay_route_is_refused_and_named(fake, monkeypatch, how):  # noqa: F811
    fake(1)
    n = 6 if how == "six ranks" else 5 if how == "user rings" else 4
    if how == "env":
        monkeypatch.setenv("MCCS_ALLTOALL_HOPS", "relay")
    cfg = C.CommConfig(buffer_size=SR.BUFF, channel_count=1 if how == "one channel" else None,
                       rings=[[(i * 2) % 5 for i in range(5)]] * 3 if how == "user rings" else None)
    if how == "user rings":
        cfg.channel_count = 3
    comms = C.init_all([0] * n, cfg)
    try:
        _log()
        assert comms[0].all_to_all_route()["hops"] == n - 1
        for fn, name in ((C.send, "mccsSend"), (C.recv, "mccsRecv")):
            _refused(INVALID_USAGE, f"{name}: the AllToAll route is not one hop",
                     lambda: fn(comms[0], _addr(0), 8, U8, 1, stream=0))
            err = _lib.last_error()
            assert f"hops = {n - 1}" in err and ("MCCS_ALLTOALL_HOPS=relay" in err) == (how == "env"), err
        assert not _launches()
        with C.group():  # the comms stay usable
            for r, c in enumerate(comms):
                C.all_to_all(c, _addr(r), _addr(r, 0x200000), 64, stream=0)
        assert len(_launches()) == 1
    finally:
        for c in comms:
            c.destroy()


def test_c_abi_declaration_compiles_as_c(tmp_path):
    src = tmp_path / "sr.c"
    src.write_text('#include "mccs_hip.h"\n'
                   "mccsResult_t f(const void *s, void *r, mccsComm_t comm, hipStream_t st) {\n"
                   "  mccsResult_t e = mccsSend(s, 4, 7, 1, comm, st);\n"
                   "  return e ? e : mccsRecv(r, 4, 7, 1, comm, st);\n}\n"
                   "mccsResult_t g(const int *i, void *const *b, const size_t *c) {\n"
                   "  return mccs_host_ring_send_recv(2, 2, i, i, i, b, c, 4, 544, 1 << 16, 0);\n}\n")
    r = subprocess.run(build.capi_cmd(str(src), str(tmp_path / "unused"), syntax_only=True), capture_output=True,
                       text=True)
    assert r.returncode == 0, r.stderr
