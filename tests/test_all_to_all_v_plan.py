"""CPU: how the planner launches an AllToAllv, on the recording fake device
runtime (see tests/test_all_to_all_plan.py).  Every channel runs; per channel
the launch record's a2av= key gives each element's route word, bid, nChannels,
count, redOpArg and the two pre-offset buffers, held here against
tests/a2a_ref.py's route and tests/a2av_ref.py's (S, R) per channel.  Then
captured and batched launches, and every refusal of the entry point.
"""
import ctypes
import os
import subprocess

import pytest

import a2a_ref
import a2av_ref as V
from mccs_amd import _lib
from mccs_amd import build
from mccs_amd import comm as C
from mccs_amd._lib import MccsError

INVALID_ARGUMENT, INVALID_USAGE = 4, 5


def _parse(line):
    kind, *kv = line.split()
    return kind, dict(x.split("=", 1) for x in kv)


@pytest.fixture
def fake(monkeypatch):
    lib = _lib.load()
    monkeypatch.setenv("MCCS_TEST_HOOKS", "1")
    monkeypatch.setenv("MCCS_GATE", "0")
    monkeypatch.delenv("MCCS_ALLTOALL_HOPS", raising=False)

    def install(ndev):
        assert lib.mccs_test_fake_runtime(ndev) == 0

    yield install
    lib.mccs_test_fake_runtime(0)


def _log():
    lib = _lib.load()
    n = lib.mccs_test_fake_log(None, 0, 0)
    assert n >= 0, "fake runtime not installed"
    buf = ctypes.create_string_buffer(n + 1)
    lib.mccs_test_fake_log(buf, n + 1, 1)
    return [_parse(x) for x in buf.value.decode().splitlines() if x]


def _send(r):
    return 0x10000000 * (r + 1)  # the fake never touches "device" buffers


def _recv(r):
    return _send(r) + 0x8000000


def _group(comms, cnt, lay, off=0, stream=0):
    n = len(comms)
    with C.group():
        for r, c in enumerate(comms):
            C.all_to_all_v(c, _send(r) + off, cnt[r], lay["sdispls"][r], _recv(r) + off,
                           [cnt[s][r] for s in range(n)], lay["rdispls"][r], stream=stream)


def _elems(kv):
    """a2av= of a launch: per rank slot a list of dicts."""
    out = []
    for slot in kv["a2av"].split("/"):
        es = []
        for e in slot.split(","):
            route, bid, nch, count, arg, send, recv = e.split(":")
            route = int(route, 16)
            es.append({"hops": route & 0xff, "recv_bid": route >> 8 & 0xff, "part": route >> 16 & 0xff,
                       "parts": route >> 24, "bid": int(bid), "nch": int(nch), "count": int(count), "arg": int(arg),
                       "send": int(send, 16), "recv": int(recv, 16)})
        out.append(es)
    return out


def _want(n, rings, cnt, lay, r, off=0):
    """Rank r's elements in channel order: the FIFO element, then the self element if any."""
    model = a2a_ref.route(n, rings)
    nxt, prv = V.ring_next_prev(rings, n)
    out = []
    for c in range(len(rings)):
        t, p = nxt[c][r], prv[c][r]
        out.append({"hops": 1, "recv_bid": model["recv_bid"][r][c], "part": 0, "parts": 0,
                    "bid": model["send_bid"][r][c], "nch": model["m"], "count": cnt[r][t], "arg": cnt[p][r],
                    "send": _send(r) + off + lay["sdispls"][r][t], "recv": _recv(r) + off + lay["rdispls"][r][p]})
        if cnt[r][r]:
            out.append({"hops": 0, "recv_bid": 0, "part": c, "parts": len(rings), "bid": 0, "nch": 1,
                        "count": cnt[r][r], "arg": 0, "send": _send(r) + off + lay["sdispls"][r][r],
                        "recv": _recv(r) + off + lay["rdispls"][r][r]})
    return out


@pytest.mark.parametrize("n,mat", [(8, "cyc5"), (8, "zero_self"), (4, "s1r3"), (4, "zero_row"), (2, "s3r0"),
                                   (3, "zero_col")])
def test_every_channel_carries_its_pair(fake, n, mat):
    fake(1)
    comms = C.init_all([0] * n, C.CommConfig(buffer_size=V.BUFF))
    try:
        _log()
        rings = comms[0].rings()
        route = comms[0].all_to_all_route()
        assert route["hops"] == 1
        cnt = V.matrices(n, route["m"], rings)[mat]
        lay = V.layout(cnt, "gaps")
        _group(comms, cnt, lay)
        launches = [kv for k, kv in _log() if k == "launch"]
        assert len(launches) == 1 and launches[0]["kind"] == "ring", launches
        gx, gy = (int(v) for v in launches[0]["grid"].split("x"))
        assert gy == n and gx == comms[0].nchannels * comms[0].lanes  # every channel, whatever the sizes
        got = _elems(launches[0])
        for r in range(n):
            assert got[r] == _want(n, rings, cnt, lay, r), r
        has_self = any(cnt[r][r] for r in range(n))
        assert any(e["hops"] == 0 for slot in got for e in slot) == has_self
        assert all(c.last_algo() == "ring" for c in comms)
        assert "a2a" not in launches[0]
    finally:
        for c in comms:
            c.destroy()


def test_one_rank_is_the_self_copy(fake):
    fake(1)
    comms = C.init_all([0], C.CommConfig(buffer_size=V.BUFF))
    try:
        _log()
        C.all_to_all_v(comms[0], _send(0), [4099], [7], _recv(0), [4099], [21], stream=0)
        launches = [kv for k, kv in _log() if k == "launch"]
        assert len(launches) == 1
        es = _elems(launches[0])[0]
        assert all(e["hops"] == 0 and e["count"] == 4099 and e["send"] == _send(0) + 7 and e["recv"] == _recv(0) + 21
                   for e in es)
        assert [e["bid"] for e in es] == list(range(len(es))) and all(e["nch"] == len(es) for e in es)
        C.all_to_all_v(comms[0], None, [0], [0], None, [0], [0], stream=0)
        assert not any(k == "launch" for k, _ in _log())
    finally:
        comms[0].destroy()


def test_captured_and_batched_launches_carry_their_own_elements(fake):
    fake(1)
    lib = _lib.load()
    n = 4
    comms = C.init_all([0] * n, C.CommConfig(buffer_size=V.BUFF))
    try:
        _log()
        rings, m = comms[0].rings(), comms[0].all_to_all_route()["m"]
        mats = V.matrices(n, m, rings)
        a, b = mats["s1r3"], mats["cyc5"]
        la, lb = V.layout(a, "descending"), V.layout(b, "misaligned")
        stream = 0x5000
        assert lib.mccs_test_fake_capture(stream, 7) == 0
        _group(comms, a, la, stream=stream)
        _group(comms, b, lb, off=0x400000, stream=stream)
        assert lib.mccs_test_fake_capture(stream, 0) == 0
        launches = [kv for k, kv in _log() if k == "launch"]
        assert len(launches) == 2 and all(kv["inline_works"] == "0" for kv in launches), launches
        for kv, (cnt, lay, off) in zip(launches, ((a, la, 0), (b, lb, 0x400000))):
            assert _elems(kv) == [_want(n, rings, cnt, lay, r, off) for r in range(n)]
        assert lib.mccs_test_fake_destroy_graph(7) >= 1
        # one group, two matrices: one launch, each channel's elements in issue order
        with C.group():
            for cnt, lay, off in ((a, la, 0), (b, lb, 0x400000)):
                for r, c in enumerate(comms):
                    C.all_to_all_v(c, _send(r) + off, cnt[r], lay["sdispls"][r], _recv(r) + off,
                                   [cnt[s][r] for s in range(n)], lay["rdispls"][r], stream=0)
        launches = [kv for k, kv in _log() if k == "launch"]
        assert len(launches) == 1 and launches[0]["grid"].endswith("x4")
        got = _elems(launches[0])
        for r in range(n):
            wa, wb = _want(n, rings, a, la, r), _want(n, rings, b, lb, r, 0x400000)
            per_a, per_b = len(wa) // len(rings), len(wb) // len(rings)
            want = []
            for c in range(len(rings)):
                want += wa[c * per_a:(c + 1) * per_a] + wb[c * per_b:(c + 1) * per_b]
            assert got[r] == want, r
    finally:
        for c in comms:
            c.destroy()


def test_a_call_without_a_self_block_rides_inline(fake):
    """One element per channel goes in the launch arguments; the self element
    makes two, which take the work FIFO."""
    fake(1)
    comms = C.init_all([0] * 2, C.CommConfig(buffer_size=V.BUFF))
    try:
        _log()
        for self_bytes, inline in ((0, True), (64, False)):
            cnt = [[self_bytes, 100], [200, self_bytes]]
            _group(comms, cnt, V.layout(cnt, "packed"))
            kv = [kv for k, kv in _log() if k == "launch"][0]
            assert (kv["inline_works"] != "0") == inline, kv
    finally:
        for c in comms:
            c.destroy()


def test_mixing_with_another_function_in_a_group_is_refused(fake):
    fake(2)
    comms = C.init_all([0, 1], C.CommConfig(buffer_size=V.BUFF))
    lib = _lib.load()
    sz = lambda *v: (ctypes.c_size_t * len(v))(*v)
    try:
        _log()
        assert lib.mccsGroupStart() == 0
        assert lib.mccsAllToAllv(_send(0), sz(8, 8), sz(0, 8), _recv(0), sz(8, 8), sz(0, 8), comms[0]._h, 0) == 0
        assert lib.mccsAllToAll(_send(0), _recv(0), 4096, comms[0]._h, 0) == INVALID_USAGE
        assert _lib.last_error().startswith("mccsAllToAll"), _lib.last_error()
        assert lib.mccsGroupEnd() == INVALID_USAGE
        assert lib.mccsGroupStart() == 0
        assert lib.mccsAllToAll(_send(0), _recv(0), 4096, comms[0]._h, 0) == 0
        assert lib.mccsAllToAllv(_send(0), sz(8, 8), sz(0, 8), _recv(0), sz(8, 8), sz(0, 8), comms[0]._h,
                                 0) == INVALID_USAGE
        assert _lib.last_error().startswith("mccsAllToAllv"), _lib.last_error()
        assert lib.mccsGroupEnd() == INVALID_USAGE
        assert not any(k == "launch" for k, _ in _log())
        cnt = [[8, 8], [8, 8]]
        _group(comms, cnt, V.layout(cnt, "packed"))  # the comms stay usable
        assert sum(1 for k, _ in _log() if k == "launch") == 2
    finally:
        for c in comms:
            c.destroy()


def _refused(code, start, call):
    with pytest.raises(MccsError) as ei:
        call()
    assert ei.value.code == code, (ei.value.code, _lib.last_error())
    assert _lib.last_error().startswith(start), _lib.last_error()


def test_argument_refusals_and_empty_calls(fake):
    fake(2)
    comms = C.init_all([0, 1], C.CommConfig(buffer_size=V.BUFF))
    c = comms[0]  # rank 0
    S, R = _send(0), _recv(0)
    v = lambda **kw: lambda: C.all_to_all_v(
        c, kw.get("send", S), kw.get("sc", [16, 32]), kw.get("sd", [0, 16]), kw.get("recv", R), kw.get("rc", [16, 64]),
        kw.get("rd", [0, 16]), stream=0)
    try:
        _log()
        for name in ("sc", "sd", "rc", "rd"):
            _refused(INVALID_ARGUMENT, "mccsAllToAllv: null count or displacement array", v(**{name: None}))
        _refused(INVALID_ARGUMENT, "mccsAllToAllv: null buffer", v(send=None))
        _refused(INVALID_ARGUMENT, "mccsAllToAllv: null buffer", v(recv=None))
        _refused(INVALID_ARGUMENT, "mccsAllToAllv: sendcounts[rank] != recvcounts[rank]", v(sc=[17, 32]))
        _refused(INVALID_ARGUMENT, "mccsAllToAllv: two receive segments overlap", v(rd=[0, 15]))
        _refused(INVALID_ARGUMENT, "mccsAllToAllv: two receive segments overlap", v(rd=[70, 8]))
        # the receive segment of rank 1 ends on the first byte of the send segment for rank 0
        _refused(INVALID_ARGUMENT, "mccsAllToAllv: a receive segment overlaps a send segment", v(recv=S - 79))
        _refused(INVALID_ARGUMENT, "mccsAllToAllv: a receive segment overlaps a send segment", v(recv=S + 40))
        assert not any(k == "launch" for k, _ in _log())
        # allowed: overlapping send segments, a null buffer on a side that moves nothing, touching segments
        v(sd=[0, 0])()
        v(send=None, sc=[0, 0], rc=[0, 64])()
        v(recv=None, rc=[0, 0], sc=[0, 32])()
        v(recv=S + 48)()  # receive segments start where the last send segment ends
        v(rc=[16, 0], rd=[0, 0])()  # a zero-length segment overlaps nothing
        assert sum(1 for k, _ in _log() if k == "launch") == 5
        # all counts zero: success, nothing launched, whatever the buffers
        v(sc=[0, 0], rc=[0, 0])()
        v(send=None, recv=None, sc=[0, 0], rc=[0, 0])()
        assert not any(k == "launch" for k, _ in _log())
        with pytest.raises(ValueError):
            v(sc=[1, 2, 3])()
    finally:
        for x in comms:
            x.destroy()


@pytest.mark.parametrize("how", ["six ranks", "env", "one channel", "user rings"])
def test_a_relay_route_is_refused_and_named(fake, monkeypatch, how):
    fake(1)
    n = 6 if how == "six ranks" else 5 if how == "user rings" else 4
    if how == "env":
        monkeypatch.setenv("MCCS_ALLTOALL_HOPS", "relay")
    cfg = C.CommConfig(buffer_size=V.BUFF, channel_count=1 if how == "one channel" else None,
                       rings=[[(i * 2) % 5 for i in range(5)]] * 3 if how == "user rings" else None)
    if how == "user rings":
        cfg.channel_count = 3
    comms = C.init_all([0] * n, cfg)
    try:
        _log()
        assert comms[0].all_to_all_route()["hops"] == n - 1
        cnt = [[8] * n for _ in range(n)]
        lay = V.layout(cnt, "packed")
        _refused(INVALID_USAGE, "mccsAllToAllv: the AllToAll route is not one hop",
                 lambda: C.all_to_all_v(comms[0], _send(0), cnt[0], lay["sdispls"][0], _recv(0), cnt[0],
                                        lay["rdispls"][0], stream=0))
        err = _lib.last_error()
        assert f"hops = {n - 1}" in err and ("MCCS_ALLTOALL_HOPS=relay" in err) == (how == "env"), err
        assert not any(k == "launch" for k, _ in _log())
        with C.group():  # the comms stay usable
            for r, c in enumerate(comms):
                C.all_to_all(c, _send(r), _recv(r), 64, stream=0)
        assert sum(1 for k, _ in _log() if k == "launch") == 1
    finally:
        for c in comms:
            c.destroy()


def test_a_group_keeps_its_first_error(fake):
    fake(2)
    comms = C.init_all([0, 1], C.CommConfig(buffer_size=V.BUFF))
    lib = _lib.load()
    sz = lambda *v: (ctypes.c_size_t * len(v))(*v)
    try:
        assert lib.mccsGroupStart() == 0
        assert lib.mccsAllToAllv(_send(0), sz(9, 8), sz(0, 16), _recv(0), sz(8, 8), sz(0, 8), comms[0]._h,
                                 0) == INVALID_ARGUMENT
        assert lib.mccsAllToAllv(_send(1), None, sz(0, 8), _recv(1), sz(8, 8), sz(0, 8), comms[1]._h,
                                 0) == INVALID_ARGUMENT
        assert lib.mccsGroupEnd() == INVALID_ARGUMENT
        assert _lib.last_error().startswith("mccsAllToAllv: sendcounts[rank]"), _lib.last_error()
    finally:
        for c in comms:
            c.destroy()


def test_c_abi_declaration_compiles_as_c(tmp_path):
    src = tmp_path / "v.c"
    src.write_text('#include "mccs_hip.h"\n'
                   "mccsResult_t f(const void *s, const size_t *c, void *r, mccsComm_t comm, hipStream_t st) {\n"
                   "  return mccsAllToAllv(s, c, c, r, c, c, comm, st);\n}\n"
                   "mccsResult_t g(const void *const *s, void *const *r, const size_t *c) {\n"
                   "  return mccs_host_ring_all_to_all_v(2, s, r, c, c, c, 4, 544, 1 << 16, 0, 0);\n}\n")
    r = subprocess.run(build.capi_cmd(str(src), str(tmp_path / "unused"), syntax_only=True), capture_output=True,
                       text=True)
    assert r.returncode == 0, r.stderr
