"""CPU: how the planner launches an AllToAllvDev, on the recording fake device
runtime (see tests/test_all_to_all_v_plan.py).  The host knows no count, so
every channel carries its FIFO element and its self element whatever the
sizes turn out to be; the launch record's a2avd= key gives each element's
route word, bid, nChannels, count (the size table's address), redOpArg (0) and
the two base pointers, held here against tests/a2avd_ref.py's model.  Then
captured and batched launches, and every refusal of the entry point.
"""
import ctypes
import subprocess

import pytest

import a2avd_ref as D
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
    return 0x10000000 * (r + 1)  # the fake never touches "device" memory


def _recv(r):
    return _send(r) + 0x8000000


def _table(r, k=0):
    return _send(r) + 0x4000000 + 0x1000 * k


def _group(comms, off=0, k=0, stream=0):
    with C.group():
        for r, c in enumerate(comms):
            C.all_to_all_v_dev(c, _send(r) + off, _recv(r) + off, _table(r, k), stream=stream)


def _elems(kv):
    """a2avd= of a launch: per rank slot a list of dicts."""
    out = []
    for slot in kv["a2avd"].split("/"):
        es = []
        for e in slot.split(","):
            route, bid, nch, count, arg, send, recv = e.split(":")
            route = int(route, 16)
            es.append({"hops": route & 0xff, "recv_bid": route >> 8 & 0xff, "part": route >> 16 & 0xff,
                       "parts": route >> 24, "bid": int(bid), "nch": int(nch), "count": int(count), "arg": int(arg),
                       "send": int(send, 16), "recv": int(recv, 16)})
        out.append(es)
    return out


def _want(n, rings, r, off=0, k=0):
    return D.want_elements(n, rings, r, _send(r) + off, _recv(r) + off, _table(r, k))


@pytest.mark.parametrize("n", [2, 3, 4, 8])
def test_every_channel_carries_both_elements(fake, n):
    fake(1)
    comms = C.init_all([0] * n, C.CommConfig(buffer_size=V.BUFF))
    try:
        _log()
        rings = comms[0].rings()
        assert comms[0].all_to_all_route()["hops"] == 1
        _group(comms)
        launches = [kv for k, kv in _log() if k == "launch"]
        assert len(launches) == 1 and launches[0]["kind"] == "ring", launches
        gx, gy = (int(v) for v in launches[0]["grid"].split("x"))
        assert gy == n and gx == comms[0].nchannels * comms[0].lanes
        assert launches[0]["inline_works"] == "0"  # two elements per channel: the work FIFO
        got = _elems(launches[0])
        for r in range(n):
            want = _want(n, rings, r)
            assert len(want) == 2 * len(rings)
            assert got[r] == want, r
            # the pointers are the call's own, the count is the table, whatever the sizes will be
            assert all(e["send"] == _send(r) and e["recv"] == _recv(r) and e["count"] == _table(r) and e["arg"] == 0
                       for e in got[r])
            assert [e["hops"] for e in got[r]] == [1, 0] * len(rings)
            assert [(e["part"], e["parts"]) for e in got[r] if e["hops"] == 0] == [(c, len(rings))
                                                                                    for c in range(len(rings))]
        assert all(c.last_algo() == "ring" for c in comms)
        assert "a2av" not in launches[0] and "a2a" not in launches[0]
    finally:
        for c in comms:
            c.destroy()


def test_one_rank_is_the_self_element_and_still_the_fifo(fake):
    fake(1)
    comms = C.init_all([0], C.CommConfig(buffer_size=V.BUFF))
    try:
        _log()
        C.all_to_all_v_dev(comms[0], _send(0), _recv(0), _table(0), stream=0)
        launches = [kv for k, kv in _log() if k == "launch"]
        assert len(launches) == 1 and launches[0]["inline_works"] == "0", launches
        es = _elems(launches[0])[0]
        assert es == _want(1, comms[0].rings(), 0)
        assert len(es) == comms[0].nchannels and "a2av" not in launches[0]
    finally:
        comms[0].destroy()


def test_captured_and_batched_launches_carry_their_own_elements(fake):
    fake(1)
    lib = _lib.load()
    n = 4
    comms = C.init_all([0] * n, C.CommConfig(buffer_size=V.BUFF))
    try:
        _log()
        rings = comms[0].rings()
        stream = 0x5000
        assert lib.mccs_test_fake_capture(stream, 7) == 0
        _group(comms, stream=stream)
        _group(comms, off=0x400000, k=1, stream=stream)
        assert lib.mccs_test_fake_capture(stream, 0) == 0
        launches = [kv for k, kv in _log() if k == "launch"]
        assert len(launches) == 2 and all(kv["inline_works"] == "0" for kv in launches), launches
        for kv, (off, k) in zip(launches, ((0, 0), (0x400000, 1))):
            assert _elems(kv) == [_want(n, rings, r, off, k) for r in range(n)]
            assert "a2av" not in kv
        assert lib.mccs_test_fake_destroy_graph(7) >= 1
        # one group, two calls with tables of their own: one launch, each channel's elements in issue order
        with C.group():
            for off, k in ((0, 0), (0x400000, 1)):
                for r, c in enumerate(comms):
                    C.all_to_all_v_dev(c, _send(r) + off, _recv(r) + off, _table(r, k), stream=0)
        launches = [kv for k, kv in _log() if k == "launch"]
        assert len(launches) == 1 and launches[0]["grid"].endswith("x4") and launches[0]["inline_works"] == "0"
        got = _elems(launches[0])
        for r in range(n):
            wa, wb = _want(n, rings, r), _want(n, rings, r, 0x400000, 1)
            want = []
            for c in range(len(rings)):
                want += wa[2 * c:2 * c + 2] + wb[2 * c:2 * c + 2]
            assert got[r] == want, r
    finally:
        for c in comms:
            c.destroy()


def _refused(code, start, call):
    with pytest.raises(MccsError) as ei:
        call()
    assert ei.value.code == code, (ei.value.code, _lib.last_error())
    assert _lib.last_error().startswith(start), _lib.last_error()


def test_argument_refusals(fake):
    fake(2)
    comms = C.init_all([0, 1], C.CommConfig(buffer_size=V.BUFF))
    c = comms[0]
    v = lambda **kw: lambda: C.all_to_all_v_dev(c, kw.get("send", _send(0)), kw.get("recv", _recv(0)),
                                                kw.get("table", _table(0)), stream=0)
    try:
        _log()
        _refused(INVALID_ARGUMENT, "mccsAllToAllvDev: null size table", v(table=None))
        _refused(INVALID_ARGUMENT, "mccsAllToAllvDev: null size table", v(table=0))
        for off in (1, 4, 7):
            _refused(INVALID_ARGUMENT, "mccsAllToAllvDev: the size table is not 8-byte aligned",
                     v(table=_table(0) + off))
        _refused(INVALID_ARGUMENT, "mccsAllToAllvDev: null buffer", v(send=None))
        _refused(INVALID_ARGUMENT, "mccsAllToAllvDev: null buffer", v(recv=None))
        assert not any(k == "launch" for k, _ in _log())
        _group(comms)  # the comms stay usable
        assert sum(1 for k, _ in _log() if k == "launch") == 2  # one device each
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
        _refused(INVALID_USAGE, "mccsAllToAllvDev: the AllToAll route is not one hop",
                 lambda: C.all_to_all_v_dev(comms[0], _send(0), _recv(0), _table(0), stream=0))
        err = _lib.last_error()
        assert f"hops = {n - 1}" in err and ("MCCS_ALLTOALL_HOPS=relay" in err) == (how == "env"), err
        # the same diagnosis as the host-count call's
        cnt = [[8] * n for _ in range(n)]
        lay = V.layout(cnt, "packed")
        with pytest.raises(MccsError):
            C.all_to_all_v(comms[0], _send(0), cnt[0], lay["sdispls"][0], _recv(0), cnt[0], lay["rdispls"][0], stream=0)
        assert _lib.last_error().split(": ", 1)[1] == err.split(": ", 1)[1]
        assert not any(k == "launch" for k, _ in _log())
        with C.group():  # the comms stay usable
            for r, c in enumerate(comms):
                C.all_to_all(c, _send(r), _recv(r), 64, stream=0)
        assert sum(1 for k, _ in _log() if k == "launch") == 1
    finally:
        for c in comms:
            c.destroy()


def test_mixing_with_the_host_count_call_in_a_group_is_refused(fake):
    fake(2)
    comms = C.init_all([0, 1], C.CommConfig(buffer_size=V.BUFF))
    lib = _lib.load()
    sz = lambda *v: (ctypes.c_size_t * len(v))(*v)
    hostv = lambda: lib.mccsAllToAllv(_send(0), sz(8, 8), sz(0, 8), _recv(0), sz(8, 8), sz(0, 8), comms[0]._h, 0)
    devv = lambda: lib.mccsAllToAllvDev(_send(0), _recv(0), _table(0), comms[0]._h, 0)
    try:
        _log()
        assert lib.mccsGroupStart() == 0
        assert hostv() == 0
        assert devv() == INVALID_USAGE
        assert _lib.last_error().startswith("mccsAllToAllvDev"), _lib.last_error()
        assert "mixes collectives" in _lib.last_error()
        assert lib.mccsGroupEnd() == INVALID_USAGE
        assert lib.mccsGroupStart() == 0
        assert devv() == 0
        assert hostv() == INVALID_USAGE
        assert _lib.last_error().startswith("mccsAllToAllv:"), _lib.last_error()
        assert lib.mccsGroupEnd() == INVALID_USAGE
        assert lib.mccsGroupStart() == 0
        assert devv() == 0
        assert lib.mccsAllToAll(_send(0), _recv(0), 4096, comms[0]._h, 0) == INVALID_USAGE
        assert lib.mccsGroupEnd() == INVALID_USAGE
        assert not any(k == "launch" for k, _ in _log())
        _group(comms)  # the comms stay usable
        assert sum(1 for k, _ in _log() if k == "launch") == 2
    finally:
        for c in comms:
            c.destroy()


def test_the_table_argument_of_the_python_face(fake):
    torch = pytest.importorskip("torch")
    fake(1)
    comms = C.init_all([0, 0], C.CommConfig(buffer_size=V.BUFF))
    try:
        for bad in (torch.zeros(8, dtype=torch.int32), torch.zeros(7, dtype=torch.int64),
                    torch.zeros(8, dtype=torch.float64)):
            with pytest.raises(ValueError):
                C.all_to_all_v_dev(comms[0], _send(0), _recv(0), bad, stream=0)
            with pytest.raises(ValueError):
                C.exchange_counts(comms[0], bad, stream=0)
        with pytest.raises(ValueError):  # a host tensor is not memory the GPU reads
            C.all_to_all_v_dev(comms[0], _send(0), _recv(0), torch.zeros(8, dtype=torch.int64), stream=0)
        _log()
        # exchange_counts: the uniform call, 8 bytes per peer, row 0 -> row 2
        with C.group():
            for r, c in enumerate(comms):
                c.exchange_counts(_table(r), stream=0)
        launches = [kv for k, kv in _log() if k == "launch"]
        assert len(launches) == 1 and "a2a" in launches[0] and "a2avd" not in launches[0]
    finally:
        for c in comms:
            c.destroy()


def test_the_table_index_is_the_librarys():
    lib = _lib.load()
    for n in (1, 2, 5, 8, 64):
        for row in range(4):
            for peer in (0, n // 2, n - 1):
                assert lib.mccs_a2avd_index(row, n, peer) == D.index(row, n, peer)
    assert lib.mccs_a2avd_index(4, 2, 0) == -1 and lib.mccs_a2avd_index(0, 2, 2) == -1


def test_c_abi_declaration_compiles_as_c(tmp_path):
    src = tmp_path / "v.c"
    src.write_text('#include "mccs_hip.h"\n'
                   "mccsResult_t f(const void *s, void *r, const uint64_t *t, mccsComm_t comm, hipStream_t st) {\n"
                   "  return mccsAllToAllvDev(s, r, t, comm, st);\n}\n"
                   "mccsResult_t g(const void *const *s, void *const *r, const uint64_t *const *t) {\n"
                   "  return mccs_host_ring_all_to_all_v_tables(2, s, r, t, 4, 544, 1 << 16, 0, 0);\n}\n")
    r = subprocess.run(build.capi_cmd(str(src), str(tmp_path / "unused"), syntax_only=True), capture_output=True,
                       text=True)
    assert r.returncode == 0, r.stderr
