"""CPU: how the planner launches an AllToAll, on the recording fake device
runtime (csrc/host/rt.cpp, mccs_test_fake_runtime: host memory, no kernel runs;
see tests/test_reduce_scatter_plan.py).  One ring launch per device over all
the comm's channels in one-hop mode, task_schema's channels in relay mode, the
route carried by every work element (the launch record's a2a= key:
hops:bid:recv_bid:nChannels per element), batching, and the refusals.
"""
import ctypes
import os
import subprocess

import pytest

import a2a_ref
from mccs_amd import _lib
from mccs_amd import build
from mccs_amd import comm as C
from mccs_amd._lib import MccsError

F32, SUM = 7, 0
INVALID_ARGUMENT, INVALID_USAGE = 4, 5


def _parse(line):
    kind, *kv = line.split()
    return kind, dict(x.split("=", 1) for x in kv)


@pytest.fixture
def fake(monkeypatch):
    lib = _lib.load()
    monkeypatch.setenv("MCCS_TEST_HOOKS", "1")  # the hook is refused without it
    monkeypatch.setenv("MCCS_GATE", "0")  # the fake runs no kernel: the node gate's sums would never match
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


def _a2a_group(comms, nbytes, off=0):
    with C.group():
        for r, c in enumerate(comms):
            C.all_to_all(c, _send(r) + off, _recv(r) + off, nbytes, stream=0)


def _routes(kv):
    """a2a= of a launch record: per rank slot a list of (hops, bid, recv_bid, nChannels)."""
    return [[tuple(int(v) for v in e.split(":")) for e in slot.split(",")] for slot in kv["a2a"].split("/")]


@pytest.mark.parametrize("nbytes", [1 << 20, 8])
def test_eight_devices_one_hop_uses_every_channel(fake, nbytes):
    fake(8)
    comms = C.init_all(list(range(8)), C.CommConfig(buffer_size=1 << 20))
    try:
        _log()
        nch, lanes = comms[0].nchannels, comms[0].lanes
        assert nch == 7 and all(c.all_to_all_route() == {"hops": 1, "m": 1} for c in comms)
        _a2a_group(comms, nbytes)  # 8 bytes per peer too: every arc is some pair's only way
        ev = _log()
        launches = [(i, kv) for i, (k, kv) in enumerate(ev) if k == "launch"]
        assert sorted(int(kv["dev"]) for _, kv in launches) == list(range(8)), ev
        model = a2a_ref.route(8, comms[0].rings())
        for _, kv in launches:
            assert kv["kind"] == "ring" and kv["grid"] == f"{nch * lanes}x1" and kv["comms_on_dev"] == "1", kv
            r = int(kv["dev"])
            assert _routes(kv) == [[(1, model["send_bid"][r][c], model["recv_bid"][r][c], 1) for c in range(nch)]]
        last = max(i for i, _ in launches)
        waits = [i for i, (k, _) in enumerate(ev) if k == "host_wait"]
        assert not waits or min(waits) > last, f"host waited before every rank was launched: {ev}"
        assert all(c.last_algo() == "ring" for c in comms)
        for c in comms:
            c.sync()
    finally:
        for c in comms:
            c.destroy()


def test_four_ranks_on_one_device_are_one_fused_launch_with_per_rank_parts(fake):
    fake(1)
    comms = C.init_all([0] * 4, C.CommConfig(buffer_size=1 << 20))
    try:
        _log()
        assert comms[0].all_to_all_route() == {"hops": 1, "m": 2}
        _a2a_group(comms, 4099)
        launches = [kv for k, kv in _log() if k == "launch"]
        assert len(launches) == 1, launches
        gx, gy = (int(v) for v in launches[0]["grid"].split("x"))
        assert gy == 4 and gx == comms[0].nchannels * comms[0].lanes and launches[0]["kind"] == "ring"
        model = a2a_ref.route(4, comms[0].rings())
        want = [[(1, model["send_bid"][r][c], model["recv_bid"][r][c], 2) for c in range(6)] for r in range(4)]
        assert _routes(launches[0]) == want
        # the two parts differ somewhere: the kernel cannot take recv_bid for bid
        assert any(e[1] != e[2] for slot in want for e in slot)
    finally:
        for c in comms:
            c.destroy()


@pytest.mark.parametrize("how", ["six ranks", "env", "one channel"])
def test_relay_follows_task_schema(fake, monkeypatch, how):
    fake(1)
    n = 6 if how == "six ranks" else 4
    if how == "env":
        monkeypatch.setenv("MCCS_ALLTOALL_HOPS", "relay")
    cfg = C.CommConfig(buffer_size=1 << 20, channel_count=1 if how == "one channel" else None)
    comms = C.init_all([0] * n, cfg)
    try:
        _log()
        nch, lanes = comms[0].nchannels, comms[0].lanes
        assert comms[0].all_to_all_route() == {"hops": n - 1, "m": 0}
        for nbytes in (8, 40000, 1 << 20):
            want_ch, _ = C.task_schema(nbytes * n, nch)
            _a2a_group(comms, nbytes)
            launches = [kv for k, kv in _log() if k == "launch"]
            assert len(launches) == 1 and launches[0]["grid"] == f"{want_ch * lanes}x{n}", (nbytes, launches)
            assert _routes(launches[0]) == [[(n - 1, b, b, want_ch) for b in range(want_ch)]] * n
            assert all(c.last_algo() == "ring" for c in comms)
    finally:
        for c in comms:
            c.destroy()


def test_a_captured_launch_keeps_the_route(fake):
    fake(1)
    lib = _lib.load()
    comms = C.init_all([0] * 4, C.CommConfig(buffer_size=1 << 20))
    try:
        _log()
        stream = 0x5000
        assert lib.mccs_test_fake_capture(stream, 7) == 0
        with C.group():
            for r, c in enumerate(comms):
                C.all_to_all(c, _send(r), _recv(r), 70001, stream=stream)
        assert lib.mccs_test_fake_capture(stream, 0) == 0
        launches = [kv for k, kv in _log() if k == "launch"]
        assert len(launches) == 1 and launches[0]["inline_works"] == "0", launches  # the graph work arena
        model = a2a_ref.route(4, comms[0].rings())
        assert _routes(launches[0]) == [[(1, model["send_bid"][r][c], model["recv_bid"][r][c], 2) for c in range(6)]
                                        for r in range(4)]
        assert lib.mccs_test_fake_destroy_graph(7) >= 1
    finally:
        for c in comms:
            c.destroy()


def test_a_batched_group_of_three_sizes_is_one_launch(fake):
    fake(1)
    comms = C.init_all([0] * 4, C.CommConfig(buffer_size=1 << 20))
    try:
        _log()
        with C.group():
            for j, nbytes in enumerate((15, 4099, 300000)):
                for r, c in enumerate(comms):
                    C.all_to_all(c, _send(r) + j * 0x200000, _recv(r) + j * 0x200000, nbytes, stream=0)
        launches = [kv for k, kv in _log() if k == "launch"]
        assert len(launches) == 1 and launches[0]["grid"].endswith("x4") and launches[0]["kind"] == "ring", launches
        slots = _routes(launches[0])
        assert len(slots) == 4 and all(len(s) == 3 * 6 for s in slots)  # three elements on each of six channels
    finally:
        for c in comms:
            c.destroy()


def test_mixing_with_allgather_in_a_group_is_refused(fake):
    fake(2)
    comms = C.init_all([0, 1], C.CommConfig(buffer_size=1 << 20))
    lib = _lib.load()
    try:
        _log()
        assert lib.mccsGroupStart() == 0
        for r, c in enumerate(comms):
            assert lib.mccsAllToAll(_send(r), _recv(r), 4096, c._h, 0) == 0
        assert lib.mccsAllGather(_send(0), _recv(0), 4096, comms[0]._h, 0) == INVALID_USAGE
        assert _lib.last_error().startswith("mccsAllGather"), _lib.last_error()
        assert lib.mccsGroupEnd() == INVALID_USAGE
        assert not any(k == "launch" for k, _ in _log())
        assert lib.mccsGroupStart() == 0
        assert lib.mccsAllGather(_send(0), _recv(0), 4096, comms[0]._h, 0) == 0
        assert lib.mccsAllToAll(_send(0), _recv(0), 4096, comms[0]._h, 0) == INVALID_USAGE
        assert _lib.last_error().startswith("mccsAllToAll"), _lib.last_error()
        assert lib.mccsGroupEnd() == INVALID_USAGE
        assert not any(k == "launch" for k, _ in _log())
        _a2a_group(comms, 1024)  # the comms stay usable
        assert sum(1 for k, _ in _log() if k == "launch") == 2
    finally:
        for c in comms:
            c.destroy()


def test_refusals_and_empty_calls(fake):
    fake(2)
    comms = C.init_all([0, 1], C.CommConfig(buffer_size=1 << 20))
    c = comms[0]
    try:
        _log()
        for call in (lambda: C.all_to_all(c, None, _recv(0), 1024, stream=0),
                     lambda: C.all_to_all(c, _send(0), None, 1024, stream=0),
                     lambda: C.all_to_all(c, None, None, 1024, stream=0)):
            with pytest.raises(MccsError) as ei:
                call()
            assert ei.value.code == INVALID_ARGUMENT
            assert "null" in _lib.last_error()
        # both buffers hold 2 * 1024 bytes: any common byte is an overlap
        for send, recv in ((_send(0), _send(0)), (_send(0), _send(0) + 2047), (_send(0) + 2047, _send(0)),
                           (_send(0), _send(0) + 1024)):
            with pytest.raises(MccsError) as ei:
                C.all_to_all(c, send, recv, 1024, stream=0)
            assert ei.value.code == INVALID_ARGUMENT
            assert "overlap" in str(ei.value) and "overlap" in _lib.last_error()
        assert not any(k == "launch" for k, _ in _log())
        # a zero size succeeds and launches nothing (whatever the buffers)
        C.all_to_all(c, _send(0), _recv(0), 0, stream=0)
        C.all_to_all(c, None, None, 0, stream=0)
        _a2a_group(comms, 0)
        assert not any(k == "launch" for k, _ in _log())
        assert c.last_algo() is None
        # adjacent buffers do not overlap
        with C.group():
            for r, x in enumerate(comms):
                C.all_to_all(x, _send(r), _send(r) + 2048, 1024, stream=0)
        assert sum(1 for k, _ in _log() if k == "launch") == 2
    finally:
        for x in comms:
            x.destroy()


def test_never_the_direct_kernels(fake):
    """With the direct, one-shot and LL variants configured, an AllGather of a
    small block takes LL and an AllToAll of the same bytes the ring."""
    fake(8)
    comms = C.init_all(list(range(8)), C.CommConfig(direct_bytes=8 << 20, oneshot_bytes=256 << 10, ll_bytes=32 << 10))
    try:
        for nbytes in (8, 1000, 32768, 1 << 20):
            with C.group():
                for r, c in enumerate(comms):
                    C.all_reduce(c, _send(r), _recv(r), 1000, F32, SUM, stream=0)
            assert [c.last_algo() for c in comms] == ["ll"] * 8  # the thresholds are live
            _log()
            _a2a_group(comms, nbytes)
            kinds = [kv["kind"] for k, kv in _log() if k == "launch"]
            assert kinds == ["ring"] * 8, (nbytes, kinds)
            assert [c.last_algo() for c in comms] == ["ring"] * 8, nbytes
        for c in comms:
            c.sync()
    finally:
        for c in comms:
            c.destroy()


def test_other_launches_carry_no_route_key(fake):
    fake(2)
    comms = C.init_all([0, 1], C.CommConfig(buffer_size=1 << 20))
    try:
        _log()
        with C.group():
            for r, c in enumerate(comms):
                C.all_gather(c, _send(r), _recv(r), 4096, stream=0)
        launches = [kv for k, kv in _log() if k == "launch"]
        assert len(launches) == 2 and all("a2a" not in kv for kv in launches)
    finally:
        for c in comms:
            c.destroy()


def test_connect_refuses_ranks_that_disagree_on_the_override(fake, monkeypatch):
    """MCCS_ALLTOALL_HOPS travels in the connect handle, as MCCS_GATE does."""
    fake(2)
    lib = _lib.load()
    hsize = lib.mccsConnectHandleSize()
    cfg, _ = C.CommConfig(buffer_size=1 << 20).to_c(2)
    hs, handles = [], []
    try:
        for r in range(2):
            if r == 1:
                monkeypatch.setenv("MCCS_ALLTOALL_HOPS", "relay")
            h, mine = ctypes.c_void_p(), (ctypes.c_char * hsize)()
            assert lib.mccsCommSetupRank(ctypes.byref(h), r, 2, r, ctypes.byref(cfg), mine) == 0
            hs.append(h)
            handles.append(bytes(mine))
        buf = ctypes.create_string_buffer(b"".join(handles), 2 * hsize)
        assert lib.mccsCommConnect(hs[0], buf) == INVALID_ARGUMENT
        assert "MCCS_ALLTOALL_HOPS" in _lib.last_error()
    finally:
        for h in hs:
            lib.mccsCommDestroy(h)


def test_c_abi_declaration_compiles_as_c(tmp_path):
    """tests/capi/capi_all_to_all.c calls mccsAllToAll, the route inspection and
    the host helpers through include/mccs_hip.h as a C11 compiler sees it."""
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "capi", "capi_all_to_all.c")
    r = subprocess.run(build.capi_cmd(src, str(tmp_path / "unused"), syntax_only=True), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
