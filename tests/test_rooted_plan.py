"""CPU: how the planner launches a Broadcast and a Reduce, on the recording
fake device runtime (csrc/host/rt.cpp, mccs_test_fake_runtime: host memory, no
kernel runs; see tests/test_reduce_scatter_plan.py).  One ring launch per
device, ranks sharing a device fused into one, never the direct / LL kernels,
roots that differ inside one batched launch, and the refusals.
"""
import ctypes
import os
import subprocess

import pytest

from mccs_amd import _lib
from mccs_amd import build
from mccs_amd import comm as C
from mccs_amd._lib import MccsError

F16, F32, SUM = 6, 7, 0
INVALID_ARGUMENT, INVALID_USAGE = 4, 5


def _parse(line):
    kind, *kv = line.split()
    return kind, dict(x.split("=", 1) for x in kv)


@pytest.fixture
def fake(monkeypatch):
    lib = _lib.load()
    monkeypatch.setenv("MCCS_TEST_HOOKS", "1")  # the hook is refused without it
    monkeypatch.setenv("MCCS_GATE", "0")  # the fake runs no kernel: the node gate's sums would never match

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


def _broadcast_group(comms, nbytes, root=0, off=0):
    with C.group():
        for r, c in enumerate(comms):
            C.broadcast(c, _send(r) + off if r == root else None, _recv(r) + off, nbytes, root, stream=0)


def _reduce_group(comms, count, root=0, dtype=F32):
    with C.group():
        for r, c in enumerate(comms):
            C.reduce(c, _send(r), _recv(r) if r == root else None, count, dtype, SUM, root, stream=0)


CALLS = [("broadcast", lambda comms, root: _broadcast_group(comms, 1 << 23, root)),
         ("reduce", lambda comms, root: _reduce_group(comms, 1 << 21, root))]


@pytest.mark.parametrize("name,call", CALLS, ids=[c[0] for c in CALLS])
def test_eight_devices_one_launch_per_device(fake, name, call):
    fake(8)
    comms = C.init_all(list(range(8)), C.CommConfig(buffer_size=1 << 20))
    try:
        _log()
        nch, lanes = comms[0].nchannels, comms[0].lanes
        call(comms, 3)  # 8 MiB: every channel
        ev = _log()
        launches = [(i, kv) for i, (k, kv) in enumerate(ev) if k == "launch"]
        assert sorted(int(kv["dev"]) for _, kv in launches) == list(range(8)), ev
        for _, kv in launches:
            assert kv["kind"] == "ring" and kv["grid"] == f"{nch * lanes}x1" and kv["comms_on_dev"] == "1", kv
        last = max(i for i, _ in launches)
        waits = [i for i, (k, _) in enumerate(ev) if k == "host_wait"]
        assert not waits or min(waits) > last, f"host waited before every rank was launched: {ev}"
        assert all(c.last_algo() == "ring" for c in comms)
        for c in comms:
            c.sync()
    finally:
        for c in comms:
            c.destroy()


@pytest.mark.parametrize("name,call", CALLS, ids=[c[0] for c in CALLS])
def test_four_ranks_on_one_device_are_one_fused_launch(fake, name, call):
    fake(1)
    comms = C.init_all([0] * 4, C.CommConfig(buffer_size=1 << 20))
    try:
        _log()
        call(comms, 2)
        launches = [kv for k, kv in _log() if k == "launch"]
        assert len(launches) == 1, launches
        gx, gy = (int(v) for v in launches[0]["grid"].split("x"))
        assert gy == 4 and gx == comms[0].nchannels * comms[0].lanes and launches[0]["kind"] == "ring"
    finally:
        for c in comms:
            c.destroy()


def test_two_broadcasts_with_different_roots_are_one_launch(fake):
    """The root is per work element: calls of one function in a group are
    batched whatever their roots."""
    fake(1)
    comms = C.init_all([0] * 4, C.CommConfig(buffer_size=1 << 20))
    try:
        _log()
        with C.group():
            for j, root in enumerate((1, 3)):
                for r, c in enumerate(comms):
                    C.broadcast(c, _send(r) + j * 0x100000 if r == root else None, _recv(r) + j * 0x100000, 4000, root,
                                stream=0)
        launches = [kv for k, kv in _log() if k == "launch"]
        assert len(launches) == 1 and launches[0]["grid"].endswith("x4") and launches[0]["kind"] == "ring", launches
        with C.group():
            for j, root in enumerate((0, 2, 3)):
                for r, c in enumerate(comms):
                    C.reduce(c, _send(r) + j * 0x100000, _recv(r) + j * 0x100000 if r == root else None, 1000, F32, SUM,
                             root, stream=0)
        launches = [kv for k, kv in _log() if k == "launch"]
        assert len(launches) == 1 and launches[0]["grid"].endswith("x4"), launches
    finally:
        for c in comms:
            c.destroy()


def test_broadcast_plus_reduce_in_a_group_is_refused(fake):
    fake(2)
    comms = C.init_all([0, 1], C.CommConfig(buffer_size=1 << 20))
    lib = _lib.load()
    try:
        _log()
        assert lib.mccsGroupStart() == 0
        for r, c in enumerate(comms):
            assert lib.mccsBroadcast(_send(r), _recv(r), 4096, 0, c._h, 0) == 0
        assert lib.mccsReduce(_send(0), _recv(0), 1024, F32, SUM, 0, comms[0]._h, 0) == INVALID_USAGE
        assert _lib.last_error().startswith("mccsReduce"), _lib.last_error()
        assert lib.mccsGroupEnd() == INVALID_USAGE
        assert not any(k == "launch" for k, _ in _log())
        # Broadcast is function 0: an AllReduce pending first refuses it too
        assert lib.mccsGroupStart() == 0
        assert lib.mccsAllReduce(_send(0), _recv(0), 4096, F32, SUM, comms[0]._h, 0) == 0
        assert lib.mccsBroadcast(_send(0), _recv(0), 4096, 0, comms[0]._h, 0) == INVALID_USAGE
        assert lib.mccsGroupEnd() == INVALID_USAGE
        assert not any(k == "launch" for k, _ in _log())
        _broadcast_group(comms, 1024)  # the comms stay usable
        _reduce_group(comms, 1024, root=1)
        assert sum(1 for k, _ in _log() if k == "launch") == 4
    finally:
        for c in comms:
            c.destroy()


def test_refusals_and_empty_calls(fake):
    fake(2)
    comms = C.init_all([0, 1], C.CommConfig(buffer_size=1 << 20))
    c = comms[0]
    n = len(comms)
    try:
        _log()
        for root in (-1, n):
            for what, call in (("mccsBroadcast", lambda: C.broadcast(c, _send(0), _recv(0), 1024, root, stream=0)),
                               ("mccsReduce", lambda: C.reduce(c, _send(0), _recv(0), 1024, F32, SUM, root, stream=0))):
                with pytest.raises(MccsError) as ei:
                    call()
                assert ei.value.code == INVALID_ARGUMENT, (what, root)
                assert f"root {root}" in str(ei.value), (what, root, str(ei.value))
                assert f"root {root}" in _lib.last_error(), (what, root, _lib.last_error())
        for dtype, op in ((10, SUM), (-1, SUM), (F32, 4), (F32, -1)):
            with pytest.raises(MccsError) as ei:
                C.reduce(c, _send(0), _recv(0), 1024, dtype, op, 0, stream=0)
            assert ei.value.code == INVALID_ARGUMENT, (dtype, op)
        # a null buffer is refused where the rank's role uses it, and only there
        for call in (lambda: C.broadcast(c, None, _recv(0), 1024, 0, stream=0),   # the root's sendbuff
                     lambda: C.broadcast(c, _send(0), None, 1024, 0, stream=0),   # any rank's recvbuff
                     lambda: C.broadcast(c, None, None, 1024, 1, stream=0),
                     lambda: C.reduce(c, None, _recv(0), 1024, F32, SUM, 0, stream=0),  # any rank's sendbuff
                     lambda: C.reduce(c, None, None, 1024, F32, SUM, 1, stream=0),
                     lambda: C.reduce(c, _send(0), None, 1024, F32, SUM, 0, stream=0)):  # the root's recvbuff
            with pytest.raises(MccsError) as ei:
                call()
            assert ei.value.code == INVALID_ARGUMENT
        assert not any(k == "launch" for k, _ in _log())
        # a zero size succeeds and launches nothing (whatever the buffers)
        C.broadcast(c, _send(0), _recv(0), 0, 0, stream=0)
        C.broadcast(c, None, None, 0, 1, stream=0)
        C.reduce(c, _send(0), _recv(0), 0, F32, SUM, 0, stream=0)
        C.reduce(c, None, None, 0, F32, SUM, 1, stream=0)
        _broadcast_group(comms, 0)
        _reduce_group(comms, 0)
        assert not any(k == "launch" for k, _ in _log())
        assert c.last_algo() is None
        # the buffer a role does not use may be null
        _broadcast_group(comms, 1024, root=1)
        _reduce_group(comms, 1024, root=1)
        assert sum(1 for k, _ in _log() if k == "launch") == 4
    finally:
        for x in comms:
            x.destroy()


def test_never_the_direct_kernels(fake):
    """With the direct, one-shot and LL variants configured, an AllReduce of a
    small bucket takes LL and a Broadcast or Reduce of the same bytes the ring."""
    fake(8)
    comms = C.init_all(list(range(8)), C.CommConfig(direct_bytes=8 << 20, oneshot_bytes=256 << 10, ll_bytes=32 << 10))
    try:
        with C.group():
            for r, c in enumerate(comms):
                C.all_reduce(c, _send(r), _recv(r), 1000, F32, SUM, stream=0)
        assert [c.last_algo() for c in comms] == ["ll"] * 8  # the thresholds are live
        for count in (1, 125, 1000, 8192, 65536, 1 << 20):  # 4 B .. 4 MiB: LL, one-shot and two-shot sizes
            for call in (lambda: _broadcast_group(comms, 4 * count, root=count % 8),
                         lambda: _reduce_group(comms, count, root=count % 8)):
                with C.group():  # back to LL in between, so "ring" below is this call's
                    for r, c in enumerate(comms):
                        C.all_reduce(c, _send(r), _recv(r), 1000, F32, SUM, stream=0)
                _log()
                call()
                kinds = [kv["kind"] for k, kv in _log() if k == "launch"]
                assert kinds == ["ring"] * 8, (count, kinds)
                assert [c.last_algo() for c in comms] == ["ring"] * 8, count
        for c in comms:
            c.sync()
    finally:
        for c in comms:
            c.destroy()


def test_no_reference_named_entry_point():
    """The reference has no Broadcast or Reduce kernel to name: the
    symbol-level interface keeps refusing the functions."""
    lib = _lib.load()
    broadcast, reduce_, allreduce = 0, 1, 4  # mccsDevFunc_t
    assert (C.FUNC_BROADCAST, C.FUNC_REDUCE) == (broadcast, reduce_)
    assert lib.mccs_hip_coll_kernel(allreduce, F32, SUM)
    for func in (broadcast, reduce_):
        assert not lib.mccs_hip_coll_kernel(func, F32, SUM)
        assert lib.mccs_hip_launch_coll(func, F32, SUM, 0x1000, 1, 0x2000, 1, 96, None) == INVALID_ARGUMENT


def test_c_abi_declaration_compiles_as_c(tmp_path):
    """tests/capi/capi_rooted.c calls mccsBroadcast, mccsReduce and the host
    rings through include/mccs_hip.h as a C11 compiler sees it."""
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "capi", "capi_rooted.c")
    r = subprocess.run(build.capi_cmd(src, str(tmp_path / "unused"), syntax_only=True), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
