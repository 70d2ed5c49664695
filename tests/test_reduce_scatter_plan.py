"""CPU: how the planner launches a ReduceScatter, on the recording fake device
runtime (csrc/host/rt.cpp, mccs_test_fake_runtime: host memory, no kernel
runs; see tests/test_multidevice_launch.py).  One launch per device, ranks
sharing a device fused into one, never the direct / LL kernels, and the same
refusals as mccsAllReduce.
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


def _reduce_scatter_group(comms, count, dtype=F32):
    with C.group():
        for r, c in enumerate(comms):
            C.reduce_scatter(c, _send(r), _recv(r), count, dtype, SUM, stream=0)


def test_eight_devices_one_launch_per_device(fake):
    fake(8)
    comms = C.init_all(list(range(8)), C.CommConfig(buffer_size=1 << 20))
    try:
        _log()
        nch, lanes = comms[0].nchannels, comms[0].lanes
        _reduce_scatter_group(comms, 1 << 18)  # 8 MiB enter the ring: every channel
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


def test_four_ranks_on_one_device_are_one_fused_launch(fake):
    fake(1)
    comms = C.init_all([0] * 4, C.CommConfig(buffer_size=1 << 20))
    try:
        _log()
        _reduce_scatter_group(comms, 1 << 18)
        launches = [kv for k, kv in _log() if k == "launch"]
        assert len(launches) == 1, launches
        gx, gy = (int(v) for v in launches[0]["grid"].split("x"))
        assert gy == 4 and gx == comms[0].nchannels * comms[0].lanes and launches[0]["kind"] == "ring"
        # several ReduceScatters of each comm in one group: batched into one launch
        with C.group():
            for j in range(3):
                for r, c in enumerate(comms):
                    C.reduce_scatter(c, _send(r) + j * 0x100000, _recv(r) + j * 0x100000, 1000, F32, SUM, stream=0)
        launches = [kv for k, kv in _log() if k == "launch"]
        assert len(launches) == 1 and launches[0]["grid"].endswith("x4"), launches
    finally:
        for c in comms:
            c.destroy()


def test_mixing_functions_in_a_group_is_refused_at_group_end(fake):
    fake(2)
    comms = C.init_all([0, 1], C.CommConfig(buffer_size=1 << 20))
    lib = _lib.load()
    try:
        _log()
        assert lib.mccsGroupStart() == 0
        for r, c in enumerate(comms):
            assert lib.mccsAllReduce(_send(r), _recv(r), 4096, F32, SUM, c._h, 0) == 0
        assert lib.mccsReduceScatter(_send(0), _recv(0), 1024, F32, SUM, comms[0]._h, 0) == INVALID_USAGE
        assert _lib.last_error().startswith("mccsReduceScatter"), _lib.last_error()
        assert lib.mccsGroupEnd() == INVALID_USAGE
        assert not any(k == "launch" for k, _ in _log())
        _reduce_scatter_group(comms, 1024)  # the comms stay usable
        assert sum(1 for k, _ in _log() if k == "launch") == 2
    finally:
        for c in comms:
            c.destroy()


@pytest.mark.parametrize("second", [(F16, SUM), (F32, 2)], ids=["dtype", "op"])
def test_mixing_dtypes_or_ops_in_a_group_is_refused_at_group_end(fake, second):
    """Several ReduceScatters of one communicator in a group must share dtype
    and op (tests/test_gpu_reduce_scatter_fuzz.py's rsgroup keeps to that)."""
    fake(2)
    comms = C.init_all([0, 1], C.CommConfig(buffer_size=1 << 20))
    lib = _lib.load()
    try:
        _log()
        assert lib.mccsGroupStart() == 0
        for r, c in enumerate(comms):
            assert lib.mccsReduceScatter(_send(r), _recv(r), 1024, F32, SUM, c._h, 0) == 0
        assert lib.mccsReduceScatter(_send(0) + 0x100000, _recv(0) + 0x100000, 1024, second[0], second[1],
                                     comms[0]._h, 0) == INVALID_USAGE
        assert lib.mccsGroupEnd() == INVALID_USAGE
        assert not any(k == "launch" for k, _ in _log())
        _reduce_scatter_group(comms, 1024)  # the comms stay usable
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
        for args in ((_send(0), _recv(0), 1024, 10, SUM), (_send(0), _recv(0), 1024, -1, SUM),
                     (_send(0), _recv(0), 1024, F32, 4), (_send(0), _recv(0), 1024, F32, -1),
                     (0, _recv(0), 1024, F32, SUM), (_send(0), 0, 1024, F32, SUM)):
            with pytest.raises(MccsError) as ei:
                C.reduce_scatter(c, *args, stream=0)
            assert ei.value.code == INVALID_ARGUMENT, args
        # recvcount = 0 succeeds and launches nothing (whatever the buffers)
        C.reduce_scatter(c, _send(0), _recv(0), 0, F32, SUM, stream=0)
        C.reduce_scatter(c, 0, 0, 0, F32, SUM, stream=0)
        _reduce_scatter_group(comms, 0)
        assert not any(k == "launch" for k, _ in _log())
        assert c.last_algo() is None
    finally:
        for x in comms:
            x.destroy()


def test_never_the_direct_kernels(fake):
    """With the direct, one-shot and LL variants configured, an AllReduce of a
    small bucket takes LL and a ReduceScatter of the same bytes the ring."""
    fake(8)
    comms = C.init_all(list(range(8)), C.CommConfig(direct_bytes=8 << 20, oneshot_bytes=256 << 10, ll_bytes=32 << 10))
    try:
        with C.group():
            for r, c in enumerate(comms):
                C.all_reduce(c, _send(r), _recv(r), 1000, F32, SUM, stream=0)
        assert [c.last_algo() for c in comms] == ["ll"] * 8  # the thresholds are live
        for count in (1, 125, 1000, 8192, 65536, 1 << 20):  # 4 B .. 4 MiB per block: LL, one-shot and two-shot sizes
            _log()
            _reduce_scatter_group(comms, count)
            kinds = [kv["kind"] for k, kv in _log() if k == "launch"]
            assert kinds == ["ring"] * 8, (count, kinds)
            assert [c.last_algo() for c in comms] == ["ring"] * 8, count
        for c in comms:
            c.sync()
    finally:
        for c in comms:
            c.destroy()


def test_no_reference_named_entry_point():
    """The reference has no ReduceScatter kernel to name: the symbol-level
    interface keeps refusing the function."""
    lib = _lib.load()
    reduce_scatter, allreduce = 3, 4  # mccsDevFunc_t
    assert lib.mccs_hip_coll_kernel(allreduce, F32, SUM)
    assert not lib.mccs_hip_coll_kernel(reduce_scatter, F32, SUM)
    assert lib.mccs_hip_launch_coll(reduce_scatter, F32, SUM, 0x1000, 1, 0x2000, 1, 96, None) == INVALID_ARGUMENT


def test_c_abi_declaration_compiles_as_c(tmp_path):
    """tests/capi/capi_reduce_scatter.c calls mccsReduceScatter and the host
    ring through include/mccs_hip.h as a C11 compiler sees it."""
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "capi", "capi_reduce_scatter.c")
    r = subprocess.run(build.capi_cmd(src, str(tmp_path / "unused"), syntax_only=True), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
