"""CPU: how the planner launches the opt-in direct / LL ReduceScatter, on the
recording fake device runtime (see tests/test_reduce_scatter_plan.py).

With both limits at 0 every ReduceScatter plans as on the parent commit:
tests/golden/rs_direct_parent_launches.json holds the parent's `launch` records
of parent_cases(), recorded with that commit's library, and the records of this
one are held to them string for string (but for guard_order, which sorts heap
addresses).  With limits set the record is kind=direct mode=rs-oneshot / rs-ll
and carries the walk (count, nch, nthr), the workgroups, the pieces and, per
rank slot, the rank and both buffers; the rest checks which calls take it, G,
and every refusal.
"""
import ctypes
import json
import os

import pytest

import vnode
from mccs_amd import _lib
from mccs_amd import comm as C
from mccs_amd._lib import MccsError

F16, F32, BF16, I32 = 6, 7, 9, 2
SUM, MAX, PREMULSUM, SUMPOSTDIV = 0, 2, 4, 5
INVALID_ARGUMENT, INVALID_USAGE = 4, 5
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rs_direct_parent_launches.json")
BUFF = 1 << 20
ONESHOT, LL_BYTES = 64 << 10, 16 << 10
CAP, LL_CAP = ONESHOT, LL_BYTES  # layout.oneshot_slot (64 KiB steps) and ll_slot / 2
THREADS = 512
ESIZE = vnode.ESIZE


def _parse(line):
    kind, *kv = line.split()
    return kind, dict(x.split("=", 1) for x in kv)


@pytest.fixture
def fake(monkeypatch):
    lib = _lib.load()
    monkeypatch.setenv("MCCS_TEST_HOOKS", "1")
    monkeypatch.setenv("MCCS_GATE", "0")
    for v in ("MCCS_RS_DIRECT_BYTES", "MCCS_RS_LL_BYTES", "MCCS_DIRECT_BLOCKS", "MCCS_DIRECT_WG_BYTES"):
        monkeypatch.delenv(v, raising=False)

    def install(ndev):
        assert lib.mccs_test_fake_runtime(ndev) == 0

    yield install
    lib.mccs_test_fake_runtime(0)


def _raw_log():
    lib = _lib.load()
    n = lib.mccs_test_fake_log(None, 0, 0)
    assert n >= 0, "fake runtime not installed"
    buf = ctypes.create_string_buffer(n + 1)
    lib.mccs_test_fake_log(buf, n + 1, 1)
    return [x for x in buf.value.decode().splitlines() if x]


def _launches():
    return [kv for k, kv in map(_parse, _raw_log()) if k == "launch"]


def _send(r):
    return 0x10000000 * (r + 1)  # the fake never touches "device" memory


def _recv(r):
    return _send(r) + 0x8000000


def _cfg(**kw):
    kw.setdefault("buffer_size", BUFF)
    return C.CommConfig(direct_bytes=-1, oneshot_bytes=ONESHOT, ll_bytes=LL_BYTES, **kw)


def _destroy(comms):
    for c in comms:
        c.destroy()


def _rs(comms, count, dtype=F32, op=SUM, stream=0, op_arg=None, calls=1):
    with C.group():
        for k in range(calls):
            for r, c in enumerate(comms):
                C.reduce_scatter(c, _send(r) + k * 0x100000, _recv(r) + k * 0x100000, count, dtype, op, stream=stream,
                                 op_arg=op_arg)


def _set(comms, block=0, ll=0):
    for c in comms:
        c.set_reduce_scatter_direct(block_bytes=block, ll_block_bytes=ll)


# ---- limits at 0: the parent's records --------------------------------------
def parent_cases():
    """(name, n, dtype, op, op_arg, how) of every record in the golden file."""
    out = []
    for n in (2, 4, 8):
        for what, dtype, op, arg in (("fp32 Sum", F32, SUM, None), ("bf16 Max", BF16, MAX, None),
                                     ("fp32 PreMulSum", F32, PREMULSUM, 0x3F000000)):  # 0.5f
            for how in ("eager", "captured", "batched pair"):
                out.append((f"n={n} {what} {how}", n, dtype, op, arg, how))
    return out


def record_parent_cases(install):
    """name -> the raw `launch` lines of the case, on fresh communicators whose
    limits were never set."""
    lib = _lib.load()
    out = {}
    for name, n, dtype, op, arg, how in parent_cases():
        install(1)
        comms = C.init_all([0] * n, _cfg())
        try:
            _raw_log()
            if how == "captured":
                stream = 0x5000
                assert lib.mccs_test_fake_capture(stream, 9) == 0
                _rs(comms, 1000, dtype, op, stream=stream, op_arg=arg)
                assert lib.mccs_test_fake_capture(stream, 0) == 0
            else:
                _rs(comms, 1000, dtype, op, op_arg=arg, calls=2 if how == "batched pair" else 1)
            out[name] = [x for x in _raw_log() if x.startswith("launch ")]
            if how == "captured":
                lib.mccs_test_fake_destroy_graph(9)
        finally:
            _destroy(comms)
    return out


def _no_guard_order(line):
    return " ".join(x for x in line.split() if not x.startswith("guard_order="))


def test_with_both_limits_off_every_record_is_the_parents(fake):
    want = json.load(open(GOLDEN))
    got = record_parent_cases(fake)
    assert sorted(got) == sorted(want) and len(got) == 27
    for name in want:
        assert len(got[name]) == 1
        assert [_no_guard_order(x) for x in got[name]] == [_no_guard_order(x) for x in want[name]], name
        assert "mode=rs-" not in got[name][0] and " kind=ring " in got[name][0]


# ---- limits set ---------------------------------------------------------------
def _slots(kv):
    out = []
    for s in kv["slots"].split("/"):
        rank, send, recv = s.split(":")
        out.append({"rank": int(rank), "send": int(send, 16), "recv": int(recv, 16)})
    return out


@pytest.mark.parametrize("n", [2, 4, 8])
@pytest.mark.parametrize("variant", ["oneshot", "ll"])
def test_a_block_within_the_limit_is_one_direct_launch_with_the_rings_walk(fake, n, variant):
    fake(1)
    comms = C.init_all([0] * n, _cfg())
    try:
        assert all(c.reduce_scatter_direct_max() == (CAP, LL_CAP) for c in comms)
        _set(comms, block=CAP if variant == "oneshot" else 0, ll=LL_CAP if variant == "ll" else 0)
        _raw_log()
        for dtype, op, count in ((F32, SUM, 1000), (BF16, MAX, 4097), (F16, SUM, 1)):
            _rs(comms, count, dtype, op)
            (kv,) = _launches()
            assert kv["kind"] == "direct" and kv["mode"] == "rs-" + variant and kv["count"] == str(count)
            block = count * ESIZE[dtype]
            nch, nthr, _ = vnode.Planner(comms[0].nchannels, comms[0].rings()).select(n * block, block)
            assert (int(kv["nch"]), int(kv["nthr"])) == (nch, nthr), (kv, nch, nthr)
            gx, gy = (int(v) for v in kv["grid"].split("x"))
            assert gy == n and gx == int(kv["gx"]) and kv["block"] == str(THREADS) and kv["comms_on_dev"] == "1"
            assert kv["llslot"] == str(2 * LL_BYTES)
            assert _slots(kv) == [{"rank": r, "send": _send(r), "recv": _recv(r)} for r in range(n)]
            assert all(c.last_algo() == variant for c in comms)
    finally:
        _destroy(comms)


def test_the_limit_itself_takes_the_new_mode_and_one_element_more_the_parents_ring(fake):
    fake(1)
    n, limit = 4, 4096
    comms = C.init_all([0] * n, _cfg())
    try:
        _raw_log()
        _rs(comms, limit // 4 + 1)  # limits still 0
        (before,) = _launches()
        assert before["kind"] == "ring"
        for block, ll, mode in ((limit, 0, "rs-oneshot"), (0, limit, "rs-ll")):
            _set(comms, block=block, ll=ll)
            _rs(comms, limit // 4)
            (kv,) = _launches()
            assert kv["mode"] == mode and comms[0].last_algo() == mode[3:]
            _rs(comms, limit // 4 + 1)
            (after,) = _launches()
            assert after["kind"] == "ring" and comms[0].last_algo() == "ring"
            assert _no_guard_order(" ".join(f"{k}={v}" for k, v in after.items())) == \
                _no_guard_order(" ".join(f"{k}={v}" for k, v in before.items()))
    finally:
        _destroy(comms)


def test_ll_wins_where_both_fit(fake):
    fake(1)
    comms = C.init_all([0] * 4, _cfg())
    try:
        _set(comms, block=CAP, ll=1024)
        _raw_log()
        _rs(comms, 256)
        (kv,) = _launches()
        assert kv["mode"] == "rs-ll" and comms[0].last_algo() == "ll"
        _rs(comms, 257)
        (kv,) = _launches()
        assert kv["mode"] == "rs-oneshot" and comms[0].last_algo() == "oneshot"
        _rs(comms, CAP // 4 + 1)
        (kv,) = _launches()
        assert kv["kind"] == "ring"
    finally:
        _destroy(comms)


def test_two_calls_in_a_group_take_the_ring(fake):
    fake(1)
    comms = C.init_all([0] * 4, _cfg())
    try:
        _raw_log()
        _rs(comms, 500, calls=2)
        (before,) = _launches()
        _set(comms, block=CAP, ll=LL_CAP)
        _rs(comms, 500, calls=2)
        (kv,) = _launches()
        assert kv["kind"] == "ring" and comms[0].last_algo() == "ring"
        assert {k: v for k, v in kv.items() if k != "guard_order"} == \
            {k: v for k, v in before.items() if k != "guard_order"}
        _rs(comms, 500)  # and a single call afterwards is direct again
        (kv,) = _launches()
        assert kv["mode"] == "rs-ll"
    finally:
        _destroy(comms)


def test_premulsum_sumpostdiv_and_avg_take_the_ring(fake):
    fake(1)
    n = 4
    comms = C.init_all([0] * n, _cfg())
    try:
        _set(comms, block=CAP, ll=LL_CAP)
        _raw_log()
        _rs(comms, 500, F32, PREMULSUM, op_arg=0x3F000000)
        (kv,) = _launches()
        assert kv["kind"] == "ring" and comms[0].last_algo() == "ring"
        _rs(comms, 500, I32, SUMPOSTDIV, op_arg=n)
        (kv,) = _launches()
        assert kv["kind"] == "ring"
        for dtype in (F32, I32):
            with C.group():
                for r, c in enumerate(comms):
                    c.reduce_scatter_avg(_send(r), _recv(r), 500, dtype, stream=0)
            (kv,) = _launches()
            assert kv["kind"] == "ring" and comms[0].last_algo() == "ring"
        _rs(comms, 500, F32, SUM, op_arg=0)  # the OpArg entry with a plain op is a plain call
        (kv,) = _launches()
        assert kv["mode"] == "rs-ll"
    finally:
        _destroy(comms)


@pytest.mark.parametrize("n", [1, 9])
def test_outside_two_to_eight_ranks_the_caps_are_zero_and_the_ring_runs(fake, n):
    fake(1)
    comms = C.init_all([0] * n, _cfg())
    try:
        assert all(c.reduce_scatter_direct_max() == (0, 0) for c in comms)
        _set(comms, 0, 0)
        _raw_log()
        _rs(comms, 64)
        assert all(kv["kind"] == "ring" for kv in _launches())
        assert comms[0].last_algo() == "ring"
    finally:
        _destroy(comms)


def test_captured_and_per_device_launches_are_recorded(fake):
    fake(2)
    lib = _lib.load()
    comms = C.init_all([0, 0, 1, 1], _cfg())
    try:
        _set(comms, block=CAP, ll=1024)
        _raw_log()
        stream = 0x5000
        assert lib.mccs_test_fake_capture(stream, 9) == 0
        _rs(comms, 256, stream=stream)
        _rs(comms, 2000, stream=stream)
        assert lib.mccs_test_fake_capture(stream, 0) == 0
        got = _launches()
        # two devices, two fused rank slots each; a captured launch has no stop event
        assert len(got) == 4 and all(kv["grid"].endswith("x2") and kv["stop_event"] == "0" for kv in got)
        assert [kv["mode"] for kv in got] == ["rs-ll", "rs-ll", "rs-oneshot", "rs-oneshot"]
        for i, kv in enumerate(got):
            assert [s["rank"] for s in _slots(kv)] == ([0, 1] if i % 2 == 0 else [2, 3])
            assert all(s["send"] == _send(s["rank"]) and s["recv"] == _recv(s["rank"]) for s in _slots(kv))
        lib.mccs_test_fake_destroy_graph(9)
        _rs(comms, 2000)  # eager: the stop event rides on the launch
        got = _launches()
        assert len(got) == 2 and all(kv["stop_event"] != "0" and kv["mode"] == "rs-oneshot" for kv in got)
    finally:
        _destroy(comms)


@pytest.mark.parametrize("blocks", [None, 1])
def test_workgroups_follow_phase_one_and_are_capped(fake, monkeypatch, blocks):
    if blocks:
        monkeypatch.setenv("MCCS_DIRECT_BLOCKS", str(blocks))
    fake(1)
    n = 4
    comms = C.init_all([0] * n, _cfg())
    try:
        _set(comms, block=CAP, ll=0)
        _raw_log()
        # count-based: 4 KiB of the (n - 1) foreign blocks per workgroup; the fake device holds 256
        # workgroups at once, 64 for each of the four fused rank slots
        for count in (1, 1024, 1025, 4096, CAP // 4):
            _rs(comms, count)
            (kv,) = _launches()
            want = -(-(n - 1) * count * 4 // 4096)
            assert int(kv["gx"]) == (1 if blocks else min(want, 64)), (count, kv["gx"])
            assert int(kv["piece"]) * 4 % 4096 == 0 and int(kv["piece2"]) * 4 % 4096 == 0
        _set(comms, block=0, ll=LL_CAP)
        # LL: one 8-byte word of the (n - 1) foreign blocks per thread
        for count in (1, 2 * THREADS // (n - 1), 2 * THREADS // (n - 1) + 2, LL_CAP // 4):
            _rs(comms, count)
            (kv,) = _launches()
            want = -(-(n - 1) * -(-count * 4 // 8) // THREADS)
            assert kv["mode"] == "rs-ll" and int(kv["gx"]) == (1 if blocks else min(want, 64)), (count, kv["gx"])
    finally:
        _destroy(comms)


# ---- refusals -------------------------------------------------------------------
def _refused(code, start, call, also=()):
    with pytest.raises(MccsError) as ei:
        call()
    assert ei.value.code == code, (ei.value.code, _lib.last_error())
    err = _lib.last_error()
    assert err.startswith(start), err
    for word in also:
        assert word in err, err


def test_setter_refusals(fake):
    fake(1)
    comms = C.init_all([0, 0], _cfg())
    c = comms[0]
    try:
        _raw_log()
        _refused(INVALID_ARGUMENT, "mccsCommSetReduceScatterDirect: block_bytes",
                 lambda: c.set_reduce_scatter_direct(CAP + 1, 0), also=(str(CAP + 1), str(CAP)))
        _refused(INVALID_ARGUMENT, "mccsCommSetReduceScatterDirect: ll_block_bytes",
                 lambda: c.set_reduce_scatter_direct(0, LL_CAP + 8), also=(str(LL_CAP + 8), str(LL_CAP)))
        c.set_reduce_scatter_direct(CAP, LL_CAP)  # the capacities themselves are fine
        c.set_reduce_scatter_direct(0, 0)

        def in_group():
            with C.group():
                c.set_reduce_scatter_direct(64, 64)

        _refused(INVALID_USAGE, "mccsCommSetReduceScatterDirect: the communicator has a group open", in_group)
        lib = _lib.load()
        assert lib.mccsGroupStart() == 0
        assert lib.mccsReduceScatter(_send(0), _recv(0), 16, F32, SUM, c._h, 0) == 0
        assert lib.mccsCommSetReduceScatterDirect(c._h, 64, 64) == INVALID_USAGE
        assert "a call pending" in _lib.last_error()
        assert lib.mccsReduceScatter(_send(1), _recv(1), 16, F32, SUM, comms[1]._h, 0) == 0
        assert lib.mccsGroupEnd() == 0
        (kv,) = _launches()
        assert kv["kind"] == "ring"  # the refused setter changed nothing
    finally:
        _destroy(comms)


def test_on_a_cached_arena_with_its_system_scope_fences_the_ll_cap_is_zero(fake):
    fake(1)
    comms = C.init_all([0, 0], _cfg(fifo_memory=C.FIFO_DEVICE))
    try:
        cap, ll_cap = comms[0].reduce_scatter_direct_max()
        assert ll_cap == 0 and cap == CAP  # the count-based variant fences as the arena needs
        _refused(INVALID_ARGUMENT, "mccsCommSetReduceScatterDirect: ll_block_bytes 8 is above the 0 bytes",
                 lambda: comms[0].set_reduce_scatter_direct(0, 8), also=("the LL path is closed here",))
        _set(comms, block=CAP, ll=0)
        _raw_log()
        _rs(comms, 8)
        (kv,) = _launches()
        assert kv["mode"] == "rs-oneshot" and kv["fence"] == "0"  # MCCS_FENCE_SYSTEM
    finally:
        _destroy(comms)


def test_the_environment_sets_both_limits_at_creation_clamped_to_the_caps(fake, monkeypatch):
    monkeypatch.setenv("MCCS_RS_DIRECT_BYTES", str(1 << 30))
    monkeypatch.setenv("MCCS_RS_LL_BYTES", "512")
    fake(1)
    comms = C.init_all([0, 0], _cfg())
    monkeypatch.delenv("MCCS_RS_DIRECT_BYTES")  # read at creation, not per call
    monkeypatch.delenv("MCCS_RS_LL_BYTES")
    try:
        _raw_log()
        _rs(comms, 128)
        (kv,) = _launches()
        assert kv["mode"] == "rs-ll"
        _rs(comms, 129)
        (kv,) = _launches()
        assert kv["mode"] == "rs-oneshot"
        _rs(comms, CAP // 4)  # the count-based limit was clamped to the cap
        (kv,) = _launches()
        assert kv["mode"] == "rs-oneshot"
        _rs(comms, CAP // 4 + 1)
        (kv,) = _launches()
        assert kv["kind"] == "ring"
        others = C.init_all([0, 0], _cfg())  # created without the variables: off
        try:
            _raw_log()
            _rs(others, 128)
            (kv,) = _launches()
            assert kv["kind"] == "ring"
        finally:
            _destroy(others)
    finally:
        _destroy(comms)


def test_new_exports_and_their_c_declarations(tmp_path):
    import subprocess

    from mccs_amd import build

    lib = _lib.load()
    for name in ("mccsCommSetReduceScatterDirect", "mccsCommReduceScatterDirectMax"):
        assert getattr(lib, name) is not None
        assert name in _lib.SIGNATURES
    src = tmp_path / "rs.c"
    src.write_text('#include "mccs_hip.h"\n'
                   "mccsResult_t f(mccsComm_t comm, size_t *cap, size_t *ll_cap) {\n"
                   "  mccsResult_t r = mccsCommReduceScatterDirectMax(comm, cap, ll_cap);\n"
                   "  return r ? r : mccsCommSetReduceScatterDirect(comm, *cap, *ll_cap);\n}\n")
    r = subprocess.run(build.capi_cmd(str(src), str(tmp_path / "unused"), syntax_only=True), capture_output=True,
                       text=True)
    assert r.returncode == 0, r.stderr
