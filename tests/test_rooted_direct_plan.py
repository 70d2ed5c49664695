"""CPU: how the planner launches the opt-in direct / LL Broadcast and Reduce, on
the recording fake device runtime (see tests/test_reduce_scatter_direct_plan.py).

With all four limits at 0 every Broadcast and Reduce plans as on the parent
commit: tests/golden/rooted_direct_parent_launches.json holds the parent's
`launch` records of parent_cases(), recorded with that commit's library through
record_parent_cases, and the records of this one are held to them string for
string (but for guard_order, which sorts heap addresses).  With limits set the
record is kind=direct mode=bc-oneshot / bc-ll / rd-oneshot / rd-ll and carries
the root, the walk (count, nch, nthr), the workgroups, the pieces and, per rank
slot, the rank and both buffers; the rest checks which calls take it, G, and
every refusal.
"""
import ctypes
import json
import os

import pytest

import vnode
from mccs_amd import _lib
from mccs_amd import comm as C
from mccs_amd._lib import MccsError

I8, F16, F32, BF16, I32 = 0, 6, 7, 9, 2
SUM, MAX, PREMULSUM, SUMPOSTDIV = 0, 2, 4, 5
INVALID_ARGUMENT, INVALID_USAGE = 4, 5
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rooted_direct_parent_launches.json")
BUFF = 1 << 20
ONESHOT, LL_BYTES = 64 << 10, 16 << 10
CAP, LL_CAP = ONESHOT, LL_BYTES  # layout.oneshot_slot (64 KiB steps) and ll_slot / 2
THREADS = 512
ESIZE = vnode.ESIZE
ENV = ("MCCS_BC_DIRECT_BYTES", "MCCS_BC_LL_BYTES", "MCCS_RD_DIRECT_BYTES", "MCCS_RD_LL_BYTES")
FUNCS = ["bc", "rd"]


def _parse(line):
    kind, *kv = line.split()
    return kind, dict(x.split("=", 1) for x in kv)


@pytest.fixture
def fake(monkeypatch):
    lib = _lib.load()
    monkeypatch.setenv("MCCS_TEST_HOOKS", "1")
    monkeypatch.setenv("MCCS_GATE", "0")
    for v in ENV + ("MCCS_RS_DIRECT_BYTES", "MCCS_RS_LL_BYTES", "MCCS_DIRECT_BLOCKS", "MCCS_DIRECT_WG_BYTES"):
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


def _call(func, comms, count, dtype=F32, op=SUM, roots=(0,), stream=0, op_arg=None):
    """One group: a Broadcast of count * esize(dtype) bytes or a Reduce of count
    elements per root of `roots`, on every comm; only the ranks whose role uses
    a buffer pass it."""
    with C.group():
        for k, root in enumerate(roots):
            off = k * 0x100000
            for r, c in enumerate(comms):
                if func == "bc":
                    C.broadcast(c, _send(r) + off if r == root else None, _recv(r) + off, count * ESIZE[dtype], root,
                                stream=stream)
                else:
                    C.reduce(c, _send(r) + off, _recv(r) + off if r == root else None, count, dtype, op, root,
                             stream=stream, op_arg=op_arg)


def _set(comms, func, oneshot=0, ll=0):
    for c in comms:
        if func == "bc":
            c.set_rooted_direct(bcast_bytes=oneshot, bcast_ll_bytes=ll)
        else:
            c.set_rooted_direct(reduce_bytes=oneshot, reduce_ll_bytes=ll)


# ---- limits at 0: the parent's records --------------------------------------
def parent_cases():
    """(name, func, n, dtype, op, op_arg, how) of every record in the golden
    file.  A Broadcast has neither dtype nor op: its three cases move the
    bytes of the Reduce beside them."""
    out = []
    for func in FUNCS:
        for n in (2, 4, 8):
            for what, dtype, op, arg in (("fp32 Sum", F32, SUM, None), ("bf16 Max", BF16, MAX, None),
                                         ("fp32 PreMulSum", F32, PREMULSUM, 0x3F000000)):  # 0.5f
                for how in ("eager", "captured", "batched pair"):
                    out.append((f"{func} n={n} {what} {how}", func, n, dtype, op, arg, how))
    return out


def record_parent_cases(install):
    """name -> the raw `launch` lines of the case, on fresh communicators whose
    limits were never set.  Uses nothing the parent commit lacks."""
    lib = _lib.load()
    out = {}
    for name, func, n, dtype, op, arg, how in parent_cases():
        install(1)
        comms = C.init_all([0] * n, _cfg())
        try:
            _raw_log()
            roots = (n - 1, 0) if how == "batched pair" else (n - 1,)  # a pair's roots differ
            if how == "captured":
                stream = 0x5000
                assert lib.mccs_test_fake_capture(stream, 9) == 0
                _call(func, comms, 1000, dtype, op, roots, stream=stream, op_arg=arg)
                assert lib.mccs_test_fake_capture(stream, 0) == 0
            else:
                _call(func, comms, 1000, dtype, op, roots, op_arg=arg)
            out[name] = [x for x in _raw_log() if x.startswith("launch ")]
            if how == "captured":
                lib.mccs_test_fake_destroy_graph(9)
        finally:
            _destroy(comms)
    return out


def _no_guard_order(line):
    return " ".join(x for x in line.split() if not x.startswith("guard_order="))


def test_with_all_four_limits_off_every_record_is_the_parents(fake):
    want = json.load(open(GOLDEN))
    got = record_parent_cases(fake)
    assert sorted(got) == sorted(want) and len(got) == 54
    for name in want:
        assert len(got[name]) == 1
        assert [_no_guard_order(x) for x in got[name]] == [_no_guard_order(x) for x in want[name]], name
        assert "mode=" not in got[name][0] and " kind=ring " in got[name][0]


# ---- limits set ---------------------------------------------------------------
def _slots(kv):
    out = []
    for s in kv["slots"].split("/"):
        rank, send, recv = s.split(":")
        out.append({"rank": int(rank), "send": int(send, 16), "recv": int(recv, 16)})
    return out


def _want_slots(func, n, root, off=0):
    """Every rank slot's buffers as the call gave them: NULL where the role uses none."""
    if func == "bc":
        return [{"rank": r, "send": _send(r) + off if r == root else 0, "recv": _recv(r) + off} for r in range(n)]
    return [{"rank": r, "send": _send(r) + off, "recv": _recv(r) + off if r == root else 0} for r in range(n)]


@pytest.mark.parametrize("n", [2, 4, 8])
@pytest.mark.parametrize("variant", ["oneshot", "ll"])
@pytest.mark.parametrize("func", FUNCS)
def test_a_buffer_within_the_limit_is_one_direct_launch_with_the_root_and_the_rings_walk(fake, func, n, variant):
    fake(1)
    comms = C.init_all([0] * n, _cfg())
    try:
        assert all(c.rooted_direct_max() == (CAP, LL_CAP) for c in comms)
        _set(comms, func, oneshot=CAP if variant == "oneshot" else 0, ll=LL_CAP if variant == "ll" else 0)
        _raw_log()
        for (dtype, op, count), root in zip(((F32, SUM, 1000), (BF16, MAX, 4097), (F16, SUM, 1)), (n - 1, 0, n // 2)):
            _call(func, comms, count, dtype, op, (root,))
            (kv,) = _launches()
            nbytes = count * ESIZE[dtype]
            assert kv["kind"] == "direct" and kv["mode"] == f"{func}-{variant}" and kv["root"] == str(root)
            assert kv["count"] == str(nbytes if func == "bc" else count)
            nch, nthr, _ = vnode.Planner(comms[0].nchannels, comms[0].rings()).select(nbytes, nbytes)
            assert (int(kv["nch"]), int(kv["nthr"])) == (nch, nthr), (kv, nch, nthr)
            gx, gy = (int(v) for v in kv["grid"].split("x"))
            assert gy == n and gx == int(kv["gx"]) and kv["block"] == str(THREADS) and kv["comms_on_dev"] == "1"
            assert kv["llslot"] == str(2 * LL_BYTES)
            assert _slots(kv) == _want_slots(func, n, root)
            assert all(c.last_algo() == variant for c in comms)
    finally:
        _destroy(comms)


@pytest.mark.parametrize("func", FUNCS)
def test_the_limit_itself_takes_the_new_mode_and_one_more_the_parents_ring(fake, func):
    fake(1)
    n, limit = 4, 4096
    dtype = I8 if func == "bc" else F32  # one byte / one element more
    at = limit // ESIZE[dtype]
    comms = C.init_all([0] * n, _cfg())
    try:
        _raw_log()
        _call(func, comms, at + 1, dtype, roots=(2,))  # limits still 0
        (before,) = _launches()
        assert before["kind"] == "ring"
        for oneshot, ll, mode in ((limit, 0, "oneshot"), (0, limit, "ll")):
            _set(comms, func, oneshot=oneshot, ll=ll)
            _call(func, comms, at, dtype, roots=(2,))
            (kv,) = _launches()
            assert kv["mode"] == f"{func}-{mode}" and kv["root"] == "2" and comms[0].last_algo() == mode
            _call(func, comms, at + 1, dtype, roots=(2,))
            (after,) = _launches()
            assert after["kind"] == "ring" and comms[0].last_algo() == "ring"
            assert _no_guard_order(" ".join(f"{k}={v}" for k, v in after.items())) == \
                _no_guard_order(" ".join(f"{k}={v}" for k, v in before.items()))
    finally:
        _destroy(comms)


def test_the_two_functions_limits_are_apart(fake):
    fake(1)
    comms = C.init_all([0] * 4, _cfg())
    try:
        _raw_log()
        for c in comms:
            c.set_rooted_direct(bcast_bytes=CAP)
        _call("bc", comms, 100)
        assert _launches()[0]["mode"] == "bc-oneshot"
        _call("rd", comms, 100)
        assert _launches()[0]["kind"] == "ring"
        for c in comms:
            c.set_rooted_direct(reduce_ll_bytes=LL_CAP)  # and every call sets all four
        _call("bc", comms, 100)
        assert _launches()[0]["kind"] == "ring"
        _call("rd", comms, 100)
        assert _launches()[0]["mode"] == "rd-ll"
    finally:
        _destroy(comms)


@pytest.mark.parametrize("func", FUNCS)
def test_ll_wins_where_both_fit(fake, func):
    fake(1)
    comms = C.init_all([0] * 4, _cfg())
    try:
        _set(comms, func, oneshot=CAP, ll=1024)
        _raw_log()
        _call(func, comms, 256)
        (kv,) = _launches()
        assert kv["mode"] == func + "-ll" and comms[0].last_algo() == "ll"
        _call(func, comms, 257)
        (kv,) = _launches()
        assert kv["mode"] == func + "-oneshot" and comms[0].last_algo() == "oneshot"
        _call(func, comms, CAP // 4 + 1)
        (kv,) = _launches()
        assert kv["kind"] == "ring"
    finally:
        _destroy(comms)


@pytest.mark.parametrize("func", FUNCS)
def test_two_calls_in_a_group_take_the_ring_with_both_roots(fake, func):
    fake(1)
    comms = C.init_all([0] * 4, _cfg())
    try:
        _raw_log()
        _call(func, comms, 500, roots=(3, 1))
        before = _raw_log()
        _set(comms, func, oneshot=CAP, ll=LL_CAP)
        _call(func, comms, 500, roots=(3, 1))
        after = _raw_log()
        # the whole log, work uploads included: the held first call went back to the ring with its root
        assert [_no_guard_order(x) for x in after] == [_no_guard_order(x) for x in before]
        (kv,) = [kv for k, kv in map(_parse, after) if k == "launch"]
        assert kv["kind"] == "ring" and comms[0].last_algo() == "ring"
        _call(func, comms, 500, roots=(1,))  # and a single call afterwards is direct again
        (kv,) = _launches()
        assert kv["mode"] == func + "-ll" and kv["root"] == "1"
    finally:
        _destroy(comms)


def test_premulsum_sumpostdiv_and_avg_take_the_ring(fake):
    fake(1)
    n = 4
    comms = C.init_all([0] * n, _cfg())
    try:
        _set(comms, "rd", oneshot=CAP, ll=LL_CAP)
        _raw_log()
        _call("rd", comms, 500, F32, PREMULSUM, op_arg=0x3F000000)
        (kv,) = _launches()
        assert kv["kind"] == "ring" and comms[0].last_algo() == "ring"
        _call("rd", comms, 500, I32, SUMPOSTDIV, op_arg=n)
        (kv,) = _launches()
        assert kv["kind"] == "ring"
        for dtype in (F32, I32):
            with C.group():
                for r, c in enumerate(comms):
                    c.reduce_avg(_send(r), _recv(r) if r == 1 else None, 500, dtype, root=1, stream=0)
            (kv,) = _launches()
            assert kv["kind"] == "ring" and comms[0].last_algo() == "ring"
        _call("rd", comms, 500, F32, SUM, op_arg=0)  # the OpArg entry with a plain op is a plain call
        (kv,) = _launches()
        assert kv["mode"] == "rd-ll"
    finally:
        _destroy(comms)


@pytest.mark.parametrize("n", [1, 9])
def test_outside_two_to_eight_ranks_the_caps_are_zero_and_the_ring_runs(fake, n):
    fake(1)
    comms = C.init_all([0] * n, _cfg())
    try:
        assert all(c.rooted_direct_max() == (0, 0) for c in comms)
        for c in comms:
            c.set_rooted_direct(0, 0, 0, 0)
            with pytest.raises(MccsError):
                c.set_rooted_direct(8, 0, 0, 0)
        _raw_log()
        for func in FUNCS:
            _call(func, comms, 64, roots=(n - 1,))
            assert all(kv["kind"] == "ring" for kv in _launches())
            assert comms[0].last_algo() == "ring"
    finally:
        _destroy(comms)


@pytest.mark.parametrize("func", FUNCS)
def test_captured_and_per_device_launches_are_recorded(fake, func):
    fake(2)
    lib = _lib.load()
    comms = C.init_all([0, 0, 1, 1], _cfg())
    try:
        _set(comms, func, oneshot=CAP, ll=1024)
        _raw_log()
        stream = 0x5000
        assert lib.mccs_test_fake_capture(stream, 9) == 0
        _call(func, comms, 256, roots=(2,), stream=stream)
        _call(func, comms, 2000, roots=(1,), stream=stream)
        assert lib.mccs_test_fake_capture(stream, 0) == 0
        got = _launches()
        # two devices, two fused rank slots each; a captured launch has no stop event
        assert len(got) == 4 and all(kv["grid"].endswith("x2") and kv["stop_event"] == "0" for kv in got)
        assert [kv["mode"] for kv in got] == [func + "-ll"] * 2 + [func + "-oneshot"] * 2
        assert [kv["root"] for kv in got] == ["2", "2", "1", "1"]
        for i, kv in enumerate(got):
            want = _want_slots(func, 4, 2 if i < 2 else 1)
            assert _slots(kv) == (want[:2] if i % 2 == 0 else want[2:])
        lib.mccs_test_fake_destroy_graph(9)
        _call(func, comms, 2000, roots=(3,))  # eager: the stop event rides on the launch
        got = _launches()
        assert len(got) == 2 and all(kv["stop_event"] != "0" and kv["mode"] == func + "-oneshot" for kv in got)
    finally:
        _destroy(comms)


@pytest.mark.parametrize("blocks", [None, 1])
@pytest.mark.parametrize("func", FUNCS)
def test_workgroups_follow_the_data_phase_and_are_capped(fake, monkeypatch, func, blocks):
    if blocks:
        monkeypatch.setenv("MCCS_DIRECT_BLOCKS", str(blocks))
    fake(1)
    n = 4
    copies = n - 1 if func == "bc" else 1  # the root's n-1 copies; a Reduce sender's one buffer
    comms = C.init_all([0] * n, _cfg())
    try:
        _set(comms, func, oneshot=CAP, ll=0)
        _raw_log()
        # count-based: 4 KiB of the busiest rank's data phase per workgroup; the fake device holds 256
        # workgroups at once, 64 for each of the four fused rank slots
        for count in (1, 1024, 1025, 4096, CAP // 4):
            _call(func, comms, count)
            (kv,) = _launches()
            want = -(-copies * count * 4 // 4096)
            assert int(kv["gx"]) == (1 if blocks else min(want, 64)), (count, kv["gx"])
            esz = 1 if func == "bc" else 4
            assert int(kv["piece"]) * esz % 4096 == 0 and int(kv["piece2"]) * esz % 4096 == 0
        _set(comms, func, oneshot=0, ll=LL_CAP)
        # LL: one 8-byte word of the buffer per thread
        for count in (1, 2 * THREADS, 2 * THREADS + 2, LL_CAP // 4):
            _call(func, comms, count)
            (kv,) = _launches()
            want = -(-(-(-count * 4 // 8)) // THREADS)
            assert kv["mode"] == func + "-ll" and int(kv["gx"]) == (1 if blocks else min(want, 64)), (count, kv["gx"])
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
        for k, name in enumerate(("bcast_bytes", "bcast_ll_bytes", "reduce_bytes", "reduce_ll_bytes")):
            cap = LL_CAP if k % 2 else CAP
            args = [0, 0, 0, 0]
            args[k] = cap + 8
            _refused(INVALID_ARGUMENT, f"mccsCommSetRootedDirect: {name}", lambda: c.set_rooted_direct(*args),
                     also=(str(cap + 8), str(cap)))
        c.set_rooted_direct(CAP, LL_CAP, CAP, LL_CAP)  # the capacities themselves are fine
        c.set_rooted_direct()

        def in_group():
            with C.group():
                c.set_rooted_direct(64, 64, 64, 64)

        _refused(INVALID_USAGE, "mccsCommSetRootedDirect: the communicator has a group open", in_group)
        lib = _lib.load()
        assert lib.mccsGroupStart() == 0
        assert lib.mccsReduce(_send(0), _recv(0), 16, F32, SUM, 0, c._h, 0) == 0
        assert lib.mccsCommSetRootedDirect(c._h, 64, 64, 64, 64) == INVALID_USAGE
        assert "a call pending" in _lib.last_error()
        assert lib.mccsReduce(_send(1), None, 16, F32, SUM, 0, comms[1]._h, 0) == 0
        assert lib.mccsGroupEnd() == 0
        (kv,) = _launches()
        assert kv["kind"] == "ring"  # the refused setter changed nothing
    finally:
        _destroy(comms)


def test_argument_checks_come_first_and_keep_their_code_and_diagnosis(fake):
    """Root out of range and a NULL buffer by role, refused as on a
    communicator that never opted in; NULL where the role uses no buffer is
    accepted by the direct path as by the ring."""
    fake(1)
    comms = C.init_all([0, 0], _cfg())
    plain = C.init_all([0, 0], _cfg())
    try:
        for c in comms:
            c.set_rooted_direct(CAP, LL_CAP, CAP, LL_CAP)
        _raw_log()
        said = []
        for c in (comms[0], plain[0]):
            errs = []
            for root in (-1, 2):
                for what, call in (("mccsBroadcast", lambda: C.broadcast(c, _send(0), _recv(0), 1024, root, stream=0)),
                                   ("mccsReduce", lambda: C.reduce(c, _send(0), _recv(0), 256, F32, SUM, root,
                                                                   stream=0))):
                    with pytest.raises(MccsError) as ei:
                        call()
                    assert ei.value.code == INVALID_ARGUMENT
                    assert f"root {root} outside 0..1" in _lib.last_error()
                    errs.append(_lib.last_error())
            for call in (lambda: C.broadcast(c, None, _recv(0), 1024, 0, stream=0),   # the root's sendbuff
                         lambda: C.broadcast(c, _send(0), None, 1024, 0, stream=0),   # any rank's recvbuff
                         lambda: C.broadcast(c, None, None, 1024, 1, stream=0),
                         lambda: C.reduce(c, None, _recv(0), 256, F32, SUM, 0, stream=0),  # any rank's sendbuff
                         lambda: C.reduce(c, None, None, 256, F32, SUM, 1, stream=0),
                         lambda: C.reduce(c, _send(0), None, 256, F32, SUM, 0, stream=0)):  # the root's recvbuff
                with pytest.raises(MccsError) as ei:
                    call()
                assert ei.value.code == INVALID_ARGUMENT and "null send or recv buffer" in _lib.last_error()
                errs.append(_lib.last_error())
            for dtype, op in ((10, SUM), (-1, SUM), (F32, 4), (F32, -1)):
                with pytest.raises(MccsError) as ei:
                    C.reduce(c, _send(0), _recv(0), 256, dtype, op, 0, stream=0)
                assert ei.value.code == INVALID_ARGUMENT and "unknown dtype or reduction op" in _lib.last_error()
                errs.append(_lib.last_error())
            said.append(errs)
        assert said[0] == said[1]
        assert _launches() == []
        _call("bc", comms, 1024, I8, roots=(1,))  # NULL send on the non-root, as the ring allows
        (kv,) = _launches()
        assert kv["mode"] == "bc-ll" and _slots(kv)[0]["send"] == 0
        _call("rd", comms, 256, roots=(1,))  # NULL recv on the non-root
        (kv,) = _launches()
        assert kv["mode"] == "rd-ll" and _slots(kv)[0]["recv"] == 0
    finally:
        _destroy(comms)
        _destroy(plain)


def test_on_a_cached_arena_with_its_system_scope_fences_the_ll_cap_is_zero(fake):
    fake(1)
    comms = C.init_all([0, 0], _cfg(fifo_memory=C.FIFO_DEVICE))
    try:
        cap, ll_cap = comms[0].rooted_direct_max()
        assert ll_cap == 0 and cap == CAP  # the count-based variant fences as the arena needs
        _refused(INVALID_ARGUMENT, "mccsCommSetRootedDirect: reduce_ll_bytes 8 is above the 0 bytes",
                 lambda: comms[0].set_rooted_direct(reduce_ll_bytes=8), also=("the LL path is closed here",))
        for func in FUNCS:
            _set(comms, func, oneshot=CAP, ll=0)
            _raw_log()
            _call(func, comms, 8, roots=(1,))
            (kv,) = _launches()
            assert kv["mode"] == func + "-oneshot" and kv["fence"] == "0"  # MCCS_FENCE_SYSTEM
    finally:
        _destroy(comms)


def test_the_environment_sets_the_four_limits_at_creation_clamped_to_the_caps(fake, monkeypatch):
    monkeypatch.setenv("MCCS_BC_DIRECT_BYTES", str(1 << 30))
    monkeypatch.setenv("MCCS_BC_LL_BYTES", "512")
    monkeypatch.setenv("MCCS_RD_DIRECT_BYTES", "2048")
    monkeypatch.setenv("MCCS_RD_LL_BYTES", str(1 << 30))
    fake(1)
    comms = C.init_all([0, 0], _cfg())
    for v in ENV:
        monkeypatch.delenv(v)  # read at creation, not per call
    try:
        _raw_log()

        def mode(func, count):
            _call(func, comms, count, roots=(1,))
            (kv,) = _launches()
            return kv.get("mode", kv["kind"])

        assert mode("bc", 128) == "bc-ll" and mode("bc", 129) == "bc-oneshot"
        assert mode("bc", CAP // 4) == "bc-oneshot"  # the count-based limit was clamped to the cap
        assert mode("bc", CAP // 4 + 1) == "ring"
        assert mode("rd", LL_CAP // 4) == "rd-ll"  # the LL limit was clamped to its cap
        assert mode("rd", LL_CAP // 4 + 1) == "ring"  # above reduce_bytes = 2048 too
        others = C.init_all([0, 0], _cfg())  # created without the variables: off
        try:
            _raw_log()
            for func in FUNCS:
                _call(func, others, 128)
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
    for name in ("mccsCommSetRootedDirect", "mccsCommRootedDirectMax"):
        assert getattr(lib, name) is not None
        assert name in _lib.SIGNATURES
    src = tmp_path / "rooted.c"
    src.write_text('#include "mccs_hip.h"\n'
                   "mccsResult_t f(mccsComm_t comm, size_t *cap, size_t *ll_cap) {\n"
                   "  mccsResult_t r = mccsCommRootedDirectMax(comm, cap, ll_cap);\n"
                   "  return r ? r : mccsCommSetRootedDirect(comm, *cap, *ll_cap, *cap, *ll_cap);\n}\n")
    r = subprocess.run(build.capi_cmd(str(src), str(tmp_path / "unused"), syntax_only=True), capture_output=True,
                       text=True)
    assert r.returncode == 0, r.stderr
