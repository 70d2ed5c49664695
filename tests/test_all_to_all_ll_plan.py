"""CPU: how the planner launches the LL all-to-all, on the recording fake device
runtime (see tests/test_all_to_all_v_plan.py).

With both limits at 0 every AllToAll / AllToAllv / AllToAllvDev plans as on the
parent commit: tests/golden/a2a_ll_parent_launches.json holds the parent's
`launch` records of parent_cases(), recorded with that commit's library, and the
records of this one are held to them string for string (but for guard_order,
which sorts heap addresses).  With limits set the record is kind=direct
mode=ll-a2a and carries, per rank slot, the rank, both buffers and the four rows
of the call (or the size table's address); the rest checks which calls take it,
G, and every refusal.
"""
import ctypes
import json
import os

import pytest

import a2av_ref as V
from mccs_amd import _lib
from mccs_amd import comm as C
from mccs_amd._lib import MccsError

INVALID_ARGUMENT, INVALID_USAGE = 4, 5
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "a2a_ll_parent_launches.json")
LL_BYTES = 16 << 10
CAP = LL_BYTES - 8  # ll_slot / 2 - 8 with ll_slot = 2 * ll_bytes
THREADS = 512


def _parse(line):
    kind, *kv = line.split()
    return kind, dict(x.split("=", 1) for x in kv)


@pytest.fixture
def fake(monkeypatch):
    lib = _lib.load()
    monkeypatch.setenv("MCCS_TEST_HOOKS", "1")
    monkeypatch.setenv("MCCS_GATE", "0")
    for v in ("MCCS_ALLTOALL_HOPS", "MCCS_A2A_LL_BYTES", "MCCS_A2AV_LL_BYTES", "MCCS_DIRECT_BLOCKS"):
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


def _table(r, k=0):
    return _send(r) + 0x4000000 + 0x1000 * k


def _cfg(**kw):
    return C.CommConfig(buffer_size=V.BUFF, ll_bytes=LL_BYTES, **kw)


def _destroy(comms):
    for c in comms:
        c.destroy()


def _uniform(comms, B, stream=0):
    with C.group():
        for r, c in enumerate(comms):
            C.all_to_all(c, _send(r), _recv(r), B, stream=stream)


def _v(comms, cnt, lay, stream=0):
    n = len(comms)
    with C.group():
        for r, c in enumerate(comms):
            C.all_to_all_v(c, _send(r), cnt[r], lay["sdispls"][r], _recv(r), [cnt[s][r] for s in range(n)],
                           lay["rdispls"][r], stream=stream)


def _dev(comms, k=0, stream=0):
    with C.group():
        for r, c in enumerate(comms):
            C.all_to_all_v_dev(c, _send(r), _recv(r), _table(r, k), stream=stream)


def _small(n, top=4099):
    """A count matrix within the capacity, with zeros, a byte tail and a zero self block."""
    vals = [0, 1, 7, 8, 9, 15, top]
    cnt = [[vals[(3 * s + t) % len(vals)] for t in range(n)] for s in range(n)]
    cnt[0][0] = 0
    return cnt


def _slots(kv):
    """slots= of an ll-a2a record: per rank slot its rank, buffers and rows (or table)."""
    out = []
    for s in kv["slots"].split("/"):
        rank, send, recv, rest = s.split(":", 3)
        d = {"rank": int(rank), "send": int(send, 16), "recv": int(recv, 16)}
        if rest.startswith("table="):
            d["table"] = int(rest[6:], 16)
        else:
            d["rows"] = [[int(x) for x in row.split(",")] for row in rest.split("|")]
        out.append(d)
    return out


def _want_rows(cnt, lay, r):
    n = len(cnt)
    return [list(cnt[r]), list(lay["sdispls"][r]), [cnt[s][r] for s in range(n)], list(lay["rdispls"][r])]


# ---- limits at 0: the parent's records --------------------------------------
def parent_cases():
    """(name, n, call) of every record in the golden file."""
    out = []
    for n in (2, 4, 6, 8):
        out.append((f"a2a n={n}", n, lambda comms: _uniform(comms, 4099)))
        if n == 6:
            continue  # the v calls are refused on the relay route (tests/test_all_to_all_v_plan.py)
        cnt = _small(n)
        lay = V.layout(cnt, "gaps")
        out.append((f"a2av n={n}", n, lambda comms, cnt=cnt, lay=lay: _v(comms, cnt, lay)))
        out.append((f"a2avd n={n}", n, lambda comms: _dev(comms)))
    return out


def record_parent_cases(install):
    """name -> the raw `launch` lines of the case, on fresh communicators."""
    out = {}
    for name, n, call in parent_cases():
        install(1)
        comms = C.init_all([0] * n, C.CommConfig(buffer_size=V.BUFF))
        try:
            _raw_log()
            call(comms)
            out[name] = [x for x in _raw_log() if x.startswith("launch ")]
        finally:
            _destroy(comms)
    return out


def _no_guard_order(line):
    return " ".join(x for x in line.split() if not x.startswith("guard_order="))


def test_with_both_limits_off_every_record_is_the_parents(fake):
    want = json.load(open(GOLDEN))
    got = record_parent_cases(fake)
    assert sorted(got) == sorted(want) and len(got) == 10
    for name in want:
        assert len(got[name]) == 1
        assert [_no_guard_order(x) for x in got[name]] == [_no_guard_order(x) for x in want[name]], name
        assert "mode=ll-a2a" not in got[name][0] and " kind=ring " in got[name][0]


# ---- limits set ---------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 4, 6, 8])
def test_uniform_call_within_the_limit_is_one_ll_launch_with_every_slots_rows(fake, n):
    fake(1)
    comms = C.init_all([0] * n, _cfg())
    try:
        assert all(c.all_to_all_ll_max() == CAP for c in comms)
        for c in comms:
            c.set_all_to_all_ll(bytes_per_peer=4099)
        _raw_log()
        B = 4099
        _uniform(comms, B)
        (kv,) = _launches()
        assert kv["kind"] == "direct" and kv["mode"] == "ll-a2a" and kv["n"] == str(n) and kv["table"] == "0"
        assert kv["llslot"] == str(2 * LL_BYTES) and kv["block"] == str(THREADS) and kv["comms_on_dev"] == "1"
        gx, gy = (int(v) for v in kv["grid"].split("x"))
        assert gy == n and gx == int(kv["gx"])
        slots = _slots(kv)
        for r, s in enumerate(slots):
            assert s["rank"] == r and s["send"] == _send(r) and s["recv"] == _recv(r)
            assert s["rows"] == [[B] * n, [t * B for t in range(n)], [B] * n, [t * B for t in range(n)]]
        assert all(c.last_algo() == "ll" for c in comms)
    finally:
        _destroy(comms)


def test_the_limit_itself_takes_ll_and_one_byte_more_the_parents_ring_elements(fake):
    fake(1)
    n, limit = 4, 1024
    comms = C.init_all([0] * n, _cfg())
    try:
        _raw_log()
        _uniform(comms, limit + 1)  # limits still 0
        (before,) = _launches()
        for c in comms:
            c.set_all_to_all_ll(bytes_per_peer=limit)
        _uniform(comms, limit)
        (kv,) = _launches()
        assert kv["mode"] == "ll-a2a" and comms[0].last_algo() == "ll"
        _uniform(comms, limit + 1)
        (after,) = _launches()
        assert after["kind"] == "ring" and comms[0].last_algo() == "ring"
        for key in ("grid", "block", "a2a", "inline_works", "redop_args", "fence"):
            assert after[key] == before[key], key
    finally:
        _destroy(comms)


def test_two_calls_in_a_group_take_the_ring(fake):
    fake(1)
    n = 4
    comms = C.init_all([0] * n, _cfg())
    cnt = _small(n)
    lay = V.layout(cnt, "packed")
    try:
        for c in comms:
            c.set_all_to_all_ll(bytes_per_peer=CAP, v_bytes_per_peer=CAP)
        _raw_log()
        with C.group():
            for k in range(2):
                for r, c in enumerate(comms):
                    C.all_to_all(c, _send(r) + k * 0x100000, _recv(r) + k * 0x100000, 512, stream=0)
        (kv,) = _launches()
        assert kv["kind"] == "ring" and "a2a" in kv and comms[0].last_algo() == "ring"
        assert all(len(slot.split(",")) == 2 * comms[0].nchannels for slot in kv["a2a"].split("/"))
        with C.group():
            for k in range(2):
                for r, c in enumerate(comms):
                    C.all_to_all_v(c, _send(r), cnt[r], lay["sdispls"][r], _recv(r), [cnt[s][r] for s in range(n)],
                                   lay["rdispls"][r], stream=0)
        (kv,) = _launches()
        assert kv["kind"] == "ring" and "a2av" in kv
        with C.group():
            for k in range(2):
                for r, c in enumerate(comms):
                    C.all_to_all_v_dev(c, _send(r), _recv(r), _table(r, k), stream=0)
        (kv,) = _launches()
        assert kv["kind"] == "ring" and "a2avd" in kv
        # an all-zero first call changes nothing: the second one still takes the ring, as on its peers
        zero = [0] * n
        with C.group():
            for r, c in enumerate(comms):
                C.all_to_all_v(c, None, zero, zero, None, zero, zero, stream=0)
            for r, c in enumerate(comms):
                C.all_to_all_v(c, _send(r), cnt[r], lay["sdispls"][r], _recv(r), [cnt[s][r] for s in range(n)],
                               lay["rdispls"][r], stream=0)
        (kv,) = _launches()
        assert kv["kind"] == "ring" and "a2av" in kv
        _v(comms, cnt, lay)  # and a single call afterwards is LL again
        (kv,) = _launches()
        assert kv["mode"] == "ll-a2a"
    finally:
        _destroy(comms)


@pytest.mark.parametrize("how", ["six ranks", "env"])
def test_v_and_dev_calls_need_no_route(fake, monkeypatch, how):
    fake(1)
    n = 6 if how == "six ranks" else 4
    if how == "env":
        monkeypatch.setenv("MCCS_ALLTOALL_HOPS", "relay")
    comms = C.init_all([0] * n, _cfg())
    cnt = _small(n)
    lay = V.layout(cnt, "misaligned")
    try:
        assert comms[0].all_to_all_route()["hops"] == n - 1
        for c in comms:
            c.set_all_to_all_ll(v_bytes_per_peer=4099)
        _raw_log()
        _v(comms, cnt, lay)
        (kv,) = _launches()
        assert kv["mode"] == "ll-a2a" and kv["table"] == "0"
        for r, s in enumerate(_slots(kv)):
            assert s["rank"] == r and s["rows"] == _want_rows(cnt, lay, r), r
        _dev(comms)
        (kv,) = _launches()
        assert kv["mode"] == "ll-a2a" and kv["table"] == "1"
        # a Dev record carries the table's address and no counts
        assert _slots(kv) == [{"rank": r, "send": _send(r), "recv": _recv(r), "table": _table(r)} for r in range(n)]
        assert all(c.last_algo() == "ll" for c in comms)
        _uniform(comms, 64)  # the uniform limit is 0: the relay ring
        (kv,) = _launches()
        assert kv["kind"] == "ring"
        # two v calls in one group fall back to the ring's rules: the relay refusal
        with pytest.raises(MccsError) as ei:
            with C.group():
                for k in range(2):
                    C.all_to_all_v(comms[0], _send(0), cnt[0], lay["sdispls"][0], _recv(0),
                                   [cnt[s][0] for s in range(n)], lay["rdispls"][0], stream=0)
        assert ei.value.code == INVALID_USAGE and "the AllToAll route is not one hop" in _lib.last_error()
        assert not _launches()
    finally:
        _destroy(comms)


def test_an_all_zero_v_call_still_launches(fake):
    fake(1)
    n = 4
    comms = C.init_all([0] * n, _cfg())
    zero = [0] * n
    try:
        _raw_log()
        with C.group():
            for c in comms:
                C.all_to_all_v(c, None, zero, zero, None, zero, zero, stream=0)
        assert not _launches()  # the ring launches nothing
        for c in comms:
            c.set_all_to_all_ll(v_bytes_per_peer=64)
        with C.group():
            for c in comms:
                C.all_to_all_v(c, None, zero, zero, None, zero, zero, stream=0)
        (kv,) = _launches()
        assert kv["mode"] == "ll-a2a" and kv["grid"] == f"1x{n}"
        assert all(s["rows"] == [zero] * 4 for s in _slots(kv))
    finally:
        _destroy(comms)


def test_captured_and_per_device_launches_are_recorded(fake):
    fake(2)
    lib = _lib.load()
    n = 4
    comms = C.init_all([0, 0, 1, 1], _cfg())
    cnt = _small(n)
    lay = V.layout(cnt, "descending")
    try:
        for c in comms:
            c.set_all_to_all_ll(bytes_per_peer=2048, v_bytes_per_peer=4099)
        _raw_log()
        stream = 0x5000
        assert lib.mccs_test_fake_capture(stream, 9) == 0
        _uniform(comms, 2048, stream=stream)
        _v(comms, cnt, lay, stream=stream)
        _dev(comms, stream=stream)
        assert lib.mccs_test_fake_capture(stream, 0) == 0
        got = _launches()
        # two devices, two fused rank slots each; a captured launch has no stop event
        assert len(got) == 6 and all(kv["mode"] == "ll-a2a" and kv["grid"].endswith("x2") for kv in got)
        assert all(kv["stop_event"] == "0" for kv in got)
        for i, kv in enumerate(got):
            assert [s["rank"] for s in _slots(kv)] == ([0, 1] if i % 2 == 0 else [2, 3])
        for kv in got[2:4]:
            for s in _slots(kv):
                assert s["rows"] == _want_rows(cnt, lay, s["rank"])
        for kv in got[4:]:
            assert kv["table"] == "1" and all(s["table"] == _table(s["rank"]) for s in _slots(kv))
        lib.mccs_test_fake_destroy_graph(9)
        _v(comms, cnt, lay)  # eager: the stop event rides on the launch
        got = _launches()
        assert len(got) == 2 and all(kv["stop_event"] != "0" for kv in got)
    finally:
        _destroy(comms)


def _words(c):
    return -(-c // 8)


@pytest.mark.parametrize("blocks", [None, 1])
def test_workgroups_follow_the_larger_side_one_word_per_thread(fake, monkeypatch, blocks):
    if blocks:
        monkeypatch.setenv("MCCS_DIRECT_BLOCKS", str(blocks))
    fake(1)
    n = 4
    comms = C.init_all([0] * n, _cfg())
    try:
        for c in comms:
            c.set_all_to_all_ll(bytes_per_peer=CAP, v_bytes_per_peer=CAP)
        _raw_log()
        for B in (1, 8 * THREADS // n, 8 * THREADS // n + 1, CAP):
            _uniform(comms, B)
            (kv,) = _launches()
            # every slot sends n blocks (its own is copied in the send phase) and receives n - 1
            want = -(-n * _words(B) // THREADS)
            # the fake device holds 256 workgroups at once: 64 for each of the four fused rank slots
            assert int(kv["gx"]) == (1 if blocks else min(want, 64)), (B, kv["gx"])
        # skewed counts: G is the largest slot's; rank 2 receives CAP from everyone
        cnt = [[CAP if t == 2 and s != 2 else 1 for t in range(n)] for s in range(n)]
        _v(comms, cnt, V.layout(cnt, "packed"))
        (kv,) = _launches()
        want = -(-max(3 * _words(CAP), 2 * _words(1) + _words(1) + _words(CAP)) // THREADS)
        assert int(kv["gx"]) == (1 if blocks else want)
        # Dev: the host knows no count, so n blocks of the promise
        _dev(comms)
        (kv,) = _launches()
        assert int(kv["gx"]) == (1 if blocks else min(-(-n * _words(CAP) // THREADS), 64))
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
        _refused(INVALID_ARGUMENT, "mccsCommSetAllToAllLL: bytes_per_peer", lambda: c.set_all_to_all_ll(CAP + 1, 0),
                 also=(str(CAP + 1), str(CAP)))
        _refused(INVALID_ARGUMENT, "mccsCommSetAllToAllLL: v_bytes_per_peer", lambda: c.set_all_to_all_ll(0, CAP + 8))
        c.set_all_to_all_ll(CAP, CAP)  # the capacity itself is fine
        c.set_all_to_all_ll(0, 0)

        def in_group():
            with C.group():
                c.set_all_to_all_ll(64, 64)

        _refused(INVALID_USAGE, "mccsCommSetAllToAllLL: the communicator has a group open", in_group)
        lib = _lib.load()
        assert lib.mccsGroupStart() == 0
        assert lib.mccsAllToAll(_send(0), _recv(0), 64, c._h, 0) == 0
        assert lib.mccsCommSetAllToAllLL(c._h, 64, 64) == INVALID_USAGE
        assert lib.mccsAllToAll(_send(1), _recv(1), 64, comms[1]._h, 0) == 0
        assert lib.mccsGroupEnd() == 0
        (kv,) = _launches()
        assert kv["kind"] == "ring"  # the refused setter changed nothing
    finally:
        _destroy(comms)


def test_a_host_count_above_the_v_limit_is_refused_and_names_the_peer(fake):
    fake(1)
    n = 4
    comms = C.init_all([0] * n, _cfg())
    try:
        for c in comms:
            c.set_all_to_all_ll(v_bytes_per_peer=1000)
        _raw_log()
        sc, rc = [8, 8, 1001, 8], [8, 8, 8, 8]
        d = [0, 1024, 2048, 4096]
        _refused(INVALID_ARGUMENT, "mccsAllToAllv: sendcounts[2] = 1001",
                 lambda: C.all_to_all_v(comms[0], _send(0), sc, d, _recv(0), rc, d, stream=0), also=("1000",))
        _refused(INVALID_ARGUMENT, "mccsAllToAllv: recvcounts[3] = 2000",
                 lambda: C.all_to_all_v(comms[0], _send(0), rc, d, _recv(0), [8, 8, 8, 2000], d, stream=0))
        # the other argument rules stay
        _refused(INVALID_ARGUMENT, "mccsAllToAllv: sendcounts[rank] != recvcounts[rank]",
                 lambda: C.all_to_all_v(comms[0], _send(0), [9, 8, 8, 8], d, _recv(0), rc, d, stream=0))
        _refused(INVALID_ARGUMENT, "mccsAllToAllv: null buffer",
                 lambda: C.all_to_all_v(comms[0], None, rc, d, _recv(0), rc, d, stream=0))
        _refused(INVALID_ARGUMENT, "mccsAllToAllvDev: null size table",
                 lambda: C.all_to_all_v_dev(comms[0], _send(0), _recv(0), None, stream=0))
        assert not _launches()
        cnt = [[1000] * n for _ in range(n)]
        _v(comms, cnt, V.layout(cnt, "packed"))  # the limit itself passes, and the comms stay usable
        (kv,) = _launches()
        assert kv["mode"] == "ll-a2a"
    finally:
        _destroy(comms)


@pytest.mark.parametrize("how", ["cached arena", "one rank", "nine ranks", "ll off"])
def test_where_the_lines_cannot_be_used_the_capacity_is_zero(fake, how):
    fake(1)
    n = {"one rank": 1, "nine ranks": 9}.get(how, 2)
    cfg = _cfg(fifo_memory=1) if how == "cached arena" else _cfg()  # MCCS_FIFO_DEVICE
    if how == "ll off":
        cfg.ll_bytes = -1
    comms = C.init_all([0] * n, cfg)
    try:
        assert all(c.all_to_all_ll_max() == 0 for c in comms)
        _refused(INVALID_ARGUMENT, "mccsCommSetAllToAllLL: bytes_per_peer 8 is above the 0 bytes",
                 lambda: comms[0].set_all_to_all_ll(8, 0), also=("the LL path is closed here",))
        comms[0].set_all_to_all_ll(0, 0)
        _raw_log()
        _uniform(comms, 8)
        assert all(kv["kind"] == "ring" for kv in _launches())
    finally:
        _destroy(comms)


def test_the_environment_sets_both_limits_at_creation_clamped_to_the_capacity(fake, monkeypatch):
    monkeypatch.setenv("MCCS_A2A_LL_BYTES", "512")
    monkeypatch.setenv("MCCS_A2AV_LL_BYTES", str(1 << 30))
    fake(1)
    n = 2
    comms = C.init_all([0] * n, _cfg())
    monkeypatch.delenv("MCCS_A2A_LL_BYTES")  # read at creation, not per call
    monkeypatch.delenv("MCCS_A2AV_LL_BYTES")
    try:
        _raw_log()
        _uniform(comms, 512)
        (kv,) = _launches()
        assert kv["mode"] == "ll-a2a"
        _uniform(comms, 513)
        (kv,) = _launches()
        assert kv["kind"] == "ring"
        # the v limit was clamped to the capacity: a count of CAP passes, CAP + 1 is above the limit
        cnt = [[CAP] * n for _ in range(n)]
        _v(comms, cnt, V.layout(cnt, "packed"))
        (kv,) = _launches()
        assert kv["mode"] == "ll-a2a"
        _refused(INVALID_ARGUMENT, f"mccsAllToAllv: sendcounts[0] = {CAP + 1}",
                 lambda: C.all_to_all_v(comms[0], _send(0), [CAP + 1] * n, [0, 1 << 20], _recv(0), [CAP + 1] * n,
                                        [0, 1 << 20], stream=0), also=(f"limit of {CAP} bytes",))
        others = C.init_all([0] * n, _cfg())  # created without the variables: off
        try:
            _raw_log()
            _uniform(others, 512)
            (kv,) = _launches()
            assert kv["kind"] == "ring"
        finally:
            _destroy(others)
    finally:
        _destroy(comms)


def test_exchange_counts_takes_ll_once_the_uniform_limit_is_set(fake):
    fake(1)
    comms = C.init_all([0, 0], _cfg())
    try:
        for c in comms:
            c.set_all_to_all_ll(bytes_per_peer=8)
        _raw_log()
        with C.group():
            for r, c in enumerate(comms):
                c.exchange_counts(_table(r), stream=0)
        (kv,) = _launches()
        assert kv["mode"] == "ll-a2a"
        for r, s in enumerate(_slots(kv)):
            assert s["send"] == _table(r) and s["recv"] == _table(r) + 2 * 2 * 8 and s["rows"][0] == [8, 8]
    finally:
        _destroy(comms)


def test_c_abi_declarations_compile_as_c(tmp_path):
    import subprocess

    from mccs_amd import build

    src = tmp_path / "ll.c"
    src.write_text('#include "mccs_hip.h"\n'
                   "mccsResult_t f(mccsComm_t comm, size_t *cap) {\n"
                   "  mccsResult_t r = mccsCommAllToAllLLMax(comm, cap);\n"
                   "  return r ? r : mccsCommSetAllToAllLL(comm, *cap, *cap);\n}\n")
    r = subprocess.run(build.capi_cmd(str(src), str(tmp_path / "unused"), syntax_only=True), capture_output=True,
                       text=True)
    assert r.returncode == 0, r.stderr
