"""CPU: how the planner launches PreMulSum, SumPostDiv and Avg collectives, on
the recording fake device runtime (csrc/host/rt.cpp, mccs_test_fake_runtime:
host memory, no kernel runs; see tests/test_rooted_plan.py).  The uploaded work
elements carry each call's op_arg in redOpArg (the fake's launch record lists
them as redop_args), the new ops always take the ring, the refusals, and the
reference-named kernel handles.
"""
import os
import re
import subprocess

import pytest

import avg_ref as A
from mccs_amd import _lib
from mccs_amd import build
from mccs_amd import comm as C
from mccs_amd._lib import MccsError
from test_rooted_plan import _log, _recv, _send, fake  # noqa: F401  (the fixture)

I8, I32, U32, I64, F16, F32, F64, BF16 = 0, 2, 3, 4, 6, 7, 8, 9
SUM, PROD, PMS, SPD = 0, 1, A.PREMULSUM, A.SUMPOSTDIV
INVALID_ARGUMENT, INVALID_USAGE = 4, 5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "mccs_amd", "libmccs_hip.so")


def _launches():
    return [kv for k, kv in _log() if k == "launch"]


def _args_of(kv):
    """redop_args of a launch record: per rank slot, the redOpArg of every work element."""
    return [[int(x, 16) for x in slot.split(",") if x] for slot in kv["redop_args"].split("/")]


def _call(name, c, r, count, dtype, op, arg, root=0, off=0):
    if name == "all_reduce":
        C.all_reduce(c, _send(r) + off, _recv(r) + off, count, dtype, op, stream=0, op_arg=arg)
    elif name == "reduce_scatter":
        C.reduce_scatter(c, _send(r) + off, _recv(r) + off, count, dtype, op, stream=0, op_arg=arg)
    else:
        C.reduce(c, _send(r) + off, _recv(r) + off if r == root else None, count, dtype, op, root, stream=0,
                 op_arg=arg)


NAMES = ["all_reduce", "reduce_scatter", "reduce"]


@pytest.mark.parametrize("name", NAMES)
def test_work_elements_carry_the_op_arg(fake, name):
    fake(1)
    comms = C.init_all([0] * 4, C.CommConfig(buffer_size=1 << 20))
    third = A.avg_scalar_bits(F32, 3)
    try:
        _log()
        for dtype, op, arg in ((F32, PMS, third), (F64, PMS, A.avg_scalar_bits(F64, 7)), (I64, PMS, (1 << 64) - 1),
                               (I32, SPD, 4), (U32, SPD, A.INT32_MAX), (BF16, PMS, 0x3EAB), (F32, SUM, 0)):
            for count in (1000, 1 << 20):  # inline works and the work FIFO
                with C.group():
                    for r, c in enumerate(comms):
                        _call(name, c, r, count, dtype, op, arg)
                (kv,) = _launches()
                assert kv["kind"] == "ring" and kv["grid"].endswith("x4"), kv
                slots = _args_of(kv)
                assert len(slots) == 4 and all(s and set(s) == {arg} for s in slots), (dtype, op, hex(arg), kv)
        # two calls of one function, dtype and op with different arguments: one launch, each element its own
        a1, a2 = third, A.encode(F32, 3)
        with C.group():
            for j, arg in enumerate((a1, a2)):
                for r, c in enumerate(comms):
                    _call(name, c, r, 1 << 18, F32, PMS, arg, root=j, off=j * 0x400000)
        (kv,) = _launches()
        for s in _args_of(kv):
            assert set(s) == {a1, a2} and s.count(a1) == s.count(a2), (s, kv)
    finally:
        for c in comms:
            c.destroy()


def test_captured_launch_keeps_the_scalar_in_its_work_list(fake):
    fake(1)
    lib = _lib.load()
    import ctypes

    lib.mccs_test_fake_capture.argtypes = [ctypes.c_void_p, ctypes.c_int]
    comms = C.init_all([0] * 2, C.CommConfig(buffer_size=1 << 20))
    arg = A.avg_scalar_bits(F16, 2)
    try:
        _log()
        assert lib.mccs_test_fake_capture(0x7200, 1) == 0
        with C.group():
            for r, c in enumerate(comms):
                C.all_reduce(c, _send(r), _recv(r), 1 << 20, F16, PMS, stream=0x7200, op_arg=arg)
        assert lib.mccs_test_fake_capture(0x7200, 0) == 0
        (kv,) = _launches()
        assert all(s and set(s) == {arg} for s in _args_of(kv)), kv
    finally:
        for c in comms:
            c.destroy()


def test_new_ops_always_take_the_ring(fake):
    """Direct, one-shot and LL configured at 8 ranks: a small Avg AllReduce
    takes the ring while a Sum of the same bytes takes LL."""
    fake(8)
    comms = C.init_all(list(range(8)), C.CommConfig(direct_bytes=8 << 20, oneshot_bytes=256 << 10, ll_bytes=32 << 10))
    try:
        for dtype in (F32, I32):
            op, arg = A.avg_op(dtype, 8)
            for count in (1, 1000, 8192, 65536, 1 << 20):  # LL, one-shot and two-shot sizes
                with C.group():
                    for r, c in enumerate(comms):
                        C.all_reduce(c, _send(r), _recv(r), 1000, dtype, SUM, stream=0)
                assert [c.last_algo() for c in comms] == ["ll"] * 8  # the thresholds are live
                with C.group():  # Sum through the OpArg entry is the plain call: LL too
                    for r, c in enumerate(comms):
                        C.all_reduce(c, _send(r), _recv(r), 1000, dtype, SUM, stream=0, op_arg=0)
                assert [c.last_algo() for c in comms] == ["ll"] * 8
                _log()
                with C.group():
                    for r, c in enumerate(comms):
                        C.all_reduce_avg(c, _send(r), _recv(r), count, dtype, stream=0)
                ls = _launches()
                assert [kv["kind"] for kv in ls] == ["ring"] * 8, (dtype, count, ls)
                assert all(_args_of(kv) and set(_args_of(kv)[0]) == {arg} for kv in ls)
                assert [c.last_algo() for c in comms] == ["ring"] * 8, (dtype, count)
        for c in comms:
            c.sync()
    finally:
        for c in comms:
            c.destroy()


@pytest.mark.parametrize("name", NAMES)
def test_sum_through_oparg_is_the_plain_call(fake, name):
    fake(2)
    comms = C.init_all([0, 1], C.CommConfig(buffer_size=1 << 20))
    try:
        _log()
        rec = []
        for arg in (None, 0):
            for count in (1000, 1 << 20):
                with C.group():
                    for r, c in enumerate(comms):
                        _call(name, c, r, count, F32, PROD, arg, root=1)
            ls = _launches()
            for kv in ls:
                kv.pop("stop_event", None)
            rec.append(ls)
        assert len(rec[0]) == 4 and rec[0] == rec[1], rec
    finally:
        for c in comms:
            c.destroy()


def test_refusals(fake):
    fake(2)
    comms = C.init_all([0, 1], C.CommConfig(buffer_size=1 << 20))
    c = comms[0]
    bad = [  # dtype, op, op_arg, a word of the message
        (F32, SUM, 1, "must be 0"), (I32, 3, 7, "must be 0"),
        (F16, PMS, 0x13C00, "above the element width"), (I8, PMS, 0x100, "above the element width"),
        (F32, PMS, 1 << 32, "above the element width"),
        (F32, SPD, 2, "integer dtype"), (BF16, SPD, 2, "integer dtype"), (F64, SPD, 2, "integer dtype"),
        (I32, SPD, 0, "outside 1..INT32_MAX"), (I64, SPD, 1 << 31, "outside 1..INT32_MAX"),
        (U32, SPD, (1 << 64) - 1, "outside 1..INT32_MAX"),
        (I32, 6, 0, "unknown dtype or reduction op"), (I32, -1, 0, "unknown dtype or reduction op"),
        (10, PMS, 0, "unknown dtype or reduction op"),
    ]
    try:
        _log()
        for name in NAMES:
            for dtype, op, arg, word in bad:
                with pytest.raises(MccsError) as ei:
                    _call(name, c, 0, 1024, dtype, op, arg)
                assert ei.value.code == INVALID_ARGUMENT, (name, dtype, op, arg)
                assert word in str(ei.value) and word in _lib.last_error(), (name, dtype, op, arg, str(ei.value))
            # the plain entry points keep refusing ops 4 and 5
            for op in (PMS, SPD):
                with pytest.raises(MccsError) as ei:
                    _call(name, c, 0, 1024, I32, op, None)
                assert ei.value.code == INVALID_ARGUMENT
            # count 0 succeeds and launches nothing
            _call(name, c, 0, 0, F32, PMS, A.avg_scalar_bits(F32, 2))
            _call(name, c, 0, 0, I32, SPD, 2)
        assert not _launches()
        assert c.last_algo() is None
    finally:
        for x in comms:
            x.destroy()


def test_sum_plus_premulsum_in_a_group_is_refused(fake):
    fake(2)
    comms = C.init_all([0, 1], C.CommConfig(buffer_size=1 << 20))
    lib = _lib.load()
    try:
        _log()
        assert lib.mccsGroupStart() == 0
        for r, c in enumerate(comms):
            assert lib.mccsAllReduce(_send(r), _recv(r), 1024, F32, SUM, c._h, 0) == 0
        assert lib.mccsAllReduceOpArg(_send(0) + 0x100000, _recv(0) + 0x100000, 1024, F32, PMS, 0x3F000000,
                                      comms[0]._h, 0) == INVALID_USAGE
        assert lib.mccsGroupEnd() == INVALID_USAGE
        assert not _launches()
        with C.group():  # the comms stay usable
            for r, c in enumerate(comms):
                C.all_reduce_avg(c, _send(r), _recv(r), 1024, F32, stream=0)
        assert len(_launches()) == 2
    finally:
        for c in comms:
            c.destroy()


# ---- the reference-named handles ------------------------------------------------------------
def _avg_header_symbols():
    src = open(os.path.join(ROOT, "include", "mccs_kernels_avg.h")).read()
    return set(re.findall(r"^MCCS_KERNEL_SYMBOL\((\w+)\);", src, flags=re.M))


def _exported():
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], check=True, capture_output=True, text=True).stdout
    return {line.split()[-1]: line.split()[0] for line in out.splitlines() if line.strip()}


def test_reference_named_handles_and_aliases_exported():
    addr = _exported()
    types = build.REF_TYPES
    handles = [f"mccsKernel_AllReduce_RING_SIMPLE_PreMulSum_{t}" for t in types] + \
              [f"mccsKernel_AllReduce_RING_SIMPLE_SumPostDiv_{t}" for t in types[:6]]
    assert len(handles) == 16
    decl = _avg_header_symbols()
    assert set(handles) <= decl and len(decl) == 17  # + the ___nv_bfloat16 spelling
    for k in decl:
        assert k in addr, k
    for h in handles:
        assert build.cxx_mangled(h) in addr and addr[build.cxx_mangled(h)] == addr[h], h
    nv = "mccsKernel_AllReduce_RING_SIMPLE_PreMulSum___nv_bfloat16"
    bf = "mccsKernel_AllReduce_RING_SIMPLE_PreMulSum_bfloat16"
    assert addr[nv] == addr[bf] and addr[build.cxx_mangled(nv)] == addr[bf]
    for t in types[6:]:
        assert f"mccsKernel_AllReduce_RING_SIMPLE_SumPostDiv_{t}" not in addr


def test_coll_kernel_returns_and_refuses():
    lib = _lib.load()
    allreduce = 4
    seen = set()
    for dtype in range(10):
        p = lib.mccs_hip_coll_kernel(allreduce, dtype, PMS)
        assert p and p not in seen
        seen.add(p)
        q = lib.mccs_hip_coll_kernel(allreduce, dtype, SPD)
        if dtype < 6:
            assert q and q not in seen
            seen.add(q)
        else:
            assert not q
            assert lib.mccs_hip_launch_coll(allreduce, dtype, SPD, 0x1000, 1, 0x2000, 1, 96, None) == INVALID_ARGUMENT
    assert not lib.mccs_hip_coll_kernel(allreduce, F32, 6)
    for func in (1, 3):  # Reduce / ReduceScatter have no reference-named kernels, new ops included
        assert not lib.mccs_hip_coll_kernel(func, I32, PMS)


def test_c_abi_declarations_compile_as_c(tmp_path):
    src = tmp_path / "avg_decls.c"
    src.write_text('#include "mccs_hip.h"\n#include "mccs_kernels.h"\n#include "mccs_kernels_avg.h"\n'
                   "void (*const handle)(struct mccsDevComm *, uint64_t, struct mccsDevWork *) =\n"
                   "    mccsKernel_AllReduce_RING_SIMPLE_PreMulSum_half;\n"
                   "int use(void) {\n  int op; uint64_t arg;\n"
                   "  if (mccsAvgOp(mccsFloat32, 4, &op, &arg)) return 1;\n"
                   "  if (mccsRedOpArgFromDouble(mccsBfloat16, 3.0, &arg)) return 1;\n"
                   "  return (int)mccsAllReduceOpArg(0, 0, 0, mccsFloat32, op, arg, 0, 0) +\n"
                   "         (int)mccsReduceScatterOpArg(0, 0, 0, mccsInt32, mccsDevSumPostDiv, 4, 0, 0) +\n"
                   "         (int)mccsReduceOpArg(0, 0, 0, mccsInt32, mccsDevSumPostDiv, 4, 0, 0, 0);\n}\n")
    r = subprocess.run(build.capi_cmd(str(src), str(tmp_path / "unused"), syntax_only=True), capture_output=True,
                       text=True)
    assert r.returncode == 0, r.stderr
