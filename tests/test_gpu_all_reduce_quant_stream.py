"""GPU: the opt-in block-scaled FP8 streamed AllReduce (csrc/direct_quant_stream_ar.h) on the virtual node, bit for bit
(NaN payloads aside) against tests/quant_ref.py on every rank; every run asserts last_algo().  Rounds hold <= 63488 elements."""
import contextlib

import numpy as np
import pytest

from mccs_amd import comm as C
import quant_ref
import vnode
import wide_ref
from test_gpu_reduce_wide import _scalar

pytestmark = pytest.mark.gpu
DIRECT_DEFAULTS = True  # the configuration below sets every threshold
F16, F32, BF16, SUM, BAND = 6, 7, 9, 0, 64


@contextlib.contextmanager
def _comms(n, window=(1 << 20, 0, 1024)):
    comms = C.init_all([0] * n, C.CommConfig(ll_bytes=4 << 10, oneshot_bytes=64 << 10, direct_bytes=128 << 10, timeout_ms=8000))
    try:
        for c in comms if window else []:
            c.set_all_reduce_quant_stream(*window)
        yield comms
    finally:
        vnode.destroy(comms)


def _issue(comms, xs, code, inplace=False, op=SUM, op_arg=None, shift=0, algo="quant-stream"):  # one grouped call, not
    # awaited; the operands lie `shift` bytes into frames of 0xA5 bytes with bands of 64 bytes
    import torch

    n, nb, lo = len(comms), xs[0].size * xs[0].itemsize, BAND + shift
    frames = [[torch.full((lo + nb + BAND,), 0xA5, dtype=torch.uint8, device="cuda") for _ in range(n)] for _ in range(2)]
    for r in range(n):
        frames[0][r][lo:lo + nb] = vnode.to_dev(xs[r])
    with C.group():
        for r in range(n):
            C.all_reduce(comms[r], frames[0][r].data_ptr() + lo, frames[not inplace][r].data_ptr() + lo, xs[0].size, code, op,
                         op_arg=op_arg)
    assert [c.last_algo() for c in comms] == [algo] * n
    return frames, lo, nb


def _check(comms, issued, xs, code, want, inplace=False, tag=None):  # the output; bands and send buffer untouched
    (send, recv), lo, nb = issued
    for c in comms:
        c.sync()
    for r in range(len(comms)):
        got = (send if inplace else recv)[r]
        out = vnode.from_dev(got[lo:lo + nb], code)
        assert wide_ref.same(out, want, code) if code != F32 else np.array_equal(out, want), (tag, r)
        assert bool((got[:lo] == 0xA5).all() and (got[lo + nb:] == 0xA5).all()), ("band", tag, r)
        assert bool((recv[r] == 0xA5).all()) if inplace else send[r].cpu().numpy()[lo:lo + nb].tobytes() == xs[r].tobytes(), tag


def _all_four(comms, counts, code, rng, shift=0):  # in and out of place, Sum and PreMulSum (1/n); one reference each
    for cnt in counts:
        xs = [vnode.gen(code, cnt, rng) for _ in comms] if isinstance(cnt, int) else cnt
        for op, arg in ((SUM, None), C.avg_op(code, len(comms))):
            want = quant_ref.all_reduce(xs, code, _scalar(code, arg))
            for inplace in (False, True):
                _check(comms, _issue(comms, xs, code, inplace, op, arg, shift), xs, code, want, inplace, (cnt, op, inplace))


@pytest.mark.parametrize("code", [F16, BF16])
@pytest.mark.parametrize("n", [2, 3, 8])
def test_bits_across_the_round_structure(code, n):
    """Rounds of one unit, count = (n-1) 512 u + last: partial tail blocks and units, a last share exhausted early."""
    rng = np.random.default_rng(n)
    with _comms(n) as comms:
        _all_four(comms, [(n - 1) * 512 * u + last for u in (1, 2, 3, 5)
                          for last in (1, 31, 512 * u) + ((513,) if u >= 2 else ())], code, rng)
        for c in comms:
            c.set_all_reduce_quant_stream(1 << 20, 0, 2048)  # two units a round
        _all_four(comms, [(n - 1) * 1024 * 2 + 513], code, rng)


@pytest.mark.parametrize("blocks, n, round_bytes, shift, counts", [
    ("1", 3, 8192, 0, (3 * 4097, 6 * 4096 + 77, 2 * 4096 * 5 + 1)),  # K = 2, 3, 4; four workgroups wanted: with one or
    ("3", 3, 8192, 0, (3 * 4097, 6 * 4096 + 77, 2 * 4096 * 5 + 1)),  # three, some hold no piece of a leg in a round
    ("128", 2, 1024, 2, (1024 + 37,))])  # send and recv 2 bytes off a 16-byte boundary: the bounded 2-byte path, K = 2
def test_bits_with_idle_workgroups_and_misaligned_operands(monkeypatch, blocks, n, round_bytes, shift, counts):
    monkeypatch.setenv("MCCS_DIRECT_BLOCKS", blocks)
    with _comms(n, (1 << 20, 0, round_bytes)) as comms:
        for code in (F16, BF16):
            _all_four(comms, counts, code, np.random.default_rng(7), shift)


def test_neighbours_on_one_communicator_without_a_sync():
    """Previous-launch and next-launch hazards on the scatter slots and the gather halves; each result checked."""
    n, rng, runs = 4, np.random.default_rng(11), []
    with _comms(n, (20000, 2048, 1024)) as comms:
        for c in comms:
            c.set_all_reduce_quant(60000, 40000), c.set_all_reduce_wide_stream(200000, 8192)
        for algo, code, cnt in (("quant-stream", BF16, 3 * 512 * 3 + 31), ("quant-direct", BF16, 25000),
                                ("quant-stream", F16, 3 * 512 * 2 + 1), ("wide-stream", BF16, 45000),
                                ("quant-stream", BF16, 3 * 512 + 512), ("oneshot", F32, 3000),
                                ("quant-stream", F16, 3 * 512 * 4 + 513)):
            xs = [vnode.gen(code, cnt, rng, "exact" if code == F32 else "uniform") for _ in range(n)]
            runs.append((algo, code, xs, _issue(comms, xs, code, algo=algo)))
        for algo, code, xs, issued in runs:  # (the fp32 inputs sum exactly in any order)
            want = sum(xs) if code == F32 else (wide_ref if algo == "wide-stream" else quant_ref).all_reduce(xs, code)
            _check(comms, issued, xs, code, want, tag=(algo, xs[0].size))


def test_the_same_bits_as_the_two_shot_and_a_live_comparison():
    """One buffer on the two-shot quant kernel, on the stream only (four rounds) and on the ring (other bits)."""
    n, cnt, rng = 4, 100003, np.random.default_rng(5)
    xs = [wide_ref.narrow(rng.standard_normal(cnt).astype(np.float32), BF16) for _ in range(n)]
    want = quant_ref.all_reduce(xs, BF16)  # finite: both paths equal it bit for bit, so each other
    with _comms(n, None) as two, _comms(n, (1 << 20, 0, 16384)) as stream, _comms(n, None) as plain:
        for c in two:
            c.set_all_reduce_quant(cnt * 2)  # (refused above all_reduce_quant_max())
        _check(two, _issue(two, xs, BF16, algo="quant-direct"), xs, BF16, want, tag="two-shot")
        _check(stream, _issue(stream, xs, BF16), xs, BF16, want, tag="stream")
        issued = _issue(plain, xs, BF16, algo="ring")
        with pytest.raises(AssertionError):  # the ring's bits differ: the comparisons above are live
            _check(plain, issued, xs, BF16, want, tag="ring")


@pytest.mark.parametrize("code", [F16, BF16])
def test_value_rows(code):
    """One block per row: an Inf and a NaN make their blocks NaN everywhere, not their neighbours; denormals, zeros."""
    n, ramp, rng = 3, np.arange(32, dtype=np.float32), np.random.default_rng(31)
    rows = np.zeros((6, n, 32), np.float32)
    rows[0] = np.where(ramp % 2 == 0, -0.0, 0.0)             # -0 on every rank stays -0 ...
    rows[0, 0] = np.where((ramp % 2 == 0) | (ramp % 3 == 0), -0.0, 0.0)  # ... -0 on one rank alone gives +0
    rows[1], rows[2], rows[3], rows[4] = ramp - 11, ramp - 20, (ramp - 16) / 8, ramp / 4
    rows[1, 1, 5], rows[3, 0, 3] = np.inf, np.nan
    rows[5] = (2.0 ** -24 if code == F16 else 2.0 ** -133) * np.where(ramp % 2 == 0, ramp % 7, -(ramp % 5))  # subnormals of T
    xs = [np.concatenate([wide_ref.narrow(rows[:, r].reshape(-1), code), vnode.gen(code, 1000, rng)]) for r in range(n)]
    want = wide_ref.widen(quant_ref.all_reduce(xs, code)[:6 * 32], code).reshape(6, 32)
    assert [int(np.isnan(x).sum()) for x in want] == [0, 32, 0, 32, 0, 0] and np.any(want[5] != 0)  # the rows do what they say
    with _comms(n) as comms:
        _all_four(comms, [xs], code, rng)
