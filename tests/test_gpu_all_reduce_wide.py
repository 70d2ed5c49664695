"""GPU: the opt-in wide-accumulate direct AllReduce (csrc/direct_wide.h) on the
virtual node, bit for bit (NaN payloads aside) against tests/wide_ref.py: fp16
and bf16, Sum and PreMulSum, summed in binary32 in rank order, rounded once.
Every run asserts last_algo().  LL slots for 32 KiB, one-shot slots of 256 KiB,
two-shot slots of 1 MiB; pieces are 4 KiB (2048 elements) to 64 KiB.
"""
import numpy as np
import pytest

from mccs_amd import comm as C
from mccs_amd._lib import MccsError
import vnode
import wide_ref

pytestmark = pytest.mark.gpu
DIRECT_DEFAULTS = True  # CFG sets every threshold

I32, F16, F32, BF16 = 2, 6, 7, 9
SUM, MAX, PREMULSUM, SUMPOSTDIV = 0, 2, 4, 5
CAPS = (32 << 10, 256 << 10, 1 << 20)
BODIES = ["wide-ll", "wide-oneshot", "wide-direct"]
ABOVE = ["oneshot", "direct", "ring"]  # what one element above each body's cap takes
WRAP = [8197, 131059, 500003]          # more words / pieces than 3 workgroups hold at once
each_body = pytest.mark.parametrize("body", BODIES)
each_dtype = pytest.mark.parametrize("code", [F16, BF16])


def _comms(n, body, **kw):
    comms = C.init_all([0] * n, C.CommConfig(ll_bytes=CAPS[0], oneshot_bytes=CAPS[1], direct_bytes=CAPS[2],
                                             timeout_ms=8000, **kw))
    assert comms[0].all_reduce_wide_max() == CAPS
    for c in comms:
        c.set_all_reduce_wide(*[cap if body == b else 0 for b, cap in zip(BODIES, CAPS)])
    return comms


def _run(comms, inputs, code, algo, want=None, inplace=False, op=SUM, op_arg=None):
    """One grouped all_reduce, checked on every rank; out of place the send buffers must stay as they were."""
    n, cnt = len(comms), inputs[0].size
    send = [vnode.to_dev(x) for x in inputs]
    recv = send if inplace else [vnode.to_dev(np.zeros_like(x)) for x in inputs]
    with C.group():
        for r in range(n):
            C.all_reduce(comms[r], send[r], recv[r], cnt, code, op, op_arg=op_arg)
    assert [c.last_algo() for c in comms] == [algo] * n
    for c in comms:
        c.sync()
    got = [vnode.from_dev(t, code).copy() for t in recv]
    for r in range(n):
        assert inplace or vnode.from_dev(send[r], code).tobytes() == inputs[r].tobytes(), ("send buffer written", r)
        assert want is None or wide_ref.same(got[r], want, code), (algo, cnt, inplace, op_arg, r)
    return got


def _bits(code, values):
    """float values as T (fp16 arrays, bf16 raw bits; exact for the values used here)."""
    f = np.asarray(values, np.float32)
    return f.astype(np.float16) if code == F16 else (f.view(np.uint32) >> 16).astype(np.uint16)


@pytest.mark.parametrize("n", [2, 3, 5, 8])
@each_dtype
@each_body
def test_counts_in_place_and_out_of_place(monkeypatch, body, code, n):
    """The LL word (1, 3, 4, 5), the pack (7, 8, 9), n - 1 (ranks that own nothing), 8n +- 1 (every share one
    pack), one piece +- 1, the cap; then a deal that wraps, on communicators held to three workgroups."""
    top = CAPS[BODIES.index(body)] // 2
    for counts, blocks in (({1, 3, 4, 5, 7, 8, 9, n - 1, 8 * n - 1, 8 * n + 1, 2047, 2049, top}, None),
                           ({WRAP[BODIES.index(body)]}, "3")):
        if blocks:
            monkeypatch.setenv("MCCS_DIRECT_BLOCKS", blocks)
        comms = _comms(n, body)
        try:
            rng = np.random.default_rng(n)
            for cnt in sorted(counts):
                xs = [vnode.gen(code, cnt, rng) for _ in range(n)]
                for inplace in (False, True):
                    _run(comms, xs, code, body, wide_ref.all_reduce(xs, code), inplace)
            # one element above the cap: a ring-order path again
            _run(comms, [vnode.gen(code, top + 1, rng) for _ in range(n)], code, ABOVE[BODIES.index(body)])
        finally:
            vnode.destroy(comms)


@each_dtype
@each_body
def test_misaligned_send_and_recv_inside_sentinel_bands(body, code):
    import torch

    n, cnt, band = 3, 4099, 32
    comms = _comms(n, body)
    try:
        xs = [vnode.gen(code, cnt, np.random.default_rng(19)) for _ in range(n)]
        want = vnode.to_dev(wide_ref.all_reduce(xs, code))
        frames = [[torch.empty(band + 16 + cnt * 2 + band, dtype=torch.uint8, device="cuda") for _ in range(n)]
                  for _ in range(2)]
        for a in (2, 6, 14):
            for b in (2, 6, 14):
                for r in range(n):
                    frames[0][r].fill_(0xA5)
                    frames[0][r][band + a:band + a + cnt * 2] = vnode.to_dev(xs[r])
                    frames[1][r].fill_(0xA5)
                keep = [f.clone() for f in frames[0]]
                with C.group():
                    for r in range(n):
                        C.all_reduce(comms[r], frames[0][r].data_ptr() + band + a, frames[1][r].data_ptr() + band + b, cnt,
                                     code, SUM)
                assert comms[0].last_algo() == body
                for c in comms:
                    c.sync()
                for r in range(n):
                    lo, hi = band + b, band + b + cnt * 2
                    assert torch.equal(frames[1][r][lo:hi], want), (a, b, r, "payload")
                    assert bool((frames[1][r][:lo] == 0xA5).all() and (frames[1][r][hi:] == 0xA5).all()), (a, b, r, "band")
                    assert torch.equal(frames[0][r], keep[r]), (a, b, r, "send buffer written")
    finally:
        vnode.destroy(comms)


@pytest.mark.parametrize("n", [3, 5, 8])
@each_dtype
@each_body
def test_value_rows_sum_and_premulsum(body, code, n):
    """Eight value rows (exact in T) with seeded random data behind them."""
    tiny = 2.0 ** -24 if code == F16 else 2.0 ** -133  # the smallest subnormal of T
    # a sum above T's largest finite value that binary32 still holds
    over = [60000.0, 8000.0] if code == F16 else [(2 - 2.0 ** -7) * 2.0 ** 127, 1.5 * 2.0 ** 119]
    rows = np.array([[256.0] + [1.0] * (n - 1),            # absorption: 256 + (n - 1) here
                     [np.inf, -np.inf] + [1.0] * (n - 2),  # NaN
                     [np.inf] + [1.0] * (n - 1),
                     [-0.0] * n,                           # -0
                     [-0.0, 0.0] + [-0.0] * (n - 2),       # +0
                     [tiny] * n,
                     [tiny, -tiny] + [tiny * 3] * (n - 2),
                     over + [0.0] * (n - 2)], np.float32)
    rng = np.random.default_rng(31)
    xs = [np.concatenate([_bits(code, rows[:, r]), vnode.gen(code, 1000, rng)]) for r in range(n)]
    comms = _comms(n, body)
    try:
        w = wide_ref.widen(_run(comms, xs, code, body, wide_ref.all_reduce(xs, code))[0][:8], code)
        assert np.isnan(w[1]) and np.isposinf(w[2]) and np.signbit(w[3]) and w[3] == 0 and not np.signbit(w[4])
        assert w[5] != 0 and np.isposinf(w[7])
        assert code == F16 or w[0] == {3: 258.0, 5: 260.0, 8: 264.0}[n]  # 263 lies between 262 and 264: to even
        # PreMulSum: 1/n (the average), 0, and a bf16 scalar whose product underflows binary32
        assert C.avg_op(code, n)[0] == PREMULSUM
        for s in [C.avg_op(code, n)[1], 0] + ([int(_bits(BF16, [2.0 ** -120])[0])] if code == BF16 else []):
            scalar = np.array([s], np.uint16).view(vnode.NPDT[code])[0]
            _run(comms, xs, code, body, wide_ref.all_reduce(xs, code, scalar), op=PREMULSUM, op_arg=s)
    finally:
        vnode.destroy(comms)


def test_controls_and_refusals():
    """Element r holds 256 on rank r and 1 elsewhere.  Wide: 264 everywhere.  The ring rounds to bf16 after every
    addition, so whichever rank its order sums first, that element stays 256: the comparisons here are live.
    Reversed and doubled rings give the same wide bits.  A limit above its cap is refused, and other dtypes and
    ops on an opted-in communicator keep their old algorithm."""
    n = 8
    xs = [_bits(BF16, [256.0 if r == e else 1.0 for e in range(n)]) for r in range(n)]
    rings = C.default_rings(8, 0)
    plain, twisted = _comms(n, None), _comms(n, None, rings=rings + [list(reversed(r)) for r in rings])
    try:
        assert twisted[0].nchannels == 14
        assert all(np.any(wide_ref.widen(g, BF16) == 256.0) for g in _run(plain, xs, BF16, "ll"))
        rng = np.random.default_rng(17)
        for k, (body, cnt) in enumerate(zip(BODIES, (5003, 28749, 200001))):
            with pytest.raises(MccsError):
                plain[0].set_all_reduce_wide(*[CAPS[j] + (j == k) for j in range(3)])
            for c in twisted:
                c.set_all_reduce_wide(*[cap if body == b else 0 for b, cap in zip(BODIES, CAPS)])
            assert all(np.all(wide_ref.widen(g, BF16) == 264.0) for g in _run(twisted, xs, BF16, body))
            for code in (F16, BF16):
                ys = [vnode.gen(code, cnt, rng) for _ in range(n)]
                _run(twisted, ys, code, body, wide_ref.all_reduce(ys, code))
        for c in twisted:
            c.set_all_reduce_wide(*CAPS)
        for code, op, arg, algo in ((F32, SUM, None, "ll"), (BF16, MAX, None, "ll"), (I32, SUMPOSTDIV, n, "ring")):
            _run(twisted, [vnode.gen(code, 1000, rng) for _ in range(n)], code, algo, op=op, op_arg=arg)
    finally:
        vnode.destroy(plain)
        vnode.destroy(twisted)
