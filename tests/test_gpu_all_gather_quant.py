"""GPU: the explicit block-scaled FP8 streamed AllGather (csrc/direct_quant_ag.h) on the virtual node, bit for bit (NaN
payloads aside) against narrow(qdq(pad(widen(x_r)))[:c]) per source, the same on every rank, whatever the rounds.  Every
buffer lies inside bands of 0xA5 bytes; every run asserts last_algo() == "quant-stream"."""
import numpy as np
import pytest

from mccs_amd import comm as C
import quant_ref
import quant_rs_ref
import vnode
import wide_ref

pytestmark = pytest.mark.gpu
DIRECT_DEFAULTS = True  # the configuration below sets every threshold
F16, F32, BF16, BAND = 6, 7, 9, 64
COUNTS = (1, 31, 33, 511, 512, 513, 1024, 2 * 512 + 7, 4 * 512 + 511)  # one to five rounds of 512 elements
WIDE = (2 * 8192 + 4097, 8192 + 77, 4 * 8192 + 1)  # three, two and five rounds of 8192: two pieces a round, one in a tail


def _comms(n, round_bytes):
    comms = C.init_all([0] * n, C.CommConfig(ll_bytes=4 << 10, oneshot_bytes=64 << 10, direct_bytes=128 << 10, timeout_ms=8000))
    [c.set_all_gather_quant(round_bytes) for c in comms]
    return comms


def _want(xs, code):  # the definition: every source through QDQ in blocks of 32 from its own start, one rounding
    return np.concatenate([quant_ref.narrow(quant_ref.qdq(np.pad(quant_ref.widen(x, code), (0, -x.size % 32)))[:x.size], code)
                           for x in xs])


def _run(comms, xs, code, inplace, shift=0):
    """One grouped call, send and recv `shift` bytes off alignment inside frames of 0xA5 bytes (in place: send is the
    rank's block of recv), and its checks."""
    import torch

    n, cnt, nb, lo = len(comms), xs[0].size, xs[0].size * 2, BAND + shift
    send = [torch.full((lo + nb + BAND,), 0xA5, dtype=torch.uint8, device="cuda") for _ in range(n)]
    recv = [torch.full((lo + n * nb + BAND,), 0xA5, dtype=torch.uint8, device="cuda") for _ in range(n)]
    for r in range(n):
        (recv[r][lo + r * nb:lo + (r + 1) * nb] if inplace else send[r][lo:lo + nb]).copy_(vnode.to_dev(xs[r]))
    with C.group():
        for r, c in enumerate(comms):
            c.all_gather_quant(recv[r].data_ptr() + lo + r * nb if inplace else send[r].data_ptr() + lo,
                               recv[r].data_ptr() + lo, cnt, code)
    assert [c.last_algo() for c in comms] == ["quant-stream"] * n
    [c.sync() for c in comms]
    want = _want(xs, code)
    for r in range(n):
        tag = (n, code, cnt, inplace, shift, r)
        assert quant_ref.same(vnode.from_dev(recv[r][lo:lo + n * nb], code), want, code), tag
        assert bool((recv[r][:lo] == 0xA5).all() and (recv[r][lo + n * nb:] == 0xA5).all()), ("band", tag)
        keep = send[r].cpu().numpy()
        assert (keep == 0xA5).all() if inplace else keep[lo:lo + nb].tobytes() == xs[r].tobytes() and (
            keep[:lo] == 0xA5).all() and (keep[lo + nb:] == 0xA5).all(), ("send buffer", tag)


@pytest.mark.parametrize("code", [F16, BF16])
@pytest.mark.parametrize("n, blocks, round_bytes, counts", [
    (2, None, 1024, COUNTS), (3, None, 1024, COUNTS), (8, None, 1024, COUNTS),
    (3, "1", 16384, WIDE), (3, "3", 16384, WIDE)])  # four workgroups wanted: held to three, one has no piece of a send
def test_bits_across_rounds_alignments_and_workgroups(monkeypatch, code, n, blocks, round_bytes, counts):
    monkeypatch.setenv("MCCS_DIRECT_BLOCKS", blocks or "128")  # (128: the default)
    comms, rng = _comms(n, round_bytes), np.random.default_rng(n)
    try:
        for k, cnt in enumerate(counts):
            xs = [vnode.gen(code, cnt, rng) for _ in range(n)]
            for inplace in (False, True):  # every count in and out of place; 0, 2, 6 and 14 bytes off alignment in turn
                _run(comms, xs, code, inplace, (0, 2, 6, 14)[(k + inplace) % 4])
    finally:
        vnode.destroy(comms)


@pytest.mark.parametrize("code", [F16, BF16])
def test_value_rows(code):
    """One quantisation block per row at the head of every rank's block."""
    n, ramp, rng = 3, np.arange(32, dtype=np.float32), np.random.default_rng(31)
    top = 65504.0 if code == F16 else (2 - 2.0 ** -7) * 2.0 ** 127  # the largest finite T
    rows = np.zeros((6, n, 32), np.float32)
    rows[0] = np.where(ramp % 2 == 0, -0.0, 0.0)  # signed zeros keep their signs
    rows[1], rows[2], rows[3] = ramp - 11, ramp - 20, (ramp - 16) / 8
    rows[1, 1, 5], rows[2, 0, 3] = np.inf, np.nan  # rank 1's Inf and rank 0's NaN: their blocks NaN on EVERY rank, no other
    rows[4] = (2.0 ** -24 if code == F16 else 2.0 ** -133) * np.where(ramp % 2 == 0, ramp % 7, -(ramp % 5))  # subnormals of T
    rows[5, :, 9] = top, -top, top / 2  # an amax at the largest finite value
    xs = [np.concatenate([quant_ref.narrow(rows[:, r].reshape(-1), code), vnode.gen(code, 1000, rng)]) for r in range(n)]
    w = quant_ref.widen(_want(xs, code), code).reshape(n, -1)[:, :6 * 32].reshape(n, 6, 32)
    assert [[int(np.isnan(b).sum()) for b in w[r]] for r in range(n)] == [[0, 0, 32, 0, 0, 0], [0, 32, 0, 0, 0, 0], [0] * 6]
    assert np.array_equal(np.signbit(w[:, 0]), np.signbit(rows[0].reshape(n, 32))) and np.any(w[:, 4] != 0)
    comms = _comms(n, 1024)
    try:
        for inplace in (False, True):
            _run(comms, xs, code, inplace)
    finally:
        vnode.destroy(comms)


@pytest.mark.parametrize("setting", ["one stream", "graph"])
@pytest.mark.parametrize("n", [2, 3])
def test_sequence(n, setting):
    """AllGatherQuant calls of 3, 1 and 4 rounds, back to back and between the other kinds of launch; every result checked."""
    import torch

    agq = {3: 2 * 512 + 7, 1: 511, 4: 3 * 512 + 1}
    seq = [("agq", BF16, agq[3]), ("agq", F16, agq[1]), ("agq", BF16, agq[4]), ("rs", BF16, 1500, "quant-stream"),
           ("agq", F16, agq[3]), ("ar", BF16, 3000, "wide-oneshot"), ("agq", BF16, agq[1]), ("ar", F32, 500, "ll"),
           ("agq", F16, agq[4]), ("ag", F32, 5000, "oneshot"), ("agq", BF16, agq[3]), ("ar", F32, 40000, "ring"),
           ("agq", F16, agq[1])]
    comms, rng = _comms(n, 1024), np.random.default_rng(n)
    [(c.set_reduce_scatter_quant(1 << 20, 0, 1024), c.set_all_reduce_wide(0, 64 << 10, 0)) for c in comms]

    def fill(step):  # fresh inputs (fp32: sums exact in any order) and what every rank must receive
        kind, code, cnt = step[:3]
        xs = [vnode.gen(code, cnt * (n if kind == "rs" else 1), rng, "exact" if code == F32 else "uniform") for _ in range(n)]
        want = {"agq": lambda: [_want(xs, code)] * n, "rs": lambda: quant_rs_ref.reduce_scatter(xs, code),
                "ag": lambda: [np.concatenate(xs)] * n,
                "ar": lambda: [sum(xs) if code == F32 else wide_ref.all_reduce(xs, code)] * n}[kind]()
        return xs, want

    def issue(step, send, recv):
        kind, code, cnt = step[:3]
        with C.group():
            for r, c in enumerate(comms):
                if kind == "agq":
                    c.all_gather_quant(send[r], recv[r], cnt, code)
                elif kind == "ag":
                    C.all_gather(c, send[r], recv[r], cnt * 4)
                else:
                    (C.reduce_scatter if kind == "rs" else C.all_reduce)(c, send[r], recv[r], cnt, code, 0)
        assert [c.last_algo() for c in comms] == [(step[3:] or ("quant-stream",))[0]] * n, step

    try:
        data = [fill(step) for step in seq]
        send = [[vnode.to_dev(x) for x in xs] for xs, _ in data]
        recv = [[torch.zeros(w.nbytes, dtype=torch.uint8, device="cuda") for w in want] for _, want in data]
        g = torch.cuda.CUDAGraph() if setting == "graph" else None
        for k, step in enumerate(seq):  # eager, on one stream, nothing awaited in between
            issue(step, send[k], recv[k])
        if g:
            torch.cuda.synchronize()
            with torch.cuda.graph(g):
                for k, step in enumerate(seq):
                    issue(step, send[k], recv[k])
        for rep in range(4 if g else 1):  # the eager run, then three replays with the inputs rewritten
            if rep:
                data = [fill(step) for step in seq]
                for k, (xs, _) in enumerate(data):
                    for r in range(n):
                        send[k][r].copy_(vnode.to_dev(xs[r]))
                        recv[k][r].zero_()
                torch.cuda.synchronize()
                g.replay()
            torch.cuda.synchronize()
            for k, (step, (_, want)) in enumerate(zip(seq, data)):
                for r in range(n):
                    got = vnode.from_dev(recv[k][r], step[1])
                    assert np.array_equal(got, want[r]) if step[1] == F32 else quant_ref.same(got, want[r], step[1]), (rep, k, step, r)
    finally:
        vnode.destroy(comms)
