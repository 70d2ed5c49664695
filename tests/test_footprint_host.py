"""CPU: the guard-band helper (tests/footprint.py) tested on itself, then the
host ring and the C oracle held to it.

mccs_host_ring_allreduce and oracle_reduce_copy run on `Guarded` numpy views:
send and receive buffers at independent offsets from a 16-byte boundary that
differ between ranks, out of place and in place.  The results equal the
oracle's bit for bit, nothing outside [recv, recv + count) is written and no
send buffer changes.
"""
import ctypes

import numpy as np
import pytest

import footprint as F
import ring_sim
from footprint import PAD, Guarded
from mccs_amd import comm as C

NPDT = {2: np.int32, 6: np.float16, 7: np.float32}


# ---- 1. the helper itself -------------------------------------------------------------
def _flip(g, pos):
    a = g.lo + pos
    g.buf[a] = int(g.buf[a]) ^ 0x01  # behind the helper's back: `want` keeps the old byte


@pytest.mark.parametrize("nbytes,offset", [(1, 0), (100, 0), (100, 2), (4099, 12), (64, 255)])
def test_guarded_layout_and_clean_buffer(nbytes, offset):
    g = Guarded(nbytes, offset)
    assert g.buf.data_ptr() % 256 == 0 and g.ptr == g.buf.data_ptr() + PAD + offset
    assert g.ptr % 16 == offset % 16 and g.ptr % 256 == offset
    assert g.buf.numel() == PAD + offset + nbytes + PAD
    assert g.check().size == 0 and g.unchanged() and not g.pads_message()
    # writing the payload, every byte of it, is no finding
    g.write(np.arange(nbytes, dtype=np.uint8))
    g.payload.copy_(~g.payload)
    assert g.check().size == 0 and not g.unchanged()
    assert g.changed().tolist() == list(range(nbytes))


def test_guarded_pads_are_not_periodic_and_differ_per_buffer():
    a, b = Guarded(64, 0, seed=1), Guarded(64, 0, seed=2)
    assert not np.array_equal(a.want[:PAD], b.want[:PAD])
    pad = a.want[:PAD]
    assert len(set(pad.tolist())) == 256
    for shift in (1, 2, 4, 8, 16, 64, 256, 1024, 4096):  # a shifted copy of the pad is noticed
        assert np.count_nonzero(pad[shift:] == pad[:-shift]) < (PAD - shift) // 16


@pytest.mark.parametrize("offset", [0, 2, 12])
@pytest.mark.parametrize("where", ["-1", "nbytes", "far left", "far right"])
def test_guarded_reports_one_flipped_byte(where, offset):
    nbytes = 1000
    pos = {"-1": -1, "nbytes": nbytes, "far left": -(PAD + offset), "far right": nbytes + PAD - 1}[where]
    g = Guarded(nbytes, offset)
    g.write(np.zeros(nbytes, np.uint8))
    _flip(g, pos)
    assert g.check().tolist() == [pos]
    assert not g.unchanged() and g.changed().tolist() == [pos]
    assert f"[{pos}]" in g.pads_message() and "got" in g.pads_message() and "want" in g.pads_message()
    with pytest.raises(AssertionError, match="wrote outside"):
        g.assert_pads()


def test_guarded_reports_a_block_of_zeros_past_the_payload():
    """What a whole 16-byte pack stored over a typed tail leaves behind."""
    nbytes = 1000
    g = Guarded(nbytes, 0, seed=3)
    g.buf[g.lo + nbytes:g.lo + nbytes + 16] = 0
    want = [nbytes + i for i in range(16) if g.want[g.lo + nbytes + i] != 0]
    assert len(want) >= 15  # a random byte is 0 once in 256; this seed's 16 are fixed
    assert g.check().tolist() == want


def test_prefill_not_differs_in_every_byte():
    exp = np.random.default_rng(0).integers(0, 256, 333, dtype=np.uint8)
    g = Guarded(333, 4)
    g.prefill_not(exp)
    assert np.all(g.read() ^ exp == 0xFF)
    assert F.diff_message(g.read(), exp).startswith("333 of 333")
    assert g.check().size == 0 and g.unchanged()


# ---- 2. the host ring ---------------------------------------------------------------
def _gen(code, count, rng):
    if code == 2:
        return rng.integers(-1000, 1000, count).astype(np.int32)
    return (rng.random(count, dtype=np.float32) * 2 - 1).astype(NPDT[code])


def _offsets(es):
    return sorted({0, es, 8, 16 - es})


BUFF = 1 << 16
# 40001 walks several loops of this buffer at n = 2 only; 100001 walks at
# least two, the last one partial, at every (n, channels, type) below
COUNTS = [1, 7, 4097, 40001, 100001]
SHAPES = {2: (1, 96), 3: (2, 288), 5: (1, 160)}  # n: (channels, reference threads)


def _loops(n, count, nch, nthr, es):
    prog = list(ring_sim.rank_program(0, n, count, nch, 0, nthr, BUFF, es))
    return len(prog) // (2 * n - 1)


@pytest.mark.parametrize("code", [6, 7, 2])
@pytest.mark.parametrize("n", [2, 3, 5])
def test_host_ring_footprint(orc, n, code):
    es = np.dtype(NPDT[code]).itemsize
    offs = _offsets(es)
    nz = [o for o in offs if o]
    nch, nthr = SHAPES[n]
    # the shape under test walks several loops, the last one partial: a slice's
    # base moves through the user buffers
    loop = nch * n * ring_sim.chunk_size_elems(BUFF, es)
    assert _loops(n, COUNTS[-1], nch, nthr, es) == -(-COUNTS[-1] // loop) >= 2 and COUNTS[-1] % loop != 0
    if n == 2:
        assert _loops(n, 40001, nch, nthr, es) >= 2 and 40001 % loop != 0
    rng = np.random.default_rng(100 * n + code)
    bad = {}
    for count in COUNTS:
        xs = [_gen(code, count, rng) for _ in range(n)]
        exp = orc.ring_allreduce(code, 0, xs, nchannels=nch, nthreads=nthr, buff_size=BUFF)
        # (a, b): rank r sends from offs[(r + a) % k] and receives at
        # offs[(2 r + b) % k]; None: in place at a nonzero offset per rank
        for assign in [(0, 1), (1, 3), (2, 0), (3, 2), None]:
            if assign is None:
                send = [Guarded(count * es, nz[r % len(nz)]) for r in range(n)]
                recv = send
            else:
                a, b = assign
                send = [Guarded(count * es, offs[(r + a) % len(offs)]) for r in range(n)]
                recv = [Guarded(count * es, offs[(2 * r + b) % len(offs)]) for r in range(n)]
                assert len({g.offset for g in send}) > 1 and len({g.offset for g in recv}) > 1
            for r in range(n):
                send[r].write(xs[r])
                if assign is not None:
                    recv[r].prefill_not(exp)
            C.host_ring_allreduce([g.ptr for g in send], [g.ptr for g in recv], count, code, 0, channels=nch,
                                  nthreads=nthr, buffer_size=BUFF)
            for r in range(n):
                msg = (F.diff_message(recv[r].read(), exp) or recv[r].pads_message()
                       or (send[r].source_message() if assign is not None else ""))
                if msg:
                    bad[(count, assign, r)] = msg
    assert not bad, F.brief(bad)


# ---- 3. the checker's own reduce ----------------------------------------------------
@pytest.mark.parametrize("code", [6, 7, 2])
@pytest.mark.parametrize("nsrcs,ndsts", [(2, 1), (3, 2)])
def test_oracle_reduce_copy_footprint(orc, code, nsrcs, ndsts):
    es = np.dtype(NPDT[code]).itemsize
    offs = _offsets(es)
    rng = np.random.default_rng(code + nsrcs)
    vp = ctypes.c_void_p
    bad = {}
    for count in COUNTS:
        xs = [_gen(code, count, rng) for _ in range(nsrcs)]
        exp = orc.reduce_copy(code, 0, xs, ndsts)
        if nsrcs == 2:  # one correctly rounded add per element: numpy's own
            assert np.array_equal(exp[0].view(np.uint8), (xs[0] + xs[1]).astype(NPDT[code]).view(np.uint8))
        for shift in range(len(offs)):
            srcs = [Guarded(count * es, offs[(i + shift) % len(offs)]) for i in range(nsrcs)]
            dsts = [Guarded(count * es, offs[(2 * i + shift + 1) % len(offs)]) for i in range(ndsts)]
            for g, x in zip(srcs, xs):
                g.write(x)
            for g, e in zip(dsts, exp):
                g.prefill_not(e)
            rc = orc.lib().oracle_reduce_copy(code, 0, (vp * nsrcs)(*[g.ptr for g in srcs]), nsrcs,
                                              (vp * ndsts)(*[g.ptr for g in dsts]), ndsts, count)
            assert rc == 0
            for i, g in enumerate(dsts):
                msg = F.diff_message(g.view(NPDT[code]), exp[i]) or g.pads_message()
                if msg:
                    bad[(count, shift, "dst", i)] = msg
            for i, g in enumerate(srcs):
                if g.source_message():
                    bad[(count, shift, "src", i)] = g.source_message()
    assert not bad, F.brief(bad)
