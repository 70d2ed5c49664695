"""Test helper: buffers with guard bands, to see every byte a kernel writes.

The other suites read back exactly `count` elements of an output and nothing
else, from buffers whose allocator rounds them up, so a store that lands next
to the output goes unseen.  A `Guarded` buffer is

    | left pad (PAD + offset bytes) | payload (nbytes) | right pad (PAD bytes) |

with the start of the left pad on a 256-byte boundary, so the payload's
address modulo 16 (and its phase within a 256-byte line) is exactly the
`offset` the test asked for.  PAD is 16 KiB: two of the largest contiguous
stores one wave issues in this library (a wave unit is 64 lanes x 16 B x U
with U <= 8, 8 KiB).  The pads hold the output of a generator seeded per
buffer: not constant and without a short period, so zeros, a copy of real data
and a shifted copy of the pad itself all show.

Works on torch uint8 buffers on any device ("cpu" here, "cuda" on the GPU);
on the CPU `view()` hands out a numpy array over the payload's own memory for
the host ring and the C oracle.  Not a conftest: tests import it by name.
"""
from __future__ import annotations

import itertools

import numpy as np

PAD = 16 << 10
ALIGN = 256
_seeds = itertools.count(1)


class Guarded:
    """nbytes of payload `offset` bytes past a 256-byte boundary, PAD guard
    bytes on both sides."""

    def __init__(self, nbytes: int, offset: int = 0, device: str = "cpu", seed: int | None = None):
        import torch

        assert nbytes >= 0 and 0 <= offset < ALIGN
        self.nbytes, self.offset, self.device = int(nbytes), int(offset), device
        self.lo = PAD + self.offset  # payload's position in the buffer
        total = self.lo + self.nbytes + PAD
        raw = torch.empty(total + ALIGN, dtype=torch.uint8, device=device)
        skip = -raw.data_ptr() % ALIGN
        self.buf = raw[skip:skip + total]
        assert self.buf.data_ptr() % ALIGN == 0 and self.buf.numel() == total
        assert (self.buf.data_ptr() + self.lo) % 16 == self.offset % 16
        rng = np.random.default_rng(next(_seeds) if seed is None else seed)
        # what the buffer must hold wherever nobody is allowed to write: the
        # pads for ever, the payload until write() / prefill_not() replace it
        self.want = rng.integers(0, 256, total, dtype=np.uint8)
        self.buf.copy_(torch.from_numpy(self.want))

    # -- addresses and views ----------------------------------------------------
    @property
    def ptr(self) -> int:
        return self.buf.data_ptr() + self.lo

    @property
    def payload(self):
        return self.buf[self.lo:self.lo + self.nbytes]

    def view(self, npdt) -> np.ndarray:
        """numpy array over the payload's own memory (CPU buffers only)."""
        assert self.device == "cpu"
        return self.payload.numpy().view(npdt)

    # -- filling ------------------------------------------------------------------
    def poke(self, pos: int, data) -> None:
        """Sets bytes at `pos` relative to the payload (pads included) and
        takes them as this buffer's expected content from now on."""
        import torch

        b = np.ascontiguousarray(data).view(np.uint8).reshape(-1)
        a = self.lo + pos
        assert 0 <= a and a + b.size <= self.want.size
        self.want[a:a + b.size] = b
        self.buf[a:a + b.size].copy_(torch.from_numpy(b.copy()))

    def write(self, data) -> None:
        """The payload := data (a source's input)."""
        b = np.ascontiguousarray(data).view(np.uint8).reshape(-1)
        assert b.size == self.nbytes
        self.poke(0, b)

    def prefill_not(self, expected) -> None:
        """A destination's payload := bitwise NOT of the expected bytes: an
        element the kernel never wrote then differs from the expectation in
        every byte."""
        b = np.ascontiguousarray(expected).view(np.uint8).reshape(-1)
        assert b.size == self.nbytes
        self.poke(0, ~b)

    # -- reading and checking -------------------------------------------------------
    def host(self) -> np.ndarray:
        return self.buf.cpu().numpy()

    def read(self, npdt=np.uint8) -> np.ndarray:
        return self.host()[self.lo:self.lo + self.nbytes].copy().view(npdt)

    def _describe(self, got: np.ndarray, pos: np.ndarray) -> str:
        first = pos[:6]
        return (f"{pos.size} bytes at payload offsets {first.tolist()} (payload is [0, {self.nbytes})): got "
                f"{[hex(v) for v in got[first + self.lo].tolist()]} want "
                f"{[hex(v) for v in self.want[first + self.lo].tolist()]}")

    def check(self, got: np.ndarray | None = None) -> np.ndarray:
        """Positions of modified pad bytes relative to the payload: negative
        before it, >= nbytes after it; empty when the pads are intact."""
        got = self.host() if got is None else got
        bad = np.flatnonzero(got != self.want) - self.lo
        return bad[(bad < 0) | (bad >= self.nbytes)]

    def changed(self, got: np.ndarray | None = None) -> np.ndarray:
        """Positions, pads and payload, that differ from the content last set."""
        got = self.host() if got is None else got
        return np.flatnonzero(got != self.want) - self.lo

    def unchanged(self) -> bool:
        """A source after an out-of-place call: the whole buffer still holds
        what was put there."""
        return self.changed().size == 0

    def pads_message(self) -> str:
        """'' when the pads are intact, else the first offsets, got and want."""
        got = self.host()
        bad = self.check(got)
        return "" if bad.size == 0 else "wrote outside: " + self._describe(got, bad)

    def source_message(self) -> str:
        got = self.host()
        bad = self.changed(got)
        return "" if bad.size == 0 else "source modified: " + self._describe(got, bad)

    def assert_pads(self) -> None:
        msg = self.pads_message()
        assert not msg, msg

    def assert_unchanged(self) -> None:
        msg = self.source_message()
        assert not msg, msg


def brief(bad: dict) -> str:
    """A sweep's failures for an assert message: how many, and the first few."""
    return f"{len(bad)} cases failed, the first: {dict(list(bad.items())[:4])}"


def diff_message(got: np.ndarray, exp: np.ndarray) -> str:
    """'' when got equals exp bit for bit, else a short description."""
    g, e = got.view(np.uint8).reshape(-1), np.ascontiguousarray(exp).view(np.uint8).reshape(-1)
    if g.size != e.size:
        return f"{g.size} bytes, expected {e.size}"
    bad = np.flatnonzero(g != e)
    if bad.size == 0:
        return ""
    return (f"{bad.size} of {e.size} bytes differ, first at {bad[:6].tolist()}: got "
            f"{[hex(v) for v in g[bad[:6]].tolist()]} want {[hex(v) for v in e[bad[:6]].tolist()]}")
