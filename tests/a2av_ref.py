"""Expected bytes and models for the AllToAllv tests (numpy only, no library code).

expected():   recv_r[rdispl_r[s] : +cnt[s][r]] = send_s[sdispl_s[r] : +cnt[s][r]],
              every other byte of the frame 0xA5.
call_list():  the call list of one work element, written from the issue's
              text: for loop i = 0 .. max(Ls, Lr) - 1: send(i) if i < Ls,
              recv(i) if i < Lr, with L = ceil(count / loopSize), 0 for 0.
elements():   per (rank, channel) the (S, R) pair a one-hop ring set gives:
              S = cnt[r][next_c(r)], R = cnt[prev_c(r)][r].
channel_cut(), slice_cut(): how a pair's block is cut over its channels and a
              call into slices, written from the description of the cut;
              boundary_values() and boundary_matrices() put counts on its
              edges, cut_situations() names what a set of counts reaches.
The count matrices are built for buffer_size = 1 << 16: 8 KiB steps, 32 KiB
chunks, so one loop of a pair is C = 32768 * m bytes.
"""
from __future__ import annotations

import numpy as np

SENTINEL = 0xA5
BUFF = 1 << 16
CHUNK = BUFF // 8 * 4  # 32 KiB
LAYOUTS = ("packed", "descending", "gaps", "misaligned", "overlap_send")


def loop_bytes(m: int) -> int:
    return CHUNK * m


def values(m: int) -> list[int]:
    C = loop_bytes(m)
    return [0, 1, 15, 4099, C, C + 1, 2 * C + 999, 3 * C]


def loops(count: int, m: int) -> int:
    return -(-count // loop_bytes(m)) if count > 0 else 0


def call_list(S: int, R: int, m: int) -> list[tuple[str, int]]:
    Ls, Lr = loops(S, m), loops(R, m)
    out = []
    for i in range(max(Ls, Lr)):
        if i < Ls:
            out.append(("send", i))
        if i < Lr:
            out.append(("recv", i))
    return out


def ring_next_prev(rings, n):
    nxt = [{ring[i]: ring[(i + 1) % n] for i in range(n)} for ring in rings]
    prv = [{b: a for a, b in d.items()} for d in nxt]
    return nxt, prv


def elements(cnt, rings) -> dict:
    """(rank, channel) -> (S, R) on a one-hop ring set."""
    n = len(cnt)
    nxt, prv = ring_next_prev(rings, n)
    return {(r, c): (cnt[r][nxt[c][r]], cnt[prv[c][r]][r]) for r in range(n) for c in range(len(rings))}


def loop_cases(cnt, rings, m) -> set:
    return {(loops(S, m), loops(R, m)) for S, R in elements(cnt, rings).values()}


def steps_per_connection(cnt, rings, m, spc_sps: int = 4) -> dict:
    """FIFO steps each connection (channel, sender) advances: its own pair's loops alone."""
    n = len(cnt)
    nxt, _ = ring_next_prev(rings, n)
    return {(c, s): loops(cnt[s][nxt[c][s]], m) * spc_sps for s in range(n) for c in range(len(rings))}


# ---- count matrices -------------------------------------------------------
def cyclic(n: int, m: int, start: int = 0, stride: int = 1, self_start: int = 0) -> list[list[int]]:
    """Off-diagonal counts drawn cyclically from values(m), the diagonal from its small values."""
    v = values(m)
    small = [4099, 0, 15, 1, loop_bytes(m) + 1]
    cnt, k = [[0] * n for _ in range(n)], start
    for s in range(n):
        for t in range(n):
            if s == t:
                cnt[s][t] = small[(self_start + s) % len(small)]
            else:
                cnt[s][t] = v[k % len(v)]
                k += stride
    return cnt


def seeded(n: int, m: int, rings, S: int, R: int, start: int) -> list[list[int]]:
    """A cyclic matrix in which channel 0 of rank 0 sends S and receives R."""
    cnt = cyclic(n, m, start)
    nxt, prv = ring_next_prev(rings, n)
    t, p = nxt[0][0], prv[0][0]
    cnt[0][t] = S
    cnt[p][0] = R
    if t == p:  # n = 2: the pair's two directions
        cnt[0][t], cnt[t][0] = S, R
    return cnt


def matrices(n: int, m: int, rings) -> dict:
    """The named count matrices of one test at n ranks."""
    C = loop_bytes(m)
    out = {}
    if n == 1:
        return {"self": [[4099]], "self0": [[0]]}
    for name, (S, R) in {"s3r0": (2 * C + 999, 0), "s0r3": (0, 2 * C + 999), "s1r3": (C, 3 * C),
                         "s1r1": (1, 15)}.items():
        out[name] = seeded(n, m, rings, S, R, start=len(out))
    out["cyc5"] = cyclic(n, m, 5, stride=3, self_start=1)
    zr = cyclic(n, m, 2)
    zr[n - 1] = [0] * n
    zr[n - 1][n - 1] = 0
    out["zero_row"] = zr
    zc = cyclic(n, m, 3)
    for s in range(n):
        zc[s][0] = 0
    out["zero_col"] = zc
    zs = cyclic(n, m, 4)
    for s in range(n):
        zs[s][s] = 0
    out["zero_self"] = zs
    out["all_zero"] = [[0] * n for _ in range(n)]
    out["uniform"] = [[4099] * n for _ in range(n)]
    return out


# ---- layouts ---------------------------------------------------------------
def layout(cnt, kind: str) -> dict:
    """Displacements per rank: sdispls[r][t], rdispls[r][s], and each buffer's payload length."""
    n = len(cnt)
    sd, rd, slen, rlen = [], [], [], []
    for r in range(n):
        sc = [cnt[r][t] for t in range(n)]
        rc = [cnt[s][r] for s in range(n)]

        def place(c, gap, order, base):
            d, off = [0] * n, base
            for i in order:
                d[i] = off
                off += c[i] + (gap(i) if gap else 0)
            return d, off

        fwd, rev = list(range(n)), list(range(n - 1, -1, -1))
        if kind == "packed":
            s, sl = place(sc, None, fwd, 0)
            d, dl = place(rc, None, fwd, 0)
        elif kind == "descending":
            s, sl = place(sc, None, rev, 0)
            d, dl = place(rc, None, rev, 0)
        elif kind == "gaps":
            s, sl = place(sc, lambda i: 1 + (5 * i + r) % 13, fwd, 3)
            d, dl = place(rc, lambda i: 1 + (7 * i + 2 * r) % 29, fwd, 5)
        elif kind == "misaligned":
            s, sl = place(sc, None, fwd, 1 + (3 * r + 1) % 15)
            d, dl = place(rc, lambda i: 1 + (i + r) % 15, fwd, 1 + (5 * r + 6) % 15)
        elif kind == "overlap_send":  # every peer reads from the start: the same bytes go to several peers
            s, sl = [0] * n, max(sc + [0])
            d, dl = place(rc, None, fwd, 0)
        else:
            raise ValueError(kind)
        sd.append(s)
        rd.append(d)
        slen.append(sl)
        rlen.append(dl)
    return {"sdispls": sd, "rdispls": rd, "send_len": slen, "recv_len": rlen}


def make_send(s: int, nbytes: int, salt: int = 0) -> np.ndarray:
    i = np.arange(nbytes, dtype=np.int64)
    return ((31 * s + 7 * (i // 97) + i + salt) % 251).astype(np.uint8)


def expected(sends, cnt, lay) -> list[np.ndarray]:
    """The receive payloads (recv_len bytes each), 0xA5 where nothing lands."""
    n = len(cnt)
    out = []
    for r in range(n):
        d = np.full(lay["recv_len"][r], SENTINEL, np.uint8)
        for s in range(n):
            c = cnt[s][r]
            a, b = lay["rdispls"][r][s], lay["sdispls"][s][r]
            d[a:a + c] = sends[s][b:b + c]
        out.append(d)
    return out


def wrong_candidates(sends, cnt, lay) -> dict:
    """Results a broken implementation would give; a case that none of them
    tells from expected() checks nothing."""
    n = len(cnt)
    B = max(max(row) for row in cnt)

    def build(count, sdisp, rdisp):
        out = []
        for r in range(n):
            d = np.full(lay["recv_len"][r], SENTINEL, np.uint8)
            for s in range(n):
                c, a, b = count(s, r), rdisp(r, s), sdisp(s, r)
                c = max(0, min(c, d.size - a, sends[s].size - b))
                d[a:a + c] = sends[s][b:b + c]
            out.append(d)
        return out

    sdv, rdv = lay["sdispls"], lay["rdispls"]
    return {
        "uniform_transpose": build(lambda s, r: B, lambda s, r: r * B, lambda r, s: s * B),
        "swapped_counts": build(lambda s, r: cnt[r][s], lambda s, r: sdv[s][r], lambda r, s: rdv[r][s]),
        "displs_ignored": build(lambda s, r: cnt[s][r], lambda s, r: sum(cnt[s][:r]),
                                lambda r, s: sum(cnt[k][r] for k in range(s))),
    }


def frame(payload_len: int, lead: int = 32, tail: int = 64):
    a = np.full(lead + payload_len + tail, SENTINEL, np.uint8)
    return a, slice(lead, lead + payload_len)


# ---- the byte cut of one pair's block, and counts on its edges ----------------
# Written from the description of the cut, not from the library: a pair's block
# of `count` bytes goes over the pair's m channels in loops of CHUNK * m bytes.
GRAN = 4096  # the granule realChunkSize is rounded up to (544 threads)
STEP = BUFF // 8  # one FIFO step
CHUNK_STEPS = 4  # steps per chunk; one slice holds sps of them, a call spc = CHUNK_STEPS / sps slices
SLICINGS = {"default": 1, "slice2": 2}  # name -> spc: one 4-step slice per call; MCCS_SLICE_STEPS=2: two 2-step slices
SELF_VALUES = (0, 1, 17, 513, 4097)


def channel_cut(count: int, m: int, gran: int = GRAN, chunk: int = CHUNK) -> list[tuple[int, int, int, int]]:
    """(gridOffset, rcs, offset, nelem) per loop and part: in the loop at g,
    rcs = round_up(min(chunk, ceil((count - g) / m)), gran); part p starts at
    g + p * rcs and gets max(0, min(rcs, count - start)) bytes."""
    rows, g = [], 0
    while g < count:
        rcs = min(chunk, -(-(count - g) // m))
        rcs = -(-rcs // gran) * gran
        for p in range(m):
            start = g + p * rcs
            rows.append((g, rcs, start, max(0, min(rcs, count - start))))
        g += chunk * m
    return rows


def slice_size(nelem: int, spc: int) -> int:
    """sliceSize of a call of nelem bytes cut into spc slices of sps = CHUNK_STEPS / spc steps."""
    sps = CHUNK_STEPS // spc
    return max(-(-nelem // (16 * spc)) * 16, STEP * sps // 32)


def slice_cut(nelem: int, spc: int) -> list[int]:
    """The bytes of each of a call's spc slices."""
    size = slice_size(nelem, spc)
    return [max(0, min(size, nelem - s * size)) for s in range(spc)]


def boundary_values(m: int) -> list[int]:
    """Counts on the edges of the cut: the 16-byte pack, the slice floors, the
    granule, the channel edges inside one loop, the loop edges."""
    G, C = GRAN, loop_bytes(m)
    vals = [1, 16, 17, 511, 512, 513, 1024, 1025, G - 1, G, G + 1, (m - 1) * G, (m - 1) * G + 1, m * G - 1, m * G,
            m * G + 1, C - G, C - G + 1, C - 1, C, C + 1, C + m * G, 2 * C - 1, 2 * C, 3 * C - G + 1]
    return sorted({v for v in vals if v > 0})


def boundary_matrices(n: int, m: int, rings) -> list[list[list[int]]]:
    """Count matrices whose off-diagonal entries walk through 0 and
    boundary_values(m): first in ascending order (neighbouring values meet in
    one element: mostly equal loop counts), then with stride 11 through the
    same list (far values meet, in both orders).  On a one-hop ring set every
    off-diagonal entry is the S of one rank's elements and the R of another's,
    so the first pass alone puts every value on both sides.  The diagonal
    cycles through SELF_VALUES."""
    vals = [0] + boundary_values(m)
    stride = 11
    while np.gcd(stride, len(vals)) != 1:
        stride += 1
    stream = vals + [vals[(3 + stride * k) % len(vals)] for k in range(len(vals))]
    slots = n * (n - 1)
    nmat = min(20, max(2, -(-(len(vals) + 14) // slots)))
    out, k = [], 0
    for i in range(nmat):
        cnt = [[0] * n for _ in range(n)]
        for s in range(n):
            for t in range(n):
                if s == t:
                    cnt[s][t] = SELF_VALUES[(i + s) % len(SELF_VALUES)]
                else:
                    cnt[s][t] = stream[k % len(stream)]
                    k += 1
        out.append(cnt)
    return out


def cut_situations(cnts, m: int) -> set:
    """What the cut of the counts `cnts` (each the S or the R of some element)
    reaches, as a set of names.  "last": the last channel of a loop whose start
    is not past the end of the block (it gets count - start >= 0 bytes);
    "past": a channel whose start is past the end; "slice2 second": the second
    slice of a call under MCCS_SLICE_STEPS=2; "default slice": the one slice
    of a call under the default slicing."""
    out = set()
    for count in cnts:
        rows = channel_cut(count, m)
        for i in range(0, len(rows), m):
            loop = rows[i:i + m]
            live = [row for row in loop if row[2] <= count]
            if len(live) < m:
                out.add("past")
            last = live[-1][3]
            for name, v in (("0", 0), ("1", 1), ("G-1", GRAN - 1), ("G", GRAN), ("chunk", CHUNK)):
                if last == v:
                    out.add("last " + name)
            if loop[0][0] > 0 and sum(row[3] for row in loop) == 1:
                out.add("second loop 1")
            for _, _, _, nelem in loop:
                a, b = slice_cut(nelem, 2)
                if a == slice_size(nelem, 2) and b == 0:  # the first slice exactly full
                    out.add("slice2 second 0")
                if b == 1:
                    out.add("slice2 second 1")
                if b > 0 and b == slice_size(nelem, 2):
                    out.add("slice2 second full")
                (a,) = slice_cut(nelem, 1)  # the default slicing has no second slice: its one slice on its floor
                floor = STEP * CHUNK_STEPS // 32
                for name, v in (("1", 1), ("floor", floor), ("floor + 1", floor + 1)):
                    if a == v:
                        out.add("default slice " + name)
    return out


SITUATIONS = {"last 0", "last 1", "last G-1", "last G", "last chunk", "past", "second loop 1", "slice2 second 0",
              "slice2 second 1", "slice2 second full", "default slice 1", "default slice floor",
              "default slice floor + 1"}
