"""GPU: the LL all-to-all between launches that share its slots, its launch count
and its parity, on one set of communicators at n = 4 and n = 8; every result
is checked byte for byte.

1. eight consecutive LL v calls (host counts and Dev tables in turn) whose
   matrices move the zero pairs around and give one rank CAP-sized blocks
   while the others send 1 byte: a rank with nothing to send or receive runs
   ahead of the busy one, and only the header of every pair in every launch
   keeps it from rewriting a slot parity that is still being polled;
2. LL AllToAlls among LL, one-shot and ring AllReduces, an LL AllGather, a ring
   AllToAll above the limit, a Broadcast and a Send/Recv group;
3. the same across two streams;
4. the same in a HIP graph replayed three times with new inputs, the Dev tables
   rewritten between replays; exchange_counts is in the graph and takes LL;
5. the same with one rank per process (tests/a2a_ll_worker.py).
ll_bytes = 16 KiB (CAP = 16376), one-shot to 256 KiB, buffer_size = 1 << 16,
an 8 s watchdog.
"""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import a2av_ref as V
import a2avd_ref as D
import sr_ref as SR
from mccs_amd import comm as C
import test_gpu_all_to_all_ll as L
import test_gpu_all_to_all_sequences as A
import test_gpu_all_to_all_v as G
import test_gpu_all_to_all_v_dev as GD
import test_gpu_rooted_sequences as S
import test_gpu_send_recv as P
import vnode

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
DIRECT_DEFAULTS = True  # CFG sets every threshold

CAP = L.CAP
ONESHOT = 256 << 10
CFG = dict(buffer_size=V.BUFF, oneshot_bytes=ONESHOT, ll_bytes=L.LL_BYTES, direct_bytes=-1)
assert S.BUFF == V.BUFF  # S.call_expected plans the AllReduces with the buffer size the comms get


def _comms(n, monkeypatch):
    monkeypatch.delenv("MCCS_ALLTOALL_HOPS", raising=False)
    comms = C.init_all([0] * n, C.CommConfig(timeout_ms=S.TIMEOUT_MS, **CFG))
    for c in comms:
        assert c.all_to_all_ll_max() == CAP
        c.set_all_to_all_ll(bytes_per_peer=CAP, v_bytes_per_peer=CAP)
    return comms


# ---- 1. the parity-reuse case ---------------------------------------------------
def skewed(n, k):
    """Matrix k of the eight: rank k % n sends CAP to everyone, the others 1
    byte; the pairs with (s + 2t + k) % 3 == 0 move nothing, the busy rank's
    included, and so do the self blocks of every second matrix."""
    busy = k % n
    cnt = [[CAP if s == busy else 1 for t in range(n)] for s in range(n)]
    for s in range(n):
        for t in range(n):
            if (s != t and (s + 2 * t + k) % 3 == 0) or (s == t and k % 2):
                cnt[s][t] = 0
    return cnt


@pytest.mark.parametrize("n", [4, 8])
def test_eight_consecutive_v_calls_with_moving_zero_pairs(monkeypatch, n):
    import torch

    comms = _comms(n, monkeypatch)
    try:
        mats = [skewed(n, k) for k in range(8)]
        zeros = [{(s, t) for s in range(n) for t in range(n) if s != t and c[s][t] == 0} for c in mats]
        assert all(z and z != zeros[k - 1] for k, z in enumerate(zeros))  # some pair idle in every launch, never the same set
        items = [(GD.DStaged if k % 2 else G.VStaged)(n, cnt, V.LAYOUTS[k % len(V.LAYOUTS)], salt=k)
                 for k, cnt in enumerate(mats)]
        torch.cuda.synchronize()
        for s in items:
            s.issue(comms)
            assert comms[0].last_algo() == "ll"
        S._finish(None, comms, items, ("skewed", n))
    finally:
        vnode.destroy(comms)


# ---- 2. among the other launches ---------------------------------------------------
class XStaged:
    """exchange_counts and the Dev call it feeds, over one fixed layout that
    fits every matrix of `mats` (a2avd_ref.sequence_layout): use(k) rewrites
    row 0 of the tables, the payloads and the sentinels with stream-ordered
    copies, so a captured pair of launches moves matrix k at its next replay."""

    def __init__(self, n, mats, salt=0, call=None):
        import torch

        self.n, self.mats, self.call = n, mats, call or dict(kind="xdev", root=None, count=0, salt=salt)
        self.lay = D.sequence_layout(mats)
        self.sf = [V.frame(self.lay["send_len"][r]) for r in range(n)]
        self.rf = [V.frame(self.lay["recv_len"][r]) for r in range(n)]
        self.send = [torch.from_numpy(a).cuda() for a, _ in self.sf]
        self.recv = [torch.from_numpy(a).cuda() for a, _ in self.rf]
        self.tab = [torch.from_numpy(D.table(mats[0], self.lay, r).view(np.int64)).cuda() for r in range(n)]
        self.algos = []
        self.use(0, salt)

    def use(self, k, salt):
        import torch

        n = self.n
        self.cnt = self.mats[k]
        self.xs = [V.make_send(s, self.lay["send_len"][s], salt) for s in range(n)]
        for r in range(n):
            self.tab[r][0:n].copy_(torch.tensor(self.cnt[r], dtype=torch.int64))
            self.tab[r][2 * n:3 * n].zero_()  # the host only ever writes zeros to row 2
            a, sl = self.sf[r]
            a[sl] = self.xs[r]
            self.send[r].copy_(torch.from_numpy(a))
            self.recv[r].fill_(V.SENTINEL)

    def refill(self, salt):
        self.use((self.mats.index(self.cnt) + 1) % len(self.mats), salt)

    def issue_rank(self, comm, r, stream=None, part=None):
        if part in (None, 0):
            C.exchange_counts(comm, self.tab[r], stream=stream)
        if part in (None, 1):
            C.all_to_all_v_dev(comm, self.send[r].data_ptr() + self.sf[r][1].start,
                               self.recv[r].data_ptr() + self.rf[r][1].start, self.tab[r], stream=stream)

    def issue(self, comms, stream=None):
        self.algos = []
        for part in (0, 1):
            with C.group():
                for r in range(self.n):
                    self.issue_rank(comms[r], r, stream, part)
            self.algos.append(comms[0].last_algo())

    def check_rank(self, r, tag):
        n = self.n
        assert self.tab[r].cpu().numpy().tolist() == D.table(self.cnt, self.lay, r).astype(np.int64).tolist(), (tag, r)
        want = V.expected(self.xs, self.cnt, self.lay)[r]
        a, sl = self.rf[r]
        frame = np.full_like(a, V.SENTINEL)
        frame[sl] = want
        bad = np.flatnonzero(self.recv[r].cpu().numpy() != frame)
        assert bad.size == 0, (tag, f"rank {r}: {bad.size} wrong bytes, first at {bad[0] - sl.start} of the payload")
        assert self.send[r].cpu().numpy().tobytes() == self.sf[r][0].tobytes(), (tag, r, "send buffer written")

    def check(self, orc, comm0, tag):
        for r in range(self.n):
            self.check_rank(r, tag)


def sequence(n):
    """The calls of one sequence for n ranks, the same on every rank."""
    a2a = lambda count, salt: dict(kind="a2a", count=count, salt=salt, root=None)
    ar = lambda kind, count: dict(kind=kind, code=7, op=0, root=None, inplace=False, count=count)
    v = lambda kind, mat, layout, salt: dict(kind=kind, mat=mat, layout=layout, salt=salt, root=None, count=0)
    return [a2a(4099, 0), ar("ard", 1000), v("a2av", "plain", "misaligned", 1), ar("ar", 20000),
            v("a2avd", "zero_row", "gaps", 2), ar("ar", 100000), a2a(CAP, 3),
            dict(kind="ag", code=0, op=0, root=None, inplace=False, count=5000), a2a(CAP + 1, 4),
            v("a2av", "cap_row", "packed", 5), dict(kind="xdev", salt=6, root=None, count=0),
            dict(kind="bc", code=0, op=0, root=1 % n, inplace=False, count=30000),
            dict(kind="sr", pat="c_pairwise", salt=7, root=None, count=0), v("a2avd", "zero_col", "descending", 8),
            ar("ard", 2), a2a(8, 9), v("a2av", "zero_self", "overlap_send", 10)]


def expected_algo(call):
    kind = call["kind"]
    if kind == "a2a":
        return "ll" if call["count"] <= CAP else "ring"
    if kind in ("a2av", "a2avd", "xdev"):
        return "ll"
    if kind in ("ar", "ard", "ag"):
        nbytes = call["count"] * vnode.ESIZE[call["code"]]
        return "ll" if nbytes <= L.LL_BYTES else "oneshot" if nbytes <= ONESHOT else "ring"
    return "ring"


def stage_call(call, n, rings, m, rng):
    kind = call["kind"]
    if kind == "a2a":
        return A.A2AStaged(call, n)
    if kind in ("a2av", "a2avd"):
        cls = G.VStaged if kind == "a2av" else GD.DStaged
        return cls(n, L.matrices(n)[call["mat"]], call["layout"], call["salt"], call=call)
    if kind == "xdev":
        return XStaged(n, [skewed(n, k) for k in (1, 2, 3, 4)], call["salt"], call=call)
    if kind == "sr":
        return P.SRStaged(n, SR.patterns(n, m, rings)[call["pat"]], call["salt"], call=call)
    return S.Staged(call, n, [S.call_input(call, n, rng) for _ in range(n)])


def _stage(n, rng, comms):
    rings, m = comms[0].rings(), comms[0].all_to_all_route()["m"]
    return [stage_call(call, n, rings, m, rng) for call in sequence(n)]


def _refill(items, n, rng, rep):
    for s in items:
        if s.call["kind"] in ("a2a", "a2av", "a2avd", "xdev", "sr"):
            s.refill(100 + 10 * rep + s.call["salt"])
        else:
            s.refill([S.call_input(s.call, n, rng) for _ in range(n)])


def _issue_all(items, comms, pick_stream=lambda: None):
    took = []
    for s in items:
        s.issue(comms, pick_stream())
        took.append((s.call["kind"], comms[0].last_algo(), expected_algo(s.call)))
        if s.call["kind"] == "xdev":
            took.append(("exchange_counts", s.algos[0], "ll"))
    return took


def _check_took(took):
    assert not [t for t in took if t[1] != t[2]], took
    assert {t[2] for t in took} == {"ll", "oneshot", "ring"}
    kinds = [t[0] for t in took]
    assert kinds.count("a2a") == 4 and {"a2av", "a2avd", "xdev", "ard", "ar", "ag", "bc", "sr"} <= set(kinds)


@pytest.mark.parametrize("n", [4, 8])
def test_sequence(orc, monkeypatch, n):
    import torch

    comms = _comms(n, monkeypatch)
    try:
        items = _stage(n, np.random.default_rng(n), comms)
        torch.cuda.synchronize()
        took = _issue_all(items, comms)
        S._finish(orc, comms, items, ("ll sequence", n))
        _check_took(took)
    finally:
        vnode.destroy(comms)


@pytest.mark.parametrize("n", [4, 8])
def test_sequence_across_two_streams(orc, monkeypatch, n):
    import torch

    comms = _comms(n, monkeypatch)
    streams = [torch.cuda.current_stream(), torch.cuda.Stream()]
    try:
        rng = np.random.default_rng(10 + n)
        items = _stage(n, rng, comms)
        torch.cuda.synchronize()
        _check_took(_issue_all(items, comms, lambda: streams[int(rng.integers(0, 2))]))
        S._finish(orc, comms, items, ("ll streams", n))
    finally:
        vnode.destroy(comms)


@pytest.mark.parametrize("n", [4, 8])
def test_sequence_graph_replayed_three_times(orc, monkeypatch, n):
    """Captured once, replayed three times with new inputs: host counts ride in
    the captured arguments, every Dev launch re-reads its table (the xdev
    pair's is rewritten before each replay, its receive row by the captured
    exchange_counts), and the launch count in the control block keeps counting."""
    import torch

    comms = _comms(n, monkeypatch)
    try:
        rng = np.random.default_rng(20 + n)
        items = _stage(n, rng, comms)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            took = _issue_all(items, comms)
        _check_took(took)
        (x,) = [s for s in items if s.call["kind"] == "xdev"]
        seen = []
        for rep in range(3):
            if rep:
                _refill(items, n, rng, rep)
            seen.append(x.cnt)
            g.replay()
            S._finish(orc, comms, items, ("ll graph", n, rep))
        assert seen[0] != seen[1] != seen[2] != seen[0]
        del g
        took = _issue_all(items, comms)  # and eagerly after the replays: the launch count went on
        S._finish(orc, comms, items, ("ll after graph", n))
        _check_took(took)
    finally:
        vnode.destroy(comms)


# ---- 5. one rank per process ---------------------------------------------------------
def _free_port() -> int:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_sequence_one_rank_per_process():
    world = 2
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.join(HERE, "a2a_ll_worker.py")]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("MCCS_ONESHOT_BYTES", "MCCS_DIRECT_BYTES", "MCCS_LL_BYTES", "MCCS_ALLTOALL_HOPS", "MCCS_A2A_LL_BYTES",
              "MCCS_A2AV_LL_BYTES"):
        env.pop(k, None)
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=240, env=env, cwd=os.path.dirname(HERE))
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    lib_lines = "\n".join(l for l in (r.stdout + r.stderr).splitlines() if "mccs" in l.lower() or "hip" in l)[-3000:]
    assert r.returncode == 0 and lines, lib_lines + "\n----\n" + r.stdout[-2000:] + r.stderr[-2000:]
    res = json.loads(lines[-1])
    bad = [k for k, v in res["checks"].items() if not v]
    assert res["all_ok"] and not bad, bad
    kinds = [k.split("/")[1] for k in res["checks"]]
    assert kinds.count("a2a") == 4 and {"a2av", "a2avd", "xdev", "ard", "ar", "ag", "bc", "sr"} <= set(kinds)
    assert res["cap"] == CAP
