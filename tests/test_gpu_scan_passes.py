"""GPU: the second-level scans past one pass. Three kernels turn per-workgroup results into global
positions with a scan that a single workgroup runs: k_q_carry (csrc/edc_quorum.hip: what a commit
open at a tile's start has already counted), k_sc_scan (csrc/edc_sigcache.hip: the checked counts,
the checked hole bytes, the masked lookup's misses and hits) and k_tmpl_scan (csrc/edc_tmpl.hip: the
messages' offsets in the arena). One pass covers 1024 workgroups of 256 items, P = 262,144 items;
beyond that the first two loop with a carry and the third gives every thread several elements.
Every case here has n just above P or 2 P.

The large count lives in the integer inputs only (flags, powers, offsets, hole lengths), built with
numpy and handed to the library as flat buffers; at most a few hundred votes are signed, hashed or
verified. Expected values: the pure-Python model of tests/golden/gen_quorum.py for the selection,
the tallies and the verdicts; the C oracle's code for every checked vote; SHA-512 of hashlib for
k; edc_batch_verify_prehashed_device on the list this test gathers itself for check8; numpy for the
expanded arena. Every comparison is exact."""
import ctypes
import hashlib
import os
import random
import sys

import numpy as np
import pytest

from conftest import ROOT
from test_gpu_commits import L_ORDER
from test_gpu_quorum import MAXP, _offsets, _same, _thresholds, g, qsets  # noqa: F401 (g, qsets: fixtures)

pytestmark = pytest.mark.gpu

W = 256                      # QR_TILE = SC_BLOCK = TMPL_BLOCK
P = 1024 * W                 # items one pass of each scan covers
EDC_ERR_ARG = -2
U32P, U64P = ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint64)
KEYS = ("code", "commit_verdicts", "item_verdicts", "tally", "n_bad_commits", "n_checked", "check8")


@pytest.fixture(scope="module")
def oracle_c():
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import oracle_c as oc
    return oc


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    t = torch.from_numpy(a if a.flags.writeable else a.copy()).to("cuda:0")
    torch.cuda.synchronize()
    return t


def _dev_power(power):
    return _dev(np.ascontiguousarray(power, dtype=np.uint64).view(np.int64))


def _dev_u32(a):
    return _dev(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32))


def _challenge(vk, sig, msg):
    """k of Item::from: SHA-512(R || A || M) mod l, 32 bytes little endian."""
    return (int.from_bytes(hashlib.sha512(sig[:32] + vk + msg).digest(), "little") % L_ORDER).to_bytes(32, "little")


def _rows(n, width, seed, rows):
    """n rows of `width` noise bytes with the given {index: bytes} rows laid over them."""
    a = np.random.default_rng(seed).integers(0, 256, size=(n, width), dtype=np.uint8)
    for i, b in rows.items():
        a[i] = np.frombuffer(b, dtype=np.uint8)
    return a


def _check8_of(eng, vks, sigs, ks, seed):
    """edc_batch_verify_prehashed_device on a list this test gathered: (code, check8)."""
    d = [_dev(np.frombuffer(b"".join(x) or b"\0", dtype=np.uint8)) for x in (vks, sigs, ks)]
    c8 = ctypes.create_string_buffer(32)
    rc = eng.lib.edc_batch_verify_prehashed_device(eng.ctx, len(vks), d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), seed, 0,
                                                   None, c8)
    assert rc in (0, 1), eng.lib.edc_last_error(eng.ctx)
    return rc, c8.raw


# ---------------------------------------------------------------- 1: the selection (k_q_carry, k_sc_scan)
class Votes:
    """A commit set's integer inputs, as numpy arrays for the library and as lists for the model."""

    def __init__(self, off, power, flag):
        self.off = [int(x) for x in off]
        self.n, self.nc = self.off[-1], len(self.off) - 1
        self.power, self.flag = np.ascontiguousarray(power, dtype=np.uint64), np.ascontiguousarray(flag, dtype=np.uint8)
        assert len(self.power) == len(self.flag) == self.n
        self.off_np = np.array(self.off, dtype=np.uint32)
        self.lpower, self.lflag, self.bflag = self.power.tolist(), self.flag.tolist(), self.flag.tobytes()

    @classmethod
    def random(cls, seed, off, pmax=1000):
        """Powers 0..pmax; a tenth of the votes absent and a tenth nil, as _random_votes of test_gpu_quorum.py."""
        rng = np.random.default_rng(seed)
        n = int(off[-1])
        return cls(off, rng.integers(0, pmax + 1, size=n, dtype=np.uint64),
                   np.array([0, 2, 1, 1, 1, 1, 1, 1, 1, 1], dtype=np.uint8)[rng.integers(0, 10, size=n)])

    def plan(self, engine, thr, light):
        """edc_quorum_plan on the flat buffers: (checked[n] uint8, [planned per commit], n_checked)."""
        th = np.array([int(t) for t in thr], dtype=np.uint64)
        assert len(th) == self.nc
        checked, planned = np.full(max(self.n, 1), 7, dtype=np.uint8), np.full(max(self.nc, 1), 7, dtype=np.uint64)
        cnt = ctypes.c_size_t(7)
        rc = engine.lib.edc_quorum_plan(engine.ctx, self.nc, self.off_np.ctypes.data_as(U32P), self.power.ctypes.data_as(U64P),
                                        self.bflag, th.ctypes.data_as(U64P), int(bool(light)), checked.ctypes.data,
                                        planned.ctypes.data, ctypes.byref(cnt))
        assert rc == 0, (rc, engine.lib.edc_last_error(engine.ctx))
        return checked[:self.n], planned[:self.nc].tolist(), cnt.value

    def agrees(self, engine, g, thr):
        """Both modes against gen_quorum.select, as _plan_agrees of test_gpu_quorum.py."""
        for mode in (g.FULL, g.LIGHT):
            checked, planned = g.select(self.off, self.lpower, self.lflag, thr, mode)
            got = self.plan(engine, thr, mode == g.LIGHT)
            want = np.array(checked, dtype=np.uint8)
            diff = np.flatnonzero(got[0] != want)
            assert diff.size == 0, (mode, diff.size, diff[:10].tolist())
            bad = [c for c in range(self.nc) if got[1][c] != planned[c]]
            assert not bad, (mode, bad[:10], [(got[1][c], planned[c]) for c in bad[:3]])
            assert got[2] == sum(checked), mode


N1 = P + 257


@pytest.fixture(scope="module")
def one_equal():
    return Votes([0, N1], np.full(N1, 3, dtype=np.uint64), np.ones(N1, dtype=np.uint8))


@pytest.mark.parametrize("last", [P - 2, P - 1, P, P + 1, P + 200, None], ids=lambda x: "never" if x is None else str(x - P))
def test_one_commit_quorum_around_the_pass_edge(engine, g, one_equal, last):
    """One commit of P + 257 items of power 3: the threshold 3 * last makes item `last` the last one
    that arrives before the quorum; the total and 2^64 - 1 are never passed."""
    V = one_equal
    if last is None:
        for thr in ([3 * N1], [2**64 - 1]):
            checked, planned, m = V.plan(engine, thr, True)
            assert checked.all() and planned == [3 * N1] and m == N1
            V.agrees(engine, g, thr)
        return
    checked, planned, m = V.plan(engine, [3 * last], True)
    assert checked[:last + 1].all() and not checked[last + 1:].any() and planned == [3 * (last + 1)] and m == last + 1
    V.agrees(engine, g, [3 * last])


def test_one_commit_of_random_votes(engine, g):
    """The threshold is the counted power of the items before P exactly: item P is the last one checked
    unless its neighbours count nothing."""
    V = Votes.random(11, [0, N1])
    before = int(V.power[:P][V.flag[:P] == 1].sum())
    for thr in (before, before - 1, int(V.power[V.flag == 1].sum())):
        V.agrees(engine, g, [thr])


LAYOUTS = {
    # a long commit first, so that what the first pass hands over is not zero
    "start_at_P": [0, P - 700, P, P + 100, N1],
    "start_at_P-1": [0, P - 701, P - 1, P + 100, N1],
    "start_at_P+1": [0, P - 699, P + 1, P + 100, N1],
    "mid_tiles": [0, 1000, P - W // 2, P + W // 2, N1],          # the middle of tile 1023 and of tile 1024
    "empty_at_P": [0, P - 700, P, P, P, P + 3, N1],
    "empty_inside": [0, 500, 500, N1],                           # and one commit from tile 1 to the end
}


@pytest.mark.parametrize("name", list(LAYOUTS))
def test_commit_boundaries_around_the_pass_edge(engine, g, name):
    off = LAYOUTS[name]
    assert off[-1] == N1 and off[1] >= 500
    V = Votes.random(sum(off), off)
    for kind in ("two_thirds", "zero", "total", "exact"):
        V.agrees(engine, g, _thresholds(V.off, V.lpower, V.lflag, kind))


N3 = 2 * P + 300


def test_three_passes_one_commit_through_the_middle(engine, g):
    """A commit from before P to after 2 P: the middle pass holds no commit start at all."""
    off = [0, 500, P - 300, 2 * P + 100, N3]
    assert off[2] < P and off[3] > 2 * P and not any(P <= o < 2 * P for o in off)
    V = Votes.random(33, off)
    for kind in ("two_thirds", "exact", "total"):
        V.agrees(engine, g, _thresholds(V.off, V.lpower, V.lflag, kind))


def test_three_passes_many_random_commits(engine, g):
    rnd = random.Random("three")
    sizes = []
    while sum(sizes) < N3:
        sizes.append(rnd.choice([0, 0, rnd.randrange(401), rnd.randrange(401), rnd.randrange(401)]))
    sizes[-1] -= sum(sizes) - N3
    assert sum(sizes) == N3 and min(sizes) == 0 and max(sizes) > 300
    V = Votes.random(34, _offsets(sizes))
    V.agrees(engine, g, _thresholds(V.off, V.lpower, V.lflag, "two_thirds"))
    total = _thresholds(V.off, V.lpower, V.lflag, "total")
    V.agrees(engine, g, [rnd.randrange(t + 2) for t in total])


def test_many_commits_of_up_to_three_items(engine, g):
    """More commits than half the items: the bounds of the commit searches on both sides of the edge.
    One commit of three counted votes lies across it, items P - 1, P and P + 1."""
    rnd = random.Random("tiny")
    sizes, total = [0], 0
    while total < P - 1:
        sizes.append(min(rnd.randrange(4), P - 1 - total))
        total += sizes[-1]
    across = len(sizes)
    sizes += [3] + [rnd.randrange(4) for _ in range(3300)] + [0]
    off = _offsets(sizes)
    assert off[across] == P - 1 and off[across + 1] == P + 2
    rng = np.random.default_rng(35)
    n = off[-1]
    power = rng.integers(0, 10, size=n, dtype=np.uint64)
    flag = np.array([0, 2, 1, 1, 1, 1, 1, 1, 1, 1], dtype=np.uint8)[rng.integers(0, 10, size=n)]
    power[P - 1:P + 2], flag[P - 1:P + 2] = 5, 1
    V = Votes(off, power, flag)
    assert P + 2000 < V.n < P + 8000 and V.nc > V.n // 2
    V.agrees(engine, g, _thresholds(V.off, V.lpower, V.lflag, "two_thirds"))
    V.agrees(engine, g, [rnd.randrange(12) for _ in sizes])


def test_counted_power_of_exactly_the_maximum_across_the_edge(engine, g):
    each = MAXP // N1
    power = np.full(N1, each, dtype=np.uint64)
    power[-1] = MAXP - (N1 - 1) * each
    V = Votes([0, N1], power, np.ones(N1, dtype=np.uint8))
    assert sum(V.lpower) == MAXP and g.check_args(V.off, V.lpower, V.lflag, [0])
    for thr in (2**63 - 2, 2**64 - 1):
        assert V.plan(engine, [thr], True)[1:] == ([MAXP], N1)
        V.agrees(engine, g, [thr])


# ---------------------------------------------------------------- 2: the device-side sum check across passes
class Spanning:
    """One commit of P + 257 votes whose counted power lies on both sides of P: 2^62 - 1 on a signed
    vote at item 3, a thousand small powers, and at item P + 50 what is missing to 2^63 - 1 (+ extra).
    Absent and nil votes carry large powers that count for nothing; every other byte is noise."""
    I0, I1 = 3, P + 50

    def __init__(self, engine):
        rng = np.random.default_rng(2)
        n = self.n = N1
        self.flag = np.zeros(n, dtype=np.uint8)
        self.power = rng.integers(0, 2**62, size=n, dtype=np.uint64)
        self.flag[rng.choice(n, 3000, replace=False)] = 2
        small = np.concatenate((rng.choice(np.arange(self.I0 + 1, P), 900, replace=False),
                                rng.choice(np.arange(P, n), 100, replace=False)))
        self.flag[small] = 1
        self.power[small] = rng.integers(0, 2**40, size=1000, dtype=np.uint64)
        self.flag[[self.I0, self.I1]] = 1
        self.flag[:self.I0] = 0
        self.power[self.I0] = 2**62 - 1
        self.power[self.I1] = 0
        self.power[self.I1] = MAXP - int(sum(int(p) for p in self.power[self.flag == 1]))
        msg = b"the one vote that is checked"
        (self.vk,), (self.sig,) = engine.sign([bytes(range(32))], [msg])
        self.k = _challenge(self.vk, self.sig, msg)
        self.d_vk, self.d_sig = _dev(_rows(n, 32, 3, {self.I0: self.vk})), _dev(_rows(n, 64, 4, {self.I0: self.sig}))
        self.d_k, self.d_flag = _dev(_rows(n, 32, 5, {self.I0: self.k})), _dev(self.flag)

    def powers(self, extra):
        p = self.power.copy()
        p[self.I1] += np.uint64(extra)
        return p


def test_device_sum_check_across_passes(engine, g, qsets):
    S = Spanning(engine)
    off, n = [0, S.n], S.n
    fl = S.flag.tolist()
    over, exact = S.powers(1), S.powers(0)
    count = lambda p, a, e: sum(int(x) for x in p[a:e][S.flag[a:e] == 1])   # noqa: E731
    assert count(exact, 0, n) == MAXP and count(over, 0, n) == MAXP + 1
    assert count(over, 0, P) <= MAXP and count(over, P, n) <= MAXP and int(over.max()) <= MAXP
    assert not g.check_args(off, over.tolist(), fl, [0]) and g.check_args(off, exact.tolist(), fl, [0])
    # the refused set: EDC_ERR_ARG and no output written, in both modes
    c_off, thr = (ctypes.c_uint32 * 2)(*off), (ctypes.c_uint64 * 1)(0)
    d_over = _dev_power(over)
    rnd = random.Random("span")
    for mode in (1, 0):
        cv, iv = ctypes.create_string_buffer(b"\x07", 1), ctypes.create_string_buffer(b"\x07" * n, n)
        tal, nb, cnt = (ctypes.c_uint64 * 1)(7), ctypes.c_int(7), ctypes.c_size_t(7)
        c8 = ctypes.create_string_buffer(b"\x07" * 32, 32)
        rc = engine.lib.edc_quorum_verify_device(engine.ctx, 1, c_off, S.d_vk.data_ptr(), S.d_sig.data_ptr(), None, None,
                                                 S.d_k.data_ptr(), d_over.data_ptr(), S.d_flag.data_ptr(), thr, mode,
                                                 rnd.randbytes(32), cv, iv, tal, ctypes.byref(nb), ctypes.byref(cnt), c8)
        assert rc == EDC_ERR_ARG, mode
        assert (cv.raw, iv.raw, list(tal), nb.value, cnt.value, c8.raw) == (b"\x07", b"\x07" * n, [7], 7, 7, b"\x07" * 32)
    # the context still gives a golden set's answer
    Q = qsets("valid")
    _same(Q.device(engine, rnd.randbytes(32), True, prehashed=True), Q.expect(g, g.LIGHT))
    # the same shape with a counted power of exactly 2^63 - 1: light mode, threshold 0, one vote checked
    seed = rnd.randbytes(32)
    got = engine.quorum_verify_device(off, S.d_vk, S.d_sig, None, None, _dev_power(exact), S.d_flag, [0], seed, light=True,
                                      d_k=S.d_k)
    j = g.judge(off, exact.tolist(), fl, [0], g.LIGHT, [0] * n)
    assert j["n_checked"] == 1 and j["checked"][S.I0] == 1 and j["tally"] == [2**62 - 1]
    _same(got, j)
    assert got["code"] == 0 and got["n_checked"] == 1 and got["tally"] == [int(exact[S.I0])]
    assert (0, got["check8"]) == _check8_of(engine, [S.vk], [S.sig], [S.k], seed)


# ---------------------------------------------------------------- 3: templated quorum gather (k_sc_scan twice, k_tq_gather)
def _spread(rnd, must, lo, hi, count, empty_tiles):
    """`must` and `count` more items of [lo, hi), none of them in the tiles that stay empty."""
    pool = [i for i in rnd.sample(range(lo, hi), 4 * count) if i // W not in empty_tiles and i not in must]
    return sorted(set(must) | set(pool[:count]))


class TmplSet:
    """P + 600 votes in five commits (one empty); the three templates of test_gpu_tmpl_quorum.Boundary
    (one with an empty head, one with an empty tail); hole lengths 0..17 for every item with runs of
    empty holes on both sides of P; about 150 checked votes (flag 1 or 2, full mode), signed here.
    Every other vote's key, signature and hole bytes are noise."""
    EMPTY_TILES = (1, 2, 511, 1021, 1025)
    BAD = P + 100

    def __init__(self, engine, edc, oracle_c):
        rnd, rng = random.Random("tmplset"), np.random.default_rng(6)
        n = self.n = P + 600
        self.off = [0, 1000, 1000, P - 300, P + 200, n]
        self.ctpl = [0, 2, 1, 2, 0]
        self.T = edc.batch.Templates([b"", rnd.randbytes(37), rnd.randbytes(5)], [rnd.randbytes(21), b"", rnd.randbytes(64)])
        tpl = np.repeat(np.array(self.ctpl), np.diff(self.off))
        i = np.arange(n)
        lens = (i * 7) % 18
        for a, e in ((40, 75), (P - 60, P - 20), (P - 3, P + 2), (P + 10, P + 45), (n - 3, n)):
            lens[a:e] = 0
        assert set(lens.tolist()) == set(range(18))
        self.voff = np.concatenate(([0], np.cumsum(lens))).astype(np.uint32)
        self.var_bytes = int(self.voff[-1])
        self.var = rng.integers(0, 256, size=self.var_bytes, dtype=np.uint8)
        must1 = [0, 41, 74, P - W, P - W + 1, P - 130, P - 40, P - 21, P - 2, P - 1]
        must2 = [P, P + 1, P + 12, P + 44, P + 100, P + 255, P + 512, n - 2, n - 1]
        self.sel = _spread(rnd, must1, 0, P, 95, self.EMPTY_TILES) + _spread(rnd, must2, P, n, 40, self.EMPTY_TILES)
        assert self.BAD in self.sel
        self.flag = np.zeros(n, dtype=np.uint8)
        self.flag[self.sel] = [1 + (s % 5 == 0) for s in self.sel]
        self.power = (1 + (i * 13) % 50).astype(np.uint64)
        self.thr = [int(self.power[a:e].sum()) // 3 for a, e in zip(self.off, self.off[1:])]
        var = self.var.tobytes()
        self.msgs = [self.T.heads[tpl[s]] + var[self.voff[s]:self.voff[s + 1]] + self.T.tails[tpl[s]] for s in self.sel]
        seeds = [rnd.randbytes(32) for _ in range(5)]
        self.vks, self.sigs = engine.sign(seeds, self.msgs, seed_index=[s % 5 for s in range(len(self.sel))])
        self.vk = _rows(n, 32, 7, dict(zip(self.sel, self.vks)))
        self.sig = _rows(n, 64, 8, dict(zip(self.sel, self.sigs)))
        b = self.sel.index(self.BAD)
        self.bad_sigs = list(self.sigs)
        self.bad_sigs[b] = self.sigs[b][:5] + bytes([self.sigs[b][5] ^ 1]) + self.sigs[b][6:]
        self.sig_bad = self.sig.copy()
        self.sig_bad[self.BAD] = np.frombuffer(self.bad_sigs[b], dtype=np.uint8)
        self.D = {"vk": _dev(self.vk), "sig": _dev(self.sig), "sig_bad": _dev(self.sig_bad), "var": _dev(self.var),
                  "voff": _dev_u32(self.voff), "power": _dev_power(self.power), "flag": _dev(self.flag)}
        self.lpower, self.lflag = self.power.tolist(), self.flag.tolist()
        self.oracle_c = oracle_c

    def reference(self, engine, g, bad, seed):
        """The model's selection on the C oracle's codes of the votes gathered here, and their check8."""
        sigs = self.bad_sigs if bad else self.sigs
        checked, _ = g.select(self.off, self.lpower, self.lflag, self.thr, g.FULL)
        m = sum(checked)
        assert 100 <= m <= 300                                   # the model alone: the shape stays a cheap one
        assert [i for i, c in enumerate(checked) if c] == self.sel
        codes = [0] * self.n
        for s, vk, sig, msg in zip(self.sel, self.vks, sigs, self.msgs):
            codes[s] = self.oracle_c.verify(vk, sig, msg)
        assert [s for s in self.sel if codes[s]] == ([self.BAD] if bad else [])
        j = g.judge(self.off, self.lpower, self.lflag, self.thr, g.FULL, codes)
        union, c8 = _check8_of(engine, self.vks, sigs, [_challenge(*x) for x in zip(self.vks, sigs, self.msgs)], seed)
        assert union == int(bad)
        j["check8"] = c8
        return j, m


@pytest.fixture(scope="module")
def tmplset(engine, edc, oracle_c):
    pytest.importorskip("torch")
    return TmplSet(engine, edc, oracle_c)


def test_tmplset_places_the_checked_votes(tmplset):
    S = tmplset
    sel, tiles = set(S.sel), {s // W for s in S.sel}
    assert {0, S.n - 1, P - 1, P, P + 1} <= sel and 1023 in tiles and 1024 in tiles and not tiles & set(S.EMPTY_TILES)
    assert sum(1 for s in S.sel if s < P) > 90 and sum(1 for s in S.sel if s >= P) > 40
    empty = [s for s in S.sel if S.voff[s] == S.voff[s + 1]]
    assert any(s < P for s in empty) and any(s >= P for s in empty)
    assert {int(S.flag[s]) for s in S.sel} == {1, 2} and S.BAD > P


@pytest.mark.parametrize("bad", [False, True], ids=["valid", "one_bad_in_pass_two"])
def test_templated_gather_past_one_pass(engine, g, tmplset, bad):
    S, D = tmplset, tmplset.D
    seed = random.Random("tq%d" % bad).randbytes(32)
    want, m = S.reference(engine, g, bad, seed)
    got = engine.quorum_verify_templated_device(S.T, S.off, S.ctpl, D["vk"], D["sig_bad" if bad else "sig"], D["var"], D["voff"],
                                                S.var_bytes, D["power"], D["flag"], S.thr, seed, light=False)
    for key in KEYS:
        assert got[key] == want[key], key
    assert got["code"] == (1 if bad else want["code"]) and got["n_checked"] == m == len(S.sel)
    assert engine.tmpl_quorum_last() == (S.n, m, m, sum(len(x) for x in S.msgs))


def test_templated_gather_past_one_pass_host_form(engine, g, tmplset):
    """edc_tmpl_quorum_verify on flat host buffers, with the bad vote: the codes travel back through idx."""
    S = tmplset
    seed = random.Random("tqhost").randbytes(32)
    want, m = S.reference(engine, g, True, seed)
    ts, _keep = S.T.struct()
    nc, n = len(S.ctpl), S.n
    off, ctpl, thr = (ctypes.c_uint32 * (nc + 1))(*S.off), (ctypes.c_uint16 * nc)(*S.ctpl), (ctypes.c_uint64 * nc)(*S.thr)
    cv, iv, tal = ctypes.create_string_buffer(nc), ctypes.create_string_buffer(n), (ctypes.c_uint64 * nc)()
    nb, cnt, c8 = ctypes.c_int(0), ctypes.c_size_t(0), ctypes.create_string_buffer(32)
    rc = engine.lib.edc_tmpl_quorum_verify(engine.ctx, ctypes.byref(ts), nc, off, ctpl, 1, None, S.vk.tobytes(), None,
                                           S.sig_bad.tobytes(), S.var.tobytes(), S.voff.ctypes.data_as(U32P),
                                           S.power.ctypes.data_as(U64P), S.flag.tobytes(), thr, 0, seed, cv, iv, tal,
                                           ctypes.byref(nb), ctypes.byref(cnt), c8)
    got = {"code": rc, "commit_verdicts": list(cv.raw), "item_verdicts": list(iv.raw), "tally": list(tal),
           "n_bad_commits": nb.value, "n_checked": cnt.value, "check8": c8.raw}
    for key in KEYS:
        assert got[key] == want[key], key
    assert engine.tmpl_quorum_last() == (n, m, m, sum(len(x) for x in S.msgs))


# ---------------------------------------------------------------- 4: cached quorum (k_sc_lookup_masked, k_sc_scan per count)
def test_cached_quorum_past_one_pass(edc, g):
    pytest.importorskip("torch")
    rnd = random.Random("cached")
    n = N1
    off = [0, P - 100, P + 100, n]
    must1, must2 = [0, 5, P - W, P - 2, P - 1], [P, P + 1, P + 2, P + W - 1, P + W, n - 1]
    sel = _spread(rnd, must1, 0, P, 75, (3, 1022)) + _spread(rnd, must2, P, n, 34, ())
    planted = set(sel[::2]) | {P - 1, P + 1}
    planted -= {P - 2, P, n - 1}
    fresh = [s for s in sel if s not in planted]
    for side in (lambda s: s < P, lambda s: s >= P):
        assert sum(1 for s in planted if side(s)) > 10 and sum(1 for s in fresh if side(s)) > 10
    flag = np.zeros(n, dtype=np.uint8)
    flag[sel] = [1 + (s % 7 == 0) for s in sel]
    power = (1 + (np.arange(n) * 11) % 40).astype(np.uint64)
    thr = [int(power[a:e].sum()) // 3 for a, e in zip(off, off[1:])]
    j = g.judge(off, power.tolist(), flag.tolist(), thr, g.FULL, [0] * n)
    assert j["n_checked"] == len(sel) and 100 <= len(sel) <= 140 and [i for i, c in enumerate(j["checked"]) if c] == sel
    eng = edc.Engine(0)
    try:
        eng.sigcache_create(1 << 12)
        msgs = [rnd.randbytes(20 + s % 30) for s in sel]
        vks, sigs = eng.sign([rnd.randbytes(32) for _ in range(5)], msgs, seed_index=[s % 5 for s in range(len(sel))])
        item = {s: (vk, sig, _challenge(vk, sig, m)) for s, vk, sig, m in zip(sel, vks, sigs, msgs)}
        d_vk = _dev(_rows(n, 32, 9, {s: x[0] for s, x in item.items()}))
        d_sig = _dev(_rows(n, 64, 10, {s: x[1] for s, x in item.items()}))
        d_k = _dev(_rows(n, 32, 11, {s: x[2] for s, x in item.items()}))
        d_power, d_flag = _dev_power(power), _dev(flag)
        # about half of the checked votes become records through a cached batch call on just those rows
        rows = sorted(planted)
        rc, _, miss = eng.batch_verify_cached([item[s][0] for s in rows], [item[s][1] for s in rows],
                                              ks=[item[s][2] for s in rows], z_seed=rnd.randbytes(32))
        assert (rc, miss) == (0, len(rows)) and eng.sigcache_stats()["inserted"] == len(rows)
        seed = rnd.randbytes(32)
        got = eng.quorum_verify_cached_device(off, d_vk, d_sig, None, None, d_power, d_flag, thr, seed, light=False, d_k=d_k)
        _same(got, j)
        assert got["n_miss"] == len(fresh)
        assert (0, got["check8"]) == _check8_of(eng, *[[item[s][f] for s in fresh] for f in range(3)], seed)
        assert eng.cached_quorum_last() == (n, len(sel), len(rows), len(fresh), 0, len(fresh))
        again = eng.quorum_verify_cached_device(off, d_vk, d_sig, None, None, d_power, d_flag, thr, seed, light=False, d_k=d_k)
        _same(again, j)
        assert again["n_miss"] == 0 and (0, again["check8"]) == _check8_of(eng, [], [], [], seed)
        assert eng.cached_quorum_last() == (n, len(sel), len(sel), 0, 0, 0)
    finally:
        eng.close()


# ---------------------------------------------------------------- 5: template expansion (k_tmpl_scan)
class Expansion:
    """n templated items, hole lengths 0..9, four templates (an empty head, an empty tail, both empty)."""
    HEADS, TAILS = (0, 5, 16, 0), (7, 0, 33, 0)

    def __init__(self, edc, n):
        rnd, rng = random.Random(n), np.random.default_rng(n)
        self.n = n
        self.T = edc.batch.Templates([rnd.randbytes(k) for k in self.HEADS], [rnd.randbytes(k) for k in self.TAILS])
        self.tpl = rng.integers(0, 4, size=n).astype(np.uint16)
        self.lens = rng.integers(0, 10, size=n)
        self.voff = np.concatenate(([0], np.cumsum(self.lens))).astype(np.uint32)
        self.var_bytes = int(self.voff[-1])
        self.var = rng.integers(0, 256, size=self.var_bytes, dtype=np.uint8)
        self.cap = n * (max(self.HEADS) + max(self.TAILS)) + self.var_bytes + 16      # the entry's own bound
        self.d_tpl, self.d_var = _dev(self.tpl.view(np.int16)), _dev(self.var)

    def expected(self):
        """(the n + 1 offsets, the arena bytes): message i = head[tpl[i]] + hole i + tail[tpl[i]], laid end to end."""
        hl, tl = np.array(self.HEADS)[self.tpl], np.array(self.TAILS)[self.tpl]
        off = np.concatenate(([0], np.cumsum(hl + self.lens + tl))).astype(np.int64)
        arena = np.zeros(int(off[-1]), dtype=np.uint8)
        start, vo = off[:-1], self.voff[:-1].astype(np.int64)
        for t in range(4):
            at = np.flatnonzero(self.tpl == t)
            for part, where in ((self.T.heads[t], start[at]), (self.T.tails[t], start[at] + hl[at] + self.lens[at])):
                if part:
                    arena[where[:, None] + np.arange(len(part))] = np.frombuffer(part, dtype=np.uint8)
        for k in range(1, 10):
            at = np.flatnonzero(self.lens == k)
            arena[(start[at] + hl[at])[:, None] + np.arange(k)] = self.var[vo[at][:, None] + np.arange(k)]
        return off, arena

    def run(self, engine, voff):
        import torch
        d_msg = torch.full((self.cap,), 0xEE, dtype=torch.uint8, device="cuda:0")
        d_off = torch.full((self.n + 1,), -1, dtype=torch.int64, device="cuda:0")
        d_voff = _dev_u32(voff)
        ts, _keep = self.T.struct()
        rc = engine.lib.edc_tmpl_expand_device(engine.ctx, ctypes.byref(ts), self.n, self.d_tpl.data_ptr(), self.d_var.data_ptr(),
                                               d_voff.data_ptr(), self.var_bytes, d_msg.data_ptr(), self.cap, d_off.data_ptr())
        torch.cuda.synchronize()
        return rc, d_off.cpu().numpy(), d_msg.cpu().numpy()


@pytest.mark.parametrize("n", [P + 1, 2 * P + 1, P + 7 * W + 3], ids=["P+1", "2P+1", "P+1795"])
def test_expansion_past_one_pass(edc, engine, n):
    """P + 1: 1025 workgroup sums, two per scan thread and one for the last active thread; 2 P + 1:
    three per thread; P + 1795: 1032 sums."""
    pytest.importorskip("torch")
    E = Expansion(edc, n)
    off, arena = E.expected()
    assert all(np.any(E.tpl[-W:] == t) for t in range(4)) and set(E.lens.tolist()) == set(range(10))
    rc, got_off, got = E.run(engine, E.voff)
    assert rc == 0, engine.lib.edc_last_error(engine.ctx)
    diff = np.flatnonzero(got_off != off)
    assert diff.size == 0, (diff.size, diff[:5].tolist())
    diff = np.flatnonzero(got[:len(arena)] != arena)
    assert diff.size == 0, (diff.size, diff[:5].tolist())
    assert (got[len(arena):] == 0xEE).all()                       # nothing written behind the last message
    if n == P + 7 * W + 3:
        # a decreasing var_off at item P + 5: EDC_ERR_ARG and n empty messages, nothing else written
        down = E.voff.copy()
        assert down[P + 5] > 0
        down[P + 6] = down[P + 5] - 1
        rc, got_off, got = E.run(engine, down)
        assert rc == EDC_ERR_ARG
        assert not got_off.any() and (got == 0xEE).all()
        rc, got_off, _ = E.run(engine, E.voff)                    # and the context still expands
        assert rc == 0 and (got_off == off).all()
