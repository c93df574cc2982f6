"""GPU: quorum commit sets (include/edc.h, edc_quorum_*): which votes of a commit set are verified,
what voting power the verified ones carry, and each commit's verdict.

Everything that is not a signature is judged by the pure-Python model of tests/golden/gen_quorum.py
(written from the header's definitions); the items' codes are the CPU oracle's (commits.json) and
the expected results of the signed sets are those of tests/golden/quorum.json. check8 is compared
with edc_batch_verify_prehashed_device run here on the list this test gathers itself. The selection
is driven through edc_quorum_plan, which runs the kernels every form runs, at the shapes where a
segmented scan breaks; W below is the selection kernel's workgroup tile (csrc/edc_launch.h, QR_TILE)."""
import ctypes
import random

import pytest

from conftest import golden
from test_gpu_commits import CommitSet, _gen as _gen_commits
from test_quorum_abi import gen_quorum

pytestmark = pytest.mark.gpu

W = 256
MAXP = 2**63 - 1


@pytest.fixture(scope="module")
def g():
    return gen_quorum()


def _offsets(sizes):
    off = [0]
    for s in sizes:
        off.append(off[-1] + s)
    return off


def _random_votes(rnd, n, pmax=1000):
    power = [rnd.randrange(pmax + 1) for _ in range(n)]
    flag = [rnd.choice([0, 2, 1, 1, 1, 1, 1, 1, 1, 1]) for _ in range(n)]
    return power, flag


def _plan_agrees(engine, g, off, power, flag, thr):
    for mode in (g.FULL, g.LIGHT):
        checked, planned = g.select(off, power, flag, thr, mode)
        got = engine.quorum_plan(off, power, flag, thr, light=mode == g.LIGHT)
        assert got[1] == planned, (mode, off[:8])
        assert got[0] == checked, (mode, [i for i, (a, b) in enumerate(zip(got[0], checked)) if a != b][:10])
        assert got[2] == sum(checked)


def _thresholds(off, power, flag, kind):
    """2/3 of the commit's power; 0; the total (never passed); the counted power of the commit's first half exactly."""
    out = []
    for a, e in zip(off, off[1:]):
        if kind == "two_thirds":
            out.append(2 * sum(power[a:e]) // 3)
        elif kind == "zero":
            out.append(0)
        elif kind == "total":
            out.append(sum(power[a:e]))
        else:
            out.append(sum(p for p, f in zip(power[a:(a + e) // 2], flag[a:(a + e) // 2]) if f == 1))
    return out


# ---------------------------------------------------------------- the selection
@pytest.mark.parametrize("sizes", [[W - 1], [W], [W + 1], [2 * W + 1], [W - 1, 1, W, 64, 64, 128, 2 * W + 1, 3],
                                   [64, 192, 256, 100], [1]], ids=lambda s: "-".join(map(str, s)))
def test_selection_around_the_tile(engine, g, sizes):
    """Commits of W - 1, W, W + 1 and 2 W + 1 items; commit boundaries on a wave (64) and on a tile (256, 512)."""
    off = _offsets(sizes)
    rnd = random.Random("tile%r" % sizes)
    power, flag = _random_votes(rnd, off[-1])
    for kind in ("two_thirds", "zero", "total", "exact"):
        _plan_agrees(engine, g, off, power, flag, _thresholds(off, power, flag, kind))
    _plan_agrees(engine, g, off, [7] * off[-1], [1] * off[-1], [7 * (s // 2) for s in sizes])


def test_selection_one_long_commit(engine, g):
    """5,000 items in one commit: the quorum reached inside the third tile, and never reached."""
    off, power, flag = [0, 5000], [3] * 5000, [1] * 5000
    assert 2 * W < 600 < 3 * W
    checked, planned, m = engine.quorum_plan(off, power, flag, [3 * 600], light=True)
    assert checked == [1] * 601 + [0] * 4399 and planned == [3 * 601] and m == 601
    _plan_agrees(engine, g, off, power, flag, [3 * 600])
    _plan_agrees(engine, g, off, power, flag, [3 * 5000])
    _plan_agrees(engine, g, off, power, flag, [2**64 - 1])
    rnd = random.Random(5000)
    power, flag = _random_votes(rnd, 5000)
    _plan_agrees(engine, g, off, power, flag, [sum(p for p, f in zip(power[:600], flag[:600]) if f == 1)])
    _plan_agrees(engine, g, off, power, flag, [sum(power)])


def test_selection_many_tiny_commits(engine, g):
    """600 commits of 0..5 items (the tmap_small sizes) with leading, trailing and consecutive empty commits."""
    sizes = list(_gen_commits().layout("tmap_small")["sizes"])
    sizes[300:303] = [0, 0, 0]
    assert len(sizes) == 600 and sizes[0] == sizes[-1] == 0 and max(sizes) == 5
    off = _offsets(sizes)
    rnd = random.Random(600)
    power, flag = _random_votes(rnd, off[-1], pmax=9)
    for kind in ("two_thirds", "zero", "total", "exact"):
        _plan_agrees(engine, g, off, power, flag, _thresholds(off, power, flag, kind))
    _plan_agrees(engine, g, off, power, flag, [rnd.randrange(12) for _ in sizes])
    # thousands of commits inside one workgroup's reach, most of them empty
    sizes = [rnd.choice([0, 0, 0, 1]) for _ in range(4000)]
    off = _offsets(sizes)
    power, flag = _random_votes(rnd, off[-1], pmax=3)
    _plan_agrees(engine, g, off, power, flag, [rnd.randrange(3) for _ in sizes])


def test_selection_degenerate_sets(engine, g):
    assert engine.quorum_plan([0, 0], [], [], [0]) == ([], [0], 0)               # nc = 1 with n = 0
    assert engine.quorum_plan([0, 0, 0, 0], [], [], [5, 0, 9], light=False) == ([], [0, 0, 0], 0)
    assert engine.quorum_plan([0], [], [], []) == ([], [], 0)                    # nc = 0
    for flag in (0, 1, 2):                                                       # n = 1
        _plan_agrees(engine, g, [0, 1], [9], [flag], [0])
        _plan_agrees(engine, g, [0, 1], [9], [flag], [9])


def test_selection_threshold_edges(engine, g):
    """A threshold equal to the running sum: the next item is still checked; >= the total: every flag-1 item."""
    off, power, flag = [0, 4], [5, 5, 5, 5], [1, 1, 1, 1]
    assert engine.quorum_plan(off, power, flag, [10]) == ([1, 1, 1, 0], [15], 3)
    assert engine.quorum_plan(off, power, flag, [9]) == ([1, 1, 0, 0], [10], 2)
    assert engine.quorum_plan(off, power, flag, [0]) == ([1, 0, 0, 0], [5], 1)
    assert engine.quorum_plan(off, power, flag, [20]) == ([1, 1, 1, 1], [20], 4)
    assert engine.quorum_plan(off, power, [1, 2, 0, 1], [0], light=False) == ([1, 1, 0, 1], [10], 3)


def test_selection_power_edges(engine, g):
    """One power of 2^63 - 1, zero powers, all-absent and all-nil commits, in both modes."""
    off = _offsets([1, 3, 2, 2, 300, 300])
    power = [MAXP, 0, 0, 0, 7, 7, 7, 7] + [5] * 300 + [5] * 300
    flag = [1, 1, 1, 1, 0, 0, 2, 2] + [0] * 300 + [2] * 300
    for thr in ([MAXP - 1, 0, 0, 0, 0, 0], [2**64 - 1] * 6, [0] * 6, [MAXP] * 6):
        _plan_agrees(engine, g, off, power, flag, thr)
    assert engine.quorum_plan(off, power, flag, [0] * 6)[2] == 4                 # zero powers never reach a quorum
    # a commit whose counted power is exactly 2^63 - 1, over many tiles
    n = 3 * W + 5
    _plan_agrees(engine, g, [0, n], [MAXP // n] * (n - 1) + [MAXP - (n - 1) * (MAXP // n)], [1] * n, [MAXP - 1])


# ---------------------------------------------------------------- the signed sets
class QuorumSet:
    """A commit set of commits.json with the votes gen_quorum.py lays over it."""

    def __init__(self, name, S, g, fx):
        self.name, self.S, self.off, self.n, self.nc = name, S, S.off, S.n, S.nc
        self.power, self.flag, self.thr = g.votes(name, S.off)
        self.vks, self.sigs, self.ks, self.msgs = list(S.vks), list(S.sigs), list(S.ks), S.msgs
        for i, vk, sig in g.garbage(name):           # an absent vote's bytes are never interpreted
            self.vks[i], self.sigs[i], self.ks[i] = vk, sig, b"\xff" * 32
        self.codes, self.fx = S.codes, fx["sets"][name]
        self._dev = None

    def dev(self):
        if self._dev is None:
            import torch
            d = torch.device("cuda:0")

            def up(b):
                return torch.frombuffer(bytearray(b or b"\0"), dtype=torch.uint8).to(d)
            offs = _offsets([len(m) for m in self.msgs])
            self._dev = {"vk": up(b"".join(self.vks)), "sig": up(b"".join(self.sigs)), "msg": up(b"".join(self.msgs)),
                         "off": torch.tensor(offs, dtype=torch.int64, device=d), "k": up(b"".join(self.ks)),
                         "power": self.dev_power(self.power), "flag": up(bytes(self.flag))}
            torch.cuda.synchronize()
        return self._dev

    @staticmethod
    def dev_power(power):
        import numpy as np
        import torch
        return torch.from_numpy(np.array(power or [0], dtype=np.uint64).view(np.int64)).to("cuda:0")

    def device(self, engine, seed, light, prehashed=False, power=None, flag=None, thr=None):
        D = self.dev()
        return engine.quorum_verify_device(self.off, D["vk"], D["sig"], None if prehashed else D["msg"],
                                           None if prehashed else D["off"], D["power"] if power is None else power,
                                           D["flag"] if flag is None else flag, self.thr if thr is None else thr, seed,
                                           light=light, d_k=D["k"] if prehashed else None)

    def expect(self, g, mode):
        j = g.judge(self.off, self.power, self.flag, self.thr, mode, self.codes)
        e = self.fx["light" if mode == g.LIGHT else "full"]
        for key in ("tally", "commit_verdicts", "n_checked", "n_bad_commits", "code", "planned"):
            assert j[key] == e[key], (self.name, key)           # the model and the fixture say the same
        return j


@pytest.fixture(scope="module")
def qsets(engine, oracle, g):
    pytest.importorskip("torch")
    gc, fxc, fx = _gen_commits(), golden("commits.json"), golden("quorum.json")
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = QuorumSet(name, CommitSet(name, engine, oracle, gc, fxc), g, fx)
        return cache[name]
    return get


def _same(got, j):
    assert got["code"] == j["code"]
    assert got["commit_verdicts"] == j["commit_verdicts"]
    assert got["tally"] == j["tally"]
    assert got["item_verdicts"] == j["item_verdicts"], [i for i, (a, b) in enumerate(zip(got["item_verdicts"], j["item_verdicts"])) if a != b][:10]
    assert (got["n_bad_commits"], got["n_checked"]) == (j["n_bad_commits"], j["n_checked"])


def _check8_of_gathered(engine, Q, checked, seed):
    """edc_batch_verify_prehashed_device on the checked items, gathered here in queue order."""
    import torch
    sel = [i for i, c in enumerate(checked) if c]

    def up(parts):
        return torch.frombuffer(bytearray(b"".join(parts) or b"\0"), dtype=torch.uint8).to("cuda:0")
    vk, sig, k = up([Q.vks[i] for i in sel]), up([Q.sigs[i] for i in sel]), up([Q.ks[i] for i in sel])
    torch.cuda.synchronize()
    c8 = ctypes.create_string_buffer(32)
    rc = engine.lib.edc_batch_verify_prehashed_device(engine.ctx, len(sel), vk.data_ptr(), sig.data_ptr(), k.data_ptr(),
                                                      seed, 0, None, c8)
    assert rc in (0, 1), engine.lib.edc_last_error(engine.ctx)
    return rc, c8.raw


@pytest.mark.parametrize("light", [False, True], ids=["full", "light"])
@pytest.mark.parametrize("name", ["valid", "mixed_a"])
def test_every_form_gives_the_fixture(engine, g, qsets, name, light):
    Q = qsets(name)
    mode = g.LIGHT if light else g.FULL
    j = Q.expect(g, mode)
    rnd = random.Random("forms%s%d" % (name, light))
    seed = rnd.randbytes(32)
    got = Q.device(engine, seed, light)
    _same(got, j)
    union, c8 = _check8_of_gathered(engine, Q, j["checked"], seed)
    assert got["check8"] == c8 and union == (1 if any(c not in (0, 255) for c in j["item_verdicts"]) else 0)
    got = Q.device(engine, seed, light, prehashed=True)
    _same(got, j)
    assert got["check8"] == c8
    for kw in (dict(vks=Q.vks, msgs=Q.msgs), dict(vks=Q.vks, ks=Q.ks)):
        got = engine.quorum_verify(Q.off, Q.sigs, Q.power, Q.flag, Q.thr, seed, light=light, **kw)
        _same(got, j)
        assert got["check8"] == c8
    keys = list(dict.fromkeys(Q.vks))
    pos = {k: i for i, k in enumerate(keys)}
    idx = [pos[k] for k in Q.vks]
    engine.keycache_load(keys)
    try:
        got = engine.quorum_verify(Q.off, Q.sigs, Q.power, Q.flag, Q.thr, seed, light=light, key_idx=idx, msgs=Q.msgs)
        _same(got, j)
        assert got["check8"] == c8
        _same(engine.quorum_verify(Q.off, Q.sigs, Q.power, Q.flag, Q.thr, rnd.randbytes(32), light=light, key_idx=idx, ks=Q.ks), j)
        _same(Q.device(engine, rnd.randbytes(32), light), j)                  # the device form with the key cache loaded
    finally:
        engine.keycache_clear()


def test_mixed_a_situations(g, qsets):
    """What the fixture was laid out for, read off the expected results the forms are held to above."""
    Q = qsets("mixed_a")
    full, light, sit = Q.expect(g, g.FULL), Q.expect(g, g.LIGHT), Q.fx["situations"]
    c = sit["after"][0]
    assert (light["commit_verdicts"][c], full["commit_verdicts"][c]) == (0, 1)
    c = sit["missing"][0]
    assert light["commit_verdicts"][c] == 1 and light["tally"][c] <= Q.thr[c]
    i = sit["nil_bad"][0]
    assert full["item_verdicts"][i] not in (0, 255) and light["item_verdicts"][i] == 255
    i = sit["garbage"][0]
    assert Q.flag[i] == 0 and Q.vks[i] != Q.S.vks[i] and full["item_verdicts"][i] == light["item_verdicts"][i] == 255


@pytest.mark.parametrize("name", ["valid", "mixed_a"])
def test_all_counted_full_mode_is_the_commit_set(engine, g, qsets, name):
    """Every flag 1, every threshold 0, full mode: the item codes are edc_commits_verify_device's."""
    import torch
    Q = qsets(name)
    D = Q.dev()
    seed = random.Random("all" + name).randbytes(32)
    rc, verdicts, codes, n_bad = engine.commits_verify_device(Q.off, D["vk"].data_ptr(), D["sig"].data_ptr(),
                                                              D["msg"].data_ptr(), D["off"].data_ptr(), seed)
    ones = torch.ones(Q.n, dtype=torch.uint8, device="cuda:0")
    got = Q.device(engine, seed, False, flag=ones, thr=[0] * Q.nc)
    assert got["item_verdicts"] == codes and got["n_checked"] == Q.n
    j = g.judge(Q.off, Q.power, [1] * Q.n, [0] * Q.nc, g.FULL, codes)
    _same(got, j)
    assert [v == 1 for v in got["commit_verdicts"]] == [v == 1 for v in verdicts]


@pytest.mark.parametrize("grouping", [1, 2])
def test_independent_of_the_key_grouping(engine, g, qsets, grouping):
    Q = qsets("mixed_a")
    engine.set_key_grouping(grouping)
    try:
        for light in (False, True):
            _same(Q.device(engine, random.Random(grouping * 2 + light).randbytes(32), light), Q.expect(g, g.LIGHT if light else g.FULL))
    finally:
        engine.set_key_grouping(0)


def test_python_batch_surface(engine, edc, g, qsets):
    Q = qsets("valid")
    vs, powers, flags = [], [], []
    for a, e in zip(Q.off, Q.off[1:]):
        v = edc.batch.Verifier()
        for i in range(a, e):
            v.queue((Q.vks[i], Q.sigs[i], Q.msgs[i]))
        vs.append(v)
        powers.append(Q.power[a:e])
        flags.append(Q.flag[a:e])
    j = Q.expect(g, g.LIGHT)
    verdicts, tally, codes = edc.batch.verify_quorum(vs, powers, flags, Q.thr, light=True, engine=engine)
    assert verdicts == j["commit_verdicts"] and tally == j["tally"]
    assert [c for per in codes for c in per] == j["item_verdicts"]


# ---------------------------------------------------------------- argument errors
def _bad_votes(Q):
    """(what, power, flag) of three refused variants of the valid set's votes."""
    c = max(range(Q.nc), key=lambda c: Q.off[c + 1] - Q.off[c])
    a = Q.off[c]
    edge = (a // W + 1) * W                                # the first tile edge inside the long commit
    assert a < edge - 1 and edge < Q.off[c + 1]
    flag3 = list(Q.flag)
    flag3[a + 5] = 3
    big = list(Q.power)
    big[a + 7] = 2**63
    over_p, over_f = [0 if Q.off[c] <= i < Q.off[c + 1] else p for i, p in enumerate(Q.power)], list(Q.flag)
    over_p[edge - 1] = over_p[edge] = 2**62                # 2^63 in all, half of it in each of two tiles
    over_f[edge - 1] = over_f[edge] = 1
    return [("flag", Q.power, flag3), ("power", big, Q.flag), ("overflow", over_p, over_f)]


def test_argument_errors_leave_the_context_usable(engine, edc, g, qsets):
    import torch
    Q = qsets("valid")
    j = Q.expect(g, g.LIGHT)
    rnd = random.Random("args")
    for what, power, flag in _bad_votes(Q):
        assert not g.check_args(Q.off, power, flag, Q.thr), what
        for light in (False, True):
            with pytest.raises(edc.EngineError, match="edc error -2"):
                engine.quorum_verify(Q.off, Q.sigs, power, flag, Q.thr, rnd.randbytes(32), light=light, vks=Q.vks, ks=Q.ks)
            with pytest.raises(edc.EngineError, match="edc error -2"):
                engine.quorum_plan(Q.off, power, flag, Q.thr, light=light)
            d_flag = torch.frombuffer(bytearray(bytes(flag)), dtype=torch.uint8).to("cuda:0")
            with pytest.raises(edc.EngineError, match="edc error -2"):
                Q.device(engine, rnd.randbytes(32), light, prehashed=True, power=Q.dev_power(power), flag=d_flag)
        _same(Q.device(engine, rnd.randbytes(32), True, prehashed=True), j)            # the same context still works
        _same(engine.quorum_verify(Q.off, Q.sigs, Q.power, Q.flag, Q.thr, rnd.randbytes(32), vks=Q.vks, ks=Q.ks), j)
    # what the host refuses in every form
    lib, D = engine.lib, Q.dev()
    off = (ctypes.c_uint32 * (Q.nc + 1))(*Q.off)
    thr = (ctypes.c_uint64 * Q.nc)(*Q.thr)
    seed = rnd.randbytes(32)

    def dev(nc=Q.nc, off=off, thr=thr, mode=1, seed=seed, power=D["power"].data_ptr()):
        return lib.edc_quorum_verify_device(engine.ctx, nc, off, D["vk"].data_ptr(), D["sig"].data_ptr(), None, None,
                                            D["k"].data_ptr(), power, D["flag"].data_ptr(), thr, mode, seed, None, None,
                                            None, None, None, None)
    assert dev(mode=2) == -2 and dev(seed=None) == -2 and dev(thr=None) == -2
    assert dev(power=D["power"].data_ptr() + 4) == -2                                  # d_power 8-byte aligned
    down = (ctypes.c_uint32 * (Q.nc + 1))(*([0, 5, 4] + Q.off[3:]))
    assert dev(off=down) == -2
    assert dev(nc=0) == 0                                                              # nc = 0: nothing is read
    assert dev() == j["code"]


def test_allocations_return(edc, g, qsets):
    Q = qsets("valid")
    before = edc.debug_live_allocs()
    eng = edc.Engine(0)
    try:
        _same(eng.quorum_verify(Q.off, Q.sigs, Q.power, Q.flag, Q.thr, bytes(range(32)), vks=Q.vks, msgs=Q.msgs), Q.expect(g, g.LIGHT))
        assert edc.debug_live_allocs() > before
    finally:
        eng.close()
    assert edc.debug_live_allocs() == before
