"""GPU: templated quorum commit sets (include/edc.h, edc_tmpl_quorum_*): the selection runs first and
only the checked votes are gathered, assembled and hashed.

Every expectation is the pure-Python model of tests/golden/gen_quorum.py on the oracle's item codes
(commits.json, commits_alt.json, quorum.json), or edc_quorum_verify_device run here with the same
seed on the materialised messages (for the variants: on the arena edc_tmpl_expand_device builds);
never another templated quorum call. W is the selection and gather tile (csrc/edc_launch.h, QR_TILE)."""
import ctypes
import random

import pytest

from conftest import golden
from test_gpu_commits import _gen as _gen_commits
from test_gpu_commits_alt import AltSet, _load
from test_gpu_quorum import QuorumSet, CommitSet, _offsets, _same
from test_quorum_abi import gen_quorum

pytestmark = pytest.mark.gpu

W = 256
KEYS = ("code", "commit_verdicts", "item_verdicts", "tally", "n_bad_commits", "n_checked", "check8")


@pytest.fixture(scope="module")
def g():
    return gen_quorum()


@pytest.fixture(scope="module")
def qsets(engine, oracle, g, edc):
    pytest.importorskip("torch")
    gc, fxc, fx = _gen_commits(), golden("commits.json"), golden("quorum.json")
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = QuorumSet(name, CommitSet(name, engine, oracle, gc, fxc), g, fx)
        return cache[name]
    get.templates = edc.batch.Templates(*gc.templates())
    return get


def _up(b):
    import torch
    return torch.frombuffer(bytearray(b or b"\0"), dtype=torch.uint8).to("cuda:0")


def _i32(v):
    import torch
    return torch.tensor(v, dtype=torch.int64).to(torch.int32).to("cuda:0") if max(v) < 2**31 else None


class Items:
    """Device tensors of a templated quorum set: keys, signatures, holes, variant bytes, votes."""

    def __init__(self, vks, sigs, holes, power, flag, alt=None, var_off=None):
        import torch
        voff = _offsets([len(h) for h in holes]) if var_off is None else var_off
        self.vk, self.sig, self.var = _up(b"".join(vks)), _up(b"".join(sigs)), _up(b"".join(holes))
        self.voff, self.var_bytes = _i32(voff), sum(len(h) for h in holes)
        self.alt = None if alt is None else _up(bytes(alt))
        self.power, self.flag = QuorumSet.dev_power(power), _up(bytes(flag))
        torch.cuda.synchronize()


def _tq(engine, T, off, ctpl, D, thr, seed, light, span=1, **kw):
    a = dict(d_vk=D.vk, d_sig=D.sig, d_var=D.var, d_var_off=D.voff, var_bytes=D.var_bytes, d_power=D.power, d_flag=D.flag,
             d_item_alt=D.alt)
    a.update(kw)
    return engine.quorum_verify_templated_device(T, off, ctpl, a["d_vk"], a["d_sig"], a["d_var"], a["d_var_off"],
                                                 a["var_bytes"], a["d_power"], a["d_flag"], thr, seed, light=light,
                                                 alt_span=span, d_item_alt=a["d_item_alt"])


def _ref(engine, off, D, msgs, thr, seed, light):
    """edc_quorum_verify_device on the materialised messages (keys, signatures and votes of D)."""
    import torch
    d_msg = _up(b"".join(msgs))
    d_off = torch.tensor(_offsets([len(m) for m in msgs]), dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    return engine.quorum_verify_device(off, D.vk, D.sig, d_msg, d_off, D.power, D.flag, thr, seed, light=light)


def _equal(got, want):
    for key in KEYS:
        assert got[key] == want[key], key


# ---- 1 and 5: the fixture, one template per commit; only the checked votes are hashed ----

@pytest.mark.parametrize("light", [False, True], ids=["full", "light"])
@pytest.mark.parametrize("name", ["valid", "mixed_a"])
def test_every_form_gives_the_fixture(engine, g, qsets, name, light):
    Q, T = qsets(name), qsets.templates
    S = Q.S
    assert {"valid": 2207, "mixed_a": 4310}[name] == Q.n
    j = Q.expect(g, g.LIGHT if light else g.FULL)
    rnd = random.Random("tq%s%d" % (name, light))
    seed = rnd.randbytes(32)
    want = Q.device(engine, seed, light)                       # edc_quorum_verify_device on the messages
    _same(want, j)
    D = Items(Q.vks, Q.sigs, S.holes, Q.power, Q.flag)
    got = _tq(engine, T, Q.off, S.commit_tpl, D, Q.thr, seed, light)
    _same(got, j)
    _equal(got, want)
    # only the checked votes were expanded and hashed; the arena holds their messages and nothing else
    last = engine.tmpl_quorum_last()
    m = j["n_checked"]
    assert last[:3] == (Q.n, m, m)
    assert last[3] == sum(len(Q.msgs[i]) for i, c in enumerate(j["checked"]) if c)
    if light:
        assert last[2] < Q.n
    got = engine.quorum_verify_templated(T, Q.off, S.commit_tpl, Q.sigs, S.holes, Q.power, Q.flag, Q.thr, seed, light=light,
                                         vks=Q.vks)
    _equal(got, want)
    keys = list(dict.fromkeys(Q.vks))
    pos = {k: i for i, k in enumerate(keys)}
    engine.keycache_load(keys)
    try:
        got = engine.quorum_verify_templated(T, Q.off, S.commit_tpl, Q.sigs, S.holes, Q.power, Q.flag, Q.thr, seed,
                                             light=light, key_idx=[pos[k] for k in Q.vks])
        _equal(got, want)
        _equal(_tq(engine, T, Q.off, S.commit_tpl, D, Q.thr, seed, light), want)      # device form, key cache loaded
    finally:
        engine.keycache_clear()
    _equal(_tq(engine, T, Q.off, S.commit_tpl, D, Q.thr, seed, light), want)


# ---- 2: variants ----

@pytest.fixture(scope="module")
def alt(engine, edc):
    pytest.importorskip("torch")
    gen, fx = _load("gen_commits_alt"), golden("commits_alt.json")
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = AltSet(name, engine, gen, fx)
        return cache[name]
    get.gen = gen
    get.templates = edc.batch.Templates(*gen.templates())
    return get


def _drawn_votes(name, off):
    """About 10 % absent and 10 % nil (gen_quorum.RULE's shares), powers 1..1000, thresholds floor(2T/3)."""
    rnd = random.Random("votes" + name)
    n = off[-1]
    power = [1 + rnd.randrange(1000) for _ in range(n)]
    flag = [0 if b < 26 else 2 if b < 52 else 1 for b in rnd.randbytes(n)]
    return power, flag, [2 * sum(power[a:e]) // 3 for a, e in zip(off, off[1:])]


@pytest.mark.parametrize("light", [False, True], ids=["full", "light"])
@pytest.mark.parametrize("name", ["mixed", "edge4100"])
def test_variants_equal_the_expanded_arena(engine, g, alt, name, light):
    import torch
    S, T, span = alt(name), alt.templates, alt.gen.ALT_SPAN
    assert span == 4 and sorted({len(h) for h in S.holes}) == [0, 11, 12, 13]
    assert any(a == e for a, e in zip(S.off, S.off[1:])) and (name != "edge4100" or {2048, 4096} <= set(S.off))
    power, flag, thr = _drawn_votes(name, S.off)
    j = g.judge(S.off, power, flag, thr, g.LIGHT if light else g.FULL, S.codes)
    D = Items(S.vks, S.sigs, S.holes, power, flag, alt=S.alt)
    seed = random.Random("alt%s%d" % (name, light)).randbytes(32)
    # the arena edc_tmpl_expand_device builds from the per-item template array
    cap = S.n * (max(map(len, T.heads)) + max(map(len, T.tails))) + D.var_bytes + 16      # the entry's own bound
    d_tpl = torch.tensor(S.tpl, dtype=torch.int16, device="cuda:0")
    d_msg, d_off = torch.zeros(cap, dtype=torch.uint8, device="cuda:0"), torch.zeros(S.n + 1, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    engine.tmpl_expand_device(T, S.n, d_tpl.data_ptr(), D.var.data_ptr(), D.voff.data_ptr(), D.var_bytes, d_msg.data_ptr(), cap,
                              d_off.data_ptr())
    want = engine.quorum_verify_device(S.off, D.vk, D.sig, d_msg, d_off, D.power, D.flag, thr, seed, light=light)
    _same(want, j)
    got = _tq(engine, T, S.off, S.commit_tpl, D, thr, seed, light, span=span)
    _same(got, j)
    _equal(got, want)
    got = engine.quorum_verify_templated(T, S.off, S.commit_tpl, S.sigs, S.holes, power, flag, thr, seed, light=light,
                                         alt_span=span, item_alt=S.alt, vks=S.vks)
    _equal(got, want)
    assert engine.tmpl_quorum_last()[3] == sum(len(S.msgs[i]) for i, c in enumerate(j["checked"]) if c)


# ---- 3: gather boundaries ----

class Boundary:
    """5 tiles and a part of one, four commits (one empty); 3 templates, one with an empty head and
    one with an empty tail; hole lengths 0..17 with runs of empty holes; signed here."""
    SIZES = [300, 0, 500, 517]

    def __init__(self, engine, edc):
        rnd = random.Random("boundary")
        self.off = _offsets(self.SIZES)
        self.n = n = self.off[-1]
        assert n == 5 * W + 37
        self.T = edc.batch.Templates([b"", rnd.randbytes(37), rnd.randbytes(5)], [rnd.randbytes(21), b"", rnd.randbytes(64)])
        self.ctpl = [0, 2, 1, 2]
        self.tpl = [self.ctpl[c] for c, (a, e) in enumerate(zip(self.off, self.off[1:])) for _ in range(a, e)]
        lens = [0 if 40 <= i < 75 or 250 <= i < 262 or i >= n - 3 else (i * 7) % 18 for i in range(n)]
        assert set(lens) == set(range(18))
        self.holes = [rnd.randbytes(k) for k in lens]
        self.msgs = self.T.materialize(self.tpl, self.holes)
        seeds = [rnd.randbytes(32) for _ in range(9)]
        self.vks, self.sigs = engine.sign(seeds, self.msgs, seed_index=[i % 9 for i in range(n)])
        self.power = [1 + (i * 13) % 50 for i in range(n)]

    def flags(self, m):
        """m checked votes (full mode: flag 1 or 2): the first and the last item of the set, none of
        tile 2, the runs of empty holes as far as m reaches."""
        n = self.n
        if m == n:
            return [1 + (i % 5 == 0) for i in range(n)]
        pick = ([0, n - 1] if m >= 2 else [0])[:m]
        rest = [i for i in range(40, 75)] + [i for i in range(250, 262)] + [n - 2, n - 3]
        rnd = random.Random(m)
        more = [i for i in range(1, n - 3) if not 2 * W <= i < 3 * W and i not in rest]
        rnd.shuffle(more)
        pick = (pick + rest + more)[:m]
        assert len(set(pick)) == m
        flag = [0] * n
        for i in pick:
            flag[i] = 1 + (i % 5 == 0)
        return flag


@pytest.fixture(scope="module")
def boundary(engine, edc):
    pytest.importorskip("torch")
    return Boundary(engine, edc)


@pytest.mark.parametrize("m", [0, 1, 255, 256, 257, 513, 5 * W + 37])
def test_gather_boundaries(engine, boundary, m):
    B = boundary
    flag = B.flags(m)
    assert sum(1 for f in flag if f) == m
    if 2 <= m < B.n:
        assert flag[0] and flag[-1] and not any(flag[2 * W:3 * W])
    if 47 <= m < B.n:
        assert all(flag[40:75]) and all(flag[250:262])
    thr = [sum(B.power[a:e]) // 3 for a, e in zip(B.off, B.off[1:])]
    sigs = list(B.sigs)
    if m == 257:                                                # a bad checked vote: the codes go back through idx
        bad = max(i for i in range(B.n - 1) if flag[i])
        sigs[bad] = sigs[bad][:5] + bytes([sigs[bad][5] ^ 1]) + sigs[bad][6:]
    D = Items(B.vks, sigs, B.holes, B.power, flag)
    seed = random.Random("b%d" % m).randbytes(32)
    want = _ref(engine, B.off, D, B.msgs, thr, seed, False)
    assert want["n_checked"] == m and (want["code"] == 1) == (m == 257)
    got = _tq(engine, B.T, B.off, B.ctpl, D, thr, seed, False)
    _equal(got, want)
    checked = [i for i, f in enumerate(flag) if f]
    assert engine.tmpl_quorum_last() == (B.n, m, m, sum(len(B.msgs[i]) for i in checked))
    got = engine.quorum_verify_templated(B.T, B.off, B.ctpl, sigs, B.holes, B.power, flag, thr, seed, light=False, vks=B.vks)
    _equal(got, want)


# ---- 4: unchecked bytes never matter ----

def test_unchecked_bytes_never_matter(engine, g, qsets):
    Q, T = qsets("mixed_a"), qsets.templates
    S = Q.S
    j = Q.expect(g, g.LIGHT)
    seed = random.Random("noise").randbytes(32)
    D = Items(Q.vks, Q.sigs, S.holes, Q.power, Q.flag)
    clean = _tq(engine, T, Q.off, S.commit_tpl, D, Q.thr, seed, True)
    _same(clean, j)
    rnd = random.Random("noise2")
    vks, sigs, holes = list(Q.vks), list(Q.sigs), list(S.holes)
    unchecked = [i for i, c in enumerate(j["checked"]) if not c]
    assert 1000 < len(unchecked) < Q.n
    for i in unchecked:
        vks[i], sigs[i] = rnd.randbytes(32), rnd.randbytes(64)
        holes[i] = rnd.randbytes(len(holes[i]))
        if Q.flag[i] == 0:                                      # absent: empty, or noise of another length
            holes[i] = b"" if i % 2 else rnd.randbytes(1 + i % 23)
    N = Items(vks, sigs, holes, Q.power, Q.flag)
    _equal(_tq(engine, T, Q.off, S.commit_tpl, N, Q.thr, seed, True), clean)
    _equal(engine.quorum_verify_templated(T, Q.off, S.commit_tpl, sigs, holes, Q.power, Q.flag, Q.thr, seed, vks=vks), clean)


# ---- 6: argument errors ----

def test_argument_errors_leave_the_context_usable(engine, edc, g, qsets):
    import torch
    Q, T = qsets("valid"), qsets.templates
    S = Q.S
    j = Q.expect(g, g.LIGHT)
    rnd = random.Random("tqargs")
    D = Items(Q.vks, Q.sigs, S.holes, Q.power, Q.flag)
    voff = _offsets([len(h) for h in S.holes])
    absent = next(i for i, f in enumerate(Q.flag) if f == 0 and i > W)
    unchecked = next(i for i, c in enumerate(j["checked"]) if not c and Q.flag[i] == 1)
    alt1 = [0] * Q.n
    alt1[absent] = 1                                            # >= alt_span = 1, at an absent item
    down = list(voff)
    down[unchecked + 1] = down[unchecked] - 1                   # decreasing at an item light mode leaves out
    flag3, big = list(Q.flag), list(Q.power)
    flag3[absent] = 3
    big[unchecked] = 2**63
    cases = [("alt", dict(d_item_alt=_up(bytes(alt1)))), ("down", dict(d_var_off=_i32(down))),
             ("past", dict(var_bytes=D.var_bytes - 1)), ("flag", dict(d_flag=_up(bytes(flag3)))),
             ("power", dict(d_power=QuorumSet.dev_power(big)))]
    torch.cuda.synchronize()
    for what, kw in cases:
        for light in (True, False):
            with pytest.raises(edc.EngineError, match="edc error -2"):
                _tq(engine, T, Q.off, S.commit_tpl, D, Q.thr, rnd.randbytes(32), light, **kw)
        _same(_tq(engine, T, Q.off, S.commit_tpl, D, Q.thr, rnd.randbytes(32), True), j)       # the context still works
    # the host form refuses the same inputs, and what only it can be given
    def host(**kw):
        a = dict(power=Q.power, flag=Q.flag, ctpl=S.commit_tpl, span=1, item_alt=None, var_off=None, vks=Q.vks, key_idx=None)
        a.update(kw)
        return engine.quorum_verify_templated(T, Q.off, a["ctpl"], Q.sigs, S.holes, a["power"], a["flag"], Q.thr,
                                              rnd.randbytes(32), alt_span=a["span"], item_alt=a["item_alt"], vks=a["vks"],
                                              key_idx=a["key_idx"], var_off=a["var_off"])
    last = engine.tmpl_quorum_last()
    keys = list(dict.fromkeys(Q.vks))
    pos = {k: i for i, k in enumerate(keys)}
    engine.keycache_load(keys)
    try:
        idx = [pos[k] for k in Q.vks]
        outside = list(idx)
        outside[unchecked] = len(keys)
        window = [T.count - 1 if c == 3 else t for c, t in enumerate(S.commit_tpl)]
        for kw in (dict(item_alt=alt1), dict(var_off=down), dict(flag=flag3), dict(power=big), dict(key_idx=idx),
                   dict(vks=None), dict(vks=None, key_idx=outside), dict(span=2, ctpl=window), dict(span=0), dict(span=257)):
            with pytest.raises(edc.EngineError, match="edc error -2"):
                host(**kw)
        assert engine.tmpl_quorum_last() == last                # nothing reached the selection
        _same(host(vks=None, key_idx=idx), j)
    finally:
        engine.keycache_clear()
    # pointers, alignment, mode, nc = 0
    lib = engine.lib
    ts, _keep = T.struct()
    off = (ctypes.c_uint32 * (Q.nc + 1))(*Q.off)
    ctpl = (ctypes.c_uint16 * Q.nc)(*S.commit_tpl)
    thr = (ctypes.c_uint64 * Q.nc)(*Q.thr)
    seed = rnd.randbytes(32)

    def dev(nc=Q.nc, thr=thr, mode=1, seed=seed, power=D.power.data_ptr(), span=1):
        return lib.edc_tmpl_quorum_verify_device(engine.ctx, ctypes.byref(ts), nc, off, ctpl, span, None, D.vk.data_ptr(),
                                                 D.sig.data_ptr(), D.var.data_ptr(), D.voff.data_ptr(), D.var_bytes, power,
                                                 D.flag.data_ptr(), thr, mode, seed, None, None, None, None, None, None)
    assert dev(mode=2) == -2 and dev(seed=None) == -2 and dev(thr=None) == -2 and dev(span=T.count + 1) == -2
    assert dev(power=D.power.data_ptr() + 4) == -2
    assert dev(nc=0) == 0
    assert dev() == j["code"]


# ---- 7: invariance and hygiene ----

@pytest.mark.parametrize("grouping", [1, 2])
def test_independent_of_the_key_grouping(engine, g, qsets, grouping):
    Q, T = qsets("mixed_a"), qsets.templates
    D = Items(Q.vks, Q.sigs, Q.S.holes, Q.power, Q.flag)
    engine.set_key_grouping(grouping)
    try:
        for light in (False, True):
            got = _tq(engine, T, Q.off, Q.S.commit_tpl, D, Q.thr, random.Random(grouping * 2 + light).randbytes(32), light)
            _same(got, Q.expect(g, g.LIGHT if light else g.FULL))
    finally:
        engine.set_key_grouping(0)


def test_allocations_return(edc, g, qsets):
    Q, T = qsets("valid"), qsets.templates
    D = Items(Q.vks, Q.sigs, Q.S.holes, Q.power, Q.flag)
    before = edc.debug_live_allocs()
    eng = edc.Engine(0)
    try:
        with pytest.raises(edc.EngineError, match="edc error -2"):
            eng.tmpl_quorum_last()                              # before any templated quorum call
        j = Q.expect(g, g.LIGHT)
        _same(_tq(eng, T, Q.off, Q.S.commit_tpl, D, Q.thr, bytes(range(32)), True), j)
        _same(eng.quorum_verify_templated(T, Q.off, Q.S.commit_tpl, Q.sigs, Q.S.holes, Q.power, Q.flag, Q.thr, bytes(range(32)),
                                          vks=Q.vks), j)
        assert edc.debug_live_allocs() > before
    finally:
        eng.close()
    assert edc.debug_live_allocs() == before
