"""GPU: the validator-set history (include/edc.h, edc_vhist_*): the set kept as a base plus per-version
updates, every vote joined against the set of its commit's version, and the verify entries behind it.

Everything that is not a signature is judged by the pure-Python model of tests/golden/gen_vhist.py
(written from the header's definitions, on top of gen_valset.py and gen_quorum.py). The join is
driven through edc_vhist_resolve, which runs the kernels every form runs, at the shapes where it can
break: W below is the tile of the join kernel and of the selection (csrc/edc_launch.h, QR_TILE).
The signed votes are a few hundred made here with edc_sign; the verify entries are held to the
equality contract against edc_quorum_verify[_device] on the arrays joined by the model, and
against the validator-set entries on a history of one version."""
import random

import pytest

from test_vhist_abi import gen_vhist

pytestmark = pytest.mark.gpu

W = 256


@pytest.fixture(scope="module")
def g():
    return gen_vhist()


@pytest.fixture()
def eng(engine):
    """The shared engine, left without a key list."""
    yield engine
    engine.keycache_clear()


def _offsets(sizes):
    off = [0]
    for s in sizes:
        off.append(off[-1] + s)
    return off


def _history(rnd, g, m, nv, per_version=(2, 6), busy=None):
    """A random history: a quarter of the base absent, per version a handful of updates (a fifth of them
    leave the set); position `busy` changes at every version."""
    pw = lambda: g.NOT_MEMBER if rnd.randrange(5) == 0 else rnd.randrange(1000)
    base = [g.NOT_MEMBER if rnd.randrange(4) == 0 else rnd.randrange(1000) for _ in range(m)]
    updates = []
    for v in range(nv):
        ps = rnd.sample(range(m), rnd.randrange(*per_version))
        if busy is not None and busy not in ps:
            ps.append(busy)
        updates.append([(p, 1000 + v if p == busy else pw()) for p in ps])
    return base, updates


def _register(engine, g, keys, base, updates):
    engine.keycache_load(keys)
    h = g.from_updates(keys, base, updates)
    assert engine.vhist_set(base, updates) == h["nv"] + 1 == engine.vhist_versions()
    assert engine.vhist_totals() == (h["total"], h["members"])
    return h


def _resolve_agrees(engine, g, keys, h, off, ver, flag, thr, vks=None, key_idx=None):
    for mode in (g.FULL, g.LIGHT):
        want = g.plan(keys, h, off, ver, flag, thr, mode, vks=vks, key_idx=key_idx)
        got = engine.vhist_resolve(off, ver, flag, thr, light=mode == g.LIGHT, vks=vks, key_idx=key_idx)
        for key in ("pos", "power", "flag", "planned", "n_checked", "dv", "checked"):
            assert got[key] == want[key], (key, mode, off[:6], [i for i, (a, b) in enumerate(zip(got[key], want[key])) if a != b][:10]
                                           if isinstance(want[key], list) else (got[key], want[key]))
    return want


# ---------------------------------------------------------------- edc_vhist_set
def test_set_refusals_leave_the_history(eng, edc, g):
    rnd = random.Random("vhist refusals")
    N = g.NOT_MEMBER
    keys = [rnd.randbytes(32) for _ in range(5)]
    eng.keycache_clear()
    assert eng.vhist_versions() == 0
    with pytest.raises(edc.EngineError, match="edc error -2"):
        eng.vhist_set([1, 2, 3, 4, 5])                                         # no list
    assert eng.vhist_set(None) == 0                                            # m = 0, NULL: clears, also without a list
    with pytest.raises(edc.EngineError, match="edc error -2"):
        eng.vhist_totals(0, 1)
    eng.keycache_load(keys)
    with pytest.raises(edc.EngineError, match="edc error -2"):                 # no history yet: resolve is refused
        eng.vhist_resolve([0, 1], [0], [1], [0], vks=keys[:1])
    base, updates = [5, N, 7, 0, 9], [[(1, 4)], [], [(0, N), (3, 2)]]
    h = _register(eng, g, keys, base, updates)
    off, ver, flag, thr = [0, 5, 10, 15, 20], [3, 0, 1, 2], [1] * 20, [10] * 4
    before = _resolve_agrees(eng, g, keys, h, off, ver, flag, thr, vks=keys * 4)
    lib = eng.lib

    def raw(m, b, uoff, upos, upw):
        import ctypes
        arr = lambda t, x: (t * max(len(x), 1))(*x)
        return lib.edc_vhist_set(eng.ctx, m, arr(ctypes.c_uint64, b), max(len(uoff) - 1, 0), arr(ctypes.c_uint32, uoff) if uoff else None,
                                 arr(ctypes.c_uint32, upos), arr(ctypes.c_uint64, upw))
    bad = {"length": (4, [1] * 4, [], [], []), "length+": (6, [1] * 6, [], [], []),
           "offsets": (5, [1] * 5, [1, 1], [0], [1]), "offsets2": (5, [1] * 5, [0, 2, 1], [0, 1], [1, 1]),
           "position": (5, [1] * 5, [0, 1], [5], [1]), "twice": (5, [1] * 5, [0, 2], [3, 3], [1, 2]),
           "power": (5, [1, 2**63, 1, 1, 1], [], [], []), "power upd": (5, [1] * 5, [0, 1], [0], [2**64 - 2]),
           "sum": (5, [2**62, 2**62, N, N, N], [], [], []), "sum upd": (5, [2**62, 2**62 - 1, N, N, N], [0, 0, 1], [4], [1]),
           "count": (5, [1] * 5, [0, 2**32 - 5], [], [])}
    for name, (m, b, uoff, upos, upw) in bad.items():
        assert isinstance(g.build(keys, m, b, uoff, upos, upw), str), name
        assert raw(m, b, uoff, upos, upw) == -2, name
        assert eng.vhist_versions() == 4 and eng.vhist_totals() == (h["total"], h["members"]), name      # nothing changed
    assert _resolve_agrees(eng, g, keys, h, off, ver, flag, thr, vks=keys * 4) == before
    assert raw(5, [2**62, 2**62 - 1, N, N, 0], [0, 2], [4, 0], [2**62, N]) == 0        # a slice that only passes 2^63 on its way
    assert eng.vhist_totals() == ([2**63 - 1] * 2, [3, 2])
    h = _register(eng, g, keys, base, updates)
    # the history is independent of edc_valset_set_powers, and the validator-set entries never read it
    assert eng.valset_size() == 0
    eng.valset_set_powers([1, 1, 1, 1, 1])
    assert eng.valset_resolve([0, 5], [1] * 5, [0], vks=keys)["power"] == [1] * 5
    assert _resolve_agrees(eng, g, keys, h, off, ver, flag, thr, vks=keys * 4) == before
    # a key added to the cache is not a member at any version; the history stays
    extra = rnd.randbytes(32)
    eng.keycache_add([extra] + [rnd.randbytes(32) for _ in range(40)])         # the cache's arrays grow past the history's
    assert eng.vhist_versions() == 4
    want = _resolve_agrees(eng, g, keys, h, [0, 3, 6], [0, 3], [1, 1, 2] * 2, [0, 0], vks=[keys[1], extra, keys[0]] * 2)
    assert want["pos"] == [g.NO_POS, g.NO_POS, 0, 1, g.NO_POS, g.NO_POS] and want["flag"] == [0, 0, 2, 1, 0, 0]
    # a list with a repeated key is no validator set; a new list drops the history
    eng.keycache_load(keys + keys[:1])
    assert eng.vhist_versions() == 0
    with pytest.raises(edc.EngineError, match="edc error -2"):
        eng.vhist_set([1, 2, 3, 4, 5, 6])
    eng.keycache_load(keys)
    assert eng.vhist_versions() == 0
    eng.vhist_set(base, updates)
    assert eng.vhist_set(None) == 0
    eng.vhist_set(base, updates)
    eng.keycache_clear()
    assert eng.vhist_versions() == 0


# ---------------------------------------------------------------- the join against the model
def _votes(rnd, keys, n, by_position, strangers):
    """Signers over `keys`: by position every one is in the list; by key about a third are not (keys
    added to the cache afterwards, a listed key with one bit flipped, noise)."""
    who = [rnd.randrange(len(keys)) for _ in range(n)]
    flag = [rnd.choice([0, 2, 1, 1, 1, 1, 1, 1]) for _ in range(n)]
    if by_position:
        return dict(key_idx=who), flag
    vks = []
    for w in who:
        r = rnd.randrange(9)
        flip = bytearray(keys[w])
        flip[rnd.randrange(32)] ^= 1 << rnd.randrange(8)
        vks.append(rnd.choice(strangers) if r == 0 else bytes(flip) if r == 1 else rnd.randbytes(32) if r == 2 else keys[w])
    return dict(vks=vks), flag


def _join_of(g, keys, h, off, ver, flag, signer, c):
    """the joined arrays of commit c"""
    return [x[off[c]:off[c + 1]] for x in g.resolve(keys, h, off, ver, flag, **signer)]


def _differs(g, keys, h, off, ver, flag, signer):
    """Per commit: does the join differ from the join at version 0, and from the join at the
    neighbouring commit's version? Asserted on the model, so it holds without a GPU too."""
    def at(versions):
        pos, power, fl = g.resolve(keys, h, off, versions, flag, **signer)
        return [(pos[a:e], power[a:e], fl[a:e]) for a, e in zip(off, off[1:])]
    nc = len(ver)
    own, base = at(ver), at([0] * nc)
    nb = at([ver[c + 1] if c + 1 < nc else ver[c - 1] for c in range(nc)])
    return [own[c] != base[c] for c in range(nc)], [own[c] != nb[c] for c in range(nc)]


# commits that end at item 255 / 511 and start at 256 / 512 with other versions, empty commits
# carrying a third version between them, leading and trailing empty commits
EDGES = dict(sizes=[0, 100, 156, 0, 0, 144, 112, 0, 18, 70, 0], ver=[5, 30, 7, 19, 19, 3, 3, 11, 30, 0, 2])


def _layout(rnd, name, nv):
    if name == "edges":
        off = _offsets(EDGES["sizes"])
        assert off[3] == W and off[5] == W and off[7] == 2 * W and off[8] == 2 * W and off[-1] == 600
        return off, [nv if v == 30 else v for v in EDGES["ver"]]
    while True:             # 36 commits of 0..40 items, one of which straddles each tile edge
        sizes = [rnd.choice([0, 3, 11, 20, 27, 40]) for _ in range(36)]
        off = _offsets(sizes)
        if all(any(a < t < e for a, e in zip(off, off[1:])) for t in (W, 2 * W)) and off[-1] <= 640:
            break
    ver = [rnd.randrange(nv + 1) for _ in sizes]
    ver[3:6] = [nv, nv - 1, nv - 1]                                                 # the last version; descending, repeated
    ver[8:11] = [9, 4, 0]
    return off, ver


@pytest.mark.parametrize("layout", ["edges", "random"])
@pytest.mark.parametrize("hist", ["random", "long"])
def test_resolve_against_the_model(eng, g, hist, layout):
    rnd = random.Random("vhist join %s %s" % (hist, layout))
    m = 40
    keys = [rnd.randbytes(32) for _ in range(m)]
    # "long": position 0 changes at every one of 70 versions, so its list has 71 entries
    nv = 30 if hist == "random" else 70
    base, updates = _history(rnd, g, m, nv, busy=None if hist == "random" else 0)
    h = _register(eng, g, keys, base, updates)
    strangers = [rnd.randbytes(32) for _ in range(4)]
    eng.keycache_add(strangers)                                        # known to the cache, members at no version
    off, ver = _layout(rnd, layout, nv)
    assert nv in ver and 0 in ver and ver != sorted(ver)
    for by_position in (False, True):
        signer, flag = _votes(rnd, keys, off[-1], by_position, strangers)
        if hist == "long":                                             # the long list at its first, middle and last versions
            assert h["off"][1] - h["off"][0] == 71
            a = off[[c for c in range(len(ver)) if off[c + 1] - off[c] >= 3][0]]
            for j in range(3):
                if by_position:
                    signer["key_idx"][a + j] = 0
                else:
                    signer["vks"][a + j] = keys[0]
            ver3 = [0, 35, 70]
        vs = ver
        for rep in range(3 if hist == "long" else 1):
            if hist == "long":
                c0 = [c for c in range(len(ver)) if off[c + 1] - off[c] >= 3][0]
                vs = list(ver)
                vs[c0] = ver3[rep]
            if layout == "random":
                differs0, differs1 = _differs(g, keys, h, off, vs, flag, signer)
                assert 2 * sum(differs0) >= len(vs) and 4 * sum(differs1) >= len(vs), (sum(differs0), sum(differs1), len(vs))
            else:                          # at the edges: the version of the commit on the other side, or of the empty ones, joins otherwise
                for c, other in ((2, 3), (2, 5), (5, 4), (5, 2), (6, 7), (6, 8), (8, 7), (8, 6)):
                    alt = list(vs)
                    alt[c] = vs[other]
                    assert _join_of(g, keys, h, off, vs, flag, signer, c) != _join_of(g, keys, h, off, alt, flag, signer, c), (c, other)
            total = max(h["total"])
            for thr in ([2 * total // 3] * len(vs), [0] * len(vs), [rnd.randrange(2000) for _ in vs]):
                want = _resolve_agrees(eng, g, keys, h, off, vs, flag, thr, **signer)
            if hist == "long":
                assert want["power"][a] == (1000 + ver3[rep] - 1 if ver3[rep] else (0 if base[0] == g.NOT_MEMBER else base[0]))
        if not by_position:
            assert g.NO_POS in want["pos"] and any(p != g.NO_POS for p in want["pos"])
    assert eng.vhist_resolve([0, 0, 0], [1, 2], [], [1, 2], vks=[]) == \
        {"pos": [], "power": [], "flag": [], "checked": [], "planned": [0, 0], "n_checked": 0, "dv": [0, 0]}
    assert eng.vhist_resolve([0], [], [], [], vks=[])["n_checked"] == 0                  # nc = 0


# ---------------------------------------------------------------- the signed sets
class Signed:
    """nc commits of `per` votes by distinct signers out of m keys, signed with edc_sign; a history of
    nv versions over them; flags mostly for the block."""

    def __init__(self, engine, g, name, m=40, nc=12, per=25, nv=8):
        rnd = random.Random("vhist signed " + name)
        self.seeds = [rnd.randbytes(32) for _ in range(m)]
        self.keys, _ = engine.sign(self.seeds, [b""] * m)
        self.off = _offsets([per] * nc)
        self.n, self.nc = nc * per, nc
        self.who = [w for _ in range(nc) for w in rnd.sample(range(m), per)]
        self.msgs = [b"vote %d " % i + rnd.randbytes(rnd.randrange(40)) for i in range(self.n)]
        self.vks, self.sigs = engine.sign([self.seeds[w] for w in self.who], self.msgs)
        assert self.vks == [self.keys[w] for w in self.who]
        self.ks = engine.challenge(self.vks, self.sigs, self.msgs)
        self.flag = [rnd.choice([0, 2, 1, 1, 1, 1, 1, 1]) for _ in range(self.n)]
        self.codes = [0] * self.n
        self.base, self.updates = _history(rnd, g, m, nv, per_version=(3, 8))
        self.ver = [rnd.randrange(nv + 1) for _ in range(nc)]
        self.ver[0], self.ver[1] = nv, 0
        self.h = g.from_updates(self.keys, self.base, self.updates)
        self.thr = [2 * self.h["total"][v] // 3 // 2 for v in self.ver]      # a third of the set: light mode leaves votes out
        self._dev = None

    def joined(self, g):
        return g.resolve(self.keys, self.h, self.off, self.ver, self.flag, vks=self.vks)

    def register(self, engine, g):
        _register(engine, g, self.keys, self.base, self.updates)

    def dev(self, g, joined=False):
        if self._dev is None or (joined and "power" not in self._dev):
            import numpy as np
            import torch

            def up(b):
                return torch.frombuffer(bytearray(b or b"\0"), dtype=torch.uint8).to("cuda:0")
            self._dev = {"vk": up(b"".join(self.vks)), "sig": up(b"".join(self.sigs)), "msg": up(b"".join(self.msgs)),
                         "off": torch.tensor(_offsets([len(x) for x in self.msgs]), dtype=torch.int64, device="cuda:0"),
                         "k": up(b"".join(self.ks)), "flag": up(bytes(self.flag))}
            if joined:                       # the comparator's inputs: the arrays joined by the model
                _, power, flag_out = self.joined(g)
                self._dev["flag_out"] = up(bytes(flag_out))
                self._dev["power"] = torch.from_numpy(np.array(power, dtype=np.uint64).view(np.int64)).to("cuda:0")
            torch.cuda.synchronize()
        return self._dev

    def judge(self, g, mode):
        return g.judge(self.keys, self.h, self.off, self.ver, self.flag, self.thr, mode, self.codes, vks=self.vks)

    def forge(self, i):
        """flip a bit of item i's s: Item::verify_single says 1"""
        s = bytearray(self.sigs[i])
        s[40] ^= 1
        self.sigs[i] = bytes(s)
        self.codes[i] = 1
        self._dev = None

    def run(self, engine, g, form, seed, light, entry="vhist"):
        """form: device | device_k | host | host_k | host_idx. entry: vhist, valset (no versions), or
        quorum (the comparator of the equality contract, on the arrays joined by the model)."""
        pre = form.endswith("_k")
        ver = [self.ver] if entry == "vhist" else []
        if form.startswith("device"):
            D = self.dev(g, joined=entry == "quorum")
            items = (D["vk"], D["sig"], None if pre else D["msg"], None if pre else D["off"])
            kw = dict(light=light, d_k=D["k"] if pre else None)
            if entry == "quorum":
                return engine.quorum_verify_device(self.off, *items, D["power"], D["flag_out"], self.thr, seed, **kw)
            fn = engine.quorum_verify_vhist_device if entry == "vhist" else engine.quorum_verify_valset_device
            return fn(self.off, *ver, *items, D["flag"], self.thr, seed, **kw)
        kw = dict(light=light, **(dict(key_idx=self.who) if form == "host_idx" else dict(vks=self.vks)),
                  **(dict(ks=self.ks) if pre else dict(msgs=self.msgs)))
        if entry == "quorum":
            _, power, flag_out = self.joined(g)
            return engine.quorum_verify(self.off, self.sigs, power, flag_out, self.thr, seed, **kw)
        fn = engine.quorum_verify_vhist if entry == "vhist" else engine.quorum_verify_valset
        return fn(self.off, *ver, self.sigs, self.flag, self.thr, seed, **kw)


FORMS = ["device", "device_k", "host", "host_k", "host_idx"]


def _same(got, j):
    """A verify call's dict against the model's."""
    for key in ("code", "commit_verdicts", "tally", "n_bad_commits", "n_checked"):
        assert got[key] == j[key], key
    assert got["item_verdicts"] == j["item_verdicts"], [i for i, (a, b) in enumerate(zip(got["item_verdicts"], j["item_verdicts"])) if a != b][:10]


def _equal_but_double_votes(got, ref, dv):
    """The equality contract: every output of the quorum entry, but for the commits with a double vote."""
    for key in ("item_verdicts", "tally", "n_checked", "check8"):
        assert got[key] == ref[key], key
    assert [v for v, d in zip(got["commit_verdicts"], dv) if not d] == [v for v, d in zip(ref["commit_verdicts"], dv) if not d]
    assert all(v == 4 for v, d in zip(got["commit_verdicts"], dv) if d)
    if not any(dv):
        assert (got["code"], got["n_bad_commits"]) == (ref["code"], ref["n_bad_commits"])


@pytest.fixture(scope="module")
def signed(engine, g):
    pytest.importorskip("torch")
    return Signed(engine, g, "contract")


@pytest.mark.parametrize("light", [False, True], ids=["full", "light"])
def test_equality_contract(eng, g, signed, light):
    """Every form against the model and against the quorum entries on the joined arrays, check8 included."""
    S, mode = signed, g.LIGHT if light else g.FULL
    S.register(eng, g)
    j = S.judge(g, mode)
    pos, power, flag_out = S.joined(g)
    assert g.NO_POS in pos and not any(j["dv"]) and 1 not in j["commit_verdicts"] and 0 < j["n_checked"] < S.n
    assert light == (j["n_checked"] < sum(1 for f in flag_out if f))
    for form in FORMS:
        seed = bytes([len(form) + light]) * 32
        got = S.run(eng, g, form, seed, light)
        _same(got, j)
        ref = S.run(eng, g, "device" if form == "host_idx" else form, seed, light, entry="quorum")
        _equal_but_double_votes(got, ref, j["dv"])
        assert got["check8"] == ref["check8"] == bytes([1]) + bytes(31)


@pytest.mark.parametrize("light", [False, True], ids=["full", "light"])
def test_one_version_equals_the_validator_set_entries(eng, g, light):
    """nv = 0 and an all-member base: every output is edc_valset_quorum_verify[_device]'s, double votes included."""
    S = Signed(eng, g, "one version", m=30, nc=6, per=20, nv=0)
    S.base = [1 + (7 * p) % 50 for p in range(30)]
    S.h, S.ver = g.from_updates(S.keys, S.base, []), [0] * S.nc
    S.thr = [sum(S.base) // 3] * S.nc
    # a double vote in commit 2: item 41 becomes a second vote of item 40's signer
    for arr in (S.who, S.vks, S.sigs, S.msgs, S.ks):
        arr[41] = arr[40]
    S.flag[40], S.flag[41] = 1, 2 - light          # full: commit + nil; light: two votes for the block before the quorum
    S.thr[2] = 2**62
    S.register(eng, g)
    eng.valset_set_powers(S.base)
    j = S.judge(g, g.LIGHT if light else g.FULL)
    assert j["dv"] == [0, 0, 1, 0, 0, 0] and j["code"] == 4
    for form in FORMS:
        seed = bytes([0x40 + len(form)]) * 32
        got = S.run(eng, g, form, seed, light)
        _same(got, j)
        assert got == S.run(eng, g, form, seed, light, entry="valset")


@pytest.mark.parametrize("light", [False, True], ids=["full", "light"])
def test_forgery_on_a_checked_vote_and_on_a_non_member(eng, g, light):
    S, mode = Signed(eng, g, "forgery"), g.LIGHT if light else g.FULL
    S.register(eng, g)
    clean = S.judge(g, mode)
    pos, _, _ = S.joined(g)
    # a vote whose signer is not a member at its commit's version (it is one at another): nothing changes
    out = next(i for i in range(S.n) if pos[i] == g.NO_POS and any(w != g.NOT_MEMBER for w in (s[S.who[i]] for s in S.h["states"])))
    S.forge(out)
    S.flag[out] = 1
    j = S.judge(g, mode)
    assert j["item_verdicts"][out] == g.NOT_CHECKED and j["tally"] == clean["tally"]
    assert j["commit_verdicts"] == clean["commit_verdicts"] and 1 not in j["commit_verdicts"]
    for form in ("device", "host_k"):
        _same(S.run(eng, g, form, bytes([9]) * 32, light), j)
    # a checked vote: its commit is invalid, the codes and the tally are exact
    hit = next(i for i in range(S.n) if clean["item_verdicts"][i] == 0 and S.flag[i] == 1)
    S.forge(hit)
    j = S.judge(g, mode)
    c = next(c for c in range(S.nc) if S.off[c] <= hit < S.off[c + 1])
    assert j["code"] == 1 and j["commit_verdicts"][c] == 1 and j["item_verdicts"][hit] == 1 and j["n_bad_commits"] >= 1
    assert j["tally"][c] == clean["tally"][c] - S.h["states"][S.ver[c]][S.who[hit]]
    for form in FORMS:
        seed = bytes([0x70 + len(form)]) * 32
        got = S.run(eng, g, form, seed, light)
        _same(got, j)
        ref = S.run(eng, g, "device" if form == "host_idx" else form, seed, light, entry="quorum")
        _equal_but_double_votes(got, ref, j["dv"])


def test_double_votes_by_version(eng, edc, g):
    """The same key twice among the votes of commit A, at whose version it is not a member, and of
    commit B, where it is one. Light: the second vote after the quorum raises nothing (commit C)."""
    N = g.NOT_MEMBER
    seeds = [bytes([i + 1]) * 32 for i in range(5)]
    keys, _ = eng.sign(seeds, [b""] * 5)
    base, updates = [5, 5, N, 7, 3], [[(2, 9)], [(2, 1)]]
    eng.keycache_load(keys)
    eng.vhist_set(base, updates)
    h = g.from_updates(keys, base, updates)
    who = [0, 2, 2, 1] * 3
    off, ver = [0, 4, 8, 12], [0, 1, 2]
    msgs = [b"height %d" % i for i in range(12)]
    vks, sigs = eng.sign([seeds[w] for w in who], msgs)
    # light: A ignores the stranger-at-v0; B (5 + 9 = 14 <= 14: the second vote is checked) is a double
    # vote; C (5 + 1 = 6 > 5: the second vote comes after the quorum) is none
    flag, thr = [1] * 12, [4, 14, 5]
    j = g.judge(keys, h, off, ver, flag, thr, g.LIGHT, [0] * 12, vks=vks)
    assert j["dv"] == [0, 1, 0] and j["commit_verdicts"] == [0, 4, 0] and j["code"] == 4
    assert j["item_verdicts"] == [0, 255, 255, 255, 0, 0, 0, 255, 0, 0, 255, 255]
    _same(eng.quorum_verify_vhist(off, ver, sigs, flag, thr, bytes([5]) * 32, light=True, vks=vks, msgs=msgs), j)
    _same(eng.quorum_verify_vhist(off, ver, sigs, flag, thr, bytes([5]) * 32, light=True, key_idx=who, msgs=msgs), j)
    # full: commit + nil from one validator
    flag, thr = [1, 1, 2, 1] * 3, [9, 9, 9]
    j = g.judge(keys, h, off, ver, flag, thr, g.FULL, [0] * 12, vks=vks)
    assert j["dv"] == [0, 1, 1] and j["commit_verdicts"] == [0, 4, 4] and j["code"] == 4
    assert j["item_verdicts"] == [0, 255, 255, 0] + [0] * 8 and j["tally"] == [10, 19, 11]
    got = eng.quorum_verify_vhist(off, ver, sigs, flag, thr, bytes([6]) * 32, light=False, vks=vks, msgs=msgs)
    _same(got, j)
    res = eng.vhist_resolve(off, ver, flag, thr, light=False, vks=vks)
    assert res["dv"] == [0, 1, 1] and res["pos"][:4] == [0, g.NO_POS, g.NO_POS, 1]
    # batch.verify_quorum(powers=None, versions=...) takes the same path
    vs = []
    for c in range(3):
        v = edc.batch.Verifier(eng)
        for i in range(off[c], off[c + 1]):
            v.queue((vks[i], sigs[i], msgs[i]))
        vs.append(v)
    verdicts, tally, codes = edc.batch.verify_quorum(vs, None, [flag[a:e] for a, e in zip(off, off[1:])], thr, light=False,
                                                     engine=eng, versions=ver)
    assert (verdicts, tally) == (j["commit_verdicts"], j["tally"]) and [x for c in codes for x in c] == j["item_verdicts"]


def test_argument_errors_leave_the_context_usable(eng, edc, g):
    S = Signed(eng, g, "errors", m=10, nc=3, per=8, nv=4)
    seed = bytes([3]) * 32
    eng.keycache_load(S.keys)
    for form in ("device", "host"):                                            # no history
        with pytest.raises(edc.EngineError, match="edc error -2"):
            S.run(eng, g, form, seed, True)
    S.register(eng, g)
    j = S.judge(g, g.LIGHT)
    good = list(S.ver)
    S.ver = [good[0], 5, good[2]]                                              # a version past the last
    for form in ("device", "host", "host_idx"):
        with pytest.raises(edc.EngineError, match="edc error -2"):
            S.run(eng, g, form, seed, True)
    with pytest.raises(edc.EngineError, match="edc error -2"):
        eng.vhist_resolve(S.off, S.ver, S.flag, S.thr, vks=S.vks)
    S.ver = good
    _same(S.run(eng, g, "host", seed, True), j)
    pos, _, _ = S.joined(g)
    flags = list(S.flag)
    for i in (next(i for i in range(S.n) if pos[i] == g.NO_POS), next(i for i in range(S.n) if pos[i] != g.NO_POS)):
        S.flag, S._dev = list(flags), None
        S.flag[i] = 3                                                          # a flag above 2, on a non-member and on a member
        for form in ("device", "host_k"):
            with pytest.raises(edc.EngineError, match="edc error -2"):
                S.run(eng, g, form, seed, True)
    S.flag, S._dev = flags, None
    for form in FORMS:
        _same(S.run(eng, g, form, seed, True), j)


def test_allocations_return(edc, g):
    before = edc.debug_live_allocs()
    e2 = edc.Engine(0)
    try:
        S = Signed(e2, g, "leaks", m=10, nc=3, per=8, nv=4)
        S.register(e2, g)
        _same(S.run(e2, g, "host", bytes(range(32)), True), S.judge(g, g.LIGHT))
        _same(S.run(e2, g, "device_k", bytes(range(32)), False), S.judge(g, g.FULL))
        e2.vhist_set(S.base, S.updates[:2])
        assert edc.debug_live_allocs() > before
    finally:
        e2.close()
    assert edc.debug_live_allocs() == before
