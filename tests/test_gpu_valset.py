"""GPU: validator-set quorum commit sets (include/edc.h, edc_valset_*): the powers kept with the
registered key list, the join of every vote against it, the double-vote scan and the verify entries.

Everything that is not a signature is judged by the pure-Python model of tests/golden/gen_valset.py
(written from the header's definitions, on top of gen_quorum.py). The join and the scan are driven
through edc_valset_resolve, which runs the kernels every form runs, at the shapes where they can
break: W below is the tile of the selection and of both new kernels (csrc/edc_launch.h, QR_TILE).
The signed votes are the commit sets of commits.json (150 validator keys); the verify entries are
held to the equality contract against edc_quorum_verify[_device] on the arrays joined here."""
import ctypes
import random

import pytest

from conftest import golden
from test_gpu_commits import CommitSet, _gen as _gen_commits
from test_valset_abi import gen_valset

pytestmark = pytest.mark.gpu

W = 256
MAXP = 2**63 - 1


@pytest.fixture(scope="module")
def g():
    return gen_valset()


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


def _register(engine, keys, powers):
    engine.keycache_load(keys)
    assert engine.valset_set_powers(powers) == len(keys) == engine.valset_size()


def _flip(key, rnd):
    b = bytearray(key)
    b[rnd.randrange(32)] ^= 1 << rnd.randrange(8)
    return bytes(b)


def _resolve_agrees(engine, g, keys, powers, off, flag, thr, vks=None, key_idx=None):
    for mode in (g.FULL, g.LIGHT):
        want = g.plan(keys, powers, off, flag, thr, mode, vks=vks, key_idx=key_idx)
        got = engine.valset_resolve(off, flag, thr, light=mode == g.LIGHT, vks=vks, key_idx=key_idx)
        for key in ("pos", "power", "flag", "planned", "n_checked", "dv", "checked"):
            assert got[key] == want[key], (key, mode, off[:6], [i for i, (a, b) in enumerate(zip(got[key], want[key])) if a != b][:10]
                                           if isinstance(want[key], list) else (got[key], want[key]))
    return want


# ---------------------------------------------------------------- the powers
def test_set_powers_refusals(eng, edc, g):
    rnd = random.Random("powers")
    keys = [rnd.randbytes(32) for _ in range(5)]
    eng.keycache_clear()
    assert eng.valset_size() == 0
    with pytest.raises(edc.EngineError, match="edc error -2"):
        eng.valset_set_powers([1, 2, 3, 4, 5])                                 # no list
    assert eng.valset_set_powers(None) == 0                                    # m = 0, NULL: clears, also without a list
    eng.keycache_load(keys)
    for bad in ([1, 2, 3, 4], [1, 2, 3, 4, 5, 6], [1, 2, 2**63, 4, 5], [2**63 - 4, 1, 1, 1, 1]):
        assert not g.check_powers(keys, bad)
        with pytest.raises(edc.EngineError, match="edc error -2"):
            eng.valset_set_powers(bad)
        assert eng.valset_size() == 0                                          # nothing changed
    with pytest.raises(edc.EngineError, match="edc error -2"):                 # no powers yet: resolve is refused
        eng.valset_resolve([0, 1], [1], [0], vks=keys[:1])
    assert g.check_powers(keys, [2**63 - 5, 1, 1, 1, 1])
    assert eng.valset_set_powers([2**63 - 5, 1, 1, 1, 1]) == 5                 # a total of 2^63 - 1
    assert eng.valset_set_powers([1, 2, 3, 4, 5]) == 5
    with pytest.raises(edc.EngineError, match="edc error -2"):
        eng.valset_set_powers([1, 2, 3, 4, 2**63])
    want = _resolve_agrees(eng, g, keys, [1, 2, 3, 4, 5], [0, 5], [1] * 5, [9], vks=keys)      # the refused call changed nothing
    assert want["power"] == [1, 2, 3, 4, 5]
    # a key added to the cache is not a member; the members keep their powers
    extra = rnd.randbytes(32)
    eng.keycache_add([extra] + [rnd.randbytes(32) for _ in range(40)])         # the cache's arrays grow past the powers'
    assert eng.valset_size() == 5
    want = _resolve_agrees(eng, g, keys, [1, 2, 3, 4, 5], [0, 3], [1, 1, 2], [0], vks=[keys[3], extra, keys[0]])
    assert want["pos"] == [3, g.NO_POS, 0] and want["flag"] == [1, 0, 2]
    assert eng.valset_set_powers(None) == 0
    assert eng.valset_set_powers([1, 2, 3, 4, 5]) == 5
    # a list with a repeated key is no validator set; a new list drops the powers
    eng.keycache_load(keys + keys[:1])
    assert eng.valset_size() == 0
    with pytest.raises(edc.EngineError, match="edc error -2"):
        eng.valset_set_powers([1, 2, 3, 4, 5, 6])
    eng.keycache_load(keys)
    assert eng.valset_size() == 0
    with pytest.raises(edc.EngineError, match="edc error -2"):
        eng.valset_resolve([0, 1], [1], [0], key_idx=[0])
    eng.valset_set_powers([1, 2, 3, 4, 5])
    eng.keycache_clear()
    assert eng.valset_size() == 0


# ---------------------------------------------------------------- the join and the scan against the model
def _random_set(rnd, keys, off, by_position):
    """Votes over `keys`: by position every signer is a member; by key about a third are not (the
    all-zero key, a member's key with one bit flipped, noise). Repeated signers are frequent."""
    n = off[-1]
    who = [rnd.randrange(len(keys)) for _ in range(n)]
    flag = [rnd.choice([0, 2, 1, 1, 1, 1, 1, 1]) for _ in range(n)]
    if by_position:
        return dict(key_idx=who), flag
    vks = []
    for w in who:
        r = rnd.randrange(9)
        vks.append(bytes(32) if r == 0 else _flip(keys[w], rnd) if r == 1 else rnd.randbytes(32) if r == 2 else keys[w])
    return dict(vks=vks), flag


def _thresholds(rnd, powers, off, kind):
    total = sum(powers)
    return [2 * total // 3 if kind == "two_thirds" else 0 if kind == "zero" else rnd.randrange(total + 2) for _ in off[1:]]


@pytest.mark.parametrize("nkeys", [1, 150])
@pytest.mark.parametrize("sizes", [[1], [W - 1], [W], [W + 1], [2 * W + 1], [200, 100, 213], [W - 2, 4, W, 3]],
                         ids=lambda s: "-".join(map(str, s)))
def test_resolve_around_the_tile(eng, g, sizes, nkeys):
    """n = 1, 255, 256, 257, 513 and commits that straddle a tile edge; lists of 1 key and of 150."""
    rnd = random.Random("resolve%r%d" % (sizes, nkeys))
    keys = [rnd.randbytes(32) for _ in range(nkeys)]
    powers = [rnd.randrange(1000) for _ in keys]
    _register(eng, keys, powers)
    off = _offsets(sizes)
    for by_position in (False, True):
        signer, flag = _random_set(rnd, keys, off, by_position)
        for kind in ("two_thirds", "zero", "random"):
            want = _resolve_agrees(eng, g, keys, powers, off, flag, _thresholds(rnd, powers, off, kind), **signer)
        if not by_position and off[-1] >= W - 1:
            assert g.NO_POS in want["pos"] and any(p != g.NO_POS for p in want["pos"])
    if nkeys == 1 and off[-1] > 1:                               # one validator voting again and again
        assert any(eng.valset_resolve(off, flag, [0] * len(sizes), light=False, **signer)["dv"])


def test_resolve_many_tiny_commits(eng, g):
    """600 commits of 0..5 items with leading, trailing and consecutive empty commits."""
    sizes = list(_gen_commits().layout("tmap_small")["sizes"])
    sizes[300:303] = [0, 0, 0]
    assert len(sizes) == 600 and sizes[0] == sizes[-1] == 0 and max(sizes) == 5
    off = _offsets(sizes)
    rnd = random.Random("tiny")
    keys = [rnd.randbytes(32) for _ in range(6)]
    powers = [rnd.randrange(10) for _ in keys]
    _register(eng, keys, powers)
    for by_position in (False, True):
        signer, flag = _random_set(rnd, keys, off, by_position)
        for kind in ("two_thirds", "zero", "random"):
            want = _resolve_agrees(eng, g, keys, powers, off, flag, _thresholds(rnd, powers, off, kind), **signer)
        assert 10 < sum(want["dv"]) < 590
    assert eng.valset_resolve([0, 0, 0], [], [1, 2], vks=[]) == \
        {"pos": [], "power": [], "flag": [], "checked": [], "planned": [0, 0], "n_checked": 0, "dv": [0, 0]}
    assert eng.valset_resolve([0], [], [], vks=[])["n_checked"] == 0                    # nc = 0


def test_double_votes_of_the_fixture(eng, g):
    """The situations valset.json records, in both modes and both forms."""
    fx = golden("valset.json")["cases"]
    _register(eng, g.KEYS, g.POWERS)
    for name in g.CASES:
        off, vks, flag, thr, codes = g.case(name)
        forms = [dict(vks=vks)]
        if g.STRANGER not in vks:
            forms.append(dict(key_idx=[g.KEYS.index(v) for v in vks]))
        for signer in forms:
            _resolve_agrees(eng, g, g.KEYS, g.POWERS, off, flag, thr, **signer)
            for mode, label in ((g.FULL, "full"), (g.LIGHT, "light")):
                got = eng.valset_resolve(off, flag, thr, light=mode == g.LIGHT, **signer)
                for key in ("pos", "power", "flag", "checked", "planned", "dv", "n_checked"):
                    assert got[key] == fx[name][label][key], (name, label, key)
    # just before and just after the quorum is passed: dv = 1 and 0
    assert fx["second_before_quorum"]["light"]["dv"] == [1] and fx["second_after_quorum"]["light"]["dv"] == [0]


def test_double_votes_across_a_tile_edge(eng, g):
    rnd = random.Random("edge")
    keys = [rnd.randbytes(32) for _ in range(150)]
    powers = [1 + rnd.randrange(9) for _ in keys]
    _register(eng, keys, powers)
    # commit 1 holds the items [250, 262): its two votes of validator 7 are the last item of tile 0 and the first of tile 1
    off = [0, 250, 262, 262, 400]
    who = list(range(100, 150)) * 5 + list(range(12)) + list(range(138))
    assert len(who) == 400
    who[255] = who[256] = 7
    flag = [1] * 400
    thr = [2**62] * 4
    want = _resolve_agrees(eng, g, keys, powers, off, flag, thr, key_idx=who)
    assert want["dv"] == [1, 1, 0, 0]                            # commit 0 repeats its 50 validators, commit 3 has none twice
    who[:250] = list(range(150)) + list(range(100))              # the same validators in adjacent commits only
    who[255], who[256] = 20, 21
    want = _resolve_agrees(eng, g, keys, powers, off, flag, thr, vks=[keys[w] for w in who])
    assert want["dv"] == [1, 0, 0, 0]
    who[:250] = list(range(150)) + [200] * 100
    vks = [keys[w] if w < 150 else bytes([w]) * 32 for w in who]
    assert _resolve_agrees(eng, g, keys, powers, off, flag, thr, vks=vks)["dv"] == [0, 0, 0, 0]     # a non-member 100 times
    # three occurrences, two of them in the next tile, in the last commit that has items
    off = [0, 250, 262, 400, 400, 400]
    who = list(range(150)) + list(range(100)) + list(range(12)) + list(range(138))
    who[300] = who[262]
    who[399] = who[262]
    want = _resolve_agrees(eng, g, keys, powers, off, flag, [2**62] * 5, key_idx=who)
    assert want["dv"] == [1, 0, 1, 0, 0]


# ---------------------------------------------------------------- the signed sets
class ValSet:
    """A commit set of commits.json as votes of a validator set: the registered list is every
    distinct key but each `drop`-th (all of them when drop is 0, as the key_idx form needs), the
    flags are gen_quorum's with every vote after a member's first in its commit made absent (no
    double vote), then `copies`: item j becomes a copy of item i with flag 1 (a double vote)."""

    def __init__(self, name, S, g, drop, copies=(), thr_never=()):
        rnd = random.Random("valset" + name)
        self.S, self.off, self.n, self.nc = S, S.off, S.n, S.nc
        self.vks, self.sigs, self.ks, self.msgs, self.codes = list(S.vks), list(S.sigs), list(S.ks), list(S.msgs), list(S.codes)
        distinct = list(dict.fromkeys(S.vks))
        self.keys = [k for j, k in enumerate(distinct) if not (drop and j % drop == drop - 1)]
        bad_key = [S.vks[i] for i, c in enumerate(S.codes) if c == 2]
        self.keys += [k for k in bad_key if k not in self.keys]             # a registered key that does not decode stays a member
        self.powers = [1 + rnd.randrange(1000) for _ in self.keys]
        where = {k: p for p, k in enumerate(self.keys)}
        self.flag = list(g.Q.votes(name, S.off)[1])
        for a, e in zip(self.off, self.off[1:]):
            seen = set()
            for i in range(a, e):
                p = where.get(self.vks[i])
                if p in seen:
                    self.flag[i] = g.ABSENT
                elif p is not None and self.flag[i] != g.ABSENT:
                    seen.add(p)
        for i, j in copies:
            self.vks[j], self.sigs[j], self.ks[j], self.msgs[j], self.codes[j] = S.vks[i], S.sigs[i], S.ks[i], S.msgs[i], S.codes[i]
            self.flag[i] = self.flag[j] = g.COMMIT
        self.thr = [2 * sum(self.powers[p] for p in {where[v] for v in self.vks[a:e] if v in where}) // 3
                    for a, e in zip(self.off, self.off[1:])]
        for c in thr_never:
            self.thr[c] = 2**62
        self.key_idx = [where[v] for v in self.vks] if not drop else None
        self.pos, self.power, self.flag_out = g.resolve(self.keys, self.powers, self.flag, vks=self.vks)
        self._dev = None

    def register(self, engine):
        _register(engine, self.keys, self.powers)

    def dev(self):
        if self._dev is None:
            import numpy as np
            import torch

            def up(b):
                return torch.frombuffer(bytearray(b or b"\0"), dtype=torch.uint8).to("cuda:0")
            offs = _offsets([len(m) for m in self.msgs])
            self._dev = {"vk": up(b"".join(self.vks)), "sig": up(b"".join(self.sigs)), "msg": up(b"".join(self.msgs)),
                         "off": torch.tensor(offs, dtype=torch.int64, device="cuda:0"), "k": up(b"".join(self.ks)),
                         "flag": up(bytes(self.flag)), "flag_out": up(bytes(self.flag_out)),
                         "power": torch.from_numpy(np.array(self.power, dtype=np.uint64).view(np.int64)).to("cuda:0")}
            torch.cuda.synchronize()
        return self._dev

    def judge(self, g, mode):
        return g.judge(self.keys, self.powers, self.off, self.flag, self.thr, mode, self.codes, vks=self.vks)

    def device(self, engine, seed, light, prehashed=False):
        D = self.dev()
        return engine.quorum_verify_valset_device(self.off, D["vk"], D["sig"], None if prehashed else D["msg"],
                                                  None if prehashed else D["off"], D["flag"], self.thr, seed, light=light,
                                                  d_k=D["k"] if prehashed else None)

    def quorum_device(self, engine, seed, light):
        """The comparator of the equality contract: edc_quorum_verify_device on the arrays joined here."""
        D = self.dev()
        return engine.quorum_verify_device(self.off, D["vk"], D["sig"], D["msg"], D["off"], D["power"], D["flag_out"], self.thr,
                                           seed, light=light)


@pytest.fixture(scope="module")
def commit_sets(engine, oracle):
    pytest.importorskip("torch")
    gc, fxc = _gen_commits(), golden("commits.json")
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = CommitSet(name, engine, oracle, gc, fxc)
        return cache[name]
    return get


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


@pytest.mark.parametrize("light", [False, True], ids=["full", "light"])
@pytest.mark.parametrize("name", ["valid", "mixed_a"])
def test_equality_contract_without_double_votes(eng, g, commit_sets, name, light):
    """Every form against the model and against the quorum entries on the joined arrays, check8
    included. mixed_a holds bad signatures (the fallback runs) and a registered key that does not decode."""
    mode = g.LIGHT if light else g.FULL
    rnd = random.Random("eq%s%d" % (name, light))
    V = ValSet(name, commit_sets(name), g, drop=7)
    j = V.judge(g, mode)
    assert not any(j["dv"]) and g.NO_POS in V.pos and j["n_checked"] > 100
    if name == "mixed_a":
        assert j["code"] == 1 and 2 in V.codes and all(V.vks[i] in V.keys for i, c in enumerate(V.codes) if c == 2)
    V.register(eng)
    seed = rnd.randbytes(32)
    ref = V.quorum_device(eng, seed, light)
    _same(ref, {**j, "commit_verdicts": j["quorum_verdicts"], "code": j["quorum_code"]})
    for got in (V.device(eng, seed, light), V.device(eng, seed, light, prehashed=True),
                eng.quorum_verify_valset(V.off, V.sigs, V.flag, V.thr, seed, light=light, vks=V.vks, msgs=V.msgs),
                eng.quorum_verify_valset(V.off, V.sigs, V.flag, V.thr, seed, light=light, vks=V.vks, ks=V.ks)):
        _same(got, j)
        _equal_but_double_votes(got, ref, j["dv"])
    ref_host = eng.quorum_verify(V.off, V.sigs, V.power, V.flag_out, V.thr, seed, light=light, vks=V.vks, msgs=V.msgs)
    assert ref_host == ref
    # the key_idx form needs every signer in the list
    A = ValSet(name, commit_sets(name), g, drop=0)
    ja = A.judge(g, mode)
    assert not any(ja["dv"]) and g.NO_POS not in A.pos
    A.register(eng)
    ref = eng.quorum_verify(A.off, A.sigs, A.power, A.flag_out, A.thr, seed, light=light, key_idx=A.key_idx, msgs=A.msgs)
    for kw in (dict(msgs=A.msgs), dict(ks=A.ks)):
        got = eng.quorum_verify_valset(A.off, A.sigs, A.flag, A.thr, seed, light=light, key_idx=A.key_idx, **kw)
        _same(got, ja)
        _equal_but_double_votes(got, ref, ja["dv"])
    got = A.device(eng, seed, light)
    _same(got, ja)
    _equal_but_double_votes(got, ref, ja["dv"])


def _a_good_commit(V, g, lo=100):
    """A commit of at least `lo` items whose first two are signed votes of two members with code 0."""
    for c, (a, e) in enumerate(zip(V.off, V.off[1:])):
        if e - a >= lo and all(V.codes[i] == 0 for i in range(a, e)) and V.flag[a] == V.flag[a + 1] == g.COMMIT \
                and V.pos[a] != g.NO_POS and V.pos[a + 1] != g.NO_POS:
            return c
    raise AssertionError("no such commit")


@pytest.mark.parametrize("light", [False, True], ids=["full", "light"])
@pytest.mark.parametrize("name", ["valid", "mixed_a"])
def test_one_double_vote_commit(eng, g, commit_sets, name, light):
    """One commit whose second vote is a copy of its first, among good commits ("valid": the return
    value is 4) and with invalid commits elsewhere in the set ("mixed_a": 1 wins)."""
    mode = g.LIGHT if light else g.FULL
    S = commit_sets(name)
    base = ValSet(name, S, g, drop=7)
    c = _a_good_commit(base, g)
    a = S.off[c]
    V = ValSet(name, S, g, drop=7, copies=[(a, a + 1)])
    j, jb = V.judge(g, mode), base.judge(g, mode)
    assert j["dv"] == [int(x == c) for x in range(V.nc)] and j["commit_verdicts"][c] == 4 and j["quorum_verdicts"][c] == 0
    assert j["code"] == (1 if name == "mixed_a" else 4) and j["item_verdicts"][a:a + 2] == [0, 0]
    assert [v for x, v in enumerate(j["commit_verdicts"]) if x != c] == [v for x, v in enumerate(jb["commit_verdicts"]) if x != c]
    V.register(eng)
    seed = random.Random("dv%s%d" % (name, light)).randbytes(32)
    ref = V.quorum_device(eng, seed, light)
    for got in (V.device(eng, seed, light),
                eng.quorum_verify_valset(V.off, V.sigs, V.flag, V.thr, seed, light=light, vks=V.vks, ks=V.ks)):
        _same(got, j)
        _equal_but_double_votes(got, ref, j["dv"])
        assert got["n_bad_commits"] == ref["n_bad_commits"] + 1


def test_non_member_noise_changes_nothing(eng, g, commit_sets):
    """The vk, sig, message and k bytes of a non-member are never interpreted."""
    import torch
    V = ValSet("mixed_a", commit_sets("mixed_a"), g, drop=3)
    V.register(eng)
    rnd = random.Random("noise")
    seed = rnd.randbytes(32)
    strangers = [i for i, p in enumerate(V.pos) if p == g.NO_POS]
    assert len(strangers) > V.n // 5
    before = {light: (V.device(eng, seed, light), V.device(eng, seed, light, prehashed=True),
                      eng.quorum_verify_valset(V.off, V.sigs, V.flag, V.thr, seed, light=light, vks=V.vks, msgs=V.msgs))
              for light in (False, True)}
    _same(before[False][0], V.judge(g, g.FULL))
    for i in strangers:
        V.vks[i], V.sigs[i], V.ks[i] = rnd.randbytes(32), rnd.randbytes(64), b"\xff" * 32
        V.msgs[i] = rnd.randbytes(len(V.msgs[i]))
    V._dev = None
    assert all(p == g.NO_POS for p in g.resolve(V.keys, V.powers, V.flag, vks=[V.vks[i] for i in strangers])[0])
    for light in (False, True):
        after = (V.device(eng, seed, light), V.device(eng, seed, light, prehashed=True),
                 eng.quorum_verify_valset(V.off, V.sigs, V.flag, V.thr, seed, light=light, vks=V.vks, msgs=V.msgs))
        assert after == before[light]
        # a non-canonical k on a vote that is not checked is accepted by the host form as well
        assert eng.quorum_verify_valset(V.off, V.sigs, V.flag, V.thr, seed, light=light, vks=V.vks, ks=V.ks) == after[0]
    torch.cuda.synchronize()


def test_python_batch_surface(eng, edc, g, commit_sets):
    S = commit_sets("valid")
    c = max(range(S.nc), key=lambda c: (S.off[c + 1] - S.off[c]) if S.off[c + 1] - S.off[c] <= 150 else 0)
    a, e = S.off[c], S.off[c + 1]
    keys = list(dict.fromkeys(S.vks[a:e]))[:-3]                                # the last three signers are strangers
    powers = [3 + p for p in range(len(keys))]
    _register(eng, keys, powers)
    vs, flags = [], []
    for lo, hi in ((a, e), (a, a + 2)):
        v = edc.batch.Verifier()
        for i in list(range(lo, hi)) + ([lo] if hi - lo == 2 else []):          # the second commit repeats its first vote
            v.queue((S.vks[i], S.sigs[i], S.msgs[i]))
        vs.append(v)
        flags.append([1] * v.batch_size)
    thr = [2 * sum(powers) // 3, 2**62]
    verdicts, tally, codes = edc.batch.verify_quorum(vs, None, flags, thr, light=False, engine=eng)
    assert verdicts == [0, 4] and tally == [sum(powers), 2 * powers[0] + powers[1]]
    assert codes == [[0] * (e - a - 3) + [255] * 3, [0, 0, 0]]


# ---------------------------------------------------------------- argument errors
def test_argument_errors_leave_the_context_usable(eng, edc, g, commit_sets):
    import torch
    V = ValSet("valid", commit_sets("valid"), g, drop=7)
    j = V.judge(g, g.LIGHT)
    rnd = random.Random("args")
    D = V.dev()
    lib = eng.lib
    off = (ctypes.c_uint32 * (V.nc + 1))(*V.off)
    thr = (ctypes.c_uint64 * V.nc)(*V.thr)

    def raw_device(flag=None, seed=b"\x07" * 32, mode=1, nc=V.nc):
        """The device entry with sentinel-filled outputs -> (rc, whether any output was written)."""
        cv, iv = ctypes.create_string_buffer(b"\x77" * V.nc, V.nc), ctypes.create_string_buffer(b"\x77" * V.n, V.n)
        tl = (ctypes.c_uint64 * V.nc)(*([0x77] * V.nc))
        nb, cnt, c8 = ctypes.c_int(0x77), ctypes.c_size_t(0x77), ctypes.create_string_buffer(b"\x77" * 32, 32)
        rc = lib.edc_valset_quorum_verify_device(eng.ctx, nc, off, D["vk"].data_ptr(), D["sig"].data_ptr(), None, None,
                                                 D["k"].data_ptr(), (D["flag"] if flag is None else flag).data_ptr(), thr,
                                                 mode, seed, cv, iv, tl, ctypes.byref(nb), ctypes.byref(cnt), c8)
        clean = (cv.raw == b"\x77" * V.nc and iv.raw == b"\x77" * V.n and list(tl) == [0x77] * V.nc
                 and (nb.value, cnt.value) == (0x77, 0x77) and c8.raw == b"\x77" * 32)
        return rc, clean

    def works():
        _same(V.device(eng, rnd.randbytes(32), True, prehashed=True), j)
        _same(eng.quorum_verify_valset(V.off, V.sigs, V.flag, V.thr, rnd.randbytes(32), vks=V.vks, ks=V.ks), j)

    # no powers set
    eng.keycache_load(V.keys)
    assert raw_device() == (-2, True)
    for call in (lambda: V.device(eng, rnd.randbytes(32), True),
                 lambda: eng.quorum_verify_valset(V.off, V.sigs, V.flag, V.thr, rnd.randbytes(32), vks=V.vks, msgs=V.msgs),
                 lambda: eng.valset_resolve(V.off, V.flag, V.thr, vks=V.vks)):
        with pytest.raises(edc.EngineError, match="edc error -2"):
            call()
    V.register(eng)
    works()
    # a flag of 3 on a non-member, on the device
    stranger = V.pos.index(g.NO_POS)
    flag3 = list(V.flag)
    flag3[stranger] = 3
    d_flag3 = torch.frombuffer(bytearray(bytes(flag3)), dtype=torch.uint8).to("cuda:0")
    for mode in (0, 1):
        assert raw_device(flag=d_flag3, mode=mode) == (-2, True)
    with pytest.raises(edc.EngineError, match="edc error -2"):
        eng.quorum_verify_valset(V.off, V.sigs, flag3, V.thr, rnd.randbytes(32), vks=V.vks, ks=V.ks)
    with pytest.raises(edc.EngineError, match="edc error -2"):
        eng.valset_resolve(V.off, flag3, V.thr, vks=V.vks)
    works()
    # what the host refuses
    assert raw_device(mode=2) == (-2, True) and raw_device(seed=None) == (-2, True)
    assert raw_device(nc=0)[0] == 0
    # a key index outside the list
    A = ValSet("valid", commit_sets("valid"), g, drop=0)
    ja = A.judge(g, g.LIGHT)
    A.register(eng)
    outside = list(A.key_idx)
    outside[A.n // 2] = len(A.keys)
    with pytest.raises(edc.EngineError, match="edc error -2"):
        eng.quorum_verify_valset(A.off, A.sigs, A.flag, A.thr, rnd.randbytes(32), key_idx=outside, ks=A.ks)
    with pytest.raises(edc.EngineError, match="edc error -2"):
        eng.valset_resolve(A.off, A.flag, A.thr, key_idx=outside)
    _same(eng.quorum_verify_valset(A.off, A.sigs, A.flag, A.thr, rnd.randbytes(32), key_idx=A.key_idx, ks=A.ks), ja)
    # duplicates that drive one commit's counted sum past 2^63 - 1: two votes of a member with power 2^62, one
    # on either side of the first tile edge inside the long commit
    c = max(range(A.nc), key=lambda c: A.off[c + 1] - A.off[c])
    edge = (A.off[c] // W + 1) * W
    assert A.off[c] < edge - 1 and edge < A.off[c + 1]
    heavy = A.key_idx[edge - 1]
    powers = [2**62 if p == heavy else 0 for p in range(len(A.keys))]
    assert g.check_powers(A.keys, powers)
    eng.valset_set_powers(powers)
    idx, flag = list(A.key_idx), [g.ABSENT if a == heavy else f for a, f in zip(A.key_idx, A.flag)]
    idx[edge] = heavy
    flag[edge - 1] = flag[edge] = g.COMMIT
    pos, power, flag_out = g.resolve(A.keys, powers, flag, key_idx=idx)
    assert not g.check_args(A.off, flag, power, flag_out)
    for light in (False, True):
        with pytest.raises(edc.EngineError, match="edc error -2"):
            eng.quorum_verify_valset(A.off, A.sigs, flag, A.thr, rnd.randbytes(32), light=light, key_idx=idx, ks=A.ks)
        with pytest.raises(edc.EngineError, match="edc error -2"):
            eng.valset_resolve(A.off, flag, A.thr, light=light, key_idx=idx)
    flag[edge] = g.NIL                                            # a nil vote is not counted: accepted, and a double vote in full mode
    assert eng.valset_resolve(A.off, flag, A.thr, light=False, key_idx=idx)["dv"][c] == 1
    eng.valset_set_powers(A.powers)
    _same(eng.quorum_verify_valset(A.off, A.sigs, A.flag, A.thr, rnd.randbytes(32), key_idx=A.key_idx, ks=A.ks), ja)


def test_allocations_return(edc, g, commit_sets):
    V = ValSet("valid", commit_sets("valid"), g, drop=7)
    before = edc.debug_live_allocs()
    e2 = edc.Engine(0)
    try:
        V.register(e2)
        _same(e2.quorum_verify_valset(V.off, V.sigs, V.flag, V.thr, bytes(range(32)), vks=V.vks, msgs=V.msgs), V.judge(g, g.LIGHT))
        assert edc.debug_live_allocs() > before
    finally:
        e2.close()
    assert edc.debug_live_allocs() == before
