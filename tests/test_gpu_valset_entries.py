"""GPU: the validator-set entries against one another (include/edc.h): edc_valset_quorum_verify[_device]
and edc_vhist_quorum_verify[_device] against edc_vq_verify on the same votes, what each of them accepts
and refuses, the resolve entries against the paired one, and the timing hooks.

Every expected value is another entry's result in the same test; the entries themselves are held to
the model and to the quorum entries in test_gpu_valset.py, test_gpu_vhist.py and test_gpu_vq.py. The
shapes are three or four commits around the tile W of the selection and of the join and scan kernels."""
import ctypes
import math
import random

import pytest

pytestmark = pytest.mark.gpu

W = 256
M = 300                        # registered keys: every commit's signers are distinct members
KEYS = ("code", "commit_verdicts", "item_verdicts", "tally", "n_bad_commits", "n_checked", "check8")
SEED = bytes(range(11, 43))
SHAPES = [[W - 1, W + 1, 5], [W - 2, 4, W, 3], [W + 1, 3, W - 1]]
IDS = ["-".join(map(str, s)) for s in SHAPES]


def _offsets(sizes):
    off = [0]
    for s in sizes:
        off.append(off[-1] + s)
    return off


def _up(b, shift=0):
    import torch
    t = torch.frombuffer(bytearray(bytes(shift) + bytes(b) + bytes(16)), dtype=torch.uint8).to("cuda:0")
    torch.cuda.synchronize()
    return t[shift:]


class Keys:
    """The registered list of M signers with its one set (power 10 each, the last five weightless) and
    its history of three versions: position 3 leaves at 1 and returns at 2, 7 grows at 1, 20 leaves at 2."""

    def __init__(self, eng, edc):
        rnd = random.Random("valset entries keys")
        N = edc.VHIST_NOT_MEMBER
        self.seeds = [rnd.randbytes(32) for _ in range(M)]
        self.keys, _ = eng.sign(self.seeds, [b""] * M)
        self.powers = [10] * (M - 5) + [0] * 5
        self.base = [10] * (M - 5) + [N] * 5
        self.updates = [[(3, N), (7, 25)], [(3, 10), (20, N)]]

    def register(self, eng, hist=True, valset=True):
        eng.keycache_load(self.keys)
        if valset:
            eng.valset_set_powers(self.powers)
        if hist:
            eng.vhist_set(self.base, self.updates)


class Votes:
    """Commits of `sizes` votes by distinct members in list order from a per-commit start. Commit 0
    opens with two votes of one member (a checked double vote); the first vote of the last commit of
    more than 100 votes carries a forged signature (checked in both modes); every 17th vote is absent
    and every 23rd nil. Thresholds: two thirds of the commit's set."""

    def __init__(self, eng, edc, K, sizes):
        rnd = random.Random("valset entries %r" % (sizes,))
        self.K, self.sizes = K, sizes
        self.off = _offsets(sizes)
        self.n, self.nc = self.off[-1], len(sizes)
        self.who, self.flag = [], []
        for c, s in enumerate(sizes):
            start = rnd.randrange(30, 280)          # the first signer of every commit is a member of every version
            for j in range(s):
                self.who.append((start + j) % M)
                self.flag.append(edc.VOTE_ABSENT if j % 17 == 16 else edc.VOTE_NIL if j % 23 == 22 else edc.VOTE_COMMIT)
        self.who[1] = self.who[0]
        self.msgs = [b"vote %d of %r" % (i, sizes) for i in range(self.n)]
        self.vks, self.sigs = eng.sign([K.seeds[p] for p in self.who], self.msgs)
        assert self.vks == [K.keys[p] for p in self.who]
        self.forged = self.off[max(c for c, s in enumerate(sizes) if s > 100)]
        s = self.sigs[self.forged]
        self.sigs[self.forged] = s[:40] + bytes([s[40] ^ 4]) + s[41:]
        self.ks = eng.challenge(self.vks, self.sigs, self.msgs)
        self.ver = [(c + 1) % 3 for c in range(self.nc)]
        self.tver = [(c + 2) % 3 for c in range(self.nc)]
        self._dev = None

    def thr(self, eng, hist, ver=None):
        if not hist:
            return [2 * sum(self.K.powers) // 3] * self.nc
        totals, _ = eng.vhist_totals()
        return [2 * totals[v] // 3 for v in (self.ver if ver is None else ver)]

    def signer(self, keyform):
        return dict(key_idx=list(self.who)) if keyform == "key_idx" else dict(vks=list(self.vks))

    def dev(self):
        if self._dev is None:
            import torch
            moff = torch.tensor(_offsets([len(m) for m in self.msgs]), dtype=torch.int64, device="cuda:0")
            self._dev = dict(vk=_up(b"".join(self.vks)), sig=_up(b"".join(self.sigs)), msg=_up(b"".join(self.msgs)), off=moff,
                             k=_up(b"".join(self.ks)), flag=_up(bytes(self.flag)))
            torch.cuda.synchronize()
        return self._dev


@pytest.fixture(scope="module")
def eng(edc):
    pytest.importorskip("torch")
    e = edc.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def keys(eng, edc):
    return Keys(eng, edc)


@pytest.fixture(scope="module")
def votes(eng, edc, keys):
    cache = {}

    def get(sizes):
        if tuple(sizes) not in cache:
            cache[tuple(sizes)] = Votes(eng, edc, keys, sizes)
        return cache[tuple(sizes)]
    return get


def _older(eng, V, hist, light, form, keyform, thr, ks=None, seed=SEED):
    """one of the four older entries; keyform "device": the device entry (key bytes)"""
    if keyform == "device":
        D = V.dev()
        a = (D["vk"], D["sig"], None if form == "k" else D["msg"], None if form == "k" else D["off"], D["flag"], thr, seed)
        kw = dict(light=light, d_k=D["k"] if form == "k" else None)
        return eng.quorum_verify_vhist_device(V.off, V.ver, *a, **kw) if hist else eng.quorum_verify_valset_device(V.off, *a, **kw)
    kw = dict(light=light, **V.signer(keyform))
    kw.update(dict(msgs=V.msgs) if form == "msgs" else dict(ks=V.ks if ks is None else ks))
    if hist:
        return eng.quorum_verify_vhist(V.off, V.ver, V.sigs, V.flag, thr, seed, **kw)
    return eng.quorum_verify_valset(V.off, V.sigs, V.flag, thr, seed, **kw)


def _request(eng, V, hist, light, form, keyform, thr, ks=None, seed=SEED):
    a = dict(light=light, versions=V.ver if hist else None)
    if keyform == "device":
        import torch
        D = V.dev()
        a.update(device=True, vks=D["vk"], sigs=D["sig"])
        a.update(dict(ks=D["k"]) if form == "k" else dict(msgs=D["msg"], msg_off=D["off"]))
        res = eng.vq_verify(V.off, D["flag"], thr, seed, **a)
        torch.cuda.synchronize()
        return res
    a.update(V.signer(keyform), sigs=V.sigs)
    a.update(dict(msgs=V.msgs) if form == "msgs" else dict(ks=V.ks if ks is None else ks))
    return eng.vq_verify(V.off, V.flag, thr, seed, **a)


def _same(got, want, what):
    for key in KEYS:
        assert got[key] == want[key], (what, key)


# ---------------------------------------------------------------- 1. entry equality
@pytest.mark.parametrize("light", [False, True], ids=["full", "light"])
@pytest.mark.parametrize("hist", [False, True], ids=["set", "hist"])
@pytest.mark.parametrize("sizes", SHAPES, ids=IDS)
def test_older_entries_equal_the_request(eng, edc, keys, votes, sizes, hist, light):
    V = votes(sizes)
    keys.register(eng)
    thr = V.thr(eng, hist)
    first = None
    for keyform in ("vks", "key_idx", "device"):
        for form in ("msgs", "k"):
            got = _older(eng, V, hist, light, form, keyform, thr)
            _same(got, _request(eng, V, hist, light, form, keyform, thr), (keyform, form))
            first = first or got
            _same(got, first, (keyform, form, "every form gives one result"))
    # the votes are what the docstring says they are
    cv, fc = first["commit_verdicts"], max(c for c, s in enumerate(V.sizes) if s > 100)
    assert cv[0] == edc.EDC_DOUBLE_VOTE and cv[fc] == edc.EDC_INVALID_SIGNATURE and first["code"] == edc.EDC_INVALID_SIGNATURE
    assert first["item_verdicts"][V.forged] == edc.EDC_INVALID_SIGNATURE and edc.EDC_QUORUM_SHORT in cv
    assert 0 < first["n_checked"] and (not light or first["n_checked"] < V.n)


# ---------------------------------------------------------------- 2. empty sets
def _raw_outs(nc, n):
    return (ctypes.create_string_buffer(b"\x77" * max(nc, 1), max(nc, 1)), ctypes.create_string_buffer(max(n, 1)),
            (ctypes.c_uint64 * max(nc, 1))(), ctypes.c_int(0x77), ctypes.c_size_t(0x77), ctypes.create_string_buffer(32))


def _raw(eng, name, nc, off, ver, thr, seed=SEED, mode=1, n=0, **a):
    """an older entry called below the Python layer -> (rc, verdicts, tally, n_bad, n_checked); a: its
    array arguments (host bytes / ctypes arrays or device addresses), None where not given"""
    o = (ctypes.c_uint32 * (nc + 1))(*off)
    t = (ctypes.c_uint64 * max(nc, 1))(*thr)
    v = () if "valset" in name else (None if ver is None else (ctypes.c_uint32 * max(nc, 1))(*ver),)
    cv, iv, tl, nb, cnt, c8 = _raw_outs(nc, n)
    if name.endswith("_device"):
        arrays = [a.get(x) for x in ("vk", "sig", "msg", "msg_off", "k", "flag")]
    else:
        arrays = [a.get(x) for x in ("vk", "key_idx", "sig", "msg", "msg_off", "k", "flag")]
    rc = getattr(eng.lib, name)(eng.ctx, nc, o, *v, *arrays, t, mode, seed, cv, iv, tl, ctypes.byref(nb), ctypes.byref(cnt), c8)
    return rc, list(cv.raw[:nc]), list(tl[:nc]), nb.value, cnt.value


OLDER = ("edc_valset_quorum_verify", "edc_valset_quorum_verify_device", "edc_vhist_quorum_verify", "edc_vhist_quorum_verify_device")


def test_empty_sets(eng, edc, keys):
    keys.register(eng)
    for name in OLDER:
        assert _raw(eng, name, 0, [0], [], [])[0] == 0, name                           # nc == 0
        assert _raw(eng, name, 0, [0], None, [])[0] == 0, name
        # three empty commits and no array at all: a tally of 0 passes no threshold (the quorum is strict)
        for mode in (0, 1):
            rc, cv, tl, nb, cnt = _raw(eng, name, 3, [0, 0, 0, 0], [0, 2, 1], [0, 5, 0], mode=mode)
            assert (rc, cv, tl, nb, cnt) == (edc.EDC_QUORUM_SHORT, [edc.EDC_QUORUM_SHORT] * 3, [0, 0, 0], 3, 0), name
    assert eng.vq_verify([0], [], [], SEED, vks=[], sigs=[], ks=[])["code"] == 0
    assert eng.vq_verify([0], [], [], SEED, versions=[], vks=[], sigs=[], ks=[])["n_checked"] == 0
    got = eng.vq_verify([0, 0, 0, 0], [], [0, 5, 0], SEED, versions=[0, 2, 1], key_idx=[], sigs=[], ks=[])
    assert got["commit_verdicts"] == [edc.EDC_QUORUM_SHORT] * 3 and got["n_checked"] == 0 and got["tally"] == [0, 0, 0]
    with pytest.raises(edc.EngineError, match="edc error -2"):                         # neither vk nor key_idx: refused whatever n is
        eng.vq_verify([0, 0, 0, 0], [], [0, 5, 0], SEED, versions=[0, 2, 1], sigs=[], ks=[])


# ---------------------------------------------------------------- 3. refusals
def test_refusals_leave_the_context_usable(edc, keys, votes):
    import torch
    V = votes(SHAPES[1])
    e2 = edc.Engine(0)
    try:
        e2.keycache_load(keys.keys)
        thr0 = [0] * V.nc
        D = V.dev()
        host = dict(vk=b"".join(V.vks), sig=b"".join(V.sigs), k=b"".join(V.ks), flag=bytes(V.flag))
        idx = (ctypes.c_uint32 * V.n)(*V.who)
        dev = {x: D[x].data_ptr() for x in ("vk", "sig", "k", "flag")}

        def call(name, ver=V.ver, thr=thr0, seed=SEED, **kw):
            a = dict(dev if name.endswith("_device") else host)
            a.update(kw)
            return _raw(e2, name, V.nc, V.off, ver, thr, seed=seed, n=V.n, **a)[0]

        for name in OLDER:                                                               # no powers, no history
            assert call(name) == -2, name
        keys.register(e2)
        thr = {False: V.thr(e2, False), True: V.thr(e2, True)}
        good = {name: _older(e2, V, "vhist" in name, True, "k", "device" if name.endswith("_device") else "vks",
                             thr["vhist" in name]) for name in OLDER}
        for name in OLDER:
            hist, device = "vhist" in name, name.endswith("_device")
            cases = [dict(seed=None)]
            if hist:
                cases += [dict(ver=None), dict(ver=[3] + V.ver[1:])]                     # missing; past the history
            if device:
                cases += [dict(vk=_up(host["vk"], shift=8).data_ptr()), dict(vk=None), dict(sig=None), dict(flag=None), dict(k=None)]
            else:
                past = (ctypes.c_uint32 * V.n)(*([M] + V.who[1:]))
                cases += [dict(key_idx=idx), dict(vk=None), dict(vk=None, key_idx=past)]  # both; neither; past the list
            for kw in cases:
                assert call(name, thr=thr[hist], **kw) == -2, (name, sorted(kw))
                got = _older(e2, V, hist, True, "k", "device" if device else "vks", thr[hist])
                _same(got, good[name], (name, sorted(kw), "after the refusal"))
            if not device:
                assert call(name, thr=thr[hist], vk=None, key_idx=idx) == good[name]["code"] == 1        # by position: accepted
        torch.cuda.synchronize()
    finally:
        e2.close()


# ---------------------------------------------------------------- 4. prehashed k, host forms
@pytest.mark.parametrize("hist", [False, True], ids=["set", "hist"])
def test_prehashed_k_is_canonical_where_checked(eng, edc, keys, votes, hist):
    V = votes(SHAPES[0])
    keys.register(eng)
    thr = V.thr(eng, hist)
    r = (eng.vhist_resolve(V.off, V.ver, V.flag, thr, light=True, key_idx=V.who) if hist
         else eng.valset_resolve(V.off, V.flag, thr, light=True, key_idx=V.who))
    checked = next(i for i in range(W, V.n) if r["checked"][i])                      # past the first tile
    skipped = next(i for i in range(V.n - 1, 0, -1)                                   # a member's vote behind the quorum
                   if not r["checked"][i] and V.flag[i] == edc.VOTE_COMMIT and r["power"][i] > 0)
    for run in (_older, _request):
        want = run(eng, V, hist, True, "k", "key_idx", thr)
        for bad in (b"\xff" * 32, bytes.fromhex("edd3f55c1a631258d69cf7a2def9de14" + "00" * 15 + "10")):      # 2^256 - 1 and l itself
            ks = list(V.ks)
            ks[checked] = bad
            for keyform in ("key_idx", "vks"):
                with pytest.raises(edc.EngineError, match="edc error -2"):
                    run(eng, V, hist, True, "k", keyform, thr, ks=ks)
            ks = list(V.ks)
            ks[skipped] = bad
            for keyform in ("key_idx", "vks"):
                _same(run(eng, V, hist, True, "k", keyform, thr, ks=ks), want, (run.__name__, keyform))


# ---------------------------------------------------------------- 5. the debug record
def test_debug_record_is_the_requests_alone(edc, keys, votes):
    V = votes(SHAPES[2])
    e2 = edc.Engine(0)
    try:
        keys.register(e2)
        for hist in (False, True):
            thr = V.thr(e2, hist)
            for keyform, form in (("vks", "msgs"), ("key_idx", "k"), ("device", "msgs"), ("device", "k")):
                _older(e2, V, hist, True, form, keyform, thr)
                with pytest.raises(edc.EngineError, match="edc error -2"):
                    e2.vq_last()
        got = _request(e2, V, True, True, "msgs", "vks", V.thr(e2, True))
        assert e2.vq_last() == (V.n, got["n_checked"], 0, 0, V.n, 0, 0, 0)
        _older(e2, V, True, False, "k", "key_idx", V.thr(e2, True))                     # full mode: another checked count
        assert e2.vq_last() == (V.n, got["n_checked"], 0, 0, V.n, 0, 0, 0)
    finally:
        e2.close()


# ---------------------------------------------------------------- 6. resolve
SIDE_KEYS = ("pos", "power", "flag", "checked", "planned", "dv")


@pytest.mark.parametrize("light", [False, True], ids=["full", "light"])
@pytest.mark.parametrize("sizes", SHAPES, ids=IDS)
def test_paired_resolve_is_two_history_resolves(eng, edc, keys, votes, sizes, light):
    V = votes(sizes)
    keys.register(eng)
    thr, tthr = V.thr(eng, True), V.thr(eng, True, V.tver)
    for keyform in ("key_idx", "vks"):
        signer = V.signer(keyform)
        ra = eng.vhist_resolve(V.off, V.ver, V.flag, thr, light=light, **signer)
        rb = eng.vhist_resolve(V.off, V.tver, V.flag, tthr, light=light, **signer)
        r = eng.vq_trust_resolve(V.off, V.ver, V.tver, V.flag, thr, tthr, light=light, **signer)
        for side, want in (("a", ra), ("b", rb)):
            for key in SIDE_KEYS:
                assert r[side][key] == want[key], (keyform, side, key)
        assert ra != rb and ra["dv"][0] == rb["dv"][0] == 1
        assert r["side"] == [(1 if a else 0) | (2 if b else 0) for a, b in zip(ra["checked"], rb["checked"])]
        assert r["n_checked"] == sum(1 for x in r["side"] if x)
        # every nullable output null: the counts alone, and nothing at all
        nc, off = eng._commit_offsets(V.off)
        vkb, idx = edc._tmpl_keys(V.n, signer.get("vks"), signer.get("key_idx"))
        ver, tver = eng._vhist_versions_arg(nc, V.ver), eng._vhist_versions_arg(nc, V.tver)
        fl, th, tth = eng._valset_flags(V.n, V.flag), eng._quorum_thresholds(nc, thr), eng._quorum_thresholds(nc, tthr)
        for want, args in ((ra, (ver, vkb, idx, fl, th)), (rb, (tver, vkb, idx, fl, tth))):
            cnt = ctypes.c_size_t(0x77)
            assert eng.lib.edc_vhist_resolve(eng.ctx, nc, off, *args, int(light), None, None, None, None, None,
                                             ctypes.byref(cnt), None) == 0
            assert cnt.value == want["n_checked"]
            assert eng.lib.edc_vhist_resolve(eng.ctx, nc, off, *args, int(light), None, None, None, None, None, None, None) == 0
        cnt = ctypes.c_size_t(0x77)
        assert eng.lib.edc_vq_trust_resolve(eng.ctx, nc, off, ver, tver, vkb, idx, fl, th, tth, int(light), *([None] * 13),
                                            ctypes.byref(cnt)) == 0
        assert cnt.value == r["n_checked"]
        assert eng.lib.edc_vq_trust_resolve(eng.ctx, nc, off, ver, tver, vkb, idx, fl, th, tth, int(light), *([None] * 13), None) == 0
        assert eng.vq_trust_resolve(V.off, V.ver, V.tver, V.flag, thr, tthr, light=light, **signer) == r
    if not light:                                                                      # the one set's resolve, outputs null
        signer = V.signer("key_idx")
        r1 = eng.valset_resolve(V.off, V.flag, V.thr(eng, False), light=False, **signer)
        nc, off = eng._commit_offsets(V.off)
        _, idx = edc._tmpl_keys(V.n, None, V.who)
        cnt = ctypes.c_size_t(0x77)
        assert eng.lib.edc_valset_resolve(eng.ctx, nc, off, None, idx, eng._valset_flags(V.n, V.flag),
                                          eng._quorum_thresholds(nc, V.thr(eng, False)), 0, None, None, None, None, None,
                                          ctypes.byref(cnt), None) == 0
        assert cnt.value == r1["n_checked"] and r1["dv"][0] == 1


# ---------------------------------------------------------------- 7. the timing hooks
@pytest.mark.parametrize("sizes", SHAPES[:2], ids=IDS[:2])
def test_timing_hooks_rewrite_the_same_values(eng, edc, keys, votes, sizes):
    V = votes(sizes)
    keys.register(eng)
    thr1, thr, tthr = V.thr(eng, False), V.thr(eng, True), V.thr(eng, True, V.tver)
    for light in (True, False):
        for keyform in ("key_idx", "vks"):
            signer = V.signer(keyform)

            def resolves():
                return (eng.valset_resolve(V.off, V.flag, thr1, light=light, **signer),
                        eng.vhist_resolve(V.off, V.ver, V.flag, thr, light=light, **signer),
                        eng.vq_trust_resolve(V.off, V.ver, V.tver, V.flag, thr, tthr, light=light, **signer))
            before = resolves()
            ms = (eng.valset_select_ms(V.off, V.flag, thr1, light=light, reps=3, **signer)
                  + eng.vhist_select_ms(V.off, V.ver, V.flag, thr, light=light, reps=3, **signer)
                  + eng.vq_trust_select_ms(V.off, V.ver, V.tver, V.flag, thr, tthr, light=light, reps=3, **signer))
            assert len(ms) == 7 and all(math.isfinite(t) and t >= 0 for t in ms), ms
            assert resolves() == before
            # a verify call behind a hook sees what it saw before it
            want = _older(eng, V, True, light, "k", keyform, thr)
            eng.vq_trust_select_ms(V.off, V.ver, V.tver, V.flag, thr, tthr, light=light, reps=2, **signer)
            _same(_older(eng, V, True, light, "k", keyform, thr), want, (light, keyform))
    assert eng.valset_select_ms([0], [], [], vks=[]) == (0.0, 0.0)
    assert eng.vhist_select_ms([0, 0], [0], [], [1], vks=[]) == (0.0, 0.0)
