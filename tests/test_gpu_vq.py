"""GPU: validator-set requests (include/edc.h, edc_vq_verify): the validator-set and history entries,
templates and the verified-signature table behind one request.

Every expected value is an entry that existed before, run in the same test: the join, selection and
double votes are edc_valset_resolve's / edc_vhist_resolve's; verdicts, codes, tally, counts and check8
are those of edc_[cached_][tmpl_]quorum_verify handed the joined power / flag_out (on host key bytes),
with the verdicts of double-vote commits, n_bad_commits and the return value (1 over 4 over 3) put
over them as the header says. Shapes: 13 registered keys, 5 commits of 8..12 votes; W is the tile."""
import random

import pytest

pytestmark = pytest.mark.gpu

W = 256
KEYS = ("code", "commit_verdicts", "item_verdicts", "tally", "n_bad_commits", "n_checked", "check8")
SEED = bytes(range(7, 39))
HOLES = (0, 1, 15, 16, 17, 12)


@pytest.fixture(scope="module")
def ceng(edc):
    pytest.importorskip("torch")
    eng = edc.Engine(0)
    eng.sigcache_create(1 << 12)
    yield eng
    eng.close()


def _offsets(sizes):
    off = [0]
    for s in sizes:
        off.append(off[-1] + s)
    return off


def _up(b, shift=0):
    """bytes on the device, `shift` bytes past an allocation's (256-byte aligned) start"""
    import torch
    t = torch.frombuffer(bytearray(bytes(shift) + bytes(b) + bytes(16)), dtype=torch.uint8).to("cuda:0")
    torch.cuda.synchronize()
    return t[shift:]


def _up_ints(xs, dtype):
    import torch
    t = torch.tensor(list(xs) or [0], dtype=dtype, device="cuda:0")
    torch.cuda.synchronize()
    return t


class World:
    """The registered list: positions 0 and 1 differ only in their last byte and never sign; 2..11 are
    the signers s0..s9; 12 is s10, a member of no version of the history (weightless in the one set).
    Five commits: 0 all valid; 1 with a checked double vote (s0 twice at its head), an absent and a nil
    vote; 2 with a second s0 vote behind the quorum (a double vote in full mode only) and s10's vote;
    3 left short; 4 valid in another order. The history has three versions: s3 leaves at 1 and returns
    at 2, where s9 leaves."""

    def __init__(self, eng, edc):
        rnd = random.Random("vq world 1")
        self.edc, N = edc, edc.VHIST_NOT_MEMBER
        twin = rnd.randbytes(31)
        self.seeds = [rnd.randbytes(32) for _ in range(11)]
        skeys, _ = eng.sign(self.seeds, [b""] * 11)
        self.keys = [twin + b"\x01", twin + b"\x02"] + list(skeys)
        self.stranger = rnd.randbytes(32)
        self.powers = [1, 1] + [10] * 10 + [0]
        self.base = [1, 1] + [10] * 10 + [N]
        self.updates = [[(5, N), (2, 12)], [(5, 10), (11, N)]]
        C, A, NIL = edc.VOTE_COMMIT, edc.VOTE_ABSENT, edc.VOTE_NIL
        s = lambda *xs: [x + 2 for x in xs]
        commits = [
            (s(0, 1, 2, 3, 4, 5, 6, 7, 8, 9), [C] * 10),
            (s(0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9), [C] * 8 + [A, NIL, C]),
            (s(0, 1, 2, 3, 4, 5, 6, 7, 0, 10, 8, 9), [C] * 8 + [C, C, NIL, C]),
            (s(0, 1, 2, 3, 4, 5, 6, 7), [C] * 5 + [A, NIL, A]),
            (s(9, 8, 7, 6, 5, 4, 3, 2, 1), [C] * 9),
        ]
        self.off = _offsets([len(c[0]) for c in commits])
        self.n, self.nc = self.off[-1], len(commits)
        self.who = [p for c in commits for p in c[0]]
        self.flag = [f for c in commits for f in c[1]]
        self.strange_at = self.off[2] + 9
        self.ver = [2, 1, 0, 1, 2]
        self.T = edc.batch.Templates([b"", rnd.randbytes(37), rnd.randbytes(5)], [rnd.randbytes(21), b"", rnd.randbytes(64)])
        self.ctpl, self.span = [0, 1, 0, 1, 1], 2
        self.alt = [rnd.randrange(2) for _ in range(self.n)]
        self.holes = [rnd.randbytes(HOLES[i % len(HOLES)]) for i in range(self.n)]
        self.sign(eng)

    def commit_of(self, i):
        return max(c for c in range(self.nc) if self.off[c] <= i)

    def sign(self, eng):
        self.tpl = [self.ctpl[self.commit_of(i)] + self.alt[i] for i in range(self.n)]
        self.msgs = self.T.materialize(self.tpl, self.holes)
        # no two votes are one item (same signer, same message): the table would hold them as one record
        assert len(set(zip(self.who, self.msgs))) == self.n
        self.vks, self.sigs = eng.sign([self.seeds[p - 2] for p in self.who], self.msgs)
        assert self.vks == [self.keys[p] for p in self.who]
        self.ks = eng.challenge(self.vks, self.sigs, self.msgs)

    def register(self, eng, hist):
        eng.keycache_load(self.keys)
        if hist:
            eng.vhist_set(self.base, self.updates)
            totals, _ = eng.vhist_totals()
            self.thr = [2 * totals[v] // 3 for v in self.ver]
        else:
            eng.valset_set_powers(self.powers)
            self.thr = [2 * sum(self.powers) // 3] * self.nc

    def signer(self, hist, keyform):
        """how a form names its signers; the one set has a non-member only by key bytes"""
        if keyform == "key_idx":
            return dict(key_idx=list(self.who))
        vks = list(self.vks)
        if not hist:
            vks[self.strange_at] = self.stranger
        return dict(vks=vks)


@pytest.fixture(scope="module")
def world(ceng, edc):
    return World(ceng, edc)


def _resolve(eng, Wd, hist, light, signer, flag=None):
    flag = Wd.flag if flag is None else flag
    if hist:
        return eng.vhist_resolve(Wd.off, Wd.ver, flag, Wd.thr, light=light, **signer)
    return eng.valset_resolve(Wd.off, flag, Wd.thr, light=light, **signer)


def _key_bytes(Wd, signer):
    return signer["vks"] if "vks" in signer else [Wd.keys[p] for p in signer["key_idx"]]


def _with_dv(edc, want, dv):
    """the double-vote verdicts, the count and the return value over a quorum entry's result"""
    want = dict(want)
    cv = [edc.EDC_DOUBLE_VOTE if d else v for v, d in zip(want["commit_verdicts"], dv)]
    want["commit_verdicts"] = cv
    want["n_bad_commits"] = sum(1 for v in cv if v)
    want["code"] = next((c for c in (1, 4, 3) if c in cv), 0)
    return want


def _expected(eng, Wd, hist, form, cached, light, signer, sigs=None, flag=None):
    """the contract's right-hand side from the entries that exist: (result dict, the resolve dict)"""
    r = _resolve(eng, Wd, hist, light, signer, flag)
    sigs = Wd.sigs if sigs is None else sigs
    vks = _key_bytes(Wd, signer)
    if form == "tmpl":
        fn = eng.quorum_verify_templated_cached if cached else eng.quorum_verify_templated
        want = fn(Wd.T, Wd.off, Wd.ctpl, sigs, Wd.holes, r["power"], r["flag"], Wd.thr, SEED, light=light, alt_span=Wd.span,
                  item_alt=Wd.alt, vks=vks)
    else:
        fn = eng.quorum_verify_cached if cached else eng.quorum_verify
        kw = dict(msgs=Wd.msgs) if form == "msgs" else dict(ks=Wd.ks)
        want = fn(Wd.off, sigs, r["power"], r["flag"], Wd.thr, SEED, light=light, vks=vks, **kw)
    return _with_dv(Wd.edc, want, r["dv"]), r


def _request(eng, Wd, hist, form, cached, light, signer, device=False, sigs=None, flag=None, holes=None, alt=None, shift=0,
             **kw):
    import torch
    sigs = Wd.sigs if sigs is None else sigs
    flag = Wd.flag if flag is None else flag
    holes = Wd.holes if holes is None else holes
    alt = Wd.alt if alt is None else alt
    a = dict(light=light, versions=Wd.ver if hist else None, cached=cached)
    if form == "tmpl":
        a.update(templates=Wd.T, commit_tpl=Wd.ctpl, alt_span=Wd.span)
    if not device:
        a.update(signer, sigs=sigs)
        if form == "tmpl":
            a.update(item_alt=alt, holes=holes)
        elif form == "msgs":
            a.update(msgs=Wd.msgs)
        else:
            a.update(ks=Wd.ks)
        a.update(kw)
        return eng.vq_verify(Wd.off, flag, Wd.thr, SEED, **a)
    a.update(device=True, vks=_up(b"".join(signer["vks"])), sigs=_up(b"".join(sigs)))
    if form == "tmpl":
        var = b"".join(holes)
        a.update(item_alt=_up(bytes(alt), shift), holes=_up(var, shift), var_bytes=len(var),
                 var_off=_up_ints(_offsets([len(h) for h in holes]), torch.int32))
    elif form == "msgs":
        a.update(msgs=_up(b"".join(Wd.msgs)), msg_off=_up_ints(_offsets([len(m) for m in Wd.msgs]), torch.int64))
    else:
        a.update(ks=_up(b"".join(Wd.ks)))
    a.update(kw)
    return eng.vq_verify(Wd.off, _up(bytes(flag)), Wd.thr, SEED, **a)


def _same(got, want, what):
    for key in KEYS + (("n_miss",) if "n_miss" in want else ()):
        assert got[key] == want[key], (what, key, got[key], want[key])


# ---------------------------------------------------------------- 1. the matrix
@pytest.mark.parametrize("light", [False, True], ids=["full", "light"])
@pytest.mark.parametrize("hist", [False, True], ids=["set", "hist"])
def test_matrix(ceng, world, edc, hist, light):
    Wd = world
    Wd.register(ceng, hist)
    seen = set()
    for form in ("msgs", "k", "tmpl"):
        for cached in (False, True):
            for keyform in ("vks", "key_idx", "device"):
                signer = Wd.signer(hist, "key_idx" if keyform == "key_idx" else "vks")
                ceng.sigcache_clear()
                st0 = ceng.sigcache_stats()
                want, r = _expected(ceng, Wd, hist, form, cached, light, signer)
                d_want = _delta(st0, ceng.sigcache_stats())
                ceng.sigcache_clear()
                st0 = ceng.sigcache_stats()
                got = _request(ceng, Wd, hist, form, cached, light, signer, device=keyform == "device")
                what = (form, cached, keyform)
                _same(got, want, what)
                assert _delta(st0, ceng.sigcache_stats()) == d_want == ([0, r["n_checked"], r["n_checked"], 0] if cached
                                                                         else [0, 0, 0, 0]), what
                if not cached and form != "tmpl":          # the entry this form replaces, on the same inputs
                    kw = dict(msgs=Wd.msgs) if form == "msgs" else dict(ks=Wd.ks)
                    old = (ceng.quorum_verify_vhist(Wd.off, Wd.ver, Wd.sigs, Wd.flag, Wd.thr, SEED, light=light, **signer, **kw)
                           if hist else ceng.quorum_verify_valset(Wd.off, Wd.sigs, Wd.flag, Wd.thr, SEED, light=light, **signer, **kw))
                    _same(got, old, what)
                if form == "tmpl" and not cached:          # equals the request on the materialised messages
                    _same(got, _request(ceng, Wd, hist, "msgs", False, light, signer, device=keyform == "device"), what)
                    got = _request(ceng, Wd, hist, form, cached, light, signer, device=keyform == "device")
                last = ceng.vq_last()
                m = r["n_checked"]
                assert last[0] == Wd.n and last[1] == m == got["n_checked"], what
                assert last[4] == {"msgs": Wd.n, "k": 0, "tmpl": m}[form], what          # only the checked votes hashed
                if cached:
                    assert (last[2], last[3], last[5]) == (0, m, m), what
                seen.update(got["commit_verdicts"])
                # the world is what the docstring says it is
                cv = got["commit_verdicts"]
                assert cv[1] == edc.EDC_DOUBLE_VOTE and cv[3] == edc.EDC_QUORUM_SHORT and cv[0] == cv[4] == edc.EDC_OK, what
                assert cv[2] == (edc.EDC_OK if light else edc.EDC_DOUBLE_VOTE), what
                assert r["pos"][Wd.strange_at] == (edc.NO_POS if hist or keyform != "key_idx" else 12), what
                assert got["code"] == edc.EDC_DOUBLE_VOTE
    assert seen == {0, 3, 4}
    if hist:                                               # s3 has left at version 1 and is back at version 2
        r = _resolve(ceng, Wd, True, False, Wd.signer(True, "key_idx"))
        assert [r["pos"][i] for i in range(Wd.n) if Wd.who[i] == 5] == [5, edc.NO_POS, 5, edc.NO_POS, 5]


# ---------------------------------------------------------------- 2. the table
def _plant(eng, Wd, items, vks=None):
    eng.sigcache_clear()
    vks = Wd.vks if vks is None else vks
    if items:
        eng.verify_each_cached([vks[i] for i in items], [Wd.sigs[i] for i in items], msgs=[Wd.msgs[i] for i in items])
    return eng.sigcache_stats()


def _delta(a, b):
    return [b[k] - a[k] for k in ("hits", "misses", "inserted", "dropped")]


@pytest.mark.parametrize("form", ["k", "tmpl"])
@pytest.mark.parametrize("hist", [False, True], ids=["set", "hist"])
def test_cache(ceng, world, edc, hist, form):
    Wd = world
    Wd.register(ceng, hist)
    light = True
    for keyform in ("key_idx", "vks"):
        signer = Wd.signer(hist, keyform)
        r0 = _resolve(ceng, Wd, hist, light, signer)
        checked = [i for i in range(Wd.n) if r0["checked"][i]]
        unchecked = [i for i in range(Wd.n) if not r0["checked"][i] and Wd.flag[i] == edc.VOTE_COMMIT and i != Wd.strange_at]
        assert Wd.off[1] in checked and unchecked
        partial = sorted({Wd.strange_at, unchecked[0], Wd.off[1]} | set(checked[3:9]))
        for ratio, planted in (("0", []), ("partial", partial), ("1", checked)):
            hits = [i for i in planted if i in checked]
            st0 = _plant(ceng, Wd, planted)
            want, r = _expected(ceng, Wd, hist, form, True, light, signer)
            d_want = _delta(st0, ceng.sigcache_stats())
            assert r == r0                                  # selection and dv do not see the table
            assert want["n_miss"] == len(checked) - len(hits)
            st0 = _plant(ceng, Wd, planted)
            got = _request(ceng, Wd, hist, form, True, light, signer)
            what = (keyform, ratio)
            _same(got, want, what)
            assert _delta(st0, ceng.sigcache_stats()) == d_want == [len(hits), len(checked) - len(hits),
                                                                     len(checked) - len(hits), 0], what
            last = ceng.vq_last()
            assert last[1:4] == (len(checked), len(hits), len(checked) - len(hits)) and last[5] == last[3], what
            assert _resolve(ceng, Wd, hist, light, signer) == r0
            st1 = ceng.sigcache_stats()
            again = _request(ceng, Wd, hist, form, True, light, signer)
            assert again["n_miss"] == 0 and _delta(st1, ceng.sigcache_stats()) == [len(checked), 0, 0, 0], what
            for key in KEYS:
                if key != "check8":                        # the batch of no misses has its own check8
                    assert again[key] == got[key], (what, key)


# ---------------------------------------------------------------- 3. a bad signature on a miss
@pytest.mark.parametrize("form", ["k", "tmpl"])
def test_bad_signature_on_a_miss(ceng, world, edc, form):
    Wd = world
    Wd.register(ceng, True)
    signer = Wd.signer(True, "key_idx")
    r = _resolve(ceng, Wd, True, True, signer)
    bad = [Wd.off[1] + 2, Wd.off[4] + 1]                   # in the double-vote commit and in a clean one
    assert all(r["checked"][i] for i in bad) and r["dv"][1]
    sigs = list(Wd.sigs)
    for i in bad:
        sigs[i] = sigs[i][:40] + bytes([sigs[i][40] ^ 4]) + sigs[i][41:]
    planted = [i for i in range(Wd.off[0], Wd.off[1]) if r["checked"][i]][:3]
    st0 = _plant(ceng, Wd, planted)
    want, _ = _expected(ceng, Wd, True, form, True, True, signer, sigs=sigs)
    d_want = _delta(st0, ceng.sigcache_stats())
    st0 = _plant(ceng, Wd, planted)
    got = _request(ceng, Wd, True, form, True, True, signer, sigs=sigs)
    _same(got, want, form)
    m = r["n_checked"]
    assert _delta(st0, ceng.sigcache_stats()) == d_want == [3, m - 3, m - 3 - len(bad), 0]
    assert [got["item_verdicts"][i] for i in bad] == [1, 1]
    assert got["commit_verdicts"][1] == edc.EDC_DOUBLE_VOTE and got["commit_verdicts"][4] == edc.EDC_INVALID_SIGNATURE
    assert got["code"] == edc.EDC_INVALID_SIGNATURE        # 1 over 4 over 3
    assert ceng.vq_last()[5] == m - 3 - len(bad)


# ---------------------------------------------------------------- 4. full mode, every vote kept
@pytest.mark.parametrize("form", ["k", "tmpl"])
@pytest.mark.parametrize("cached", [False, True], ids=["plain", "cached"])
def test_nothing_gathered(ceng, world, edc, form, cached):
    """full mode with every vote signed by a member: m == n, the lists are the staged arrays themselves"""
    Wd = world
    Wd.register(ceng, True)
    who = [2, 3, 4, 6, 7, 8]
    sub = World.__new__(World)
    sub.__dict__.update(Wd.__dict__)
    sub.off, sub.n, sub.nc, sub.who, sub.flag, sub.ver, sub.ctpl = [0, 6], 6, 1, who, [edc.VOTE_COMMIT] * 6, [0], [0]
    sub.alt, sub.holes = [0, 1, 0, 1, 1, 0], [b"abc", b"", b"x" * 17, b"y" * 16, b"z", b"w" * 15]
    sub.sign(ceng)
    sub.thr = [0]
    ceng.sigcache_clear()
    a = _request(ceng, sub, True, form, cached, False, dict(key_idx=who))
    assert a["n_checked"] == 6 == ceng.vq_last()[1] and a["code"] == 0 and a["tally"] == [60]
    ceng.sigcache_clear()
    _same(a, _request(ceng, sub, True, form, cached, False, dict(vks=sub.vks)), "by key bytes")
    ceng.sigcache_clear()
    want, _ = _expected(ceng, sub, True, form, cached, False, dict(key_idx=who))
    _same(a, want, "the existing entry")


# ---------------------------------------------------------------- 5. the gather's tile edges
def test_tile_edges(ceng, world, edc):
    """n = 513 in commits that straddle items 255/256 and 511/512; checked: the last lane of tile 0, the
    first lane of tile 1 and one vote of tile 2, every other vote absent or by a non-member."""
    Wd = world
    Wd.register(ceng, True)
    rnd = random.Random("vq edges")
    sub = World.__new__(World)
    sub.__dict__.update(Wd.__dict__)
    sub.off = [0, 100, 300, 511, 513]
    sub.n, sub.nc, sub.ver, sub.ctpl = 513, 4, [0, 0, 0, 0], [0, 1, 0, 1]
    keep = {W - 1: 2, W: 3, 2 * W: 4}                      # item -> registered position of its signer
    sub.who = [keep.get(i, 12 if i % 3 else 6) for i in range(513)]          # s10 is no member; the others are absent
    sub.flag = [edc.VOTE_COMMIT if i in keep or i % 3 else edc.VOTE_ABSENT for i in range(513)]
    sub.alt = [rnd.randrange(2) for _ in range(513)]
    sub.holes = [rnd.randbytes(HOLES[i % 5]) for i in range(513)]
    for i, ln in zip(keep, (17, 0, 15)):
        sub.holes[i] = rnd.randbytes(ln)
    # absent votes and a non-member's need no signature: only the three kept votes are signed
    sub.tpl = [sub.ctpl[sub.commit_of(i)] + sub.alt[i] for i in range(513)]
    sub.msgs = sub.T.materialize(sub.tpl, sub.holes)
    sub.vks = [sub.keys[p] for p in sub.who]
    sub.sigs = [rnd.randbytes(64) for _ in range(513)]
    ks = list(keep)
    _, three = ceng.sign([sub.seeds[keep[i] - 2] for i in ks], [sub.msgs[i] for i in ks])
    for i, s in zip(ks, three):
        sub.sigs[i] = s
    sub.thr = [0, 10, 5, 0]
    for light in (True, False):
        r = _resolve(ceng, sub, True, light, dict(key_idx=sub.who))
        assert [i for i in range(513) if r["checked"][i]] == ks
        for device, signer in ((False, dict(key_idx=sub.who)), (False, dict(vks=sub.vks)), (True, dict(vks=sub.vks))):
            got = _request(ceng, sub, True, "tmpl", False, light, signer, device=device, shift=5)
            last = ceng.vq_last()
            assert last[1] == last[4] == 3
            assert 0 < last[7] <= sum(len(sub.msgs[i]) + 16 for i in ks)      # the arena is sized from the checked votes
            want = _request(ceng, sub, True, "msgs", False, light, signer, device=device)
            _same(got, want, (light, device))
            assert [i for i in range(513) if got["item_verdicts"][i] == 0] == ks and got["n_checked"] == 3
            assert got["commit_verdicts"] == [3, 0, 3, 0] and got["tally"] == [0, 20, 0, 10]


# ---------------------------------------------------------------- 6. noise
@pytest.mark.parametrize("light", [False, True], ids=["full", "light"])
def test_noise_in_unchecked_votes(ceng, world, edc, light):
    Wd = world
    Wd.register(ceng, True)
    rnd = random.Random("vq noise")
    r = _resolve(ceng, Wd, True, light, Wd.signer(True, "vks"))
    quiet = [i for i in range(Wd.n) if not r["checked"][i]]
    assert Wd.strange_at in quiet and (not light or any(Wd.flag[i] == edc.VOTE_COMMIT and r["pos"][i] != edc.NO_POS for i in quiet))
    sigs, holes = list(Wd.sigs), list(Wd.holes)
    for i in quiet:
        sigs[i], holes[i] = rnd.randbytes(64), rnd.randbytes(len(holes[i]))
    for device in (False, True):
        clean = _request(ceng, Wd, True, "tmpl", False, light, Wd.signer(True, "vks"), device=device)
        vks = list(Wd.vks)
        for i in quiet:
            vks[i] = rnd.randbytes(32)                   # whoever it names, the vote stays unchecked
        noisy = _request(ceng, Wd, True, "tmpl", False, light, dict(vks=vks), device=device, sigs=sigs, holes=holes)
        _same(noisy, clean, device)
        # the all-n checks do not depend on who signed or on what is checked
        i = Wd.strange_at
        alt = list(Wd.alt)
        alt[i] = Wd.span
        with pytest.raises(edc.EngineError, match="edc error -2"):
            _request(ceng, Wd, True, "tmpl", False, light, Wd.signer(True, "vks"), device=device, alt=alt)
        voff = _offsets([len(h) for h in Wd.holes])
        voff[i + 1] = voff[i] - 1 if voff[i] else voff[-1] + 1
        import torch
        kw = dict(var_off=_up_ints(voff, torch.int32)) if device else dict(var_off=voff)
        with pytest.raises(edc.EngineError, match="edc error -2"):
            _request(ceng, Wd, True, "tmpl", False, light, Wd.signer(True, "vks"), device=device, **kw)
        _same(_request(ceng, Wd, True, "tmpl", False, light, Wd.signer(True, "vks"), device=device), clean, "after")


# ---------------------------------------------------------------- 7. errors
def test_errors_leave_the_context_usable(edc, world):
    import ctypes
    pytest.importorskip("torch")
    Wd = world
    live0 = edc.debug_live_allocs()
    eng = edc.Engine(0)
    try:
        eng.keycache_load(Wd.keys)
        signer = dict(key_idx=list(Wd.who))
        refused = lambda **kw: pytest.raises(edc.EngineError, match="edc error -2")
        with refused():                                    # before any request
            eng.vq_last()
        Wd.thr = [0] * Wd.nc
        with refused():                                    # no powers, no history
            _request(eng, Wd, False, "k", False, True, signer)
        with refused():
            _request(eng, Wd, True, "k", False, True, signer)
        with refused():                                    # cached without a table
            _request(eng, Wd, False, "k", True, True, signer)
        eng.sigcache_create(1 << 10)
        Wd.register(eng, False)
        Wd.register(eng, True)
        st0 = eng.sigcache_stats()
        good = _request(eng, Wd, True, "tmpl", True, True, signer)
        eng.sigcache_clear()
        st0 = eng.sigcache_stats()
        sz = ctypes.sizeof(edc.EdcVqRequest)
        bad_flag = list(Wd.flag)
        bad_flag[Wd.strange_at] = 3
        host = [dict(raw=dict(size=sz - 8)), dict(raw=dict(size=sz + 8)), dict(raw=dict(result_size=8)), dict(raw=dict(reserved=1)),
                dict(raw=dict(vk=None, key_idx=None)), dict(vks=Wd.vks), dict(raw=dict(z_seed=None)),
                dict(raw=dict(ts=None, commit_tpl=None, alt_span=0, item_alt=None, var=None, var_off=None)),      # no message form
                dict(ks=Wd.ks), dict(msgs=Wd.msgs), dict(raw=dict(device=1)), dict(raw=dict(device=2)),
                dict(raw=dict(mode=2)), dict(raw=dict(alt_span=0)), dict(raw=dict(alt_span=3)), dict(raw=dict(sig=None)),
                dict(raw=dict(flag=None)), dict(flag=bad_flag), dict(key_idx=[len(Wd.keys)] + Wd.who[1:]),
                dict(versions=[3] + Wd.ver[1:])]
        for kw in host:
            kw = dict(kw)
            a = dict(hist=True, form="tmpl", cached=True, light=True, signer=signer)
            if "versions" in kw:
                sub = World.__new__(World)
                sub.__dict__.update(Wd.__dict__)
                sub.ver = kw.pop("versions")
                with refused():
                    _request(eng, sub, True, "tmpl", True, True, signer)
                continue
            if "key_idx" in kw:
                a["signer"] = dict(key_idx=kw.pop("key_idx"))
            with refused():
                _request(eng, Wd, a["hist"], a["form"], a["cached"], a["light"], a["signer"], **kw)
        noncanon = list(Wd.ks)
        noncanon[0] = bytes([0xFF]) * 32                   # a checked vote's k at or above l
        sub = World.__new__(World)
        sub.__dict__.update(Wd.__dict__)
        sub.ks = noncanon
        with refused():
            _request(eng, sub, True, "k", True, True, signer)
        dev = dict(vks=Wd.vks)
        import torch
        odd = _up(b"".join(Wd.vks), shift=8)
        with refused():                                    # a device array off its alignment
            _request(eng, Wd, True, "k", True, True, dev, device=True, vks=odd)
        with refused():                                    # a flag above 2 found on the device, on a non-member's vote
            _request(eng, Wd, True, "tmpl", True, True, dev, device=True, flag=bad_flag)
        with refused():                                    # key positions are a host form's
            _request(eng, Wd, True, "k", True, True, dev, device=True, raw=dict(key_idx=1, vk=None))
        assert eng.sigcache_stats() == st0                 # nothing looked up, nothing inserted
        empty = eng.vq_verify([0], [], [], SEED, vks=[], sigs=[], ks=[])
        assert empty["code"] == 0 and empty["n_checked"] == 0
        again = _request(eng, Wd, True, "tmpl", True, True, signer)
        _same(again, good, "after the refusals")
        warm = _request(eng, Wd, True, "tmpl", True, True, signer)
        assert warm["n_miss"] == 0
        _same(_request(eng, Wd, True, "tmpl", True, True, dev, device=True), warm, "device, warm")
        torch.cuda.synchronize()
    finally:
        eng.close()
    assert edc.debug_live_allocs() == live0


# ---------------------------------------------------------------- 8. the Python interface
@pytest.mark.parametrize("hist", [False, True], ids=["set", "hist"])
def test_python_request_against_verify_quorum(ceng, world, edc, hist):
    """Engine.vq_verify through the table gives what batch.verify_quorum(powers=None) gives without
    it; verify_quorum itself keeps refusing cached=True there."""
    Wd = world
    Wd.register(ceng, hist)
    ceng.sigcache_clear()
    vs = []
    for c in range(Wd.nc):
        v = edc.batch.Verifier(engine=ceng)
        for i in range(Wd.off[c], Wd.off[c + 1]):
            v.queue((edc.VerificationKeyBytes(Wd.vks[i]), edc.Signature(Wd.sigs[i]), Wd.msgs[i]))
        vs.append(v)
    flags = [Wd.flag[a:e] for a, e in zip(Wd.off, Wd.off[1:])]
    kw = dict(versions=Wd.ver) if hist else {}
    plain = edc.batch.verify_quorum(vs, None, flags, Wd.thr, light=True, z_seed=SEED, engine=ceng, **kw)
    with pytest.raises(ValueError):
        edc.batch.verify_quorum(vs, None, flags, Wd.thr, light=True, z_seed=SEED, engine=ceng, cached=True, **kw)

    def request():
        res = ceng.vq_verify(Wd.off, Wd.flag, Wd.thr, SEED, light=True, versions=Wd.ver if hist else None, cached=True,
                             vks=Wd.vks, sigs=Wd.sigs, msgs=Wd.msgs)
        codes = [res["item_verdicts"][a:e] for a, e in zip(Wd.off, Wd.off[1:])]
        return (res["commit_verdicts"], res["tally"], codes), res["n_miss"]
    st0 = ceng.sigcache_stats()
    cold, miss = request()
    m = ceng.vq_last()[1]
    assert cold == plain and miss == m and _delta(st0, ceng.sigcache_stats()) == [0, m, m, 0]
    warm, miss = request()
    assert warm == plain and miss == 0 and _delta(st0, ceng.sigcache_stats()) == [m, m, m, 0]
    assert plain[0][1] == edc.EDC_DOUBLE_VOTE
