"""GPU: trusting pairs of validator-set requests (include/edc.h, trust_ver / trust_threshold of
edc_vq_verify, edc_vq_trust_resolve, edc_debug_vq_trust_last): one commit judged by two sets at once,
every vote verified once.

Every expected value comes from an entry that existed before, run in the same test: request A is the
same request without the trust fields, request B the same request with commit_ver := trust_ver and
threshold := trust_threshold; the selections are two edc_vhist_resolve calls; check8 is
edc_batch_verify_prehashed's on the union list. Shapes: 13 registered keys, 3 versions, 6 commits of
8..12 votes; W is the tile."""
import ctypes
import random

import pytest

pytestmark = pytest.mark.gpu

W = 256
SEED = bytes(range(11, 43))
HOLES = (0, 1, 15, 16, 17)
IDENTITY = bytes([1]) + bytes(31)


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


def _up(b):
    import torch
    t = torch.frombuffer(bytearray(bytes(b) + bytes(16)), dtype=torch.uint8).to("cuda:0")
    torch.cuda.synchronize()
    return t


def _up_ints(xs, dtype):
    import torch
    t = torch.tensor(list(xs) or [0], dtype=dtype, device="cuda:0")
    torch.cuda.synchronize()
    return t


class World:
    """Positions 0 and 1 never sign (power 1); 2..12 are the signers s0..s10. Version 0, the trusted
    set, knows s6..s10 (10 each); s0..s5 join at version 1 (10 each); at version 2 s10 leaves and s3
    goes to 12. Totals 52 / 112 / 104, so 1/3 of version 0 is 17 and 2/3 of version 2 is 69.
    Commit 0 (own 2, trusted 0), s0..s9 in order: A checks s0..s6, B checks s6 and s7: s0..s5 are
      A-only, s6 both, s7 B-only (the six early signers the trusted set does not know carry A to its
      quorum while B has counted nothing yet).
    Commit 1 (2, 1), s9..s0: B's four votes are a prefix of A's seven.
    Commit 2 (2, 0) starts with s10, a member of the trusted set only: B-only; an absent and a nil vote.
    Commit 3 (1, 0), eight votes, all checked by A.
    Commit 4 (2, 0) is short on side A and has its third of the trusted set.
    Commit 5 (2, 2), both sides on one set, with a second s5 vote behind both quorums: a double
      vote on both sides in full mode only.
    dup = (commit, signer): a second vote of that signer put at the commit's head."""

    def __init__(self, eng, edc, dup=None):
        rnd = random.Random("vq trust world")
        self.edc, N = edc, edc.VHIST_NOT_MEMBER
        twin = rnd.randbytes(31)
        self.seeds = [rnd.randbytes(32) for _ in range(11)]
        skeys, _ = eng.sign(self.seeds, [b""] * 11)
        self.keys = [twin + b"\x01", twin + b"\x02"] + list(skeys)
        self.base = [1, 1] + [N] * 6 + [10] * 5
        self.updates = [[(p, 10) for p in range(2, 8)], [(12, N), (5, 12)]]
        C, A, NIL = edc.VOTE_COMMIT, edc.VOTE_ABSENT, edc.VOTE_NIL
        s = lambda *xs: [x + 2 for x in xs]
        commits = [
            (s(0, 1, 2, 3, 4, 5, 6, 7, 8, 9), [C] * 10),
            (s(9, 8, 7, 6, 5, 4, 3, 2, 1, 0), [C] * 10),
            (s(10, 6, 7, 0, 1, 2, 3, 4, 5, 8, 9), [C, C, C, C, A, NIL, C, C, C, C, C]),
            (s(0, 1, 2, 3, 4, 5, 6, 7), [C] * 8),
            (s(0, 1, 2, 3, 4, 5, 6, 7), [C, C, C, A, A, A, C, C]),
            (s(5, 6, 7, 8, 9, 0, 1, 2, 3, 4, 5), [C] * 11),
        ]
        if dup is not None:
            c, who = dup
            commits[c] = ([who + 2] + commits[c][0], [C] + commits[c][1])
        self.off = _offsets([len(c[0]) for c in commits])
        self.n, self.nc = self.off[-1], len(commits)
        self.who = [p for c in commits for p in c[0]]
        self.flag = [f for c in commits for f in c[1]]
        self.ver = [2, 2, 2, 1, 2, 2]
        self.tver = [0, 1, 0, 0, 0, 2]
        self.T = edc.batch.Templates([b"", rnd.randbytes(37), rnd.randbytes(5)], [rnd.randbytes(21), b"", rnd.randbytes(64)])
        self.ctpl, self.span = [0, 1, 0, 1, 1, 0], 2
        while True:     # no two votes are one item (same signer, same message): the table would hold them as one record
            self.alt = [rnd.randrange(2) for _ in range(self.n)]
            self.holes = [rnd.randbytes(HOLES[(i + rnd.randrange(2)) % len(HOLES)]) for i in range(self.n)]
            self.tpl = [self.ctpl[self.commit_of(i)] + self.alt[i] for i in range(self.n)]
            self.msgs = self.T.materialize(self.tpl, self.holes)
            if len(set(zip(self.who, self.msgs))) == self.n:
                break
        assert {len(h) for h in self.holes} == set(HOLES)
        self.vks, self.sigs = eng.sign([self.seeds[p - 2] for p in self.who], self.msgs)
        self.ks = eng.challenge(self.vks, self.sigs, self.msgs)

    def commit_of(self, i):
        return max(c for c in range(self.nc) if self.off[c] <= i)

    def register(self, eng):
        eng.keycache_load(self.keys)
        eng.vhist_set(self.base, self.updates)
        totals, _ = eng.vhist_totals()
        assert totals == [52, 112, 104]
        self.thr = [2 * totals[v] // 3 for v in self.ver]
        self.tthr = [totals[v] // 3 for v in self.tver]

    def signer(self, keyform):
        return dict(key_idx=list(self.who)) if keyform == "key_idx" else dict(vks=list(self.vks))


@pytest.fixture(scope="module")
def world(ceng, edc):
    return World(ceng, edc)


def _request(eng, Wd, form, cached, light, signer, ver, thr, device=False, sigs=None, **kw):
    import torch
    sigs = Wd.sigs if sigs is None else sigs
    a = dict(light=light, versions=ver, cached=cached)
    if form == "tmpl":
        a.update(templates=Wd.T, commit_tpl=Wd.ctpl, alt_span=Wd.span)
    if not device:
        a.update(signer, sigs=sigs)
        if form == "tmpl":
            a.update(item_alt=Wd.alt, holes=Wd.holes)
        elif form == "msgs":
            a.update(msgs=Wd.msgs)
        else:
            a.update(ks=Wd.ks)
        a.update(kw)
        return eng.vq_verify(Wd.off, Wd.flag, thr, SEED, **a)
    a.update(device=True, vks=_up(b"".join(signer["vks"])), sigs=_up(b"".join(sigs)))
    if form == "tmpl":
        var = b"".join(Wd.holes)
        a.update(item_alt=_up(bytes(Wd.alt)), holes=_up(var), var_bytes=len(var),
                 var_off=_up_ints(_offsets([len(h) for h in Wd.holes]), torch.int32))
    elif form == "msgs":
        a.update(msgs=_up(b"".join(Wd.msgs)), msg_off=_up_ints(_offsets([len(m) for m in Wd.msgs]), torch.int64))
    else:
        a.update(ks=_up(b"".join(Wd.ks)))
    a.update(kw)
    return eng.vq_verify(Wd.off, _up(bytes(Wd.flag)), thr, SEED, **a)


def _model_select(off, power, flag, thr, light):
    """quorum_select (csrc/quorum.h) in Python: the checked bytes and planned[]"""
    checked, planned = [], []
    for c in range(len(off) - 1):
        run = 0
        for i in range(off[c], off[c + 1]):
            chk = (flag[i] == 1 and run <= thr[c]) if light else flag[i] != 0
            if chk and flag[i] == 1:
                run += power[i]
            checked.append(int(chk))
        planned.append(run)
    return checked, planned


def _sides(eng, Wd, light, signer, tver=None, no_trust=(), thr=None):
    """both sides' edc_vhist_resolve; the commits in no_trust have no trusting side"""
    tver = Wd.tver if tver is None else tver
    thr = Wd.thr if thr is None else thr
    ra = eng.vhist_resolve(Wd.off, Wd.ver, Wd.flag, thr, light=light, **signer)
    rb = eng.vhist_resolve(Wd.off, [0 if c in no_trust else v for c, v in enumerate(tver)], Wd.flag, Wd.tthr, light=light,
                           **signer)
    for r, thr in ((ra, thr), (rb, Wd.tthr)):         # the Python model of the selection agrees with the entry
        assert (r["checked"], r["planned"]) == _model_select(Wd.off, r["power"], r["flag"], thr, light)
    for c in no_trust:
        for i in range(Wd.off[c], Wd.off[c + 1]):
            rb["pos"][i], rb["power"][i], rb["flag"][i], rb["checked"][i] = 0xFFFFFFFF, 0, 0, 0
        rb["planned"][c], rb["dv"][c] = 0, 0
    return ra, rb


def _check_pair(eng, Wd, edc, got, A, B, ra, rb, what, no_trust=(), cached=False):
    """the contract: got (the paired request) against request A, request B and the two selections"""
    ca, cb = ra["checked"], rb["checked"]
    union = [i for i in range(Wd.n) if ca[i] or cb[i]]
    for key in ("commit_verdicts", "tally", "n_bad_commits"):
        assert got[key] == A[key], (what, key)
    tv, tt = list(B["commit_verdicts"]), list(B["tally"])
    for c in no_trust:
        tv[c], tt[c] = edc.EDC_OK, 0
    assert got["trust_verdicts"] == tv and got["trust_tally"] == tt, what
    assert got["n_bad_trust"] == sum(1 for v in tv if v), what
    both = got["commit_verdicts"] + tv
    assert got["code"] == next((c for c in (1, 4, 3) if c in both), 0), what
    assert got["n_checked"] == len(union), what
    for i in range(Wd.n):
        want = edc.NOT_CHECKED
        if ca[i]:
            want = A["item_verdicts"][i]
        if cb[i]:
            assert not ca[i] or B["item_verdicts"][i] == want, (what, i)
            want = B["item_verdicts"][i]
        assert got["item_verdicts"][i] == want, (what, i)
    counts = (sum(ca), sum(cb), sum(1 for a, b in zip(ca, cb) if a and b), len(union))
    assert eng.vq_trust_last() == counts, what
    assert eng.vq_last()[1] == len(union) and eng.vq_last()[6] == 0, what
    return union, counts


def _union_check8(eng, Wd, union, sigs=None):
    sigs = Wd.sigs if sigs is None else sigs
    return eng.batch_verify_prehashed([Wd.vks[i] for i in union], [sigs[i] for i in union], [Wd.ks[i] for i in union],
                                      z_seed=SEED, want_check8=True)


FILL = 0xA5
OUTS = ("commit_verdicts", "item_verdicts", "tally", "n_bad_commits", "n_checked", "n_miss", "check8", "trust_verdicts",
        "trust_tally", "n_bad_trust")


def _raw(eng, Wd, edc, light=True, ver=None, thr=None, tver=None, tthr=None, who=None, cached=False, rq_size=None,
         rs_size=None, trust_out=True):
    """edc_vq_verify called directly on host votes by key index with prehashed k, every result buffer
    filled with FILL beforehand -> (return value, {output name: its bytes afterwards}). ver None: no
    commit_ver; tver / tthr None: that field NULL; trust_out False: NULL trust outputs."""
    nc, n = Wd.nc, Wd.n
    u32, u64 = lambda xs: (ctypes.c_uint32 * len(xs))(*xs), lambda xs: (ctypes.c_uint64 * len(xs))(*xs)
    arrays = dict(commit_off=u32(Wd.off), threshold=u64(Wd.thr if thr is None else thr), key_idx=u32(Wd.who if who is None else who),
                  sig=ctypes.create_string_buffer(b"".join(Wd.sigs), 64 * n), flag=ctypes.create_string_buffer(bytes(Wd.flag), n),
                  k=ctypes.create_string_buffer(b"".join(Wd.ks), 32 * n), z_seed=ctypes.create_string_buffer(SEED, 32))
    if ver is not None:
        arrays["commit_ver"] = u32(ver)
    if tver is not None:
        arrays["trust_ver"] = u32(tver)
    if tthr is not None:
        arrays["trust_threshold"] = u64(tthr)
    rq = edc.EdcVqRequest(size=ctypes.sizeof(edc.EdcVqRequest) if rq_size is None else rq_size, mode=int(light),
                          cached=int(cached), nc=nc, **{name: ctypes.addressof(a) for name, a in arrays.items()})
    sizes = dict(commit_verdicts=nc, item_verdicts=n, tally=8 * nc, n_bad_commits=4, n_checked=8, n_miss=8, check8=32,
                 trust_verdicts=nc, trust_tally=8 * nc, n_bad_trust=4)
    bufs = {name: ctypes.create_string_buffer(bytes([FILL]) * size, size) for name, size in sizes.items()}
    rs = edc.EdcVqResult(size=ctypes.sizeof(edc.EdcVqResult) if rs_size is None else rs_size,
                         **{name: ctypes.addressof(b) for name, b in bufs.items() if trust_out or not name.endswith("trust")
                            and not name.startswith("trust")})
    rc = eng.lib.edc_vq_verify(eng.ctx, ctypes.byref(rq), ctypes.byref(rs))
    return rc, {name: b.raw for name, b in bufs.items()}


def _untouched(out, names=OUTS):
    return all(out[name] == bytes([FILL]) * len(out[name]) for name in names)


# ---------------------------------------------------------------- 1. the equalities, every form
FORMS = [("k", "key_idx", False), ("k", "vks", False), ("k", "vks", True), ("msgs", "key_idx", False), ("msgs", "vks", True),
         ("tmpl", "key_idx", False), ("tmpl", "vks", False), ("tmpl", "vks", True)]


@pytest.mark.parametrize("form,keyform,device", FORMS)
@pytest.mark.parametrize("light", [True, False])
def test_pair_equals_its_two_requests(ceng, world, edc, form, keyform, device, light):
    Wd = world
    Wd.register(ceng)
    signer = Wd.signer(keyform)
    ra, rb = _sides(ceng, Wd, light, signer)
    A = _request(ceng, Wd, form, False, light, signer, Wd.ver, Wd.thr, device)
    B = _request(ceng, Wd, form, False, light, signer, Wd.tver, Wd.tthr, device)
    for cached in (False, True):
        what = (form, keyform, device, light, cached)
        ceng.sigcache_clear()
        got = _request(ceng, Wd, form, cached, light, signer, Wd.ver, Wd.thr, device, trust_versions=Wd.tver,
                       trust_thresholds=Wd.tthr)
        union, counts = _check_pair(ceng, Wd, edc, got, A, B, ra, rb, what)
        a, b, ab, u = counts
        assert a - ab > 0 and b - ab > 0 and ab > 0, what            # A-only, B-only and shared votes
        assert got["n_checked"] == u < a + b, what
        code, check8 = _union_check8(ceng, Wd, union)
        assert (code, check8) == (0, IDENTITY) and got["check8"] == check8, what
        if cached:
            assert got["n_miss"] == u, what
    if light:                                                        # the world is what its docstring says
        side = [(1 if a else 0) | (2 if b else 0) for a, b in zip(ra["checked"], rb["checked"])]
        assert side[:10] == [1, 1, 1, 1, 1, 1, 3, 2, 0, 0] and side[Wd.off[2]] == 2
        assert got["commit_verdicts"] == [0, 0, 0, 0, edc.EDC_QUORUM_SHORT, 0] and got["trust_verdicts"] == [0] * 6
    else:
        assert got["commit_verdicts"][5] == got["trust_verdicts"][5] == edc.EDC_DOUBLE_VOTE


def test_resolve_equals_two_history_resolves(ceng, world, edc):
    Wd = world
    Wd.register(ceng)
    for light in (True, False):
        for keyform in ("key_idx", "vks"):
            signer = Wd.signer(keyform)
            ra, rb = _sides(ceng, Wd, light, signer)
            r = ceng.vq_trust_resolve(Wd.off, Wd.ver, Wd.tver, Wd.flag, Wd.thr, Wd.tthr, light=light, **signer)
            for side, want in (("a", ra), ("b", rb)):
                for key in ("pos", "power", "flag", "checked", "planned", "dv"):
                    assert r[side][key] == want[key], (light, keyform, side, key)
            assert r["side"] == [(1 if a else 0) | (2 if b else 0) for a, b in zip(ra["checked"], rb["checked"])]
            assert r["n_checked"] == sum(1 for x in r["side"] if x)


# ---------------------------------------------------------------- 2. one bad signature
@pytest.mark.parametrize("where,item,a_bad,b_bad", [("b_only", 7, False, True), ("a_only", 0, True, False), ("both", 6, True, True)])
@pytest.mark.parametrize("form", ["k", "tmpl"])
def test_one_bad_signature(ceng, world, edc, form, where, item, a_bad, b_bad):
    Wd = world
    Wd.register(ceng)
    signer = Wd.signer("vks")
    sigs = list(Wd.sigs)
    sigs[item] = sigs[item][:40] + bytes([sigs[item][40] ^ 4]) + sigs[item][41:]
    thr = list(Wd.thr)
    thr[4] = 40                 # commit 4's five votes carry 50: with this threshold every commit is OK on side A
    ra, rb = _sides(ceng, Wd, True, signer, thr=thr)
    assert (bool(ra["checked"][item]), bool(rb["checked"][item])) == (where != "b_only", where != "a_only")
    A = _request(ceng, Wd, form, False, True, signer, Wd.ver, thr, sigs=sigs)
    B = _request(ceng, Wd, form, False, True, signer, Wd.tver, Wd.tthr, sigs=sigs)
    got = _request(ceng, Wd, form, False, True, signer, Wd.ver, thr, sigs=sigs, trust_versions=Wd.tver, trust_thresholds=Wd.tthr)
    union, _ = _check_pair(ceng, Wd, edc, got, A, B, ra, rb, (form, where))
    assert got["code"] == 1 and got["item_verdicts"][item] == edc.EDC_INVALID_SIGNATURE
    assert (got["commit_verdicts"][0] == edc.EDC_INVALID_SIGNATURE) == a_bad
    assert (got["trust_verdicts"][0] == edc.EDC_INVALID_SIGNATURE) == b_bad
    if not a_bad:
        assert got["commit_verdicts"] == [0] * Wd.nc and got["n_bad_commits"] == 0            # every A verdict is OK
    else:
        assert got["commit_verdicts"] == [edc.EDC_INVALID_SIGNATURE] + [0] * (Wd.nc - 1)
    assert got["trust_verdicts"] == [edc.EDC_INVALID_SIGNATURE if b_bad else 0] + [0] * (Wd.nc - 1)
    code, check8 = _union_check8(ceng, Wd, union, sigs)
    assert code == 1 and check8 != IDENTITY and got["check8"] == check8


# ---------------------------------------------------------------- 3. double votes per side
@pytest.mark.parametrize("dup,a_dv,b_dv", [((2, 10), False, True), ((0, 0), True, False)])
def test_double_vote_on_one_side(ceng, edc, dup, a_dv, b_dv):
    Wd = World(ceng, edc, dup)
    Wd.register(ceng)
    signer = Wd.signer("key_idx")
    c = dup[0]
    ra, rb = _sides(ceng, Wd, True, signer)
    assert (ra["dv"][c], rb["dv"][c]) == (int(a_dv), int(b_dv))
    A = _request(ceng, Wd, "k", False, True, signer, Wd.ver, Wd.thr)
    B = _request(ceng, Wd, "k", False, True, signer, Wd.tver, Wd.tthr)
    got = _request(ceng, Wd, "k", False, True, signer, Wd.ver, Wd.thr, trust_versions=Wd.tver, trust_thresholds=Wd.tthr)
    _check_pair(ceng, Wd, edc, got, A, B, ra, rb, dup)
    assert (got["commit_verdicts"][c] == edc.EDC_DOUBLE_VOTE) == a_dv
    assert (got["trust_verdicts"][c] == edc.EDC_DOUBLE_VOTE) == b_dv
    assert got["code"] == 4
    # the second vote behind both quorums (commit 5) raises nothing in light mode
    assert got["commit_verdicts"][5] == got["trust_verdicts"][5] == edc.EDC_OK


# ---------------------------------------------------------------- 4. commits without a trusting side
@pytest.mark.parametrize("light", [True, False])
@pytest.mark.parametrize("form", ["k", "tmpl"])
def test_no_trust_commits(ceng, world, edc, form, light):
    Wd = world
    Wd.register(ceng)
    signer = Wd.signer("key_idx")
    none = (0, 2, 5)
    tver = [edc.NO_TRUST if c in none else v for c, v in enumerate(Wd.tver)]
    ra, rb = _sides(ceng, Wd, light, signer, no_trust=none)
    A = _request(ceng, Wd, form, False, light, signer, Wd.ver, Wd.thr)
    B = _request(ceng, Wd, form, False, light, signer, [0 if c in none else v for c, v in enumerate(Wd.tver)], Wd.tthr)
    got = _request(ceng, Wd, form, False, light, signer, Wd.ver, Wd.thr, trust_versions=tver, trust_thresholds=Wd.tthr)
    _check_pair(ceng, Wd, edc, got, A, B, ra, rb, (form, light), no_trust=none)
    r = ceng.vq_trust_resolve(Wd.off, Wd.ver, tver, Wd.flag, Wd.thr, Wd.tthr, light=light, **signer)
    for key in ("pos", "power", "flag", "checked", "planned", "dv"):
        assert r["b"][key] == rb[key], key
    for c in none:
        assert got["trust_verdicts"][c] == edc.EDC_OK and got["trust_tally"][c] == 0
        assert all(r["side"][i] == ra["checked"][i] for i in range(Wd.off[c], Wd.off[c + 1]))


# ---------------------------------------------------------------- 5. tile edges
def _int_world(eng, rnd, sizes, nver=4, m=64):
    """registered keys that never sign anything: the selections run on positions and flags alone"""
    keys = [rnd.randbytes(32) for _ in range(m)]
    eng.keycache_load(keys)
    N = 0xFFFFFFFFFFFFFFFF
    base = [rnd.choice([N, 3, 5, 8]) for _ in range(m)]
    ups = [[(p, rnd.choice([N, 2, 7, 11])) for p in rnd.sample(range(m), 9)] for _ in range(nver - 1)]
    eng.vhist_set(base, ups)
    totals, _ = eng.vhist_totals()
    off = _offsets(sizes)
    ver = [rnd.randrange(nver) for _ in sizes]
    tver = [rnd.randrange(nver) for _ in sizes]
    return off, ver, tver, [2 * totals[v] // 3 for v in ver], [totals[v] // 3 for v in tver]


def _check_resolve(eng, off, ver, tver, flag, thr, tthr, kidx, light):
    ra = eng.vhist_resolve(off, ver, flag, thr, light=light, key_idx=kidx)
    rb = eng.vhist_resolve(off, tver, flag, tthr, light=light, key_idx=kidx)
    r = eng.vq_trust_resolve(off, ver, tver, flag, thr, tthr, light=light, key_idx=kidx)
    for side, want in (("a", ra), ("b", rb)):
        for key in ("pos", "power", "flag", "checked", "planned", "dv"):
            assert r[side][key] == want[key], (side, key)
    side = [(1 if a else 0) | (2 if b else 0) for a, b in zip(ra["checked"], rb["checked"])]
    assert r["side"] == side and r["n_checked"] == sum(1 for x in side if x)
    return ra, rb


# Commits begin at items 255, 256 and 257. The one that begins at 257 runs to item 1023: it ends tile 1
# and spans tiles 2 and 3 whole, so two consecutive tiles hold no commit start and the carry passes
# through two aggregates without a flag. Empty commits sit at 257 and at the tile start 1024. The
# commit that begins at the tile start 1024 spans tiles 4 and 5 whole. 1,566 items: the shape does
# not fit into fewer (257 + 3 W - 1 = 4 W).
TILE_SIZES = [255, 1, 1, 0, 0, 3 * W - 1, 0, 2 * W, 30]
assert _offsets(TILE_SIZES) == [0, 255, 256, 257, 257, 257, 4 * W, 4 * W, 6 * W, 6 * W + 30]


def test_tile_edges(ceng, edc):
    rnd = random.Random("vq trust tiles")
    off, ver, tver, thr, tthr = _int_world(ceng, rnd, TILE_SIZES)
    n = off[-1]
    kidx = [rnd.randrange(64) for _ in range(n)]
    flag = [0] * n                                  # nearly all absent
    for i in rnd.sample(range(n), 90) + [254, 255, 256, 257, 511, 512, 767, 768, 1023, 1024, 1279, 1280, 1535, 1536]:
        flag[i] = rnd.choice([1, 1, 1, 2])
    for light in (True, False):
        _check_resolve(ceng, off, ver, tver, flag, thr, tthr, kidx, light)
    dense = [1] * n                                 # every tile full of counted votes
    _check_resolve(ceng, off, ver, tver, dense, thr, tthr, kidx, True)


def test_tile_edges_verify(ceng, edc):
    """one verify of the tile-edge shape: at most 300 signed votes, the rest absent"""
    rnd = random.Random("vq trust tiles verify")
    sizes = TILE_SIZES
    m = 24
    seeds = [rnd.randbytes(32) for _ in range(m)]
    keys, _ = ceng.sign(seeds, [b""] * m)
    ceng.keycache_load(keys)
    N = edc.VHIST_NOT_MEMBER
    ceng.vhist_set([N if p % 3 == 0 else 5 for p in range(m)], [[(p, 7) for p in range(0, m, 3)], [(1, N), (2, N)]])
    totals, _ = ceng.vhist_totals()
    off = _offsets(sizes)
    n, nc = off[-1], len(sizes)
    ver, tver = [2, 1, 2, 0, 0, 2, 1, 2, 1], [0, 0, 1, 0, 0, 0, 0, 1, edc.NO_TRUST]
    thr = [2 * totals[v] // 3 for v in ver]
    tthr = [0 if v == edc.NO_TRUST else totals[v] // 3 for v in tver]
    kidx = [i % m for i in range(n)]
    flag = [0] * n
    for i in (list(range(230, 270)) + list(range(500, 530)) + list(range(1000, 1050)) + list(range(1270, 1290))
              + list(range(1520, 1566)) + rnd.sample(range(270, 500), 100)):
        flag[i] = 1
    assert sum(flag) <= 300
    msgs = [b"v%d" % i for i in range(n)]
    signed = [i for i in range(n) if flag[i]]
    _, ss = ceng.sign([seeds[kidx[i]] for i in signed], [msgs[i] for i in signed])
    sigs = [bytes(64)] * n
    for i, s in zip(signed, ss):
        sigs[i] = s
    a = dict(light=True, key_idx=kidx, sigs=sigs, msgs=msgs)
    A = ceng.vq_verify(off, flag, thr, SEED, versions=ver, **a)
    tv0 = [0 if v == edc.NO_TRUST else v for v in tver]
    B = ceng.vq_verify(off, flag, tthr, SEED, versions=tv0, **a)
    got = ceng.vq_verify(off, flag, thr, SEED, versions=ver, trust_versions=tver, trust_thresholds=tthr, **a)
    ra = ceng.vhist_resolve(off, ver, flag, thr, key_idx=kidx)
    rb = ceng.vhist_resolve(off, tv0, flag, tthr, key_idx=kidx)
    for i in range(off[8], off[9]):
        rb["checked"][i] = 0
    assert got["commit_verdicts"] == A["commit_verdicts"] and got["tally"] == A["tally"]
    assert got["trust_verdicts"][:8] == B["commit_verdicts"][:8] and got["trust_tally"][:8] == B["tally"][:8]
    assert got["trust_verdicts"][8] == 0 and got["trust_tally"][8] == 0
    union = [i for i in range(n) if ra["checked"][i] or rb["checked"][i]]
    assert got["n_checked"] == len(union) and 0 < len(union) < sum(ra["checked"]) + sum(rb["checked"])
    assert [i for i in range(n) if got["item_verdicts"][i] != edc.NOT_CHECKED] == union
    assert all(got["item_verdicts"][i] == 0 for i in union)
    ks = ceng.challenge([keys[kidx[i]] for i in union], [sigs[i] for i in union], [msgs[i] for i in union])
    code, check8 = ceng.batch_verify_prehashed([keys[kidx[i]] for i in union], [sigs[i] for i in union], ks, z_seed=SEED,
                                               want_check8=True)
    assert code == 0 and got["check8"] == check8


# ---------------------------------------------------------------- 6. past one carry pass
def test_past_one_carry_pass(ceng, edc):
    """n = 262,144 + 600 by key index: more than 1024 tiles, so the carry and the scan of the union's
    tile counts run more than one pass; a commit straddles item 262,144 and the counted-power bound
    is crossed inside it on both sides"""
    rnd = random.Random("vq trust carry")
    P = 1024 * W
    sizes = [150] * (P // 150 - 1)
    sizes.append(P - sum(sizes) + 300)              # straddles item P
    sizes += [150, 150]
    assert sum(sizes) == P + 600
    off, ver, tver, thr, tthr = _int_world(ceng, rnd, sizes)
    n = off[-1]
    c = len(sizes) - 3
    assert off[c] < P < off[c + 1]
    kidx = [rnd.randrange(64) for _ in range(n)]
    flag = [1 if rnd.random() < 0.9 else rnd.choice([0, 2]) for _ in range(n)]
    _check_resolve(ceng, off, ver, tver, flag, thr, tthr, kidx, True)
    ra, rb = _check_resolve(ceng, off, ver, tver, flag, thr, tthr, kidx, False)
    assert any(ra["checked"][P:off[c + 1]]) and any(rb["checked"][P:off[c + 1]])      # full mode checks on both sides of P
    # the bound 2^63 - 1 on a commit's counted power, crossed behind item P on side B alone: position
    # 0 carries 2^62 at version 1 only, and votes twice in the straddling commit, once on each side of P
    ceng.vhist_set([1] * 64, [[(0, 1 << 62)]])
    ver2, tver2 = [0] * len(sizes), [0] * len(sizes)
    tver2[c] = 1
    flag2, kidx2 = [0] * n, [1 + i % 63 for i in range(n)]
    for i in (P - 3, P + 5):
        flag2[i], kidx2[i] = 1, 0
    big = [1 << 62] * len(sizes)
    ok = ceng.vq_trust_resolve(off, ver2, ver2, flag2, big, big, key_idx=kidx2)
    assert ok["n_checked"] == 2
    with pytest.raises(edc.EngineError, match="edc error -2"):
        ceng.vq_trust_resolve(off, ver2, tver2, flag2, big, big, key_idx=kidx2)
    flag2[P + 5] = 0
    assert ceng.vq_trust_resolve(off, ver2, tver2, flag2, big, big, key_idx=kidx2)["b"]["planned"][c] == 1 << 62


# ---------------------------------------------------------------- 7. the previous sizeof
def test_previous_sizeof(ceng, world, edc):
    """full mode, where a pair writes trust_verdicts[5] = EDC_DOUBLE_VOTE; every buffer pre-filled"""
    Wd = world
    Wd.register(ceng)
    old_rq, old_rs = edc.EdcVqRequest.trust_ver.offset, edc.EdcVqResult.trust_verdicts.offset
    assert (old_rq, old_rs) == (ctypes.sizeof(edc.EdcVqRequest) - 16, ctypes.sizeof(edc.EdcVqResult) - 24)
    TRUST = ("trust_verdicts", "trust_tally", "n_bad_trust")
    kw = dict(light=False, ver=Wd.ver)
    pair = dict(tver=Wd.tver, tthr=Wd.tthr)
    rc_pair, out_pair = _raw(ceng, Wd, edc, **kw, **pair)
    assert rc_pair == 4 and out_pair["trust_verdicts"][5] == edc.EDC_DOUBLE_VOTE and not _untouched(out_pair, TRUST)
    # the request: with the previous sizeof the trust fields read as NULL, whatever lies behind it
    rc_null, out_null = _raw(ceng, Wd, edc, **kw)
    assert _untouched(out_null, TRUST + ("n_miss",)) and out_null["n_checked"] != out_pair["n_checked"]
    for rs_size in (None, old_rs):
        assert _raw(ceng, Wd, edc, rq_size=old_rq, rs_size=rs_size, **kw, **pair) == (rc_null, out_null)
    # the result: with the previous sizeof the trust outputs read as NULL; the pair itself still runs
    rc_nout, out_nout = _raw(ceng, Wd, edc, trust_out=False, **kw, **pair)
    assert rc_nout == rc_pair and _untouched(out_nout, TRUST) and out_nout["n_checked"] == out_pair["n_checked"]
    assert _raw(ceng, Wd, edc, rs_size=old_rs, **kw, **pair) == (rc_nout, out_nout)
    for key in OUTS[:7]:
        assert out_nout[key] == out_pair[key], key
    for bad in (old_rq - 8, old_rq + 8, ctypes.sizeof(edc.EdcVqRequest) + 8):
        rc, out = _raw(ceng, Wd, edc, rq_size=bad, **kw, **pair)
        assert rc == -2 and _untouched(out), bad
    for bad in (old_rs - 8, old_rs + 8, old_rs + 16, ctypes.sizeof(edc.EdcVqResult) + 8):
        rc, out = _raw(ceng, Wd, edc, rs_size=bad, **kw, **pair)
        assert rc == -2 and _untouched(out), bad


# ---------------------------------------------------------------- 8. errors
def test_errors_change_nothing(ceng, world, edc):
    Wd = world
    Wd.register(ceng)
    signer = Wd.signer("key_idx")
    pair = dict(trust_versions=Wd.tver, trust_thresholds=Wd.tthr)
    ceng.sigcache_clear()
    good = _request(ceng, Wd, "k", True, True, signer, Wd.ver, Wd.thr, **pair)
    state = lambda: (ceng.vq_last(), ceng.vq_trust_last(), ceng.sigcache_stats())
    before = state()
    past = list(Wd.tver)
    past[3] = 3
    host = [
        dict(ver=None, tver=Wd.tver, tthr=Wd.tthr),            # trust_ver without commit_ver
        dict(ver=Wd.ver, tver=Wd.tver),                        # ... without trust_threshold
        dict(ver=Wd.ver, tthr=Wd.tthr),                        # ... and the reverse
        dict(ver=Wd.ver, tver=past, tthr=Wd.tthr),             # a version past the history that is no sentinel
    ]
    for kw in host:
        rc, out = _raw(ceng, Wd, edc, cached=True, **kw)        # every output keeps its fill
        assert rc == -2 and _untouched(out) and state() == before, kw
        a = dict(light=True, cached=True, ks=Wd.ks, sigs=Wd.sigs, versions=kw["ver"], trust_versions=kw.get("tver"),
                 trust_thresholds=kw.get("tthr"), **signer)
        with pytest.raises(edc.EngineError, match="edc error -2"):      # and through the Python layer
            ceng.vq_verify(Wd.off, Wd.flag, Wd.thr, SEED, **a)
        assert state() == before, kw
    # a device-side error on side B alone: s10 carries 2^62 at version 0 only and votes twice in commit 2,
    # so side B's counted power reaches 2^63 there while side A never counts it
    N = edc.VHIST_NOT_MEMBER
    ceng.vhist_set([1, 1] + [N] * 6 + [10] * 4 + [1 << 62], Wd.updates)
    who = list(Wd.who)
    who[Wd.off[2] + 1] = 12
    big = [1 << 62] * Wd.nc
    rc, out = _raw(ceng, Wd, edc, ver=Wd.ver, who=who, cached=True)          # side A alone is a good request
    assert rc >= 0 and not _untouched(out, ("commit_verdicts",))
    for light in (True, False):
        before = state()
        rc, out = _raw(ceng, Wd, edc, light=light, ver=Wd.ver, tver=Wd.tver, tthr=big, who=who, cached=True)
        assert rc == -2 and _untouched(out) and state() == before, light
    with pytest.raises(edc.EngineError, match="edc error -2"):
        ceng.vq_verify(Wd.off, Wd.flag, Wd.thr, SEED, versions=Wd.ver, key_idx=who, sigs=Wd.sigs, ks=Wd.ks, cached=True,
                       trust_versions=Wd.tver, trust_thresholds=big)
    assert state() == before
    # the context stays usable
    Wd.register(ceng)
    ceng.sigcache_clear()
    again = _request(ceng, Wd, "k", True, True, signer, Wd.ver, Wd.thr, **pair)
    assert again == good


# ---------------------------------------------------------------- 8b. batch.verify_quorum
@pytest.mark.parametrize("light", [True, False])
def test_batch_verify_quorum_reports_both_sides(ceng, world, edc, light):
    Wd = world
    Wd.register(ceng)
    vs = []
    for c in range(Wd.nc):
        v = edc.batch.Verifier()
        for i in range(Wd.off[c], Wd.off[c + 1]):
            v.queue((Wd.vks[i], Wd.sigs[i], Wd.msgs[i]))
        vs.append(v)
    flags = [Wd.flag[Wd.off[c]:Wd.off[c + 1]] for c in range(Wd.nc)]
    want = ceng.vq_verify(Wd.off, Wd.flag, Wd.thr, SEED, light=light, versions=Wd.ver, vks=Wd.vks, sigs=Wd.sigs, msgs=Wd.msgs,
                          trust_versions=Wd.tver, trust_thresholds=Wd.tthr)
    got = edc.batch.verify_quorum(vs, None, flags, Wd.thr, light=light, z_seed=SEED, engine=ceng, versions=Wd.ver,
                                  trust_versions=Wd.tver, trust_thresholds=Wd.tthr)
    assert len(got) == 5
    assert got[0] == want["commit_verdicts"] and got[1] == want["tally"]
    assert [x for c in got[2] for x in c] == want["item_verdicts"]
    assert got[3] == want["trust_verdicts"] and got[4] == want["trust_tally"]
    three = edc.batch.verify_quorum(vs, None, flags, Wd.thr, light=light, z_seed=SEED, engine=ceng, versions=Wd.ver)
    assert len(three) == 3 and three[0] == got[0] and three[1] == got[1]
    if light:
        assert three[2] != got[2]           # the pair also checks side B's votes


# ---------------------------------------------------------------- 9. cached
@pytest.mark.parametrize("form", ["k", "tmpl"])
def test_cached_pair(ceng, world, edc, form):
    Wd = world
    Wd.register(ceng)
    signer = Wd.signer("key_idx")
    pair = dict(trust_versions=Wd.tver, trust_thresholds=Wd.tthr)
    plain = _request(ceng, Wd, form, False, True, signer, Wd.ver, Wd.thr, **pair)
    ceng.sigcache_clear()
    s0 = ceng.sigcache_stats()
    first = _request(ceng, Wd, form, True, True, signer, Wd.ver, Wd.thr, **pair)
    s1 = ceng.sigcache_stats()
    assert first["n_miss"] == first["n_checked"] == plain["n_checked"]
    assert s1["inserted"] - s0["inserted"] == first["n_checked"] and ceng.vq_last()[5] == first["n_checked"]
    second = _request(ceng, Wd, form, True, True, signer, Wd.ver, Wd.thr, **pair)
    assert second["n_miss"] == 0 and ceng.sigcache_stats()["hits"] - s1["hits"] == first["n_checked"]
    for key in ("code", "commit_verdicts", "tally", "n_bad_commits", "trust_verdicts", "trust_tally", "n_bad_trust",
                "item_verdicts", "n_checked"):
        assert first[key] == plain[key] and second[key] == plain[key], key
    # a B-only vote with a bad signature is never recorded: the failing call inserts nothing for it
    ceng.sigcache_clear()
    sigs = list(Wd.sigs)
    sigs[7] = sigs[7][:40] + bytes([sigs[7][40] ^ 4]) + sigs[7][41:]
    bad1 = _request(ceng, Wd, form, True, True, signer, Wd.ver, Wd.thr, sigs=sigs, **pair)
    assert bad1["code"] == 1 and bad1["trust_verdicts"][0] == 1 and bad1["commit_verdicts"][0] == 0
    assert ceng.vq_last()[5] == bad1["n_checked"] - 1
    bad2 = _request(ceng, Wd, form, True, True, signer, Wd.ver, Wd.thr, sigs=sigs, **pair)
    assert bad2["n_miss"] == 1 and bad2["item_verdicts"][7] == edc.EDC_INVALID_SIGNATURE
    assert bad2["trust_verdicts"] == bad1["trust_verdicts"] and bad2["commit_verdicts"] == bad1["commit_verdicts"]
