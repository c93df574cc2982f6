"""GPU: cached quorum commit sets (include/edc.h, edc_cached_quorum_*): the quorum entries with the
verified-signature table between the selection and the batch.

Expected values: the selection, tally and verdicts are the pure-Python model's (tests/golden/
gen_quorum.py) on the oracle's item codes (commits.json; every vote of the sets signed here is
valid); which checked items are records is asked of edc_sigcache_lookup_device BEFORE the call; the
miss list is gathered here and its check8 is edc_batch_verify_prehashed_device's. Nothing expected
comes from a cached quorum call. W is the lookup's and the selection's tile (SC_BLOCK = QR_TILE)."""
import ctypes
import random

import pytest

from test_gpu_quorum import QuorumSet, _check8_of_gathered, _offsets, _same, g, qsets  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu

W = 256
BAD = [346, 645, 700, 800, 2047]
KEYS = ("code", "commit_verdicts", "item_verdicts", "tally", "n_bad_commits", "n_checked", "check8")


@pytest.fixture(scope="module")
def ceng(edc):
    """An engine of this module's own: its table is nobody else's."""
    pytest.importorskip("torch")
    eng = edc.Engine(0)
    eng.sigcache_create(1 << 14)
    yield eng
    eng.close()


def _up(b):
    import torch
    return torch.frombuffer(bytearray(b or b"\0"), dtype=torch.uint8).to("cuda:0")


def _records(eng, Q, D=None):
    """edc_sigcache_lookup_device over all n items (their prehashed k): 1 = a live record."""
    import torch
    D = D or Q.dev()
    hit = torch.zeros(max(Q.n, 1), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    eng.sigcache_lookup(Q.n, D["vk"].data_ptr(), D["sig"].data_ptr(), D["k"].data_ptr(), hit.data_ptr())
    return hit.cpu().tolist()[:Q.n]


def _call(eng, Q, form, seed, light, D=None):
    D = D or Q.dev()
    if form == "dev_msg":
        return eng.quorum_verify_cached_device(Q.off, D["vk"], D["sig"], D["msg"], D["off"], D["power"], D["flag"], Q.thr, seed,
                                               light=light)
    if form == "dev_k":
        return eng.quorum_verify_cached_device(Q.off, D["vk"], D["sig"], None, None, D["power"], D["flag"], Q.thr, seed,
                                               light=light, d_k=D["k"])
    kw = dict(msgs=Q.msgs) if form == "host_msg" else dict(ks=Q.ks)
    return eng.quorum_verify_cached(Q.off, Q.sigs, Q.power, Q.flag, Q.thr, seed, light=light, vks=Q.vks, **kw)


def _held(eng, Q, g, form, seed, light, D=None):
    """One cached call held to everything the contract says about it, at whatever the table holds."""
    mode = g.LIGHT if light else g.FULL
    j = g.judge(Q.off, Q.power, Q.flag, Q.thr, mode, Q.codes)
    rec, st0 = _records(eng, Q, D), eng.sigcache_stats()
    miss = [int(c and not r) for c, r in zip(j["checked"], rec)]
    hits = sum(1 for c, r in zip(j["checked"], rec) if c and r)
    got = _call(eng, Q, form, seed, light, D)
    _same(got, j)
    assert got["n_miss"] == sum(miss), (form, light)
    union, c8 = _check8_of_gathered(eng, Q, miss, seed)
    assert got["check8"] == c8, (form, light)
    assert union == (1 if any(m and Q.codes[i] for i, m in enumerate(miss)) else 0)
    st1 = eng.sigcache_stats()
    assert (st1["hits"] - st0["hits"], st1["misses"] - st0["misses"]) == (hits, sum(miss))
    good = sum(1 for i, m in enumerate(miss) if m and Q.codes[i] == 0)
    assert st1["dropped"] == st0["dropped"] and st1["inserted"] - st0["inserted"] == good
    hashed = Q.n if form.endswith("msg") else 0
    assert eng.cached_quorum_last() == (Q.n, j["n_checked"], hits, sum(miss), hashed, good)
    after = _records(eng, Q, D)
    for i in range(Q.n):                         # the valid misses are records now; nothing else changed
        assert after[i] == (1 if rec[i] or (miss[i] and Q.codes[i] == 0) else 0), i
    return got, j, miss


# ---- 1 and 2: cold table, then the same call again ----

@pytest.mark.parametrize("light", [False, True], ids=["full", "light"])
@pytest.mark.parametrize("form", ["dev_msg", "dev_k", "host_msg", "host_k"])
def test_cold_then_warm_mixed_a(ceng, g, qsets, form, light):
    Q = qsets("mixed_a")
    assert [i for i, c in enumerate(Q.codes) if c] == BAD
    seed = random.Random("cold%s%d" % (form, light)).randbytes(32)
    ceng.sigcache_clear()
    want = Q.device(ceng, seed, light, prehashed=form.endswith("k"))               # edc_quorum_verify_device
    cold, j, miss = _held(ceng, Q, g, form, seed, light)
    for key in KEYS:
        assert cold[key] == want[key], key
    assert cold["n_miss"] == cold["n_checked"] == j["n_checked"] and miss == j["checked"]
    warm, _, miss = _held(ceng, Q, g, form, seed, light)
    assert warm["n_miss"] == sum(1 for i in BAD if j["checked"][i]) and [i for i, m in enumerate(miss) if m] == \
        [i for i in BAD if j["checked"][i]]
    for key in KEYS[:-1]:
        assert warm[key] == cold[key], key
    # 5: a bad vote never becomes a record, and a repeat gives the same commits and codes
    rec = _records(ceng, Q)
    assert [rec[i] for i in BAD] == [0] * 5
    again, _, _ = _held(ceng, Q, g, form, seed, light)
    for key in KEYS:
        assert again[key] == warm[key], key


@pytest.mark.parametrize("light", [False, True], ids=["full", "light"])
def test_warm_set_with_no_bad_item(ceng, g, qsets, light):
    Q = qsets("valid")
    seed = random.Random("valid%d" % light).randbytes(32)
    ceng.sigcache_clear()
    cold, j, _ = _held(ceng, Q, g, "dev_msg", seed, light)
    want = Q.device(ceng, seed, light)
    for key in KEYS:
        assert cold[key] == want[key], key
    for form in ("dev_k", "host_msg"):
        warm, j, _ = _held(ceng, Q, g, form, seed, light)
        # the fixture lays short commits over its valid votes: no commit is invalid, the tally is the plan
        assert warm["n_miss"] == 0 and warm["code"] == j["code"] != 1 and warm["tally"] == j["planned"]
        c8 = ctypes.create_string_buffer(32)
        assert ceng.lib.edc_batch_verify_prehashed_device(ceng.ctx, 0, None, None, None, seed, 0, None, c8) == 0
        assert warm["check8"] == c8.raw
    # and a set in which every commit has its quorum: EDC_OK
    Q = Small(ceng, 300, [150, 150])
    ceng.sigcache_clear()
    cold, j, _ = _held(ceng, Q, g, "dev_msg", seed, light)
    warm, j, _ = _held(ceng, Q, g, "dev_k", seed, light)
    assert (cold["code"], warm["code"], warm["n_miss"]) == (0, 0, 0) and warm["tally"] == j["planned"]
    assert warm["check8"] == c8.raw


# ---- 3: partly warm ----

@pytest.mark.parametrize("light", [False, True], ids=["full", "light"])
def test_partly_warm(ceng, g, qsets, light):
    Q = qsets("mixed_a")
    j = g.judge(Q.off, Q.power, Q.flag, Q.thr, g.LIGHT if light else g.FULL, Q.codes)
    rnd = random.Random("partly%d" % light)
    sub = sorted(rnd.sample(range(Q.n), Q.n // 2))
    sub = sorted(set(sub) | {BAD[0]})
    assert any(not j["checked"][i] for i in sub) and any(Q.flag[i] == 0 for i in sub)
    ceng.sigcache_clear()
    codes, _ = ceng.verify_each_cached([Q.vks[i] for i in sub], [Q.sigs[i] for i in sub], msgs=[Q.msgs[i] for i in sub])
    assert [c for i, c in zip(sub, codes) if Q.flag[i] != 0] == [Q.codes[i] for i in sub if Q.flag[i] != 0]
    rec = _records(ceng, Q)
    fed = set(sub)
    assert all(rec[i] == (1 if i in fed and Q.codes[i] == 0 else 0) for i in range(Q.n) if Q.flag[i] != 0)
    for form in ("dev_k", "host_msg"):
        got, _, miss = _held(ceng, Q, g, form, rnd.randbytes(32), light)
        if form == "dev_k":
            assert 0 < got["n_miss"] < got["n_checked"]
            assert [i for i, m in enumerate(miss) if m] == [i for i in range(Q.n) if j["checked"][i] and not rec[i]]


# ---- 4: the selection is blind to the table ----

def test_selection_is_blind_to_the_table(ceng, g, qsets):
    Q = qsets("mixed_a")
    ceng.sigcache_clear()
    rnd = random.Random("blind")
    _held(ceng, Q, g, "dev_k", rnd.randbytes(32), False)                    # full mode warms every valid vote
    got, j, _ = _held(ceng, Q, g, "dev_k", rnd.randbytes(32), True)
    checked, _ = g.select(Q.off, Q.power, Q.flag, Q.thr, g.LIGHT)
    assert [int(v != 255) for v in got["item_verdicts"]] == checked and got["n_checked"] == sum(checked)
    assert ceng.quorum_plan(Q.off, Q.power, Q.flag, Q.thr, light=True)[2] == got["n_checked"]
    assert 0 < got["n_checked"] < sum(1 for f in Q.flag if f)               # light mode still stops at the quorum


# ---- 5: a record's (vk, sig) with another message is a miss and gets its real code ----

def test_another_message_is_a_miss(ceng, g, qsets):
    Q = qsets("valid")
    ceng.sigcache_clear()
    rnd = random.Random("othermsg")
    _held(ceng, Q, g, "host_msg", rnd.randbytes(32), False)
    j = g.judge(Q.off, Q.power, Q.flag, Q.thr, g.FULL, Q.codes)
    i = next(i for i in range(W + 3, Q.n) if j["checked"][i] and Q.flag[i] == 1)
    msgs, codes = list(Q.msgs), list(Q.codes)
    msgs[i], codes[i] = msgs[i] + b"!", 1                                   # EDC_INVALID_SIGNATURE, by definition
    want = g.judge(Q.off, Q.power, Q.flag, Q.thr, g.FULL, codes)
    got = ceng.quorum_verify_cached(Q.off, Q.sigs, Q.power, Q.flag, Q.thr, rnd.randbytes(32), light=False, vks=Q.vks, msgs=msgs)
    _same(got, want)
    assert got["n_miss"] == 1 and got["code"] == 1
    assert ceng.cached_quorum_last()[5] == 0                                # and it planted nothing
    _held(ceng, Q, g, "host_msg", rnd.randbytes(32), False)                 # the original is still a record


# ---- 6: tile edges, on sets signed here ----

class Small:
    """n valid votes signed with edc_sign, in the shape QuorumSet gives the helpers."""

    def __init__(self, eng, n, sizes, flag=None, thr=None):
        import numpy as np
        import torch
        rnd = random.Random("small%d%r" % (n, sizes))
        self.n, self.off, self.nc = n, _offsets(sizes), len(sizes)
        assert self.off[-1] == n
        self.msgs = [rnd.randbytes(20 + i % 50) for i in range(n)]
        self.vks, self.sigs = eng.sign([rnd.randbytes(32) for _ in range(7)], self.msgs, seed_index=[i % 7 for i in range(n)])
        self.ks = eng.challenge(self.vks, self.sigs, self.msgs)
        self.codes = [0] * n
        self.power = [1 + i % 9 for i in range(n)]
        self.flag = flag or [1] * n
        self.thr = thr or [2 * sum(self.power[a:e]) // 3 for a, e in zip(self.off, self.off[1:])]
        self._D = {"vk": _up(b"".join(self.vks)), "sig": _up(b"".join(self.sigs)), "msg": _up(b"".join(self.msgs)),
                   "off": torch.tensor(_offsets([len(m) for m in self.msgs]), dtype=torch.int64, device="cuda:0"),
                   "k": _up(b"".join(self.ks)),
                   "power": torch.from_numpy(np.array(self.power, dtype=np.uint64).view(np.int64)).to("cuda:0"),
                   "flag": _up(bytes(self.flag))}
        torch.cuda.synchronize()

    def dev(self):
        return self._D


def _warm(eng, Q, items):
    eng.sigcache_clear()
    items = sorted(items)
    if items:
        codes, _ = eng.verify_each_cached([Q.vks[i] for i in items], [Q.sigs[i] for i in items], ks=[Q.ks[i] for i in items])
        assert codes == [0] * len(items)


@pytest.mark.parametrize("commits", ["one", "of64"])
@pytest.mark.parametrize("n", [W - 1, W, W + 1, 2 * W + 1])
def test_tile_edges(ceng, g, n, commits):
    sizes = [n] if commits == "one" else [64] * (n // 64) + ([n % 64] if n % 64 else [])
    Q = Small(ceng, n, sizes)
    full = set(range(n))
    last_tile = (n - 1) // W * W
    patterns = {"first tile hits, the rest misses": set(range(min(W, n))) if n > W else set(range(n // 2)),
                "only the first item of a tile misses": full - {last_tile},
                "only the last item of a tile misses": full - {min(W, n) - 1},
                "a single miss at n - 1": full - {n - 1},
                "all hits": full, "all misses": set()}
    rnd = random.Random("edges%d%s" % (n, commits))
    for what, warm in patterns.items():
        _warm(ceng, Q, warm)
        got, j, miss = _held(ceng, Q, g, "dev_k", rnd.randbytes(32), False)
        assert [i for i, m in enumerate(miss) if m] == sorted(full - warm), what
        assert got["n_miss"] == n - len(warm) and got["item_verdicts"] == [0] * n and got["code"] == 0, what
    # every checked item a hit while the unchecked ones are not: light mode stops inside each commit
    checked, _ = g.select(Q.off, Q.power, Q.flag, Q.thr, g.LIGHT)
    assert 0 < sum(checked) < n
    _warm(ceng, Q, [i for i, c in enumerate(checked) if c])
    got, j, miss = _held(ceng, Q, g, "dev_msg", rnd.randbytes(32), True)
    assert got["n_miss"] == 0 and got["code"] == 0 and got["tally"] == j["planned"]
    assert _records(ceng, Q) == checked                                     # an unchecked vote is never inserted
    # and the other way round: only unchecked items are records, so every checked one misses
    _warm(ceng, Q, [i for i, c in enumerate(checked) if not c])
    got, j, miss = _held(ceng, Q, g, "dev_k", rnd.randbytes(32), True)
    assert got["n_miss"] == got["n_checked"] == sum(checked) and miss == checked


# ---- 7: ageing ----

def test_ageing(edc, g, qsets):
    Q = qsets("mixed_a")
    eng = edc.Engine(0)
    try:
        keep = 3
        eng.sigcache_create(1 << 14, keep=keep)
        rnd = random.Random("ageing")
        seed = rnd.randbytes(32)
        cold, _, _ = _held(eng, Q, g, "dev_k", seed, True)
        for _ in range(keep):
            eng.sigcache_advance()
        warm, _, _ = _held(eng, Q, g, "dev_k", seed, True)                 # keep generations on: still alive
        assert warm["n_miss"] < cold["n_miss"]
        eng.sigcache_advance()
        old, _, miss = _held(eng, Q, g, "dev_k", seed, True)
        assert old["n_miss"] == old["n_checked"]
        for key in KEYS:
            assert old[key] == cold[key], key
    finally:
        eng.close()


# ---- 8: noise in the items that are not checked ----

@pytest.mark.parametrize("light", [False, True], ids=["full", "light"])
def test_unchecked_bytes_never_matter(ceng, g, qsets, light):
    Q = qsets("mixed_a")
    j = g.judge(Q.off, Q.power, Q.flag, Q.thr, g.LIGHT if light else g.FULL, Q.codes)
    rnd = random.Random("noise%d" % light)
    warm = [i for i in range(0, Q.n, 3) if Q.flag[i] != 0 and Q.codes[i] == 0]
    seed = rnd.randbytes(32)

    def run(D):
        _warm(ceng, Q, warm)
        st0 = ceng.sigcache_stats()
        got = ceng.quorum_verify_cached_device(Q.off, D["vk"], D["sig"], None, None, D["power"], D["flag"], Q.thr, seed,
                                               light=light, d_k=D["k"])
        st1 = ceng.sigcache_stats()
        return got, [st1[k] - st0[k] for k in ("hits", "misses", "inserted", "dropped")], ceng.cached_quorum_last()
    clean = run(Q.dev())
    _same(clean[0], j)
    vks, sigs, ks = list(Q.vks), list(Q.sigs), list(Q.ks)
    unchecked = [i for i, c in enumerate(j["checked"]) if not c]
    assert len(unchecked) > 100
    for i in unchecked:
        vks[i], sigs[i], ks[i] = rnd.randbytes(32), rnd.randbytes(64), rnd.randbytes(32)
    N = dict(Q.dev(), vk=_up(b"".join(vks)), sig=_up(b"".join(sigs)), k=_up(b"".join(ks)))
    assert run(N) == clean


# ---- 9: errors ----

def test_no_table_is_an_argument_error(edc, qsets):
    Q = qsets("valid")
    D = Q.dev()
    eng = edc.Engine(0)
    try:
        off = (ctypes.c_uint32 * (Q.nc + 1))(*Q.off)
        thr = (ctypes.c_uint64 * Q.nc)(*Q.thr)
        cv, iv = ctypes.create_string_buffer(b"\x07" * Q.nc, Q.nc), ctypes.create_string_buffer(b"\x07" * Q.n, Q.n)
        tal = (ctypes.c_uint64 * Q.nc)(*[7] * Q.nc)
        nb, cnt, miss = ctypes.c_int(7), ctypes.c_size_t(7), ctypes.c_size_t(7)
        c8 = ctypes.create_string_buffer(b"\x07" * 32, 32)

        def dev(nc=Q.nc):
            return eng.lib.edc_cached_quorum_verify_device(eng.ctx, nc, off, D["vk"].data_ptr(), D["sig"].data_ptr(), None, None,
                                                           D["k"].data_ptr(), D["power"].data_ptr(), D["flag"].data_ptr(), thr, 1,
                                                           bytes(32), cv, iv, tal, ctypes.byref(nb), ctypes.byref(cnt),
                                                           ctypes.byref(miss), c8)
        assert dev() == -2 and dev(nc=0) == -2
        assert (cv.raw, iv.raw, list(tal), nb.value, cnt.value, miss.value, c8.raw) == \
            (b"\x07" * Q.nc, b"\x07" * Q.n, [7] * Q.nc, 7, 7, 7, b"\x07" * 32)
        with pytest.raises(edc.EngineError, match="edc error -2"):
            eng.quorum_verify_cached(Q.off, Q.sigs, Q.power, Q.flag, Q.thr, bytes(32), vks=Q.vks, ks=Q.ks)
        with pytest.raises(edc.EngineError, match="edc error -2"):
            eng.cached_quorum_last()
        eng.sigcache_create(1 << 12)                                        # with a table the same call works
        assert dev() in (0, 3) and miss.value == cnt.value > 0
        eng.sigcache_create(0)
        assert dev() == -2
    finally:
        eng.close()


def test_device_checks_change_nothing(ceng, edc, g, qsets):
    import torch
    Q = qsets("mixed_a")
    D = Q.dev()
    rnd = random.Random("cqargs")
    j = g.judge(Q.off, Q.power, Q.flag, Q.thr, g.LIGHT, Q.codes)
    unchecked = next(i for i, c in enumerate(j["checked"]) if not c and Q.flag[i] == 1 and i > W)
    flag3, big = list(Q.flag), list(Q.power)
    flag3[unchecked] = 3
    big[unchecked] = 2**63
    ceng.sigcache_clear()
    st0 = ceng.sigcache_stats()
    for kw in (dict(flag=_up(bytes(flag3))), dict(power=QuorumSet.dev_power(big))):
        torch.cuda.synchronize()
        for light in (True, False):
            with pytest.raises(edc.EngineError, match="edc error -2"):
                ceng.quorum_verify_cached_device(Q.off, D["vk"], D["sig"], None, None, kw.get("power", D["power"]),
                                                 kw.get("flag", D["flag"]), Q.thr, rnd.randbytes(32), light=light, d_k=D["k"])
        assert ceng.sigcache_stats() == st0 and sum(_records(ceng, Q)) == 0
    with pytest.raises(edc.EngineError, match="edc error -2"):               # the host form refuses on the host
        ceng.quorum_verify_cached(Q.off, Q.sigs, Q.power, flag3, Q.thr, rnd.randbytes(32), vks=Q.vks, ks=Q.ks)
    assert ceng.sigcache_stats() == st0
    seed = rnd.randbytes(32)
    got, _, _ = _held(ceng, Q, g, "dev_k", seed, True)                      # the next valid call: the cold-table result
    want = Q.device(ceng, seed, True, prehashed=True)
    for key in KEYS:
        assert got[key] == want[key], key
    assert got["n_miss"] == got["n_checked"]


def test_degenerate_sets(ceng, g):
    seed = bytes(range(32))
    ceng.sigcache_clear()
    st0 = ceng.sigcache_stats()
    got = ceng.quorum_verify_cached([0], [], [], [], [], seed, vks=[], msgs=[])                       # nc = 0
    assert (got["code"], got["n_checked"], got["n_miss"], got["n_bad_commits"]) == (0, 0, 0, 0)
    got = ceng.quorum_verify_cached([0, 0, 0], [], [], [], [0, 5], seed, vks=[], msgs=[])             # empty commits
    assert (got["code"], got["commit_verdicts"], got["tally"], got["n_miss"]) == (3, [3, 3], [0, 0], 0)
    Q = Small(ceng, 70, [0, 30, 0, 40], flag=[0] * 30 + [1] * 40)                                    # an all-absent commit
    for light in (True, False):
        got, j, _ = _held(ceng, Q, g, "host_msg", seed, light)
        assert got["commit_verdicts"][:3] == [3, 3, 3] and got["commit_verdicts"][3] == 0
    A = Small(ceng, 5, [5], flag=[0] * 5)                                                            # nothing is checked
    got, j, _ = _held(ceng, A, g, "dev_k", seed, True)
    assert (got["code"], got["n_checked"], got["n_miss"], got["item_verdicts"]) == (3, 0, 0, [255] * 5)
    assert sum(_records(ceng, A)) == 0 and ceng.sigcache_stats()["dropped"] == st0["dropped"]


def test_python_batch_surface(ceng, edc, g, qsets):
    Q = qsets("valid")
    vs, powers, flags = [], [], []
    for a, e in zip(Q.off, Q.off[1:]):
        v = edc.batch.Verifier()
        for i in range(a, e):
            v.queue((Q.vks[i], Q.sigs[i], Q.msgs[i]))
        vs.append(v)
        powers.append(Q.power[a:e])
        flags.append(Q.flag[a:e])
    j = g.judge(Q.off, Q.power, Q.flag, Q.thr, g.LIGHT, Q.codes)
    ceng.sigcache_clear()
    for expect_miss in (j["n_checked"], 0):
        verdicts, tally, codes = edc.batch.verify_quorum(vs, powers, flags, Q.thr, light=True, engine=ceng, cached=True)
        assert verdicts == j["commit_verdicts"] and tally == j["tally"]
        assert [c for per in codes for c in per] == j["item_verdicts"]
        assert ceng.cached_quorum_last()[3] == expect_miss
    assert edc.batch.verify_quorum(vs, powers, flags, Q.thr, light=True, engine=ceng) == (verdicts, tally, codes)


# ---- 10: the host form with registered keys ----

@pytest.mark.parametrize("light", [False, True], ids=["full", "light"])
def test_host_form_with_key_idx(ceng, qsets, light):
    """quorum_verify_cached(key_idx=...) after keycache_load, cold and then warm: all eight fields are
    those of the same call with vks= at the same table state, and everything but n_miss is
    quorum_verify(key_idx=...)'s. check8 belongs to the list that was verified, so the warm call's,
    whose list is empty, is held to the vks= call's alone."""
    Q = qsets("valid")
    keys = list(dict.fromkeys(Q.vks))
    pos = {k: i for i, k in enumerate(keys)}
    idx = [pos[k] for k in Q.vks]
    seed = random.Random("hostidx%d" % light).randbytes(32)
    ceng.keycache_load(keys)
    try:
        want = ceng.quorum_verify(Q.off, Q.sigs, Q.power, Q.flag, Q.thr, seed, light=light, key_idx=idx, msgs=Q.msgs)
        runs = {}
        for how, kw in (("vks", dict(vks=Q.vks)), ("key_idx", dict(key_idx=idx))):
            ceng.sigcache_clear()
            runs[how] = [ceng.quorum_verify_cached(Q.off, Q.sigs, Q.power, Q.flag, Q.thr, seed, light=light, msgs=Q.msgs, **kw)
                         for _ in ("cold", "warm")]
    finally:
        ceng.keycache_clear()
    for got, same in zip(runs["key_idx"], runs["vks"]):
        assert sorted(got) == sorted(KEYS + ("n_miss",))
        assert got == same
    cold, warm = runs["key_idx"]
    for key in KEYS:
        assert cold[key] == want[key], key
    for key in KEYS[:-1]:
        assert warm[key] == want[key], key
    assert cold["n_miss"] == cold["n_checked"] > 0 and warm["n_miss"] == 0      # every vote of this set is valid
