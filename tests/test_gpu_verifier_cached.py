"""GPU: the cached incremental verifier (include/edc.h, edc_vfy_set_cached; csrc/vfy_cached.h).

In cached mode a queue call appends only the items that miss the context's verified-signature
table, in the order they were offered; verify() covers the retained items and what it proves valid
is inserted. The oracle for the expected misses is a Python set of the records (vk || sig || k) the
test knows were inserted; the expected result is the existing prehashed batch entry on that miss
list with the same seed, compared bit-exactly (check8 included). Every case uses a table of at
least 4x the records inserted and FAILS if an insert was dropped."""
import ctypes

import pytest

from conftest import golden

pytestmark = pytest.mark.gpu

IDENTITY = bytes([1]) + bytes(31)
BATCHES = golden("batches.json")["batches"]
SEED = bytes(range(7, 39))
SCAN_PASS = 1024 * 256            # items one pass of the miss-count scan covers (sigcache.h)
POOL_N = SCAN_PASS + 257
SHAPES = [1, 63, 64, 65, 257, 5000]
PATTERNS = ["none", "all", "alternating", "lead256", "only_miss_first", "only_miss_last"]


def _items(b):
    return ([bytes.fromhex(v) for v, _, _ in b["items"]], [bytes.fromhex(s) for _, s, _ in b["items"]],
            [bytes.fromhex(m) for _, _, m in b["items"]], [bytes.fromhex(k) for k in b["k"]])


def _expect(b):
    return b["expect_code"], (bytes.fromhex(b["expect_check8"]) if b["expect_check8"] is not None else bytes(32))


def _sub(lst, idx):
    return [lst[i] for i in idx]


@pytest.fixture(scope="module")
def torch_dev():
    torch = pytest.importorskip("torch")
    return torch, torch.device("cuda:0")


def _t8(torch_dev, data):
    torch, dev = torch_dev
    t = torch.frombuffer(bytearray(data or b"\0"), dtype=torch.uint8).to(dev)
    torch.cuda.synchronize()
    return t


@pytest.fixture
def table(engine):
    """make(records): an empty table on the shared engine; freed again (after a check that no
    insert was dropped) when the test ends."""
    def make(records, keep=0):
        engine.sigcache_create(max(records, 1024), keep)
        return engine
    yield make
    try:
        assert engine.sigcache_stats()["dropped"] == 0
    finally:
        engine.sigcache_create(0)


@pytest.fixture
def verifier(engine, edc):
    """make(**kw): a StreamVerifier on the shared engine, closed when the test ends."""
    made = []

    def make(**kw):
        kw.setdefault("cached", True)
        made.append(edc.batch.StreamVerifier(engine, **kw))
        return made[-1]
    yield make
    for sv in made:
        sv.close()


@pytest.fixture(scope="module")
def pool(engine):
    """POOL_N distinct valid items (64 keys) as host lists, their messages and their records."""
    n = POOL_N
    seeds = b"".join(bytes([i + 1, 0x5C]) * 16 for i in range(64))
    arena = b"".join(b"vote-%07d" % i for i in range(n))
    offs = (ctypes.c_uint64 * (n + 1))(*range(0, 12 * (n + 1), 12))
    idx = (ctypes.c_uint32 * n)(*[i % 64 for i in range(n)])
    vk, sig, k = (ctypes.create_string_buffer(w * n) for w in (32, 64, 32))
    engine._check(engine.lib.edc_sign(engine.ctx, n, seeds, 64, idx, arena, offs, vk, sig))
    engine._check(engine.lib.edc_challenge(engine.ctx, n, vk.raw, sig.raw, arena, offs, k))
    vkr, sgr, kr = vk.raw, sig.raw, k.raw
    vks = [vkr[32 * i:32 * i + 32] for i in range(n)]
    sigs = [sgr[64 * i:64 * i + 64] for i in range(n)]
    ks = [kr[32 * i:32 * i + 32] for i in range(n)]
    msgs = [arena[12 * i:12 * i + 12] for i in range(n)]
    return {"vk": vks, "sig": sigs, "k": ks, "msg": msgs}


def _hit_pattern(n, pattern):
    if pattern == "none":
        return [False] * n
    if pattern == "all":
        return [True] * n
    if pattern == "alternating":
        return [i % 2 == 0 for i in range(n)]
    if pattern == "lead256":
        return [i < 256 for i in range(n)]
    if pattern == "only_miss_first":
        return [i != 0 for i in range(n)]
    return [i != n - 1 for i in range(n)]


def _pieces(n, how):
    """[(a, b)] covering [0, n): one piece, or three uneven ones whose inner boundaries are odd
    (so never a multiple of 64 or 256)."""
    if how == "one" or n < 3:
        return [(0, n)]
    a, b = (n * 3 // 10) | 1, (n * 7 // 10) | 1
    assert 0 < a < b < n
    return [(0, a), (a, b), (b, n)]


def _forge(sig):
    """s ^ 1: another signature over the same R, hence the same k, and a record of its own"""
    return sig[:32] + bytes([sig[32] ^ 1]) + sig[33:]


def _case(pool, n, pattern):
    """(vks, sigs, ks, msgs, forged sigs, hit index list, miss index list, forged index list)"""
    vks, sigs, ks, msgs = (pool[x][:n] for x in ("vk", "sig", "k", "msg"))
    hit = _hit_pattern(n, pattern)
    hits = [i for i in range(n) if hit[i]]
    miss = [i for i in range(n) if not hit[i]]
    bad = sorted({miss[0], miss[len(miss) // 2], miss[-1]}) if miss else []
    forged = list(sigs)
    for i in bad:
        forged[i] = _forge(sigs[i])
    return vks, sigs, ks, msgs, forged, hits, miss, bad


def _plant(eng, vks, sigs, ks, hits):
    """the hit pattern's records, through the one-call cached entry: they are valid, their batch passes"""
    if hits:
        assert eng.batch_verify_cached(_sub(vks, hits), _sub(sigs, hits), ks=_sub(ks, hits), z_seed=SEED) == \
            (0, IDENTITY, len(hits))


def _oracle(eng, vks, sigs, ks, idx, seed=SEED):
    return eng.batch_verify_prehashed(_sub(vks, idx), _sub(sigs, idx), _sub(ks, idx), z_seed=seed, want_check8=True)


def _queue(sv, vks, sigs, ks, pieces):
    for a, b in pieces:
        sv.queue_many(vks[a:b], sigs[a:b], ks=ks[a:b])
        offered, hits = sv.cache_counts
        assert offered == b and offered - hits == sv.batch_size


def _lookup(eng, torch_dev, vks, sigs, ks):
    torch, dev = torch_dev
    n = len(vks)
    d_vk, d_sig, d_k = (_t8(torch_dev, b"".join(x)) for x in (vks, sigs, ks))
    d_hit = torch.full((max(n, 1),), 7, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    eng.sigcache_lookup(n, d_vk.data_ptr(), d_sig.data_ptr(), d_k.data_ptr(), d_hit.data_ptr())
    return d_hit.cpu().tolist()[:n]


# ---- 1. golden batches on an empty table ----
@pytest.mark.parametrize("b", BATCHES, ids=lambda b: b["name"])
def test_golden_batches_then_again(table, verifier, torch_dev, b):
    eng = table(8192)
    vks, sigs, msgs, ks = _items(b)
    n = len(vks)
    seed = bytes.fromhex(b["z_seed"])
    sv = verifier()
    assert sv.cached
    sv.queue_many(vks, sigs, msgs=msgs)
    assert sv.batch_size == n and sv.cache_counts == (n, 0)     # everything misses: miss j is item j
    assert sv.verify_detailed(seed) == _expect(b)
    sv.reset()
    assert sv.cached and sv.cache_counts == (0, 0)
    if b["expect_code"] == 0:
        sv.queue_many(vks, sigs, msgs=msgs)
        assert sv.batch_size == 0 and sv.cache_counts == (n, n)
        assert sv.verify_detailed(seed) == (0, IDENTITY)
        assert _lookup(eng, torch_dev, vks, sigs, ks) == [1] * n
    else:                               # a failed verify inserted nothing
        assert eng.sigcache_stats()["inserted"] == 0
        assert _lookup(eng, torch_dev, vks, sigs, ks) == [0] * n
        sv.queue_many(vks, sigs, msgs=msgs)
        assert sv.batch_size == n
        assert sv.verify_detailed(seed) == _expect(b)


# ---- 2. hit patterns x shapes x pieces ----
def _run_pattern(eng, sv, pool, n, pattern, how, again=True):
    vks, sigs, ks, _, forged, hits, miss, bad = _case(pool, n, pattern)
    _plant(eng, vks, sigs, ks, hits)
    pieces = _pieces(n, how)
    # a. three of the misses forged (first, middle, last): check8 then depends on which z_j each of
    #    them drew, i.e. on the order of the miss list
    if miss:
        exp = _oracle(eng, vks, forged, ks, miss)
        assert exp[0] == 1 and exp[1] not in (IDENTITY, bytes(32))
        inserted = eng.sigcache_stats()["inserted"]
        _queue(sv, vks, forged, ks, pieces)
        assert sv.batch_size == len(miss) and sv.cache_counts == (n, len(hits))
        assert sv.verify_detailed(SEED) == exp
        sv.reset()
        assert eng.sigcache_stats()["inserted"] == inserted          # a failed verify inserts nothing
    # b. the valid items: the misses pass and are inserted
    exp = _oracle(eng, vks, sigs, ks, miss)
    assert exp == (0, IDENTITY)
    _queue(sv, vks, sigs, ks, pieces)
    assert sv.batch_size == len(miss) and sv.cache_counts == (n, len(hits))
    assert sv.verify_detailed(SEED) == exp
    sv.reset()
    if again:
        _queue(sv, vks, sigs, ks, pieces)
        assert sv.batch_size == 0 and sv.cache_counts == (n, n)
        assert sv.verify_detailed(SEED) == (0, IDENTITY)


@pytest.mark.parametrize("how", ["one", "three"])
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("n", SHAPES)
def test_patterns_shapes_pieces(table, verifier, pool, n, pattern, how):
    _run_pattern(table(4 * n), verifier(), pool, n, pattern, how)


def test_across_a_scan_pass(table, verifier, pool):
    _run_pattern(table(4 * POOL_N), verifier(), pool, POOL_N, "alternating", "one", again=False)


# ---- 3. every queue form ----
@pytest.mark.parametrize("form", ["host_msg", "host_k", "device_k", "device_msg", "indexed_k", "indexed_msg"])
def test_every_queue_form(table, verifier, torch_dev, pool, form):
    torch, dev = torch_dev
    n = 257
    eng = table(4 * n)
    vks, sigs, ks, msgs, forged, hits, miss, bad = _case(pool, n, "alternating")
    _plant(eng, vks, sigs, ks, hits)
    exp = _oracle(eng, vks, forged, ks, miss)
    assert exp[0] == 1
    sv = verifier()
    keep = []                                       # device tensors stay alive until the verify
    try:
        for a, b in _pieces(n, "three"):
            v, s, k, m = vks[a:b], forged[a:b], ks[a:b], msgs[a:b]
            if form == "host_msg":
                sv.queue_many(v, s, msgs=m)
            elif form == "host_k":
                sv.queue_many(v, s, ks=k)
            elif form in ("device_k", "device_msg"):
                d_vk, d_sig = _t8(torch_dev, b"".join(v)), _t8(torch_dev, b"".join(s))
                keep += [d_vk, d_sig]
                if form == "device_k":
                    d_k = _t8(torch_dev, b"".join(k))
                    keep.append(d_k)
                    sv.queue_device(b - a, d_vk.data_ptr(), d_sig.data_ptr(), d_k=d_k.data_ptr())
                else:
                    d_msg = _t8(torch_dev, b"".join(m))
                    d_off = torch.tensor(list(range(0, 12 * (b - a + 1), 12)), dtype=torch.int64, device=dev)
                    torch.cuda.synchronize()
                    keep += [d_msg, d_off]
                    sv.queue_device(b - a, d_vk.data_ptr(), d_sig.data_ptr(), d_msg=d_msg.data_ptr(),
                                    d_msg_off=d_off.data_ptr())
            else:
                if a == 0:
                    keys = sorted(set(vks))
                    eng.keycache_load(keys)
                    pos = {key: i for i, key in enumerate(keys)}
                kidx = [pos[x] for x in v]
                if form == "indexed_k":
                    sv.queue_indexed(kidx, s, ks=k)
                else:
                    sv.queue_indexed(kidx, s, msgs=m)
            offered, nhits = sv.cache_counts
            assert offered == b and offered - nhits == sv.batch_size
        assert sv.batch_size == len(miss) and sv.cache_counts == (n, len(hits))
        assert sv.verify_detailed(SEED) == exp
    finally:
        eng.keycache_clear()


# ---- 4. eager and cached together ----
@pytest.mark.parametrize("n", [257, 5000])
def test_eager_and_cached(table, verifier, pool, n):
    eng = table(4 * n)
    vks, sigs, ks, _, forged, hits, miss, bad = _case(pool, n, "alternating")
    _plant(eng, vks, sigs, ks, hits)
    sv = verifier()
    sv.set_fold(64)
    for sg in (forged, sigs):           # a failing block, then (fresh seed) a passing one
        exp = _oracle(eng, vks, sg, ks, miss)
        sv.begin_eager(SEED)
        assert sv.eager and sv.cached
        _queue(sv, vks, sg, ks, _pieces(n, "three"))
        assert sv.batch_size == len(miss)
        assert sv.folded[1] > 0 and sv.folded[0] <= len(miss)
        assert sv.verify_detailed(None) == exp
        sv.reset()
        assert sv.cached and not sv.eager
    assert exp == (0, IDENTITY)
    sv.begin_eager(SEED)
    _queue(sv, vks, sigs, ks, _pieces(n, "three"))
    assert sv.batch_size == 0 and sv.verify_detailed(None) == (0, IDENTITY)


# ---- 5. per-item codes in offered order ----
def test_fallback_offered(table, verifier, torch_dev, pool, edc):
    n = 257
    eng = table(4 * n)
    vks, sigs, ks, _, forged, hits, miss, bad = _case(pool, n, "alternating")
    _plant(eng, vks, sigs, ks, hits)
    items = [edc.batch.Item.prehashed(vks[i], forged[i], ks[i]) for i in miss]
    single = edc.batch.Item.verify_single_many(items, eng)
    assert sum(1 for c in single if c) == len(bad)
    want = [0] * n
    for i, c in zip(miss, single):
        want[i] = c
    exp = _oracle(eng, vks, forged, ks, miss)
    sv = verifier()
    _queue(sv, vks, forged, ks, _pieces(n, "three"))
    assert sv.verify_with_fallback_offered(SEED) == (1, want, exp[1])
    # exactly the misses whose code is 0 are records now (and the hits still are)
    assert _lookup(eng, torch_dev, vks, forged, ks) == [0 if c else 1 for c in want]
    sv.reset()
    _queue(sv, vks, forged, ks, _pieces(n, "three"))
    assert sv.batch_size == len(bad)
    exp = _oracle(eng, vks, forged, ks, bad)
    code, codes, c8 = sv.verify_with_fallback(SEED)       # retained order, batch_size codes
    assert (code, codes, c8) == (1, [want[i] for i in bad], exp[1])
    # a verifier that is not cached: the offered entry is the plain one
    plain = verifier(cached=False)
    plain.queue_many(vks, forged, ks=ks)
    assert plain.verify_with_fallback_offered(SEED) == plain.verify_with_fallback(SEED)
    assert plain.verify_with_fallback_offered(SEED)[1] == [1 if i in bad else 0 for i in range(n)]


# ---- 6. ageing ----
def test_ageing(table, verifier, pool):
    n, keep = 300, 2
    eng = table(4 * n, keep)
    vks, sigs, ks = (pool[x][:n] for x in ("vk", "sig", "k"))
    sv = verifier()
    _queue(sv, vks, sigs, ks, [(0, n)])
    assert sv.batch_size == n and sv.verify_detailed(SEED) == (0, IDENTITY)
    for _ in range(keep):
        eng.sigcache_advance()
    sv.reset()
    _queue(sv, vks, sigs, ks, [(0, n)])
    assert sv.batch_size == 0 and sv.cache_counts == (n, n)          # keep generations old: still alive
    eng.sigcache_advance()
    sv.reset()
    _queue(sv, vks, sigs, ks, [(0, n)])
    assert sv.batch_size == n and sv.cache_counts == (n, 0)          # older than keep: all miss
    assert sv.verify_detailed(SEED) == (0, IDENTITY)                 # expired slots are reused


# ---- 7. growth ----
def test_growth_from_capacity_one(table, verifier, pool):
    n = 5000
    eng = table(4 * n)
    vks, sigs, ks, _, forged, hits, miss, bad = _case(pool, n, "alternating")
    _plant(eng, vks, sigs, ks, hits)
    sv = verifier(capacity=1)
    cuts = [0, 1, 4, 11, 37, 150, 777, 2501, n]
    _queue(sv, vks, forged, ks, list(zip(cuts, cuts[1:])))
    assert sv.batch_size == len(miss)
    exp = _oracle(eng, vks, forged, ks, miss)
    assert sv.verify_detailed(SEED) == exp
    assert sv.verify_with_fallback_offered(SEED) == (1, [1 if i in bad else 0 for i in range(n)], exp[1])


# ---- 8. ordering of the deferred insert against every other use of the table ----
def test_lookup_right_after_verify(table, verifier, torch_dev, pool):
    n = 5000
    eng = table(4 * n)
    vks, sigs, ks = (pool[x][:n] for x in ("vk", "sig", "k"))
    d_vk, d_sig, d_k = (_t8(torch_dev, b"".join(x)) for x in (vks, sigs, ks))
    torch, dev = torch_dev
    d_hit = torch.zeros(n, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    sv = verifier()
    _queue(sv, vks, sigs, ks, _pieces(n, "three"))
    assert sv.verify_detailed(SEED) == (0, IDENTITY)
    eng.sigcache_lookup(n, d_vk.data_ptr(), d_sig.data_ptr(), d_k.data_ptr(), d_hit.data_ptr())   # no wait between
    assert d_hit.cpu().tolist() == [1] * n
    st = eng.sigcache_stats()
    assert st["inserted"] == n and st["misses"] == n
    # the queue survives verify: more items, and the next verify inserts only those
    more = (pool["vk"][n:n + 100], pool["sig"][n:n + 100], pool["k"][n:n + 100])
    sv.queue_many(more[0], more[1], ks=more[2])
    assert sv.batch_size == n + 100
    assert sv.verify_detailed(SEED) == _oracle(eng, pool["vk"], pool["sig"], pool["k"], list(range(n + 100)))
    assert eng.batch_verify_cached(vks + more[0], sigs + more[1], ks=ks + more[2], z_seed=SEED) == (0, IDENTITY, 0)
    assert eng.sigcache_stats()["inserted"] == n + 100
    # another verifier's queue call right after this one's verify sees its records
    extra = (pool["vk"][n + 100:n + 200], pool["sig"][n + 100:n + 200], pool["k"][n + 100:n + 200])
    sv.queue_many(extra[0], extra[1], ks=extra[2])
    other = verifier()
    assert sv.verify_detailed(SEED)[0] == 0
    other.queue_many(extra[0], extra[1], ks=extra[2])
    assert other.batch_size == 0


def test_slot0_inserts_between_queue_calls(table, verifier, pool):
    n = 600
    eng = table(4 * n)
    vks, sigs, ks = (pool[x][:n] for x in ("vk", "sig", "k"))
    sv = verifier()
    sv.queue_many(vks[:257], sigs[:257], ks=ks[:257])
    assert sv.batch_size == 257
    assert eng.verify_each_cached(vks[257:500], sigs[257:500], ks=ks[257:500]) == ([0] * 243, 243)
    sv.queue_many(vks[257:], sigs[257:], ks=ks[257:])
    assert sv.cache_counts == (n, 243) and sv.batch_size == n - 243
    miss = list(range(257)) + list(range(500, n))
    assert sv.verify_detailed(SEED) == _oracle(eng, vks, sigs, ks, miss)


def test_mode_switch_waits_for_the_pending_insert(table, verifier, torch_dev, pool):
    """verify (its insert is left running), reset, set_cached(False) and a plain queue call that
    overwrites the retained arrays from the copy stream, back to back through the C ABI with the
    buffers built beforehand: the records must be the verified items, none of the new ones."""
    n = 131072
    eng = table(4 * n)
    lib = eng.lib
    old = [b"".join(pool[x][:n]) for x in ("vk", "sig", "k")]
    new = [b"".join(pool[x][n:2 * n]) for x in ("vk", "sig", "k")]
    sv = verifier(capacity=n)
    v = sv._handle()
    eng._check(lib.edc_verifier_queue_prehashed(v, n, old[0], old[1], old[2]))
    assert sv.batch_size == n
    rcs = (lib.edc_verifier_verify(v, SEED, None, None), lib.edc_verifier_reset(v), lib.edc_vfy_set_cached(v, 0),
           lib.edc_verifier_queue_prehashed(v, n, new[0], new[1], new[2]))
    assert rcs == (0, 0, 0, 0)
    assert not sv.cached and sv.batch_size == n
    st = eng.sigcache_stats()
    assert st["inserted"] == n and st["dropped"] == 0
    assert _lookup(eng, torch_dev, pool["vk"][:n], pool["sig"][:n], pool["k"][:n]) == [1] * n
    assert _lookup(eng, torch_dev, pool["vk"][n:2 * n], pool["sig"][n:2 * n], pool["k"][n:2 * n]) == [0] * n
    assert sv.verify_detailed(SEED) == (0, IDENTITY)          # the plain verifier inserts nothing
    assert eng.sigcache_stats()["inserted"] == n


# ---- 9. refusals ----
def test_refusals(engine, verifier, pool, edc):
    eng = engine
    eng.sigcache_create(0)
    vks, sigs, ks, msgs = (pool[x][:65] for x in ("vk", "sig", "k", "msg"))
    sv = verifier()
    for call in (lambda: sv.queue_many(vks, sigs, ks=ks), lambda: sv.queue_many(vks, sigs, msgs=msgs)):
        with pytest.raises(edc.EngineError, match="edc error -2"):
            call()
        assert sv.batch_size == 0 and sv.cache_counts == (0, 0)
    assert sv.verify_detailed(SEED) == (0, IDENTITY)
    eng.sigcache_create(1024)
    try:
        sv.queue_many(vks, sigs, ks=ks)
        assert sv.batch_size == 65 and sv.cache_counts == (65, 0)
        with pytest.raises(edc.EngineError, match="edc error -2"):
            sv.set_cached(False)
        assert sv.cached
        assert sv.verify_detailed(SEED) == (0, IDENTITY)
        sv.reset()
        sv.queue_many(vks, sigs, ks=ks)                     # all hits: nothing retained, but items were offered
        assert sv.batch_size == 0 and sv.cache_counts == (65, 65)
        with pytest.raises(edc.EngineError, match="edc error -2"):
            sv.set_cached(False)
        sv.reset()
        sv.set_cached(False)
        assert not sv.cached
        sv.queue_many(vks, sigs, ks=ks)
        assert sv.batch_size == 65 and sv.cache_counts == (0, 0)
        with pytest.raises(edc.EngineError, match="edc error -2"):
            sv.set_cached(True)
        assert eng.sigcache_stats()["dropped"] == 0
    finally:
        eng.sigcache_create(0)


# ---- 10. a verifier that is not cached never touches the table ----
def test_plain_verifier_unchanged(table, verifier):
    eng = table(8192)
    b = [x for x in BATCHES if x["name"] == "two_bad_of_300"][0]
    vks, sigs, msgs, ks = _items(b)
    good = [i for i, c in enumerate(b["expect_single"]) if c == 0]
    assert eng.verify_each_cached(vks, sigs, ks=ks) == (b["expect_single"], 300)
    before = eng.sigcache_stats()
    assert before["inserted"] > 0
    sv = verifier(cached=False)
    assert not sv.cached
    sv.queue_many(vks, sigs, msgs=msgs)
    assert sv.batch_size == 300 and sv.cache_counts == (0, 0)
    assert sv.verify_detailed(bytes.fromhex(b["z_seed"])) == _expect(b)
    code, codes, _ = sv.verify_with_fallback(SEED)
    assert (code, codes) == (1, b["expect_single"])
    sv.reset()
    sv.queue_many(_sub(vks, good), _sub(sigs, good), ks=_sub(ks, good))
    assert sv.batch_size == len(good) and sv.verify_detailed(SEED) == (0, IDENTITY)
    assert eng.sigcache_stats() == before
