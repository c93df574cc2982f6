"""GPU: the verified-signature cache (include/edc.h, edc_sigcache_*; csrc/sigcache.h).

A cached call verifies only the items that miss the table, in queue order, as one batch. The
oracle for the expected misses is a Python set of the records (vk || sig || k) the test knows were
inserted; the expected result is the existing prehashed batch entry on that miss list with the same
seed, compared bit-exactly (check8 included), and n_miss must be equal. Tests marked drop-free use
a table of at least 4x the records inserted and FAIL if an insert was dropped."""
import ctypes

import pytest

from conftest import golden

pytestmark = pytest.mark.gpu

IDENTITY = bytes([1]) + bytes(31)
L_ORDER = 2**252 + 27742317777372353535851937790883648493
BATCHES = golden("batches.json")["batches"]
SEED = bytes(range(7, 39))
SCAN_PASS = 1024 * 256            # items one pass of the miss-count scan covers (sigcache.h)
POOL_N = SCAN_PASS + 257
SHAPES = [1, 63, 64, 65, 257, 5000, POOL_N]
PATTERNS = ["none", "all", "alternating", "lead256", "only_miss_first", "only_miss_last"]


def _items(b):
    return ([bytes.fromhex(v) for v, _, _ in b["items"]], [bytes.fromhex(s) for _, s, _ in b["items"]],
            [bytes.fromhex(m) for _, _, m in b["items"]], [bytes.fromhex(k) for k in b["k"]])


def _recs(vks, sigs, ks):
    return [v + s + k for v, s, k in zip(vks, sigs, ks)]


def _sub(lst, idx):
    return [lst[i] for i in idx]


@pytest.fixture(scope="module")
def torch_dev():
    torch = pytest.importorskip("torch")
    return torch, torch.device("cuda:0")


@pytest.fixture
def cache(engine):
    """The shared engine with an empty table of 8192 records (4x the largest golden batch and
    more); freed again after the test."""
    engine.sigcache_create(8192)
    yield engine
    engine.sigcache_create(0)


def _t8(torch_dev, data):
    torch, dev = torch_dev
    t = torch.frombuffer(bytearray(data or b"\0"), dtype=torch.uint8).to(dev)
    torch.cuda.synchronize()
    return t


def _oracle(engine, vks, sigs, ks, seed=SEED):
    """The existing prehashed batch entry on a miss list: (code, check8)."""
    return engine.batch_verify_prehashed(vks, sigs, ks, z_seed=seed, want_check8=True)


def _cached_device(engine, torch_dev, vks, sigs, msgs, ks, seed=SEED):
    """edc_sigcache_batch_verify_device: prehashed when ks is given, else with the messages."""
    torch, dev = torch_dev
    n = len(vks)
    d_vk, d_sig = _t8(torch_dev, b"".join(vks)), _t8(torch_dev, b"".join(sigs))
    c8 = ctypes.create_string_buffer(32)
    miss = ctypes.c_size_t(0)
    if ks is not None:
        d_k = _t8(torch_dev, b"".join(ks))
        rc = engine.lib.edc_sigcache_batch_verify_device(engine.ctx, n, d_vk.data_ptr(), d_sig.data_ptr(), None, None,
                                                         d_k.data_ptr(), seed, c8, ctypes.byref(miss))
    else:
        offs = [0]
        for m in msgs:
            offs.append(offs[-1] + len(m))
        d_msg = _t8(torch_dev, b"".join(msgs))
        d_off = torch.tensor(offs, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        rc = engine.lib.edc_sigcache_batch_verify_device(engine.ctx, n, d_vk.data_ptr(), d_sig.data_ptr(),
                                                         d_msg.data_ptr(), d_off.data_ptr(), None, seed, c8,
                                                         ctypes.byref(miss))
    engine._check(rc)
    return rc, c8.raw, miss.value


def _lookup(engine, torch_dev, vks, sigs, ks):
    torch, dev = torch_dev
    n = len(vks)
    d_vk, d_sig, d_k = (_t8(torch_dev, b"".join(x)) for x in (vks, sigs, ks))
    d_hit = torch.full((max(n, 1),), 7, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    engine.sigcache_lookup(n, d_vk.data_ptr(), d_sig.data_ptr(), d_k.data_ptr(), d_hit.data_ptr())
    return d_hit.cpu().tolist()[:n]


def _fallback_device(engine, torch_dev, vks, sigs, ks, seed=SEED):
    d_vk, d_sig, d_k = (_t8(torch_dev, b"".join(x)) for x in (vks, sigs, ks))
    return engine.batch_verify_cached_fallback(len(vks), d_vk.data_ptr(), d_sig.data_ptr(), d_k=d_k.data_ptr(),
                                               z_seed=seed)


# ---- 1. golden batches on an empty table, host with messages / host prehashed / device ----
@pytest.mark.parametrize("form", ["host_msg", "host_k", "device_k", "device_msg"])
@pytest.mark.parametrize("b", BATCHES, ids=lambda b: b["name"])
def test_golden_batches_then_again(cache, torch_dev, b, form):
    eng = cache
    vks, sigs, msgs, ks = _items(b)
    n = len(vks)
    seed = bytes.fromhex(b["z_seed"])

    def run():
        if form == "host_msg":
            return eng.batch_verify_cached(vks, sigs, msgs=msgs, z_seed=seed)
        if form == "host_k":
            return eng.batch_verify_cached(vks, sigs, ks=ks, z_seed=seed)
        return _cached_device(eng, torch_dev, vks, sigs, msgs, ks if form == "device_k" else None, seed)

    exp_c8 = bytes.fromhex(b["expect_check8"]) if b["expect_check8"] is not None else bytes(32)
    # everything misses, so miss j is item j and the fixture's own expectation applies
    assert run() == (b["expect_code"], exp_c8, n)
    if b["expect_code"] == 0:
        assert run() == (0, IDENTITY, 0)
    else:                               # a failed batch inserted nothing
        assert run() == (b["expect_code"], exp_c8, n)
    assert eng.sigcache_stats()["dropped"] == 0


# ---- 2. the fallback entry on the golden batches ----
@pytest.mark.parametrize("b", BATCHES, ids=lambda b: b["name"])
def test_golden_fallback(cache, torch_dev, b):
    eng = cache
    vks, sigs, _, ks = _items(b)
    n = len(vks)
    seed = bytes.fromhex(b["z_seed"])
    single = b["expect_single"] if b["expect_code"] else [0] * n
    exp_c8 = bytes.fromhex(b["expect_check8"]) if b["expect_check8"] is not None else bytes(32)
    code, verdicts, nbad, c8, n_miss = _fallback_device(eng, torch_dev, vks, sigs, ks, seed)
    assert (code, verdicts, c8, n_miss) == (b["expect_code"], single, exp_c8, n)
    assert nbad == sum(1 for v in single if v)
    # the valid items are records now: only the invalid ones miss, and they are the whole batch
    inserted = set(r for r, v in zip(_recs(vks, sigs, ks), single) if v == 0)
    miss = [i for i, r in enumerate(_recs(vks, sigs, ks)) if r not in inserted]
    assert len(miss) == nbad
    ocode, osingle, onbad, oc8 = eng.batch_verify_prehashed_fallback(_sub(vks, miss), _sub(sigs, miss), _sub(ks, miss),
                                                                     seed)
    for _ in range(2):
        code, verdicts, nbad2, c8, n_miss = _fallback_device(eng, torch_dev, vks, sigs, ks, seed)
        assert (code, c8, n_miss, nbad2) == (ocode, oc8, len(miss), onbad)
        assert verdicts == single
    assert eng.sigcache_stats()["dropped"] == 0


# ---- 3. compaction shapes ----
@pytest.fixture(scope="module")
def pool(engine, torch_dev):
    """POOL_N distinct valid items (64 keys), on the host and in device memory."""
    # through the C ABI with flat buffers: one copy out per array, sliced once
    n = POOL_N
    seeds = b"".join(bytes([i + 1, 0x5C]) * 16 for i in range(64))
    arena = b"".join(b"vote-%07d" % i for i in range(n))
    offs = (ctypes.c_uint64 * (n + 1))(*range(0, 12 * (n + 1), 12))
    idx = (ctypes.c_uint32 * n)(*[i % 64 for i in range(n)])
    vk, sig, k = (ctypes.create_string_buffer(w * n) for w in (32, 64, 32))
    engine._check(engine.lib.edc_sign(engine.ctx, n, seeds, 64, idx, arena, offs, vk, sig))
    engine._check(engine.lib.edc_challenge(engine.ctx, n, vk.raw, sig.raw, arena, offs, k))
    flat = {"vk": (vk.raw, 32), "sig": (sig.raw, 64), "k": (k.raw, 32)}
    d = {name: _t8(torch_dev, raw).view(n, w) for name, (raw, w) in flat.items()}
    rec = [flat["vk"][0][32 * i:32 * i + 32] + flat["sig"][0][64 * i:64 * i + 64] + flat["k"][0][32 * i:32 * i + 32]
           for i in range(n)]
    return {"rec": rec, "d": d}


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


def _dev_call(engine, torch_dev, d, rows, entry, seed=SEED):
    """entry on the pool rows `rows` (torch index tensor) with d["sig"] possibly patched."""
    torch, _ = torch_dev
    vk, sig, k = (d[x][rows].contiguous() for x in ("vk", "sig", "k"))
    torch.cuda.synchronize()
    c8 = ctypes.create_string_buffer(32)
    n = int(rows.numel())
    if entry == "cached":
        miss = ctypes.c_size_t(0)
        rc = engine.lib.edc_sigcache_batch_verify_device(engine.ctx, n, vk.data_ptr(), sig.data_ptr(), None, None,
                                                         k.data_ptr(), seed, c8, ctypes.byref(miss))
        return engine._check(rc), c8.raw, miss.value
    rc = engine.lib.edc_batch_verify_prehashed_device(engine.ctx, n, vk.data_ptr(), sig.data_ptr(), k.data_ptr(), seed, 0,
                                                      None, c8)
    return engine._check(rc), c8.raw


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("n", SHAPES)
def test_compaction_shapes(engine, torch_dev, pool, n, pattern):
    torch, dev = torch_dev
    engine.sigcache_create(4 * POOL_N)
    try:
        hit = _hit_pattern(n, pattern)
        d = pool["d"]
        inserted = set()
        hit_rows = torch.tensor([i for i in range(n) if hit[i]], dtype=torch.int64, device=dev)
        if hit_rows.numel():                      # plant the hits: they are valid, their batch passes
            code, _, n_miss = _dev_call(engine, torch_dev, d, hit_rows, "cached")
            assert (code, n_miss) == (0, hit_rows.numel())
            inserted.update(pool["rec"][i] for i in range(n) if hit[i])
        miss = [i for i in range(n) if pool["rec"][i] not in inserted]
        rows = torch.arange(n, dtype=torch.int64, device=dev)
        miss_rows = torch.tensor(miss, dtype=torch.int64, device=dev)
        # a. three of the misses forged (first, middle, last): check8 then depends on which z_j each
        #    of them drew, i.e. on the order of the miss list; s + 1 is a record of its own
        if miss:
            bad = sorted({miss[0], miss[len(miss) // 2], miss[-1]})
            bad_rows = torch.tensor(bad, dtype=torch.int64, device=dev)
            dd = dict(d, sig=d["sig"].clone())
            dd["sig"][bad_rows, 32] ^= 1
            exp = _dev_call(engine, torch_dev, dd, miss_rows, "plain")
            assert exp[0] == 1 and exp[1] != IDENTITY
            assert _dev_call(engine, torch_dev, dd, rows, "cached") == (exp[0], exp[1], len(miss))
        # b. the valid items: the misses pass and are inserted
        exp = _dev_call(engine, torch_dev, d, miss_rows, "plain")
        assert _dev_call(engine, torch_dev, d, rows, "cached") == (exp[0], exp[1], len(miss))
        assert exp[0] == 0
        if n <= 5000:
            assert _dev_call(engine, torch_dev, d, rows, "cached") == (0, IDENTITY, 0)
        assert engine.sigcache_stats()["dropped"] == 0
    finally:
        engine.sigcache_create(0)


# ---- 4. no false hits ----
def test_no_false_hits(cache, torch_dev):
    eng = cache
    b = [x for x in BATCHES if x["name"] == "batch_verify_32"][0]
    vks, sigs, msgs, ks = _items(b)
    vk, sig, msg, k = vks[3], sigs[3], msgs[3], ks[3]
    assert eng.verify_each_cached([vk], [sig], ks=[k]) == ([0], 1)
    rec = vk + sig + k
    variants = [rec]
    for pos in (0, 31, 32, 63, 64, 95, 96, 127):
        variants.append(rec[:pos] + bytes([rec[pos] ^ 0x10]) + rec[pos + 1:])
    hits = _lookup(eng, torch_dev, [r[:32] for r in variants], [r[32:96] for r in variants],
                   [r[96:] for r in variants])
    assert hits == [1] + [0] * 8
    # k does not depend on s: a forged s meets the same vk, R and k, and must still be verified
    forged = sig[:32] + bytes([sig[32] ^ 1]) + sig[33:]
    for kw in ({"ks": [k]}, {"msgs": [msg]}):
        code, c8, n_miss = eng.batch_verify_cached([vk], [forged], z_seed=SEED, **kw)
        assert (code, n_miss) == (1, 1)
        assert (code, c8) == _oracle(eng, [vk], [forged], [k])
    assert eng.batch_verify_cached([vk], [sig], ks=[k], z_seed=SEED) == (0, IDENTITY, 0)
    # two encodings of one point are two keys, hence two records
    t = [x for x in BATCHES if x["name"] == "twin_encodings"][0]
    tv, ts, _, tk = _items(t)
    assert tv[0] != tv[1] and ts[0] == ts[1]
    assert eng.verify_each_cached(tv[:1], ts[:1], ks=tk[:1]) == ([0], 1)
    assert _lookup(eng, torch_dev, tv[:2], ts[:2], tk[:2]) == [1, 0]
    assert eng.verify_each_cached(tv[:2], ts[:2], ks=tk[:2]) == ([0, 0], 1)
    assert _lookup(eng, torch_dev, tv[:2], ts[:2], tk[:2]) == [1, 1]


# ---- 5. the ZIP215 small-order cases ----
def test_zip215_cases_feed_then_batch(cache, edc):
    eng = cache
    fx = golden("zip215_small_order.json")
    msg = bytes.fromhex(fx["msg"])
    vks = [bytes.fromhex(c["vk"]) for c in fx["cases"]]
    sigs = [bytes.fromhex(c["sig"]) for c in fx["cases"]]
    expect = [c["expect_single"] for c in fx["cases"]]
    assert len(vks) == 196 and expect == [0] * 196
    items = [edc.batch.Item(v, s, msg) for v, s in zip(vks, sigs)]
    assert edc.batch.Item.verify_single_many_cached(items, eng) == expect
    before = eng.sigcache_stats()
    assert eng.batch_verify_cached(vks, sigs, msgs=[msg] * 196, z_seed=SEED) == (0, IDENTITY, 0)
    v = edc.batch.Verifier(eng)
    for it in items:
        v.queue(it)
    assert v.verify_cached(SEED) == 0
    with pytest.raises(ValueError):
        v.verify_cached(object())
    after = eng.sigcache_stats()
    assert after["dropped"] == 0 and after["inserted"] == before["inserted"]
    assert after["hits"] == before["hits"] + 2 * 196


# ---- 6. ageing and clearing ----
def test_ageing_and_clear(engine, torch_dev):
    eng = engine
    eng.sigcache_create(1024, 2)
    try:
        b = [x for x in BATCHES if x["name"] == "batch_verify_32"][0]
        vks, sigs, _, ks = _items(b)
        n = len(vks)
        gen0 = eng.sigcache_stats()["generation"]
        assert eng.batch_verify_cached(vks, sigs, ks=ks, z_seed=SEED) == (0, IDENTITY, n)
        eng.sigcache_advance()
        assert _lookup(eng, torch_dev, vks, sigs, ks) == [1] * n          # one generation old
        eng.sigcache_advance()
        assert _lookup(eng, torch_dev, vks, sigs, ks) == [1] * n          # keep = 2: still alive
        eng.sigcache_advance()
        assert eng.sigcache_stats()["generation"] == gen0 + 3
        assert _lookup(eng, torch_dev, vks, sigs, ks) == [0] * n          # more than keep generations ago
        assert eng.batch_verify_cached(vks, sigs, ks=ks, z_seed=SEED) == (0, IDENTITY, n)   # expired slots are reused
        assert _lookup(eng, torch_dev, vks, sigs, ks) == [1] * n
        assert eng.batch_verify_cached(vks, sigs, ks=ks, z_seed=SEED) == (0, IDENTITY, 0)
        eng.sigcache_clear()
        assert _lookup(eng, torch_dev, vks, sigs, ks) == [0] * n
        assert eng.batch_verify_cached(vks, sigs, ks=ks, z_seed=SEED) == (0, IDENTITY, n)
        st = eng.sigcache_stats()
        assert st["dropped"] == 0 and st["inserted"] == 3 * n and st["capacity"] == 1024
    finally:
        eng.sigcache_create(0)


# ---- 7. a full table ----
def test_full_table_drops_but_stays_exact(engine, torch_dev):
    eng = engine
    eng.sigcache_create(256)
    try:
        b = [x for x in BATCHES if x["name"] == "c1_1024_distinct"][0]
        vks, sigs, _, ks = _items(b)
        assert len(set(_recs(vks, sigs, ks))) == 1024
        code, verdicts, nbad, _, n_miss = _fallback_device(eng, torch_dev, vks, sigs, ks)
        assert (code, verdicts, nbad, n_miss) == (0, [0] * 1024, 0, 1024)
        st = eng.sigcache_stats()
        assert st["dropped"] > 0 and st["inserted"] + st["dropped"] == 1024 and st["inserted"] <= 256
        hits = _lookup(eng, torch_dev, vks, sigs, ks)
        assert sum(hits) == st["inserted"]
        code, verdicts, nbad, c8, n_miss = _fallback_device(eng, torch_dev, vks, sigs, ks)
        assert (code, verdicts, nbad) == (0, [0] * 1024, 0)
        assert n_miss == 1024 - sum(hits)
        miss = [i for i, h in enumerate(hits) if not h]
        assert (code, c8) == _oracle(eng, _sub(vks, miss), _sub(sigs, miss), _sub(ks, miss))
    finally:
        eng.sigcache_create(0)


# ---- 8. key cache loaded, key-grouping modes ----
def test_same_results_with_keycache_and_grouping_modes(cache, torch_dev):
    eng = cache

    def scenario():
        out = []
        for name in ("two_bad_of_300", "repeated_keys_varlen", "undecodable_A"):
            eng.sigcache_clear()
            b = [x for x in BATCHES if x["name"] == name][0]
            vks, sigs, msgs, ks = _items(b)
            half = list(range(0, len(vks), 2))
            out.append(eng.verify_each_cached(_sub(vks, half), _sub(sigs, half), ks=_sub(ks, half)))
            out.append(eng.batch_verify_cached(vks, sigs, msgs=msgs, z_seed=SEED))
            out.append(_fallback_device(eng, torch_dev, vks, sigs, ks))
            out.append(eng.batch_verify_cached(vks, sigs, ks=ks, z_seed=SEED))
        return out

    try:
        base = scenario()
        b = [x for x in BATCHES if x["name"] == "two_bad_of_300"][0]
        vks, sigs, _, ks = _items(b)
        rec = _recs(vks, sigs, ks)
        single = b["expect_single"]
        half = list(range(0, 300, 2))
        inserted = set(rec[i] for i in half if single[i] == 0)
        miss = [i for i in range(300) if rec[i] not in inserted]
        assert base[0] == (_sub(single, half), len(half))
        assert base[1] == _oracle(eng, _sub(vks, miss), _sub(sigs, miss), _sub(ks, miss)) + (len(miss),)
        for mode in (1, 2, 3):
            eng.set_key_grouping(mode)
            assert scenario() == base, mode
        eng.set_key_grouping(0)
        eng.keycache_load(sorted(set(vks)))
        assert scenario() == base
        eng.set_key_grouping(3)
        assert scenario() == base
    finally:
        eng.set_key_grouping(0)
        eng.keycache_clear()


# ---- 9. k >= l in an item that misses ----
def test_noncanonical_k_in_a_miss(cache, torch_dev, edc):
    eng = cache
    b = [x for x in BATCHES if x["name"] == "batch_verify_32"][0]
    vks, sigs, _, ks = _items(b)
    assert eng.batch_verify_cached(vks[:16], sigs[:16], ks=ks[:16], z_seed=SEED) == (0, IDENTITY, 16)
    inserted = eng.sigcache_stats()["inserted"]
    k_bad = list(ks)
    k_bad[20] = (int.from_bytes(ks[20], "little") + L_ORDER).to_bytes(32, "little")   # same scalar mod l, >= l
    with pytest.raises(edc.EngineError, match="canonical"):
        eng.batch_verify_cached(vks, sigs, ks=k_bad, z_seed=SEED)
    with pytest.raises(edc.EngineError, match="canonical"):
        _fallback_device(eng, torch_dev, vks, sigs, k_bad)
    with pytest.raises(edc.EngineError, match="canonical"):
        eng.verify_each_cached(vks, sigs, ks=k_bad)
    assert eng.sigcache_stats()["inserted"] == inserted
    assert _lookup(eng, torch_dev, vks, sigs, ks) == [1] * 16 + [0] * 16
    assert eng.batch_verify_cached(vks, sigs, ks=ks, z_seed=SEED) == (0, IDENTITY, 16)    # the context stays usable


# ---- 10. no table ----
def test_no_table_is_an_argument_error(engine, torch_dev, edc):
    eng = engine
    eng.sigcache_create(0)
    b = [x for x in BATCHES if x["name"] == "one_valid"][0]
    vks, sigs, msgs, ks = _items(b)
    for call in (lambda: eng.batch_verify_cached(vks, sigs, ks=ks, z_seed=SEED),
                 lambda: eng.batch_verify_cached(vks, sigs, msgs=msgs, z_seed=SEED),
                 lambda: eng.verify_each_cached(vks, sigs, ks=ks),
                 lambda: _fallback_device(eng, torch_dev, vks, sigs, ks),
                 lambda: _cached_device(eng, torch_dev, vks, sigs, msgs, ks),
                 lambda: _lookup(eng, torch_dev, vks, sigs, ks),
                 eng.sigcache_clear, eng.sigcache_advance, eng.sigcache_stats):
        with pytest.raises(edc.EngineError, match="edc error -2"):
            call()
    assert eng.batch_verify_prehashed(vks, sigs, ks, z_seed=SEED, want_check8=True) == (0, IDENTITY)
