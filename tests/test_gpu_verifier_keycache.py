"""GPU: the incremental verifier with a registered validator set (include/edc.h, "With a registered
validator set"): verify() plans with split coefficients from [2^128] rows left at queue time, and
items may be queued by key index (edc_vfy_queue_indexed). Expected values come from
tests/golden/batches.json, from engine.batch_verify under set_key_split(1) (the unsplit one-call
path) and from the C oracle -- never from the verifier itself. last_split proves which plan ran."""
import hashlib
import os
import random
import sys

import pytest

from conftest import ROOT, golden

pytestmark = pytest.mark.gpu

BATCHES = golden("batches.json")["batches"]
BY_NAME = {b["name"]: b for b in BATCHES}
IDENTITY = bytes([1]) + bytes(31)
EDC_ERR_ARG = -2


@pytest.fixture(scope="module")
def oracle_c():
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import oracle_c as oc
    return oc


@pytest.fixture()
def cached(engine):
    yield engine
    engine.keycache_clear()
    engine.set_key_split(0)
    engine.set_key_grouping(0)


@pytest.fixture()
def sv_factory(edc, engine):
    made = []

    def make(capacity=0):
        sv = edc.batch.StreamVerifier(engine, capacity)
        made.append(sv)
        return sv

    yield make
    for sv in made:
        sv.close()


def _items(b):
    return [(bytes.fromhex(v), bytes.fromhex(s), bytes.fromhex(m)) for v, s, m in b["items"]]


def _expect(b):
    return b["expect_code"], (bytes.fromhex(b["expect_check8"]) if b["expect_check8"] is not None else bytes(32))


def _cols(items):
    return [v for v, _, _ in items], [s for _, s, _ in items], [m for _, _, m in items]


def _keys(items):
    return list(dict.fromkeys(v for v, _, _ in items))


def _queue(sv, items):
    if items:
        sv.queue_many(*_cols(items)[:2], msgs=_cols(items)[2])


def _queue_pieces(sv, items, sizes):
    at = 0
    for s in sizes:
        _queue(sv, items[at:at + s])
        at += s
    assert at >= len(items)


def _votes(engine, tag, n, m, msg_len=40):
    """n signatures from m keys (item i signed by key (7 i) mod m), deterministic per tag."""
    rnd = random.Random(tag)
    seeds = [hashlib.sha256(tag.encode() + i.to_bytes(4, "little")).digest() for i in range(m)]
    msgs = [rnd.randbytes(msg_len) for _ in range(n)]
    vks, sigs = engine.sign(seeds, msgs, seed_index=[(7 * i) % m for i in range(n)])
    return list(zip(vks, sigs, msgs))


def _corrupt(items, i):
    v, s, m = items[i]
    items[i] = (v, s[:40] + bytes([s[40] ^ 4]) + s[41:], m)


def _one_call_unsplit(engine, items, **zkw):
    engine.set_key_split(1)
    try:
        return engine.batch_verify(*_cols(items), want_check8=True, **zkw)
    finally:
        engine.set_key_split(0)


# 1. every golden batch with its distinct keys registered: split, and unsplit under set_key_split(1)
GOLDEN_CASES = [(b, p, ks) for b in BATCHES for p in ("whole", "1_2_5_rest") for ks in (0, 1)]


@pytest.mark.parametrize("b,pattern,key_split", GOLDEN_CASES,
                         ids=[f"{b['name']}-{p}-{'nosplit' if ks else 'split'}" for b, p, ks in GOLDEN_CASES])
def test_golden_batches_registered(cached, sv_factory, b, pattern, key_split):
    it = _items(b)
    if it:
        cached.keycache_load(_keys(it))
    cached.set_key_split(key_split)
    sv = sv_factory()
    _queue_pieces(sv, it, [len(it)] if pattern == "whole" else [1, 2, 5, len(it)])
    assert sv.batch_size == len(it)
    got = sv.verify_detailed(bytes.fromhex(b["z_seed"]))
    if it:
        assert sv.last_split == (0 if key_split else 1)
    assert got == _expect(b)


# 2. 150 keys, one bad signature, piece boundaries that are no multiple of 4 or 2048
@pytest.fixture(scope="module")
def votes_4100(engine):
    it = _votes(engine, "kc4100", 4100, 150)
    _corrupt(it, 3000)
    return it


@pytest.mark.parametrize("caller_z", [False, True], ids=["seed", "caller_z"])
def test_150_keys_one_bad(cached, sv_factory, oracle, oracle_c, votes_4100, caller_z):
    it = votes_4100
    seed = bytes(range(32))
    cached.keycache_load(_keys(it))
    sv = sv_factory(4100)
    _queue_pieces(sv, it, [2047, 1, 2052])
    exp = oracle_c.batch_verify(it, seed)
    assert exp[0] == 1 and exp[1] not in (IDENTITY, bytes(32))
    if caller_z:
        z = oracle.chacha20_keystream(seed, 16 * len(it))      # the z the seed gives, drawn by the caller

        class Rng:
            at = 0

            def fill_bytes(self, k):
                self.at += k
                return z[self.at - k:self.at]

        assert _one_call_unsplit(cached, it, z=z) == exp
        got = sv.verify_detailed(Rng())
    else:
        assert _one_call_unsplit(cached, it, z_seed=seed) == exp
        got = sv.verify_detailed(seed)
    assert sv.last_split == 1
    assert got == exp


# 3. n = capacity = distinct keys: the split layout fills the whole point table
@pytest.fixture(scope="module")
def distinct_2048(engine):
    return _votes(engine, "kc2048", 2048, 2048, msg_len=24)


@pytest.mark.parametrize("registered", [True, False], ids=["all_registered", "none_registered"])
def test_layout_overlap(cached, sv_factory, oracle_c, distinct_2048, registered):
    it = distinct_2048
    other = _votes(cached, "kcother", 1, 1)
    cached.keycache_load(_keys(it) if registered else _keys(other))
    seed = bytes([0x3C]) * 32
    exp = oracle_c.batch_verify(it, seed)
    assert exp == (0, IDENTITY)
    sv = sv_factory(2048)
    _queue_pieces(sv, it, [1000, 1048])
    got = sv.verify_detailed(seed)
    assert sv.last_split == 1
    assert got == exp
    # the queue, and its key rows, are still there for a second verify
    seed2 = bytes([0x3D]) * 32
    assert sv.verify_detailed(seed2) == oracle_c.batch_verify(it, seed2)
    assert sv.last_split == 1


# 4. growth from a small capacity rebuilds the [2^128] rows
def test_growth(cached, sv_factory, oracle_c):
    it = _votes(cached, "kcgrow", 300, 40)
    _corrupt(it, 123)
    cached.keycache_load(_keys(it))
    seed = bytes([0x44]) * 32
    exp = oracle_c.batch_verify(it, seed)
    assert exp[0] == 1
    sv = sv_factory(16)
    _queue_pieces(sv, it, [7] * 43)
    assert sv.batch_size == 300
    got = sv.verify_detailed(seed)
    assert sv.last_split == 1
    assert got == exp


# 5. keys missing from the cache are doubled at queue time; the verifier keeps splitting
def test_strangers(cached, sv_factory, oracle_c):
    reg = _votes(cached, "kcreg", 600, 150)
    strangers = _votes(cached, "kcstr", 9, 3)
    it = reg[:400] + strangers[:5] + reg[400:] + strangers[5:]
    bad = 402                                   # a stranger's item
    assert it[bad][0] in _keys(strangers)
    _corrupt(it, bad)
    cached.keycache_load(_keys(reg))
    seed = bytes([0x55]) * 32
    exp = oracle_c.batch_verify(it, seed)
    assert exp[0] == 1 and exp[1] != bytes(32)
    sv = sv_factory()
    _queue_pieces(sv, it, [401, 3, len(it)])
    got = sv.verify_detailed(seed)
    assert sv.last_split == 1
    assert got == exp
    code, verdicts, check8 = sv.verify_with_fallback(seed)
    assert sv.last_split == 1
    assert (code, check8) == exp
    assert verdicts == [1 if i == bad else 0 for i in range(len(it))]


# 6. a key that does not decode, registered or not
@pytest.mark.parametrize("registered", [True, False], ids=["registered", "unregistered"])
def test_undecodable_key(cached, sv_factory, oracle_c, registered):
    bad_vk = bytes.fromhex([c for c in golden("decode.json")["cases"] if not c["ok"]][0]["enc"])
    it = _votes(cached, "kcund", 40, 5)
    it[17] = (bad_vk, it[17][1], it[17][2])
    _, ok = cached.keycache_load(_keys(it) if registered else [k for k in _keys(it) if k != bad_vk])
    assert ok.count(False) == (1 if registered else 0)
    seed = bytes([0x66]) * 32
    assert oracle_c.batch_verify(it, seed) == (1, None)      # no check point: reported as a zero check8
    sv = sv_factory()
    _queue_pieces(sv, it, [17, 1, 22])
    got = sv.verify_detailed(seed)
    assert sv.last_split == 1
    assert got == (1, bytes(32))
    code, verdicts, check8 = sv.verify_with_fallback(seed)
    assert (code, check8) == (1, bytes(32))
    assert verdicts == [2 if i == 17 else 0 for i in range(len(it))]


# 7. one key term per signature (mode 2) and the on-device overflow (mode 3) under the split plan
@pytest.mark.parametrize("bad", [None, 99], ids=["valid", "one_bad"])
@pytest.mark.parametrize("n,m", [(600, 64), (256, 256)])
@pytest.mark.parametrize("mode", [2, 3])
def test_grouping_modes(cached, sv_factory, oracle_c, mode, n, m, bad):
    it = _votes(cached, f"kcgm{n}", n, m)
    if bad is not None:
        _corrupt(it, bad)
    cached.keycache_load(_keys(it))
    cached.set_key_grouping(mode)
    seed = bytes([0x70 + mode]) * 32
    exp = oracle_c.batch_verify(it, seed)
    assert exp[0] == (0 if bad is None else 1)
    sv = sv_factory()
    _queue_pieces(sv, it, [100, len(it)])
    got = sv.verify_detailed(seed)
    assert sv.last_split == 1
    assert got == exp


# 8. the queue survives verify; reset starts another batch
def test_queue_survives_verify(cached, sv_factory, oracle_c):
    it = _votes(cached, "kcsurv", 1500, 150)
    newcomer = _votes(cached, "kcnew", 4, 1)
    first, more = it[:1000], it[1000:1300] + newcomer[:2] + it[1300:1498]
    assert len(more) == 500
    cached.keycache_load(_keys(it))
    sv = sv_factory(1000)
    _queue_pieces(sv, first, [600, 400])
    s1, s2 = bytes([0x81]) * 32, bytes([0x82]) * 32
    got1 = sv.verify_detailed(s1)
    assert sv.last_split == 1
    _queue_pieces(sv, more, [250, 250])
    got2 = sv.verify_detailed(s2)
    assert sv.last_split == 1
    assert got1 == _one_call_unsplit(cached, first, z_seed=s1) == oracle_c.batch_verify(first, s1)
    assert got2 == _one_call_unsplit(cached, first + more, z_seed=s2) == oracle_c.batch_verify(first + more, s2)
    sv.reset()
    assert sv.batch_size == 0
    b = BY_NAME["mixed_corpus_one_bad"]
    _queue_pieces(sv, _items(b), [9, len(b["items"])])
    assert sv.verify_detailed(bytes.fromhex(b["z_seed"])) == _expect(b)
    assert sv.last_split == 1                   # its keys are not registered: doubled at queue time


# 9. the cache changes between queue and verify: that verify runs unsplit, same result
@pytest.mark.parametrize("change", ["add", "load", "clear"])
def test_cache_changes(cached, sv_factory, oracle_c, change):
    it = _votes(cached, "kcchg", 500, 50)
    _corrupt(it, 77)
    others = _keys(_votes(cached, "kcchg2", 20, 20))
    cached.keycache_load(_keys(it))
    seed = bytes([0x90]) * 32
    exp = oracle_c.batch_verify(it, seed)
    assert exp[0] == 1
    sv = sv_factory()
    _queue_pieces(sv, it, [300, 200])
    if change == "add":
        cached.keycache_add(others)
    elif change == "load":
        cached.keycache_load(others + _keys(it)[:10])
    else:
        cached.keycache_clear()
    got = sv.verify_detailed(seed)
    assert sv.last_split == 0
    assert got == exp
    if change == "clear":
        cached.keycache_load(_keys(it))
    sv.reset()
    _queue_pieces(sv, it, [300, 200])
    got = sv.verify_detailed(seed)
    assert sv.last_split == 1
    assert got == exp


# 10. items queued by key index
def test_queue_indexed(edc, cached, sv_factory, oracle_c):
    it = _votes(cached, "kcidx", 400, 30, msg_len=57)
    _corrupt(it, 250)
    keys = _keys(it)
    reg = keys + keys[:5] + [keys[3]]           # the registered list holds duplicates
    where = {}
    for p, k in enumerate(reg):
        where.setdefault(k, []).append(p)
    rnd = random.Random(10)
    idx = [rnd.choice(where[v]) for v, _, _ in it]
    vks, sigs, msgs = _cols(it)
    ks = cached.challenge(vks, sigs, msgs)
    cached.keycache_load(reg)
    seed = bytes([0xA0]) * 32
    exp = oracle_c.batch_verify(it, seed)
    assert exp[0] == 1

    plain = sv_factory()
    plain.queue_many(vks, sigs, msgs=msgs)
    assert plain.verify_detailed(seed) == exp

    a = sv_factory()                            # indexed, with messages
    a.queue_indexed(idx[:150], sigs[:150], msgs=msgs[:150])
    a.queue_indexed(idx[150:], sigs[150:], msgs=msgs[150:])
    b = sv_factory()                            # indexed, prehashed
    b.queue_indexed(idx, sigs, ks=ks)
    c = sv_factory()                            # mixed with the other forms
    c.queue_many(vks[:33], sigs[:33], msgs=msgs[:33])
    c.queue_indexed(idx[33:200], sigs[33:200], ks=ks[33:200])
    c.queue_many(vks[200:301], sigs[200:301], ks=ks[200:301])
    c.queue_indexed(idx[301:], sigs[301:], msgs=msgs[301:])
    for sv in (a, b, c):
        assert sv.batch_size == len(it)
        got = sv.verify_detailed(seed)
        assert sv.last_split == 1
        assert got == exp

    # an index outside the list: EDC_ERR_ARG, nothing appended
    import ctypes
    lib = cached.lib
    bad_idx = (ctypes.c_uint32 * 3)(0, len(reg), 1)
    rc = lib.edc_vfy_queue_indexed(a._handle(), 3, bad_idx, b"".join(sigs[:3]), None, None, b"".join(ks[:3]))
    assert rc == EDC_ERR_ARG and a.batch_size == len(it)
    with pytest.raises(edc.EngineError):
        a.queue_indexed([len(reg) + 7], sigs[:1], msgs=msgs[:1])
    assert a.batch_size == len(it)
    assert a.verify_detailed(seed) == exp
    # no registered list
    cached.keycache_clear()
    ok_idx = (ctypes.c_uint32 * 1)(0)
    rc = lib.edc_vfy_queue_indexed(a._handle(), 1, ok_idx, sigs[0], None, None, ks[0])
    assert rc == EDC_ERR_ARG and a.batch_size == len(it)
    cached.keycache_add(keys)                   # a cache, but no registered list
    rc = lib.edc_vfy_queue_indexed(a._handle(), 1, ok_idx, sigs[0], None, None, ks[0])
    assert rc == EDC_ERR_ARG and a.batch_size == len(it)


# 11. a one-call batch on the same context between two queue calls
def test_other_work_between_queue_calls(cached, sv_factory, oracle_c):
    it = _votes(cached, "kcbetween", 300, 25)
    _corrupt(it, 5)
    o = BY_NAME["two_bad_of_300"]
    cached.keycache_load(_keys(it))
    seed = bytes([0xB0]) * 32
    sv = sv_factory()
    _queue(sv, it[:70])
    got_o = cached.batch_verify(*_cols(_items(o)), z_seed=bytes.fromhex(o["z_seed"]), want_check8=True)
    _queue(sv, it[70:])
    assert got_o == _expect(o)
    got = sv.verify_detailed(seed)
    assert sv.last_split == 1
    assert got == oracle_c.batch_verify(it, seed)
