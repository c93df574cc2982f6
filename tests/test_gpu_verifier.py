"""GPU: the incremental verifier (edc_verifier_*, batch.StreamVerifier). Items are queued in pieces,
the per-item work runs at queue time and verify() only evaluates the equation; verdicts and
[8]*check are bit-exact against tests/golden/batches.json or against engine.batch_verify of the
same items and z."""
import hashlib
import random

import pytest

from conftest import golden

pytestmark = pytest.mark.gpu

BATCHES = golden("batches.json")["batches"]
BY_NAME = {b["name"]: b for b in BATCHES}
IDENTITY = bytes([1]) + bytes(31)


def _items(b):
    return [(bytes.fromhex(v), bytes.fromhex(s), bytes.fromhex(m)) for v, s, m in b["items"]]


def _expect_check8(b):
    return bytes.fromhex(b["expect_check8"]) if b["expect_check8"] is not None else bytes(32)


def _queue(sv, items):
    if items:
        sv.queue_many([v for v, _, _ in items], [s for _, s, _ in items], msgs=[m for _, _, m in items])


def _pieces(n, pattern):
    if pattern == "whole":
        sizes = [n]
    elif pattern == "1_2_5_rest":
        sizes = [1, 2, 5, n]
    else:
        sizes = [1] * n
    out, at = [], 0
    for s in sizes:
        if at >= n:
            break
        out.append((at, min(n, at + s)))
        at = min(n, at + s)
    return out


def _queue_pieces(sv, items, sizes):
    at = 0
    for s in sizes:
        _queue(sv, items[at:at + s])
        at += s
    assert at >= len(items)


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


# 1. every golden batch, three piece patterns
PIECE_CASES = [(b, p) for b in BATCHES for p in ("whole", "1_2_5_rest", "one_by_one")
               if p != "one_by_one" or len(b["items"]) <= 64]      # one item at a time: batches of <= 64 items


@pytest.mark.parametrize("b,pattern", PIECE_CASES, ids=[f"{b['name']}-{p}" for b, p in PIECE_CASES])
def test_golden_batches_in_pieces(sv_factory, b, pattern):
    it = _items(b)
    sv = sv_factory()
    for a, e in _pieces(len(it), pattern):
        _queue(sv, it[a:e])
    assert sv.batch_size == len(it)
    code, check8 = sv.verify_detailed(bytes.fromhex(b["z_seed"]))
    assert code == b["expect_code"]
    assert check8 == _expect_check8(b)


@pytest.fixture(scope="module")
def votes_4100(engine):
    """4,100 signatures from 150 keys, one of them wrong."""
    rnd = random.Random(4100)
    n, nkeys = 4100, 150
    seeds = [hashlib.sha256(b"v" + i.to_bytes(4, "little")).digest() for i in range(nkeys)]
    msgs = [rnd.randbytes(40) for _ in range(n)]
    vks, sigs = engine.sign(seeds, msgs, seed_index=[(7 * i) % nkeys for i in range(n)])
    sigs = list(sigs)
    sigs[3000] = sigs[3000][:40] + bytes([sigs[3000][40] ^ 4]) + sigs[3000][41:]
    return list(zip(vks, sigs, msgs))


# 2. boundaries that are no multiple of 4 or 2048
@pytest.mark.parametrize("caller_z", [False, True], ids=["seed", "caller_z"])
def test_odd_piece_boundaries(engine, sv_factory, votes_4100, caller_z):
    it = votes_4100
    sv = sv_factory(4100)
    _queue_pieces(sv, it, [2047, 1, 2052])
    vks, sigs, msgs = [v for v, _, _ in it], [s for _, s, _ in it], [m for _, _, m in it]
    seed = bytes(range(32))
    if caller_z:
        z = random.Random(5).randbytes(16 * len(it))

        class Rng:
            at = 0

            def fill_bytes(self, k):
                self.at += k
                return z[self.at - k:self.at]

        exp = engine.batch_verify(vks, sigs, msgs, z=z, want_check8=True)
        got = sv.verify_detailed(Rng())
    else:
        exp = engine.batch_verify(vks, sigs, msgs, z_seed=seed, want_check8=True)
        got = sv.verify_detailed(seed)
    assert exp[0] == 1 and exp[1] not in (IDENTITY, bytes(32))
    assert got == exp


@pytest.fixture(scope="module")
def distinct_5000(engine):
    rnd = random.Random(5000)
    n = 5000
    seeds = [hashlib.sha256(b"d" + i.to_bytes(4, "little")).digest() for i in range(n)]
    msgs = [rnd.randbytes(24) for _ in range(n)]
    vks, sigs = engine.sign(seeds, msgs)
    return list(zip(vks, sigs, msgs))


# 3. more than 4,096 new keys in the appends, one undecodable key in the second
def test_many_new_keys_one_undecodable(engine, sv_factory, distinct_5000):
    b = BY_NAME["undecodable_A"]
    bad_vk = [v for (v, _, _), c in zip(_items(b), b["expect_single"]) if c == 2][0]
    it = list(distinct_5000)
    seed = bytes([0x51]) * 32
    sv = sv_factory(5000)
    _queue_pieces(sv, it, [3000, 2000])
    assert sv.verify_detailed(seed) == (0, IDENTITY)
    it[4321] = (bad_vk, it[4321][1], it[4321][2])
    sv.reset()
    _queue_pieces(sv, it, [3000, 2000])
    assert sv.verify_detailed(seed) == (1, bytes(32))
    code, check8 = engine.batch_verify([v for v, _, _ in it], [s for _, s, _ in it], [m for _, _, m in it],
                                       z_seed=seed, want_check8=True)
    assert (code, check8) == (1, bytes(32))


# 4. growth from a capacity hint of 8
def test_growth_from_small_capacity(sv_factory):
    b = BY_NAME["two_bad_of_300"]
    it = _items(b)
    sv = sv_factory(8)
    _queue_pieces(sv, it, [7] * 43)
    assert sv.batch_size == 300
    assert sv.verify_detailed(bytes.fromhex(b["z_seed"])) == (b["expect_code"], _expect_check8(b))


# 5. grouping overflow: one key term per signature, every A_i decoded at verify
@pytest.mark.parametrize("name", ["repeated_keys_3", "two_bad_of_300", "undecodable_A"])
def test_overflow_path(engine, sv_factory, name):
    b = BY_NAME[name]
    it = _items(b)
    engine.set_key_grouping(3)
    try:
        sv = sv_factory()
        _queue_pieces(sv, it, [3, len(it)])
        got = sv.verify_detailed(bytes.fromhex(b["z_seed"]))
    finally:
        engine.set_key_grouping(0)
    assert got == (b["expect_code"], _expect_check8(b))


# 6. the three queue forms on one verifier
def test_mixed_queue_forms(engine, sv_factory):
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda:0")
    b = BY_NAME["two_bad_of_300"]
    it = _items(b)
    ks = [bytes.fromhex(k) for k in b["k"]]
    sv = sv_factory(300)
    _queue(sv, it[:100])
    sv.queue_many([v for v, _, _ in it[100:200]], [s for _, s, _ in it[100:200]], ks=ks[100:200])

    def to_dev(buf):
        return torch.tensor(list(buf) or [0], dtype=torch.uint8, device=dev)

    sub = it[200:250]
    vk, sg = to_dev(b"".join(v for v, _, _ in sub)), to_dev(b"".join(s for _, s, _ in sub))
    mg = to_dev(b"".join(m for _, _, m in sub))
    offs = [0]
    for _, _, m in sub:
        offs.append(offs[-1] + len(m))
    off = torch.tensor(offs, dtype=torch.int64, device=dev)
    sub2 = it[250:]
    vk2, sg2 = to_dev(b"".join(v for v, _, _ in sub2)), to_dev(b"".join(s for _, s, _ in sub2))
    k2 = to_dev(b"".join(ks[250:]))
    torch.cuda.synchronize()
    sv.queue_device(len(sub), vk.data_ptr(), sg.data_ptr(), mg.data_ptr(), off.data_ptr())
    sv.queue_device(len(sub2), vk2.data_ptr(), sg2.data_ptr(), d_k=k2.data_ptr())
    assert sv.batch_size == 300
    assert sv.verify_detailed(bytes.fromhex(b["z_seed"])) == (b["expect_code"], _expect_check8(b))


# 7. fallback on the retained state
@pytest.mark.parametrize("name", ["two_bad_of_300", "mixed_corpus_one_bad", "batch_verify_32"])
def test_verify_with_fallback(sv_factory, name):
    b = BY_NAME[name]
    it = _items(b)
    sv = sv_factory()
    _queue_pieces(sv, it, [11, 50, len(it)])
    code, verdicts, check8 = sv.verify_with_fallback(bytes.fromhex(b["z_seed"]))
    assert code == b["expect_code"] and check8 == _expect_check8(b)
    assert verdicts == (b["expect_single"] if code else [0] * len(it))
    # the queue is still there, and still verifies to the same result
    assert sv.verify_detailed(bytes.fromhex(b["z_seed"])) == (b["expect_code"], _expect_check8(b))


# 8. lifecycle
def test_verify_queue_more_verify_again(engine, sv_factory):
    a, c = _items(BY_NAME["repeated_keys_3"]), _items(BY_NAME["two_bad_of_300"])
    seed = bytes([0x77]) * 32
    sv = sv_factory()
    _queue(sv, a)
    ba = BY_NAME["repeated_keys_3"]
    assert sv.verify_detailed(bytes.fromhex(ba["z_seed"])) == (ba["expect_code"], _expect_check8(ba))
    _queue_pieces(sv, c, [100, 200])
    both = a + c
    exp = engine.batch_verify([v for v, _, _ in both], [s for _, s, _ in both], [m for _, _, m in both], z_seed=seed,
                              want_check8=True)
    assert exp[0] == 1
    assert sv.verify_detailed(seed) == exp


def test_reset_then_another_batch(sv_factory):
    sv = sv_factory()
    for name in ["two_bad_of_300", "zip215_corpus_batch", "undecodable_R", "repeated_keys_varlen", "empty"]:
        b = BY_NAME[name]
        _queue_pieces(sv, _items(b), [9, len(b["items"])])
        assert sv.verify_detailed(bytes.fromhex(b["z_seed"])) == (b["expect_code"], _expect_check8(b)), name
        sv.reset()
        assert sv.batch_size == 0


def test_other_calls_on_the_context_between_queues(engine, sv_factory):
    b, o = BY_NAME["mixed_corpus_one_bad"], BY_NAME["two_bad_of_300"]
    it, ot = _items(b), _items(o)
    sv = sv_factory()
    _queue(sv, it[:70])
    got_o = engine.batch_verify([v for v, _, _ in ot], [s for _, s, _ in ot], [m for _, _, m in ot],
                                z_seed=bytes.fromhex(o["z_seed"]), want_check8=True)
    _queue(sv, it[70:])
    assert got_o == (o["expect_code"], _expect_check8(o))
    assert sv.verify_detailed(bytes.fromhex(b["z_seed"])) == (b["expect_code"], _expect_check8(b))


# 9. with the keys in the context's key cache
@pytest.mark.parametrize("name", ["repeated_keys_varlen", "two_bad_of_300", "undecodable_A"])
def test_with_key_cache(engine, sv_factory, name):
    b = BY_NAME[name]
    it = _items(b)
    engine.keycache_load(list(dict.fromkeys(v for v, _, _ in it)))
    try:
        sv = sv_factory()
        _queue_pieces(sv, it, [2, len(it)])
        got = sv.verify_detailed(bytes.fromhex(b["z_seed"]))
        sv.close()
    finally:
        engine.keycache_clear()
    assert got == (b["expect_code"], _expect_check8(b))


# 10. a prehashed k >= l is an argument error, never a verdict
def test_bad_prehashed_k(edc, sv_factory):
    b = BY_NAME["batch_verify_32"]
    it = _items(b)
    ks = [bytes.fromhex(k) for k in b["k"]]
    ks[20] = bytes([0xFF]) * 32
    sv = sv_factory()
    sv.queue_many([v for v, _, _ in it[:16]], [s for _, s, _ in it[:16]], ks=ks[:16])
    with pytest.raises(edc.EngineError):
        sv.queue_many([v for v, _, _ in it[16:]], [s for _, s, _ in it[16:]], ks=ks[16:])
        sv.verify_detailed(bytes.fromhex(b["z_seed"]))
