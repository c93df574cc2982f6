"""GPU: every grow-only workspace of the host API regrows to the right contents, and nothing leaks.

The device buffers, pinned buffers, streams and events of a context / verifier are owned by the
types of csrc/devbuf.h and grown by its two helpers. Each case here runs on ONE fresh context (or
verifier), so its buffers start empty, and crosses the growth thresholds on it: 96 items (the 1,024
floor), then 1,100 (capacity 1,100 + 1,100 / 8 = 1,237), then 2,500 (above that); the message arenas
go under 4,096 bytes, over it, and over 1.125 times the second. Every expected value is the C
oracle's (oracle/edc_oracle.c through oracle_c): the batch verdict and [8]*check, and
Item::verify_single's code per item. The last case counts the library's live allocations
(edc_debug_live_allocs) around eight create / run / destroy rounds."""
import os
import random
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

SIZES = (96, 1100, 2500)
MSG_LEN = 40            # 96 x 40 < 4,096 < 1,100 x 40 = 44,000, and 2,500 x 40 > 1.125 x 44,000
POOL, KEYS, BAD = 2600, 150, 2000


@pytest.fixture(scope="module")
def oc():
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import oracle_c
    return oracle_c


class Pool:
    """POOL signed items over KEYS keys, made once: `valid`, and `items` = the same with the
    signature of item BAD corrupted; ks and the oracle's per-item codes of `items`."""

    def __init__(self, engine, oracle, oc):
        rnd = random.Random(2025)
        self.seeds = [rnd.randbytes(32) for _ in range(KEYS)]
        self.key_of = [i % KEYS for i in range(POOL)]
        msgs = [rnd.randbytes(MSG_LEN) for _ in range(POOL)]
        vks, sigs = engine.sign(self.seeds, msgs, seed_index=self.key_of)
        self.valid = list(zip(vks, sigs, msgs))
        bad = sigs[BAD][:40] + bytes([sigs[BAD][40] ^ 4]) + sigs[BAD][41:]      # a bit of s
        self.items = list(self.valid)
        self.items[BAD] = (vks[BAD], bad, msgs[BAD])
        self.ks = [oracle.challenge(s[:32], v, m).to_bytes(32, "little") for v, s, m in self.items]
        self.codes = [oc.verify(*it) for it in self.items]
        assert [i for i, c in enumerate(self.codes) if c] == [BAD]
        self._batch = {}
        self.oc = oc

    def batch(self, items, seed):
        """the oracle's (code, check8) of a batch, computed once per (batch, seed)"""
        key = (id(items), len(items), seed)
        if key not in self._batch:
            self._batch[key] = self.oc.batch_verify(items, seed)
        return self._batch[key]


@pytest.fixture(scope="module")
def pool(engine, oracle, oc):
    return Pool(engine, oracle, oc)


@pytest.fixture()
def ctx(edc, engine):
    """a fresh context: every workspace starts empty"""
    eng = edc.Engine(0)
    yield eng
    eng.close()


def cols(items):
    return [x[0] for x in items], [x[1] for x in items], [x[2] for x in items]


def test_item_growth_sync_submit_prehashed_each_fallback(ctx, pool):
    assert ctx.lib.edc_set_slots(ctx.ctx, 1) == 0       # every submission lands on the one slot that grows
    for n in SIZES:
        items, ks, seed = pool.items[:n], pool.ks[:n], bytes([n % 251]) * 32
        vks, sigs, msgs = cols(items)
        assert (sum(map(len, msgs)) < 4096) == (n == 96)
        exp = pool.oc.batch_verify(items, seed)
        assert exp[0] == (1 if n > BAD else 0)
        assert ctx.batch_verify(vks, sigs, msgs, z_seed=seed, want_check8=True) == exp
        assert ctx.batch_wait(ctx.batch_submit(vks, sigs, msgs, seed, want_check8=True), want_check8=True) == exp
        assert ctx.batch_wait(ctx.batch_submit_prehashed(vks, sigs, ks, seed, want_check8=True), want_check8=True) == exp
        assert ctx.verify_each(vks, sigs, msgs) == pool.codes[:n]
        # the fallback entry: on the failing batch its range and listed-item staging grows from empty
        code, codes, n_invalid, c8 = ctx.batch_verify_prehashed_fallback(vks, sigs, ks, seed)
        assert (code, c8) == exp and codes == pool.codes[:n] and n_invalid == sum(1 for c in codes if c)


CHUNKS = ((0, 700), (700, 1400), (1400, 2600))          # capacity hint 1: the retained arrays double and copy


def _queue_chunks(v, items):
    for a, b in CHUNKS:
        vks, sigs, msgs = cols(items[a:b])
        v.queue_many(vks, sigs, msgs=msgs)
        assert v.batch_size == b


def test_verifier_growth_with_retained_items(edc, ctx, pool):
    seed = bytes([0x51]) * 32
    v = edc.batch.StreamVerifier(ctx, capacity=1)
    _queue_chunks(v, pool.valid)
    assert v.verify_detailed(seed) == pool.batch(pool.valid, seed) == (0, bytes([1]) + bytes(31))
    v.close()
    v = edc.batch.StreamVerifier(ctx, capacity=1)
    _queue_chunks(v, pool.items)
    exp = pool.batch(pool.items, seed)
    code, codes, c8 = v.verify_with_fallback(seed)
    assert (code, c8) == exp and exp[0] == 1 and codes == pool.codes
    v.close()


def test_cached_verifier_growth(edc, ctx, pool):
    seed = bytes([0x52]) * 32
    ctx.sigcache_create(4096)
    v = edc.batch.StreamVerifier(ctx, capacity=1, cached=True)
    _queue_chunks(v, pool.items)                         # an empty table: every item is a miss and is retained
    assert v.cache_counts == (POOL, 0)
    code, codes, c8 = v.verify_with_fallback_offered(seed)
    assert (code, c8) == pool.batch(pool.items, seed) and codes == pool.codes
    v.close()


def test_templates_and_commit_sets_growth(edc, ctx, pool, oc):
    rnd = random.Random(77)
    T = edc.batch.Templates([b"vote/" + bytes([t]) * (3 + 5 * t) for t in range(3)], [b"/end" * t for t in range(3)])
    for n in (96, 1300):
        seed = bytes([n % 251]) * 32
        tpl = [i % 3 for i in range(n)]
        holes = [rnd.randbytes(8 + i % 5) for i in range(n)]
        msgs = T.materialize(tpl, holes)
        vks, sigs = ctx.sign(pool.seeds, msgs, seed_index=pool.key_of[:n])
        sigs = list(sigs)
        if n == 1300:
            sigs[1000] = sigs[1000][:40] + bytes([sigs[1000][40] ^ 4]) + sigs[1000][41:]
        items = list(zip(vks, sigs, msgs))
        exp = oc.batch_verify(items, seed)
        assert exp[0] == (1 if n == 1300 else 0)
        assert ctx.batch_verify_templated(T, sigs, tpl, holes, seed, vks=vks, want_check8=True) == exp
        # a commit set over the same items: each commit is its own batch for the oracle
        off = [0, 1, 40, 40, n] if n == 96 else [0, 7, 650, 650, 1001, n]
        codes = [oc.verify(*it) for it in items]
        verdicts = [oc.batch_verify(items[a:b], seed)[0] if b > a else 0 for a, b in zip(off, off[1:])]
        rc, got_verdicts, got_codes, n_bad = ctx.commits_verify(off, sigs, seed, vks=vks, msgs=msgs)
        assert (rc, got_verdicts, got_codes, n_bad) == (1 if any(verdicts) else 0, verdicts, codes, sum(verdicts))
        assert sum(verdicts) == (1 if n == 1300 else 0)


def test_keycache_append_growth(ctx, pool, oc):
    rnd = random.Random(5)
    first = [rnd.randbytes(32) for _ in range(64)]
    more = [rnd.randbytes(32) for _ in range(1200)]
    n = 300
    msgs = [rnd.randbytes(MSG_LEN) for _ in range(n)]
    idx = [(7 * i) % 64 for i in range(n)]
    vks, sigs = ctx.sign(first, msgs, seed_index=idx)
    reg = [None] * 64
    for i, j in enumerate(idx):
        reg[j] = vks[i]
    assert all(reg)
    more_vks, _ = ctx.sign(more, [b""] * len(more))
    assert ctx.keycache_load(reg) == (64, [True] * 64)
    u, oks = ctx.keycache_add(list(more_vks))             # the arrays grow and the 64 cached keys move
    assert u == 64 + 1200 and all(oks)
    seed = bytes([0x53]) * 32
    exp = oc.batch_verify(list(zip(vks, sigs, msgs)), seed)
    assert exp == (0, bytes([1]) + bytes(31))
    assert ctx.batch_wait(ctx.batch_submit_indexed(idx, sigs, msgs, seed, want_check8=True), want_check8=True) == exp
    bad = list(sigs)
    bad[17] = bad[17][:40] + bytes([bad[17][40] ^ 4]) + bad[17][41:]
    exp = oc.batch_verify(list(zip(vks, bad, msgs)), seed)
    assert exp[0] == 1
    assert ctx.batch_wait(ctx.batch_submit_indexed(idx, bad, msgs, seed, want_check8=True), want_check8=True) == exp


def test_no_leak_over_create_run_destroy(edc, engine, pool):
    n, seed = 1100, bytes([0x54]) * 32
    vks, sigs, msgs = cols(pool.items[:n])
    exp = pool.oc.batch_verify(pool.items[:n], seed)
    assert exp[0] == 0
    base = edc.debug_live_allocs()
    for _ in range(8):
        eng = edc.Engine(0)
        eng.sigcache_create(4096)
        v = edc.batch.StreamVerifier(eng, capacity=1)
        live = edc.debug_live_allocs()
        assert live[0] > base[0] and live[1] > base[1]    # the counters do move
        assert eng.batch_verify(vks, sigs, msgs, z_seed=seed, want_check8=True) == exp
        assert eng.batch_wait(eng.batch_submit(vks, sigs, msgs, seed, want_check8=True), want_check8=True) == exp
        v.queue_many(vks, sigs, msgs=msgs)
        assert v.verify_detailed(seed) == exp
        assert edc.debug_live_allocs()[0] > live[0]
        v.close()
        eng.close()
        assert edc.debug_live_allocs() == base
