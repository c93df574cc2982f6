"""GPU: the validator-set hashes (edc_valhash_valset, edc_valhash_vhist, edc_valhash_vhist_match) against
the model of tests/valhash_model.py (hashlib, the recursive RFC 6962 root). Every comparison is exact:
32 bytes. The member counts stand on both sides of every power of two up to 257 (where the promotion
of the lone last node and the padding of the LDS sort differ) and at the cap; the powers at every
uvarint length; the histories move members in and out."""
import ctypes
import random

import pytest

import valhash_model as vm
from test_gpu_vhist import Signed
from test_vhist_abi import gen_vhist

pytestmark = pytest.mark.gpu

N = vm.NOT_MEMBER
COUNTS = [0, 1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65, 150, 255, 256, 257]
CAP = 4096
ERR = "edc error -2"


@pytest.fixture()
def eng(engine):
    """The shared engine, left without a key list."""
    yield engine
    engine.keycache_clear()


def _set(eng, keys, base, updates=()):
    eng.keycache_load(keys)
    eng.vhist_set(base, updates)
    return vm.history_roots(keys, base, updates)


def _sized_history(rnd, counts):
    """Version j holds the positions 0 .. counts[j] - 1, with small mixed powers that repeat."""
    m = max(counts)
    pw = lambda: rnd.choice([0, 1, 1, 7, 7, 7, 300, 1 << 21])
    base = [pw() if p < counts[0] else N for p in range(m)]
    updates = []
    for a, b in zip(counts, counts[1:]):
        updates.append([(p, pw()) for p in range(a, b)] + [(p, N) for p in range(b, a)])
    return base, updates


def test_member_counts_around_powers_of_two(eng, edc):
    rnd = random.Random("valhash counts")
    keys = vm.make_keys(max(COUNTS))
    base, updates = _sized_history(rnd, COUNTS)
    want = _set(eng, keys, base, updates)
    assert eng.vhist_totals()[1] == COUNTS
    assert eng.vhist_hashes() == want                          # one launch, sized for 257 members
    for v, c in enumerate(COUNTS):                             # one launch each, sized for its own count
        assert eng.vhist_hashes(v, 1) == [want[v]], c
    assert want[0] == vm.sha256(b"") and len(set(want)) == len(COUNTS)
    assert edc.batch.validator_set_hashes(engine=eng) == want
    assert edc.batch.validator_set_hashes([5, 3, 5, 4, 15], engine=eng) == [want[v] for v in (5, 3, 5, 4, 15)]


def test_cap_and_one_past_it(eng, edc):
    """4096 members hash (112 KB of LDS); a version of 4097 is refused with nothing written."""
    rnd = random.Random("valhash cap")
    keys = vm.make_keys(CAP + 1, b"cap")
    base = [rnd.choice([1, 2, 2, 1000]) for _ in range(CAP)] + [N]
    updates = [[(CAP, 5)], [(0, N)]]                           # 4096, 4097, 4096 members
    want = _set(eng, keys, base, updates)
    assert eng.vhist_totals()[1] == [CAP, CAP + 1, CAP]
    assert eng.vhist_hashes(0, 1) == [want[0]] and eng.vhist_hashes(2, 1) == [want[2]]
    out = ctypes.create_string_buffer(b"\x07" * 96, 96)
    for v0, count in ((1, 1), (0, 3), (0, 2), (1, 2)):
        assert eng.lib.edc_valhash_vhist(eng.ctx, v0, count, out) == -2
    ok, bad = ctypes.create_string_buffer(b"\x07" * 2, 2), ctypes.c_size_t(7)
    ver = (ctypes.c_uint32 * 2)(0, 1)
    assert eng.lib.edc_valhash_vhist_match(eng.ctx, 2, ver, want[0] + want[1], ok, ctypes.byref(bad)) == -2
    assert (out.raw, ok.raw, bad.value) == (b"\x07" * 96, b"\x07" * 2, 7)
    assert eng.vhist_hash_match([2, 0], [want[2], want[0]]) == ([1, 1], 0)       # the context is usable
    # the one set at the cap's far side: 4097 powers are refused, too
    eng.valset_set_powers([1] * (CAP + 1))
    with pytest.raises(edc.EngineError, match=ERR):
        eng.valset_hash()


def test_powers(eng):
    keys = vm.make_keys(24, b"powers")
    edges = sorted({1} | {(1 << (7 * k)) - 1 for k in range(1, 9)} | {1 << (7 * k) for k in range(1, 9)})   # lengths 1..9
    assert sorted({len(vm.uvarint(x)) for x in edges}) == list(range(1, 10)) and sum(edges) <= vm.MAX_POWER
    m = len(edges)
    base = edges + [N] * (24 - m)
    updates = [
        [(p, N) for p in range(1, m)] + [(0, vm.MAX_POWER)],   # 1: 2^63 - 1 alone in its set
        [(p, 0) for p in range(m)],                            # 2: power 0, the field omitted
        [(p, 5) for p in range(24)],                           # 3: all equal: the order is by address alone
        [(p, 100 + p) for p in range(24)],                     # 4: distinct, ascending by position: the sort reverses
        [(3, 120), (20, 103)],                                 # 5: two members swap powers ...
        [(3, 103), (20, 120)],                                 # 6: ... and swap back
    ]
    want = _set(eng, keys, base, updates)
    assert eng.vhist_hashes() == want
    assert want[1] == vm.sha256(b"\x00" + vm.leaf(keys[0], vm.MAX_POWER))
    assert want[2] == vm.mth([b"\x0a\x22\x0a\x20" + k for k in sorted(keys[:m], key=vm.address)])
    assert [p for p, _, _ in vm.ordered([(p, keys[p], 100 + p) for p in range(24)])] == list(range(23, -1, -1))
    assert want[6] == want[4] != want[5] and len(set(want)) == 6


def test_history_moves(eng):
    rnd = random.Random("valhash history")
    keys = vm.make_keys(10, b"moves")
    base = [rnd.randrange(1, 50) for _ in range(9)] + [N]      # position 9 is never a member
    updates = []
    for v in range(300):
        if v == 3:
            updates.append([(2, N)])                           # removed ...
        elif v == 10:
            updates.append([(2, 33)])                          # ... and re-added
        elif v == 11:
            updates.append([(2, 33), (4, base[4])])            # restates the current state
        else:
            updates.append([(p, rnd.choice([N, 0, rnd.randrange(1, 50)])) for p in rnd.sample(range(9), rnd.randrange(0, 4))
                            if p not in (2, 4) or v > 11])
    want = _set(eng, keys, base, updates)
    assert want[11] == want[12] and want[3] != want[4] and len(set(want)) > 100
    assert eng.vhist_hashes() == want                          # 301 workgroups
    assert eng.vhist_hashes(7, 40) == want[7:47] and eng.vhist_hashes(300, 1) == want[300:]
    assert eng.vhist_hashes(301, 0) == [] and eng.vhist_hashes(0, 0) == []
    out = ctypes.create_string_buffer(b"\x07" * 64, 64)
    for v0, count in ((301, 1), (302, 0), (300, 2)):           # past nv
        assert eng.lib.edc_valhash_vhist(eng.ctx, v0, count, out) == -2
    assert eng.lib.edc_valhash_vhist(eng.ctx, 0, 1, None) == -2
    assert out.raw == b"\x07" * 64


def test_match(eng, edc):
    rnd = random.Random("valhash match")
    keys = vm.make_keys(9, b"match")
    base = [rnd.randrange(1, 50) for _ in range(9)]
    updates = [[(rnd.randrange(9), rnd.randrange(1, 50))] for _ in range(20)]
    want = _set(eng, keys, base, updates)
    ver = [20, 3, 3, 0, 17, 3, 20, 1, 0, 9]                    # repeated, unordered
    expect = [want[v] for v in ver]
    assert eng.vhist_hash_match(ver, expect) == ([1] * 10, 0)
    flip = lambda b, i, bit: b[:i] + bytes([b[i] ^ bit]) + b[i + 1:]
    expect[2], expect[6] = flip(expect[2], 0, 0x01), flip(expect[6], 31, 0x80)
    assert eng.vhist_hash_match(ver, expect) == ([1, 1, 0, 1, 1, 1, 0, 1, 1, 1], 2)
    assert edc.batch.validator_set_hashes(ver, expect, engine=eng) == ([1, 1, 0, 1, 1, 1, 0, 1, 1, 1], 2)
    assert eng.vhist_hash_match([4], [want[5]]) == ([0], 1)
    assert eng.vhist_hash_match([], []) == ([], 0)
    ok, bad = ctypes.create_string_buffer(b"\x07" * 2, 2), ctypes.c_size_t(7)
    v2 = (ctypes.c_uint32 * 2)(0, 21)                          # above nv
    assert eng.lib.edc_valhash_vhist_match(eng.ctx, 2, v2, want[0] * 2, ok, ctypes.byref(bad)) == -2
    v2[1] = 1
    assert eng.lib.edc_valhash_vhist_match(eng.ctx, 2, v2, want[0] * 2, None, ctypes.byref(bad)) == -2
    assert eng.lib.edc_valhash_vhist_match(eng.ctx, 2, v2, None, ok, ctypes.byref(bad)) == -2
    assert (ok.raw, bad.value) == (b"\x07" * 2, 7)
    assert eng.lib.edc_valhash_vhist_match(eng.ctx, 2, v2, want[0] + want[1], ok, None) == 0 and ok.raw == b"\x01\x01"


def test_set_lifecycle(eng, edc):
    keys, other = vm.make_keys(9, b"life"), vm.make_keys(12, b"other")
    base = [3, 9, 9, 1, 0, 40, 2, 9, 5]
    for call in (eng.valset_hash, eng.vhist_hashes, lambda: eng.vhist_hash_match([0], [bytes(32)])):
        with pytest.raises(edc.EngineError, match=ERR):        # no key list
            call()
    eng.keycache_load(keys)
    for call in (eng.valset_hash, lambda: eng.vhist_hashes(0, 0), lambda: eng.vhist_hash_match([0], [bytes(32)])):
        with pytest.raises(edc.EngineError, match=ERR):        # a list, but no powers and no history
            call()
    eng.valset_set_powers(base)
    eng.vhist_set(base, [[(0, N)]])
    want = vm.history_roots(keys, base, [[(0, N)]])
    one = eng.valset_hash()
    assert one == want[0] == vm.root([(p, keys[p], w) for p, w in enumerate(base)])
    assert eng.vhist_hashes() == want and edc.batch.validator_set_hashes(engine=eng) == want
    assert eng.lib.edc_valhash_valset(eng.ctx, None) == -2
    # an added key is a member of no version and of no set
    eng.keycache_add(other[:3])
    assert eng.valset_hash() == one and eng.vhist_hashes() == want
    # a new list drops the powers, the history and the address order with them
    eng.keycache_load(other)
    for call in (eng.valset_hash, eng.vhist_hashes):
        with pytest.raises(edc.EngineError, match=ERR):
            call()
    base2 = [7] * 12
    eng.vhist_set(base2, [[(11, N)], [(11, 7)]])
    want2 = vm.history_roots(other, base2, [[(11, N)], [(11, 7)]])
    assert eng.vhist_hashes() == want2 and want2[0] == want2[2] != want2[1]
    with pytest.raises(edc.EngineError, match=ERR):            # the history is set, the one set is not
        eng.valset_hash()
    # a new history on the same list: the new roots, nothing of the old ones
    eng.vhist_set([1] * 12)
    assert eng.vhist_hashes() == vm.history_roots(other, [1] * 12, [])
    eng.vhist_set(None)                                        # cleared
    with pytest.raises(edc.EngineError, match=ERR):
        eng.vhist_hashes()
    eng.valset_set_powers([2] * 12)
    assert eng.valset_hash() == vm.root([(p, other[p], 2) for p in range(12)]) == edc.batch.validator_set_hashes(engine=eng)[0]


def test_quorum_request_is_not_disturbed(eng):
    g = gen_vhist()
    S = Signed(eng, g, "valhash neighbours", m=12, nc=4, per=8, nv=5)
    S.register(eng, g)
    seed = bytes([5]) * 32
    ask = lambda: eng.vq_verify(S.off, S.flag, S.thr, seed, light=True, versions=S.ver, vks=S.vks, sigs=S.sigs, msgs=S.msgs)
    before = ask()
    want = vm.history_roots(S.keys, S.base, S.updates)
    assert eng.vhist_hashes() == want
    assert eng.vhist_hash_match(S.ver, [want[v] for v in S.ver]) == ([1] * 4, 0)
    assert ask() == before
    assert eng.vhist_hashes() == want


def test_allocations_return(edc):
    before = edc.debug_live_allocs()
    e2 = edc.Engine(0)
    try:
        keys = vm.make_keys(9, b"leaks")
        e2.keycache_load(keys)
        e2.valset_set_powers([1] * 9)
        e2.vhist_set([1] * 9, [[(0, 2)]])
        want = vm.history_roots(keys, [1] * 9, [[(0, 2)]])
        assert e2.valset_hash() == want[0] and e2.vhist_hashes() == want
        assert e2.vhist_hash_match([1, 0], want) == ([0, 0], 2)
        assert edc.debug_live_allocs() > before
    finally:
        e2.close()
    assert edc.debug_live_allocs() == before
