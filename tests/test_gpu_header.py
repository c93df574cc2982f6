"""GPU: the header hashes (edc_header_hashes, edc_header_bind) against the model of
tests/header_model.py (hashlib, the recursive RFC 6962 root, the byte rules). Every comparison is
exact: 32 bytes or one byte. The leaf counts stand on both sides of every power of two up to 64 (the
lane group of a header), the leaf lengths on both sides of every SHA-256 block boundary at all four
byte alignments, the rules on every edge the byte rule names."""
import ctypes
import random

import pytest

import header_model as hm
import valhash_model as vm
from conftest import golden

pytestmark = pytest.mark.gpu

COUNTS = [0, 1, 2, 3, 4, 5, 7, 8, 9, 13, 14, 15, 16, 17, 31, 32, 33, 63, 64]
NV = vm.NOT_MEMBER
H, V, X, L = hm.BAD_HASH, hm.BAD_VALS, hm.BAD_NEXT, hm.BAD_LINK


@pytest.fixture()
def eng(engine):
    """The shared engine, left without a key list."""
    yield engine
    engine.keycache_clear()


@pytest.fixture(scope="module")
def history():
    """10 keys, 12 versions whose sets differ -> (keys, base, updates, roots by version)"""
    rnd = random.Random("header history")
    keys = vm.make_keys(10, b"header gpu")
    base = [rnd.randrange(1, 50) for _ in range(9)] + [NV]
    updates = [[(rnd.randrange(10), rnd.choice([NV, 0, rnd.randrange(1, 50)]))] for _ in range(11)]
    roots = vm.history_roots(keys, base, updates)
    assert len(roots) == 12
    return keys, base, updates, roots


def _load(eng, history):
    keys, base, updates, roots = history
    eng.keycache_load(keys)
    eng.vhist_set(base, updates)
    return roots


def test_leaf_counts(eng):
    rnd = random.Random("header counts")
    headers = [hm.random_leaves(rnd, n, [0, 1, 33, 55, 56, 72, 120]) for n in COUNTS]
    want = [hm.mth(h) for h in headers]
    assert want[0] == hm.sha256(b"") and len(set(want)) == len(COUNTS)
    assert eng.header_hashes(headers) == want                  # one launch, groups of 64 lanes
    for h, w in zip(headers, want):                            # one launch each: G = 2, 4, 8, 16, 32, 64
        assert eng.header_hashes([h]) == [w], len(h)
    assert eng.header_hashes(headers[::-1]) == want[::-1]


def test_leaf_lengths_and_alignments(eng):
    rnd = random.Random("header lengths")
    one = lambda n: bytes(rnd.randrange(256) for _ in range(n))
    packed = [one(n) for n in hm.LENGTHS]
    starts = {sum(len(x) for x in packed[:j]) % 4 for j in range(len(packed))}
    assert starts == {0, 1, 2, 3}
    headers = [packed, packed[::-1]]
    # each length alone in its header behind 0..3 bytes of another leaf, so that it starts at every alignment
    headers += [[one(skip), one(n)] for n in hm.LENGTHS for skip in range(4)]
    headers += [[one(72)], [one(3), one(72)]]                  # the block id of a real header: two blocks
    assert eng.header_hashes(headers) == [hm.mth(h) for h in headers]
    # every leaf empty: no byte at all, bytes = NULL
    empty = [[b""] * n for n in (1, 2, 5, 14)] + [[]]
    hs, keep = eng._header_set(empty)
    assert hs.bytes is None
    assert eng.header_hashes(empty) == [hm.mth(h) for h in empty]
    assert eng.header_bind(empty, expect=[hm.mth(h) for h in empty]) == ([0] * 5, 0, [hm.mth(h) for h in empty])


def test_many_headers(eng):
    rnd = random.Random("header many")
    headers, _, _, link = hm.chain(rnd, 3000)                  # 14 leaves: 16 lanes, 4 headers a wave, 188 workgroups
    got = eng.header_hashes(headers)
    sample = rnd.sample(range(3000), 18) + [0, 2999]
    for i in sample:
        assert eng.header_hashes([headers[i]]) == [got[i]] == [hm.mth(headers[i])], i
    assert len(set(got)) == 3000
    bad, n_bad, roots = eng.header_bind(headers, expect=got, link=link)
    assert (bad, n_bad, roots) == ([0] * 3000, 0, got)


def test_rules_hold(eng, edc, history):
    set_roots = _load(eng, history)
    rnd = random.Random("header rules")
    headers, vals, nexts, link = hm.chain(rnd, 30, set_roots)
    roots = [hm.mth(h) for h in headers]
    assert eng.header_bind(headers, roots, vals, nexts, link) == ([0] * 30, 0, roots)
    assert edc.batch.verify_headers(headers, roots, vals, nexts, link, engine=eng) == ([0] * 30, 0, roots)
    assert eng.header_bind(headers)[1:] == (0, roots) and eng.header_hashes(headers) == roots
    assert edc.batch.header_hashes(headers, engine=eng) == roots
    # sentinel entries and NULL arrays set nothing, whatever the header holds
    junk = [hm.random_leaves(rnd, n) for n in (0, 3, 14, 20)]
    none = [None] * 4
    assert eng.header_bind(junk, None, none, none, none)[:2] == ([0] * 4, 0)
    assert eng.header_bind(junk, None, [hm.NONE] * 4, None, [hm.NONE] * 4)[:2] == ([0] * 4, 0)
    # the same junk under the rules: every rule fails, for want of the leaf, of its bytes, or of the match
    bad, n_bad, _ = eng.header_bind(junk, [bytes(32)] * 4, [0] * 4, [1] * 4, [0, 0, 1, 2])
    assert (bad, n_bad) == hm.bind(junk, [bytes(32)] * 4, [0] * 4, [1] * 4, [0, 0, 1, 2], set_roots)[:2] == ([15] * 4, 4)


def test_rule_edges(eng, history):
    set_roots = _load(eng, history)
    rnd = random.Random("header edges")
    base, vals, nexts, link = hm.chain(rnd, 8, set_roots)
    roots = [hm.mth(h) for h in base]
    ask = lambda hd, **kw: eng.header_bind(hd, **kw)
    # one byte flipped at P and at P + 31, each rule alone: header 5 gets exactly that rule's bit. (A changed
    # leaf changes the header's root, so under the link rule header 6, which names the old root, gets the bit too.)
    rules = {"vals": vals, "nexts": nexts, "link": link}
    for leaf, rule, bit in ((7, "vals", V), (8, "nexts", X), (4, "link", L)):
        for at in (2, 33):
            hd = [list(h) for h in base]
            hd[5][leaf] = hm.flip(hd[5][leaf], at, 0x40)
            got = ask(hd, **{rule: rules[rule]})
            assert got == hm.bind(hd, set_roots=set_roots, **{rule: rules[rule]}), (rule, at)
            assert got[0] == [0] * 5 + [bit, L if rule == "link" else 0, 0], (rule, at)
            full = ask(hd, vals=vals, nexts=nexts, link=link)
            assert full[0] == [0] * 5 + [bit, L, 0] and full[1] == 2, (rule, at)
    for at in (0, 31):
        exp = list(roots)
        exp[5] = hm.flip(exp[5], at, 0x40)
        assert ask(base, expect=exp)[:2] == ([0] * 5 + [H] + [0] * 2, 1)
    # all four at once: header 5 changed under an unchanged expect; header 6 names the old root of 5
    hd = [list(h) for h in base]
    hd[5][7] = hm.flip(hd[5][7], 2)
    hd[5][8] = hm.flip(hd[5][8], 33)
    hd[5][4] = hm.flip(hd[5][4], 20)
    got = ask(hd, expect=roots, vals=vals, nexts=nexts, link=link)
    assert got == hm.bind(hd, roots, vals, nexts, link, set_roots) and got[0] == [0] * 5 + [15, L, 0] and got[1] == 2
    # a leaf of P + 31 bytes; a rule leaf index equal to the leaf count
    hd = [list(h) for h in base]
    hd[2][7] = hd[2][7][:33]
    hd[3] = hd[3][:7]
    hd[6] = hd[6][:8]
    got = ask(hd, vals=vals, nexts=nexts)
    assert got == hm.bind(hd, vals=vals, nexts=nexts, set_roots=set_roots)
    assert got[0] == [0, 0, V, V | X, 0, 0, X, 0] and got[1] == 3
    # positions 0..3: the source at every alignment inside the leaf, leaves packed behind odd lengths
    for P in range(4):
        for pad in range(4):
            hd = [[bytes(pad), bytes(P) + set_roots[v % 12] + b"tail"[:v % 3], bytes(P) + set_roots[(v + 1) % 12]] for v in range(9)]
            vv, nn = [v % 12 for v in range(9)], [(v + 1) % 12 for v in range(9)]
            r = [hm.mth(h) for h in hd]
            hd += [[bytes(pad), bytes(P) + r[i]] for i in range(9)]
            lk = [None] * 9 + list(range(9))
            vv, nn = vv + [None] * 9, nn + [None] * 9
            got = eng.header_bind(hd, None, vv, nn, lk, vals_at=(1, P), next_at=(2, P), link_at=(1, P))
            assert got[:2] == ([0] * 18, 0), (P, pad)
            off = eng.header_bind(hd, None, vv, nn, lk, vals_at=(1, P + 1), next_at=(2, P + 1), link_at=(1, P + 1))
            assert off[:2] == hm.bind(hd, None, vv, nn, lk, set_roots, (1, P + 1), (2, P + 1), (1, P + 1))[:2] == \
                ([V | X] * 9 + [L] * 9, 18), (P, pad)


def test_links(eng):
    rnd = random.Random("header links")
    headers, _, _, link = hm.chain(rnd, 300)
    roots = [hm.mth(h) for h in headers]
    assert eng.header_bind(headers, link=link) == ([0] * 300, 0, roots)                 # backwards
    fwd = [i + 1 for i in range(299)] + [None]
    assert eng.header_bind(headers[::-1], link=fwd) == ([0] * 300, 0, roots[::-1])        # the array reversed: forwards
    # a broken chain: header 100 replaced, so 101 names a root that is no longer there
    cut = list(headers)
    cut[100] = hm.shaped(rnd, 101, roots[99], bytes(32), bytes(32))
    assert eng.header_bind(cut, link=link)[:2] == ([0] * 101 + [L] + [0] * 198, 1)
    # a header linked to itself cannot hold (it would carry its own hash); the bit is set, nothing else happens
    assert eng.header_bind(headers[:3], link=[0, 1, 2])[:2] == ([L] * 3, 3)
    assert eng.header_bind(headers[:3], link=[None, 0, 2])[:2] == ([0, 0, L], 1)
    # two headers naming the same predecessor
    twin = hm.shaped(rnd, 2, roots[0], bytes(32), bytes(32))
    assert eng.header_bind([headers[0], headers[1], twin], link=[None, 0, 0])[:2] == ([0, 0, 0], 0)
    assert eng.header_bind([headers[1], twin, headers[0]], link=[2, 2, None])[:2] == ([0, 0, 0], 0)
    assert eng.header_bind([headers[1], twin, headers[0]], link=[1, 0, None])[:2] == ([L, L, 0], 2)


def test_agreement_with_the_set_hashes(eng, history):
    set_roots = _load(eng, history)
    rnd = random.Random("header agreement")
    ver = [rnd.randrange(12) for _ in range(40)]
    expect = [set_roots[v] if rnd.random() < 0.6 else set_roots[(v + 1 + rnd.randrange(11)) % 12] for v in ver]
    expect[0], expect[7] = set_roots[ver[0]], hm.flip(set_roots[ver[7]], 31, 0x80)
    ok, n_mismatch = eng.vhist_hash_match(ver, expect)
    headers = [hm.shaped(rnd, i + 1, bytes(32), e, bytes(32)) for i, e in enumerate(expect)]
    bad, n_bad, _ = eng.header_bind(headers, vals=ver)
    assert [int(not (b & V)) for b in bad] == ok and n_bad == n_mismatch and (ok[0], ok[7]) == (1, 0)
    assert ok == [int(e == set_roots[v]) for v, e in zip(ver, expect)]


def _raw(eng, edc, headers, **fields):
    """edc_header_bind through ctypes with canaries in every output -> (rc, untouched?)"""
    hs, keep = eng._header_set(headers)
    nh = len(headers)
    for k in ("size", "reserved", "nh", "leaf_off", "byte_off", "bytes"):
        if ("hs_" + k) in fields:
            setattr(hs, k, fields.pop("hs_" + k))
    arrs = {k: (ctypes.c_uint32 * max(len(v), 1))(*v) for k, v in fields.items() if isinstance(v, list)}
    r = edc.EdcHeaderRules(ctypes.sizeof(edc.EdcHeaderRules), 0)
    r.vals_leaf, r.vals_pos, r.next_leaf, r.next_pos, r.link_leaf, r.link_pos = 7, 2, 8, 2, 4, 2
    for k, v in fields.items():
        if k in ("bad", "rules"):
            continue
        setattr(r, k, ctypes.addressof(arrs[k]) if isinstance(v, list) else v)
    bad = ctypes.create_string_buffer(b"\x07" * max(nh, 1), max(nh, 1))
    out = ctypes.create_string_buffer(b"\x07" * 32 * max(nh, 1), 32 * max(nh, 1))
    n_bad = ctypes.c_size_t(7)
    rp = None if fields.get("rules", 1) is None else ctypes.byref(r)
    rc = eng.lib.edc_header_bind(eng.ctx, ctypes.byref(hs), rp, None if fields.get("bad", 1) is None else bad, out,
                                 ctypes.byref(n_bad))
    clean = (bad.raw, out.raw, n_bad.value) == (b"\x07" * max(nh, 1), b"\x07" * 32 * max(nh, 1), 7)
    out2 = ctypes.create_string_buffer(b"\x07" * 32 * max(nh, 1), 32 * max(nh, 1))
    rc2 = eng.lib.edc_header_hashes(eng.ctx, ctypes.byref(hs), out2)
    return rc, clean, rc2, out2.raw == b"\x07" * 32 * max(nh, 1)


def test_errors(eng, edc, history):
    rnd = random.Random("header errors")
    headers, vals, nexts, link = hm.chain(rnd, 4, history[3])
    roots = [hm.mth(h) for h in headers]
    good = lambda: eng.header_bind(headers, expect=roots, link=link) == ([0] * 4, 0, roots)
    set_bad = lambda **kw: _raw(eng, edc, headers, **kw)[:2] == (-2, True)
    both_bad = lambda **kw: _raw(eng, edc, headers, **kw) == (-2, True, -2, True)
    # version rules without a registered list, and with a list but no history
    assert set_bad(vals_ver=[0] * 4) and set_bad(next_ver=[hm.NONE] * 4) and good()
    eng.keycache_load(history[0])
    assert set_bad(vals_ver=[0] * 4) and good()
    _load(eng, history)
    assert eng.header_bind(headers, roots, vals, nexts, link) == ([0] * 4, 0, roots)
    # the structures
    assert both_bad(hs_size=39) and both_bad(hs_size=0) and both_bad(hs_reserved=1) and good()
    assert set_bad(size=63) and set_bad(reserved=2) and set_bad(rules=None) and set_bad(bad=None) and good()
    hs, keep = eng._header_set(headers)
    assert eng.lib.edc_header_hashes(eng.ctx, None, ctypes.create_string_buffer(128)) == -2
    assert eng.lib.edc_header_hashes(eng.ctx, ctypes.byref(hs), None) == -2
    # the offsets: not from 0, not monotone, missing
    lo, bo, hold = list(keep[0]), list(keep[1]), []

    def arr(xs):
        hold.append((ctypes.c_uint32 * len(xs))(*xs))
        return ctypes.addressof(hold[-1])
    assert both_bad(hs_leaf_off=arr([1] + lo[1:])) and both_bad(hs_leaf_off=arr(lo[:2] + [lo[1] - 1] + lo[3:]))
    assert both_bad(hs_byte_off=arr([1] + bo[1:])) and both_bad(hs_byte_off=arr(bo[:9] + [bo[8] - 1] + bo[10:]))
    assert both_bad(hs_leaf_off=None) and both_bad(hs_byte_off=None) and both_bad(hs_bytes=None) and good()
    # versions and links past the end, other than the sentinel
    assert set_bad(vals_ver=[0, 12, 0, 0]) and set_bad(next_ver=[0, 0, 0, 12]) and set_bad(link=[0, 1, 2, 4]) and good()
    assert eng.header_bind(headers, vals=[0, 11, None, hm.NONE], link=[3, None, hm.NONE, 0])[1] == \
        hm.bind(headers, vals=[0, 11, None, None], link=[3, None, None, 0], set_roots=history[3])[1]
    # 64 leaves are accepted, 65 refused
    wide = [hm.random_leaves(rnd, 64, [0, 5, 60]), hm.random_leaves(rnd, 65, [0, 5, 60])]
    assert eng.header_hashes(wide[:1]) == [hm.mth(wide[0])]
    assert _raw(eng, edc, wide) == (-2, True, -2, True) and _raw(eng, edc, wide[::-1]) == (-2, True, -2, True) and good()
    # a version above the member cap of the set hashes
    big = vm.make_keys(4097, b"header cap")
    eng.keycache_load(big)
    eng.vhist_set([1] * 4096 + [NV], [[(4096, 1)]])
    assert set_bad(vals_ver=[0, 0, 1, 0]) and set_bad(next_ver=[1] * 4)
    assert eng.header_bind(headers, vals=[0, None, 0, None])[:2] == ([V, 0, V, 0], 2)
    # nh = 0: EDC_OK, no array read, only *n_bad written
    hs0 = edc.EdcHeaderSet(ctypes.sizeof(edc.EdcHeaderSet), 0, 0, 1, 1, 1)          # pointers that cannot be read
    r0 = edc.EdcHeaderRules(ctypes.sizeof(edc.EdcHeaderRules), 0, 1, 1, 0, 0, 1, 0, 0, 1, 0, 0)
    n_bad = ctypes.c_size_t(7)
    assert eng.lib.edc_header_bind(eng.ctx, ctypes.byref(hs0), ctypes.byref(r0), None, None, ctypes.byref(n_bad)) == 0
    assert n_bad.value == 0 and eng.lib.edc_header_hashes(eng.ctx, ctypes.byref(hs0), None) == 0
    assert eng.lib.edc_header_bind(eng.ctx, ctypes.byref(hs0), ctypes.byref(r0), None, None, None) == 0
    assert eng.header_bind([]) == ([], 0, []) and eng.header_hashes([]) == [] and good()


def test_allocations_return(edc, history):
    before = edc.debug_live_allocs()
    e2 = edc.Engine(0)
    try:
        set_roots = _load(e2, history)
        headers, vals, nexts, link = hm.chain(random.Random("header leaks"), 5, set_roots)
        roots = [hm.mth(h) for h in headers]
        assert e2.header_hashes(headers) == roots
        assert e2.header_bind(headers, roots, vals, nexts, link) == ([0] * 5, 0, roots)
        ms = e2.header_ms(headers, 2)
        assert ms["roots"] > 0 and ms["bind"] > 0
        assert edc.debug_live_allocs() > before
    finally:
        e2.close()
    assert edc.debug_live_allocs() == before


def test_fixture(eng, edc):
    g = golden("header.json")
    un = bytes.fromhex
    eng.keycache_load([un(k) for k in g["keys"]])
    eng.vhist_set(g["base"], [[tuple(pw) for pw in u] for u in g["updates"]])
    headers = [[un(x) for x in h] for h in g["headers"]]
    expect, roots = [un(e) for e in g["expect"]], [un(r) for r in g["roots"]]
    want = (g["bad"], g["n_bad"], roots)
    assert eng.header_bind(headers, expect, g["vals"], g["nexts"], g["link"]) == want
    assert edc.batch.verify_headers(headers, expect, g["vals"], g["nexts"], g["link"], engine=eng) == want
    assert edc.batch.header_hashes(headers, engine=eng) == roots
