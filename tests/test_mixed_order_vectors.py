"""CPU: the mixed-order fixture (tests/golden/mixed_order.json, built by gen_mixed_order.py from
tests/mixed_order.py) and the decode-edge fixture (tests/golden/decode_edges.json, built by
gen_decode_edges.py) are what they claim to be, checked with the oracles only: the generators
reproduce the committed files byte for byte; every item's stored code is oracle.verify's /
verify_prehashed's; every batch's (code, [8]*check) is oracle.batch_verify_seeded's, the C oracle's
and the integer formula's; the inputs reach what they are named after (all (t, u), all k mod 8, keys
outside both subgroups; every outcome of the square root and of the sign select); and the host build
of the device headers decodes every edge encoding as the oracle does."""
import ctypes
import os
import sys

import pytest

from conftest import GOLDEN, ROOT, golden

sys.path.insert(0, GOLDEN)
import gen_decode_edges  # noqa: E402
import gen_mixed_order  # noqa: E402
import mixed_order as mo  # noqa: E402
from test_native_math import hc  # noqa: F401  (the host build of csrc/*.h)

o = mo.o
se = mo.se
FX = golden("mixed_order.json")
EDGES = golden("decode_edges.json")["cases"]
SEED = bytes.fromhex(FX["seed"])
KEYS = [bytes.fromhex(k) for k in FX["keys"]]
IDENTITY = bytes([1]) + bytes(31)


@pytest.fixture(scope="module")
def oracle_c():
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import oracle_c as oc
    return oc


@pytest.mark.parametrize("name", ["mixed_order", "decode_edges"])
def test_generator_reproduces_the_fixture(name):
    gen = {"mixed_order": gen_mixed_order, "decode_edges": gen_decode_edges}[name]
    with open(os.path.join(GOLDEN, name + ".json")) as f:
        assert gen.dumps(gen.build()) == f.read()


# ---------------------------------------------------------------- mixed-order keys
def test_keys_lie_outside_both_subgroups():
    """A_{j,t} = [a_j]B + T_t: [l]A = [l mod 8]T_t has the order of T_t, so for t != 0 the key is in
    neither the prime-order subgroup nor the torsion subgroup; t = 0 is the honest control."""
    assert KEYS == mo.keys() and len(KEYS) == 8 * mo.NSECRETS
    for pos, enc in enumerate(KEYS):
        A = o.decompress(enc)
        order = o.point_order(o.scalar_mul(o.L, A))
        assert order == str(mo.TORSION_ORDER[pos % 8]), pos
        assert (int(order) > 1) == (pos % 8 != 0)
        assert o.point_order(A) == ("p" if pos % 8 == 0 else "8p")
        assert enc == o.compress(o.add(o.scalar_mul(mo.secret(pos // 8), o.B_POINT), mo.TORSION[pos % 8]))


def _torsion_index(pt):
    """u with pt - [r]B = T_u, found as [l]pt = [l mod 8]T_u = [5]T_u -> u = 5 * index mod 8."""
    enc = o.compress(o.scalar_mul(o.L, pt))
    return 5 * o.eight_torsion_encodings().index(enc) % 8


def test_message_items_cover_all_pairs():
    pairs = set()
    for j, sig, _ in FX["msg_items"]:
        pairs.add((j % 8, _torsion_index(o.decompress(bytes.fromhex(sig)[:32]))))
    assert pairs == {(t, u) for t in range(8) for u in range(8)}
    assert all(int.from_bytes(bytes.fromhex(sig)[32:], "little") != 0 for _, sig, _ in FX["msg_items"])


def test_prehashed_items_sweep_k_mod_8():
    """Per (t, u): every residue of k mod 8, and k = 8, l - 1, l - 8; T_t of each order 2, 4, 8. A
    cofactorless check would accept exactly the residues with k T_t + T_u = 0, and the sweep holds
    both kinds for every mixed-order pair."""
    seen = {}
    for j, sig, k in FX["pre_items"]:
        u = _torsion_index(o.decompress(bytes.fromhex(sig)[:32]))
        seen.setdefault((j % 8, u), []).append(int.from_bytes(bytes.fromhex(k), "little"))
    assert sorted(seen) == sorted(tuple(p) for p in FX["pre_pairs"]) == sorted(mo.PRE_PAIRS)
    assert {mo.TORSION_ORDER[t] for t, _ in seen} == {1, 2, 4, 8}
    for (t, u), ks in seen.items():
        assert {k % 8 for k in ks} == set(range(8)), (t, u)
        assert {8, o.L - 1, o.L - 8} <= set(ks) and max(ks) < o.L, (t, u)
        cancels = [k for k in ks if (k * t + u) % 8 == 0]
        if t:
            assert cancels != ks, (t, u)         # some residue leaves torsion behind


@pytest.mark.parametrize("name", sorted(FX["batches"]))
def test_every_item_has_the_oracle_verdict(name):
    form, items, codes, _ = mo.fixture_batch(FX, name)
    for (vk, sig, c), code in zip(items, codes):
        got = o.verify(vk, sig, c) if form == "msg" else o.verify_prehashed(vk, sig, int.from_bytes(c, "little"))
        assert got == code
    assert len(codes) == len(items)
    assert sum(codes) == len(FX["batches"][name]["defects"])


@pytest.mark.parametrize("name", sorted(FX["batches"]))
def test_batches_against_the_oracles(name, oracle_c):
    """(code, [8]*check): the stored value is the integer formula's, the Python oracle's batch
    equation (with the caller's k for the prehashed form) and, for messages, the C oracle's."""
    form, items, codes, exp = mo.fixture_batch(FX, name)
    b = FX["batches"][name]
    defects = [(pos, int.from_bytes(bytes.fromhex(d), "little")) for pos, d in b["defects"]]
    assert mo.expected(len(items), defects) == (codes, exp[0], exp[1])
    assert (exp[1] == IDENTITY) == (exp[0] == 0) == (not defects)
    z = o.z_values(SEED, len(items))
    if form == "msg":
        assert o.batch_verify_seeded(items, SEED) == exp
        assert oracle_c.batch_verify(items, SEED) == exp
        items = [(vk, sig, se.sc(o.challenge(sig[:32], vk, m))) for vk, sig, m in items]
    c8 = o.mul_by_cofactor(se.batch_check(items, z))
    assert (0 if o.is_identity(c8) else 1, o.compress(c8)) == exp


def test_each_mixed_key_signs_several_items():
    for form in ("msg", "pre"):
        count = {}
        for j, _, _ in FX[form + "_items"]:
            count[j] = count.get(j, 0) + 1
        assert min(v for j, v in count.items() if j % 8) >= 2, form


# ---------------------------------------------------------------- decode edges
def _classify(enc):
    """(outcome of sqrt_ratio_i, whether the sign select negates) with oracle.sqrt_ratio_i's terms:
    check = v r^2 against u ("correct") and -u ("flipped"), else rejected; the raw root r (times
    sqrt(-1) when flipped) is negated iff its parity differs from the encoding's sign bit."""
    P = o.P
    y = int.from_bytes(enc, "little") & ((1 << 255) - 1)
    u, v = (y * y - 1) % P, (o.D * y * y + 1) % P
    v3 = v * v % P * v % P
    v7 = v3 * v3 % P * v % P
    r = (u * v3 % P) * pow(u * v7 % P, (P - 5) // 8, P) % P
    check = v * r % P * r % P
    if check == u:
        outcome = "correct"
    elif check == (-u) % P:
        outcome, r = "flipped", r * o.SQRT_M1 % P
    else:
        return "rejected", None
    assert o.sqrt_ratio_i(u, v) == (True, r if r % 2 == 0 else P - r)
    return outcome, (r & 1) != enc[31] >> 7


def test_decode_edges_reach_every_arm():
    gen = gen_decode_edges
    encs = [bytes.fromhex(c["enc"]) for c in EDGES]
    assert encs == gen.encodings() and len(set(encs)) == len(encs)
    classes = {"correct": 0, "flipped": 0, "rejected": 0, "negated": 0, "kept": 0}
    for c, e in zip(EDGES, encs):
        outcome, negated = _classify(e)
        assert (outcome != "rejected") == c["ok"] == (o.decompress(e) is not None)
        classes[outcome] += 1
        if c["ok"]:
            classes["negated" if negated else "kept"] += 1
            pt = o.decompress(e)
            assert (c["x"], c["y"]) == (se.sc(pt[0]).hex(), se.sc(pt[1]).hex())
    assert min(classes.values()) >= 10, classes
    off = [(o.P + k) | (s << 255) for k in (2, 7, 8, 11, 12, 13, 17) for s in (0, 1)]
    off = [v.to_bytes(32, "little") for v in off]
    assert set(off) <= set(encs) and sorted(off) == sorted(gen.off_curve_non_canonical())
    assert all(o.decompress(e) is None for e in off)
    by_y = {int.from_bytes(e, "little"): c["ok"] for c, e in zip(EDGES, encs)}
    for y in range(2, 8):
        assert by_y[y] == by_y[y | 1 << 255] == by_y[o.P - y] == (y in (3, 4, 5, 6)), y
    assert {1 << 252, 1 << 254} <= set(by_y)
    for y in (1, o.P - 1):                       # x = 0 with the sign bit set: accepted, x stays 0
        c = EDGES[encs.index((y | 1 << 255).to_bytes(32, "little"))]
        assert c["ok"] and c["x"] == bytes(32).hex()


def test_host_build_decodes_the_edges(hc):  # noqa: F811
    """tests/native/hostcheck.cpp's hc_decompress (ge_decompress of ge25519.h compiled for the host)
    over decode_edges.json, as test_native_math.py runs it over decode.json."""
    out = ctypes.create_string_buffer(64)
    for c in EDGES:
        ok = hc.hc_decompress(bytes.fromhex(c["enc"]), out)
        assert bool(ok) == c["ok"], c["enc"]
        if ok:
            assert out.raw[:32].hex() == c["x"] and out.raw[32:].hex() == c["y"], c["enc"]
