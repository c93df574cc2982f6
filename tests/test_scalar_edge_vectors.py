"""CPU: the edge-scalar fixture (tests/golden/scalar_edges.json, built by gen_scalar_edges.py from
tests/scalar_edges.py) is what it claims to be, checked with the big-integer oracle only:
the generator reproduces the committed file byte for byte; every item verifies and every near-miss
(s +- 1, k +- 1, R + [1]B) is rejected by oracle.verify_prehashed; the reference's batch equation
summed in big integers gives the stored [8]*check and check points; the coefficients are the stored
targets; and the census holds, i.e. the vectors reach every edge they are named after."""
import os
import sys

import pytest

from conftest import GOLDEN, golden

import scalar_edges as se

o = se.o
FX = golden("scalar_edges.json")
KEYS = [bytes.fromhex(k) for k in FX["keys"]]
IDENTITY = bytes([1]) + bytes(31)


def _items(rows):
    return se.rows_items(FX, rows)


def variant_items(b, tag):
    return se.variant_items(FX, b, tag)


def test_generator_reproduces_the_fixture():
    sys.path.insert(0, GOLDEN)
    import gen_scalar_edges as gen
    with open(os.path.join(GOLDEN, "scalar_edges.json")) as f:
        assert gen.dumps(gen.build()) == f.read()


def test_keys_are_the_constructed_ones():
    assert KEYS == [o.compress(o.scalar_mul(se.secret(j), o.B_POINT)) for j in range(len(KEYS))]


def test_per_item_list_carries_the_pairs():
    items = _items(FX["per_item"])
    pairs = se.per_item_pairs()
    assert [(int.from_bytes(sig[32:], "little"), int.from_bytes(k, "little")) for _, sig, k in items] == pairs
    assert all(s < se.L and k < se.L for s, k in pairs)
    fam = se.full_scalars()
    assert set(fam) == {s for s, _ in pairs[:len(fam)]} == {k for _, k in pairs[:len(fam)]}
    assert set(pairs[len(fam):]) == {(s, k) for s in se.FIXED for k in se.FIXED}


def test_every_item_verifies_and_every_near_miss_is_rejected():
    rows = [(j, bytes.fromhex(sig), bytes.fromhex(k)) for j, sig, k in FX["per_item"]]
    for row in rows:
        assert o.verify_prehashed(KEYS[row[0]], row[1], int.from_bytes(row[2], "little")) == o.OK
        for kind in se.NEAR_KINDS:
            j, sig, k = se.near_miss(row, kind)
            assert o.verify_prehashed(KEYS[j], sig, int.from_bytes(k, "little")) == o.INVALID_SIGNATURE, kind


@pytest.mark.parametrize("b", FX["batches"], ids=lambda b: b["name"])
def test_batch_items_verify_one_by_one(b):
    for tag in ("z", "seeded"):
        rows = b["z"]["items"] if tag == "z" else b["seeded"]["solvers"]
        for vk, sig, k in _items(rows):
            assert o.verify_prehashed(vk, sig, int.from_bytes(k, "little")) == o.OK


@pytest.mark.parametrize("tag", ["z", "seeded"])
@pytest.mark.parametrize("b", FX["batches"], ids=lambda b: b["name"])
def test_batch_equation_in_big_integers(b, tag):
    """Coefficients equal the targets; the big-int MSM of the valid batch and of its twin give the
    stored code, [8]*check and affine check point; a corrupted item under z = 0 changes nothing."""
    items, z = variant_items(b, tag)
    v = b[tag]
    keys, bc = se.coefficients(items, z)
    assert bc == int.from_bytes(bytes.fromhex(b["b_target"]), "little")
    targets = [int.from_bytes(bytes.fromhex(t), "little") for t in b["key_targets"]]
    assert [keys[KEYS[j]] for j in range(len(targets))] == targets and len(keys) == len(targets)
    for name, batch in (("valid", items), ("twin", se.twin_of(items, v))):
        pt = se.batch_check(batch, z)
        c8 = o.mul_by_cofactor(pt)
        x, y = se.affine(pt)
        exp = v[name]
        assert exp["code"] == (o.OK if o.is_identity(c8) else o.INVALID_SIGNATURE) == (0 if name == "valid" else 1)
        assert exp["check8"] == o.compress(c8).hex()
        assert (exp["x"], exp["y"]) == (se.sc(x).hex(), se.sc(y).hex())
    assert v["valid"]["check8"] == IDENTITY.hex() != v["twin"]["check8"]
    if tag == "z" and b["zero_z_pos"] is not None:
        p = b["zero_z_pos"]
        assert z[p] == 0
        bad = list(items)
        j = KEYS.index(bad[p][0])
        _, sig, k = se.near_miss((j, bad[p][1], bad[p][2]), "R+B")
        bad[p] = (bad[p][0], sig, k)
        assert o.compress(se.batch_check(bad, z)) == o.compress(se.batch_check(items, z))


def test_b0_holds_the_maximal_key():
    b = FX["batches"][0]
    items, z = variant_items(b, "z")
    top = [i for i, (vk, sig, k) in enumerate(items)
           if vk == KEYS[0] and z[i] == se.M128 and sig[32:] == k == se.sc(se.L - 1)]
    assert len(top) >= 64


def test_all_zero_batch():
    b = [x for x in FX["batches"] if x["name"] == "all_zero"][0]
    for tag in ("z", "seeded"):
        keys, bc = se.coefficients(*variant_items(b, tag))
        assert bc == 0 and set(keys.values()) == {0}


def test_census():
    """The vectors reach every named edge (computed from the fixture's bytes with the recodings
    restated in scalar_edges.py). The radix-16 recoding's digits lie in [-7, 8]: its extremes are
    -7 and +8 (a digit of -8 does not exist), as radix-256's are -127 and +128."""
    batches = [variant_items(b, tag) for b in FX["batches"] for tag in ("z", "seeded")]
    c = se.census(_items(FX["per_item"]), batches)
    missing = sorted(k for k, v in c.items() if not v)
    assert not missing, missing
    assert len(c) >= 40
