"""Generate tests/golden/scalar_edges.json from tests/scalar_edges.py and the CPU oracle
(oracle/ed25519_ref.py). Run: python tests/golden/gen_scalar_edges.py

Valid prehashed items whose s and k are chosen edge scalars, and batches whose z, key coefficients
and B coefficient are chosen edge scalars (construction: tests/scalar_edges.py). Stored: the keys;
the per-item list as [key index, sig, k]; per batch its targets, its caller-drawn z and items, the
solver items again for z drawn from `seed` (the other items are the same), and for the all-valid
batch and its perturbed twin (one R moved by a multiple of B) the expected code, [8]*check and the
affine check point before the cofactor. DATA only.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
import scalar_edges as se  # noqa: E402

o = se.o


def _item(it):
    return [it[0], it[1].hex(), it[2].hex()]


def _expect(pt):
    c8 = o.mul_by_cofactor(pt)
    x, y = se.affine(pt)
    return {"code": o.OK if o.is_identity(c8) else o.INVALID_SIGNATURE, "check8": o.compress(c8).hex(),
            "x": se.sc(x).hex(), "y": se.sc(y).hex()}


def _variant(v, nfree, seeded):
    out = {"twin_pos": v["twin_pos"], "twin_sig": v["twin_sig"].hex(),
           "valid": _expect(v["valid_check"]), "twin": _expect(v["twin_check"])}
    if seeded:
        out["solvers"] = [_item(it) for it in v["items"][nfree:]]
    else:
        out["z"] = [se.sc(z, 16).hex() for z in v["z"]]
        out["items"] = [_item(it) for it in v["items"]]
    return out


def build():
    batches = se.build_batches()
    nkeys = max([b["nkeys"] for b in batches] + [se.NKEYS_PER_ITEM])
    return {
        "seed": se.SEED.hex(),
        "keys": [se.key(j)[1].hex() for j in range(nkeys)],
        "per_item": [_item(it) for it in se.per_item_items()],
        "batches": [{"name": b["name"], "b_target": se.sc(b["b_target"]).hex(),
                     "key_targets": [se.sc(t).hex() for t in b["key_targets"]],
                     "nfree": b["nfree"], "zero_z_pos": b["zero_z_pos"],
                     "z": _variant(b["variants"]["z"], b["nfree"], False),
                     "seeded": _variant(b["variants"]["seeded"], b["nfree"], True)} for b in batches],
    }


def dumps(doc):
    return json.dumps(doc, indent=0, sort_keys=True) + "\n"


def main():
    doc = build()
    with open(os.path.join(HERE, "scalar_edges.json"), "w") as f:
        f.write(dumps(doc))
    print("wrote scalar_edges.json: %d per-item items, batches %s" %
          (len(doc["per_item"]), {b["name"]: len(b["z"]["items"]) for b in doc["batches"]}))


if __name__ == "__main__":
    main()
