"""Generate tests/golden/mixed_order.json from tests/mixed_order.py and the CPU oracle
(oracle/ed25519_ref.py). Run: python tests/golden/gen_mixed_order.py

Mixed-order keys A = [a]B + T_t (every t, t = 0 the honest control) under valid signatures whose R
carries torsion too (construction: tests/mixed_order.py). Stored: the z seed; the keys (position
8 j + t); the message items [key position, sig, msg] over all 64 (t, u); the prehashed items
[key position, sig, k] with k through every residue mod 8 per (t, u); and per batch (the whole item
list of its form, z from the seed) the defects [position, delta], the expected per-item codes, the
batch code and [8]*check. DATA only.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
import mixed_order as mo  # noqa: E402

se = mo.se


def _row(it):
    return [it[0], it[1].hex(), it[2].hex()]


def build():
    rows = {"msg": mo.message_items(), "pre": mo.prehashed_items()}
    batches = {}
    for name, (form, defects) in mo.BATCHES.items():
        codes, code, c8 = mo.expected(len(rows[form]), defects)
        batches[name] = {"form": form, "defects": [[pos, se.sc(d).hex()] for pos, d in defects],
                         "codes": codes, "code": code, "check8": c8.hex()}
    return {
        "seed": mo.SEED.hex(),
        "keys": [k.hex() for k in mo.keys()],
        "pre_pairs": [list(p) for p in mo.PRE_PAIRS],
        "msg_items": [_row(it) for it in rows["msg"]],
        "pre_items": [_row(it) for it in rows["pre"]],
        "batches": batches,
    }


def dumps(doc):
    return json.dumps(doc, indent=0, sort_keys=True) + "\n"


def main():
    doc = build()
    with open(os.path.join(HERE, "mixed_order.json"), "w") as f:
        f.write(dumps(doc))
    print("wrote mixed_order.json: %d keys, %d message items, %d prehashed items, batches %s" %
          (len(doc["keys"]), len(doc["msg_items"]), len(doc["pre_items"]), sorted(doc["batches"])))


if __name__ == "__main__":
    main()
