"""Generate tests/golden/decode_edges.json from the CPU oracle (oracle/ed25519_ref.py).
Run: python tests/golden/gen_decode_edges.py

Edge encodings for ZIP215 point decoding, in the record shape of decode.json (enc, ok, x, y, order
from oracle.decompress). Every y below with both sign bits, duplicates dropped, in this order:
  * the non-canonical y = p + k, k = 0..18 (all 38 encodings; 14 of them are off the curve);
  * y = 0..20 and p - 1..p - 20 (y = +-1 with the sign bit set: x = 0, "negative zero");
  * 2^252, 2^254, 2^254 +- 1, 2^255 - 20..2^255 - 1;
  * y extreme in the device's radix-2^29 limbs (nine limbs, the top one 23 bits): every limb all
    ones, alternate limbs all ones (both phases), alternate bits (both phases), one limb all ones
    for each of the nine, the top limb's lowest and highest bit alone.
DATA only.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "oracle"))
import ed25519_ref as o  # noqa: E402

P = o.P
LIMB_BITS = [29] * 8 + [23]


def _limbs(vals):
    out, off = 0, 0
    for v, bits in zip(vals, LIMB_BITS):
        assert v < 1 << bits
        out |= v << off
        off += bits
    return out


def y_values():
    full = [(1 << b) - 1 for b in LIMB_BITS]
    ys = [P + k for k in range(19)]
    ys += list(range(21)) + [P - k for k in range(1, 21)]
    ys += [1 << 252, 1 << 254, (1 << 254) - 1, (1 << 254) + 1] + [(1 << 255) - k for k in range(20, 0, -1)]
    ys += [_limbs(full), _limbs([f if i % 2 == 0 else 0 for i, f in enumerate(full)]),
           _limbs([f if i % 2 else 0 for i, f in enumerate(full)]),
           int.from_bytes(bytes([0x55]) * 32, "little") & ((1 << 255) - 1),
           int.from_bytes(bytes([0xAA]) * 32, "little") & ((1 << 255) - 1)]
    ys += [_limbs([f if i == j else 0 for i, f in enumerate(full)]) for j in range(9)]
    ys += [1 << 232, 1 << 254]
    return list(dict.fromkeys(ys))


def encodings():
    out = []
    for y in y_values():
        assert 0 <= y < 1 << 255
        for sign in (0, 1):
            out.append((y | (sign << 255)).to_bytes(32, "little"))
    return out


def off_curve_non_canonical():
    """The 14 encodings y = p + k, k = 0..18, that do not decode (k in 2, 7, 8, 11, 12, 13, 17)."""
    return [e for e in encodings()[:38] if o.decompress(e) is None]


def build():
    cases = []
    for e in encodings():
        pt = o.decompress(e)
        cases.append({"enc": e.hex(), "ok": pt is not None,
                      "x": None if pt is None else (pt[0] % P).to_bytes(32, "little").hex(),
                      "y": None if pt is None else (pt[1] % P).to_bytes(32, "little").hex(),
                      "order": None if pt is None else o.point_order(pt)})
    return {"source": "oracle decompress (dalek CompressedEdwardsY::decompress restated) on chosen edge "
                      "encodings; see gen_decode_edges.py for the list",
            "cases": cases}


def dumps(doc):
    return json.dumps(doc, indent=1) + "\n"


def main():
    doc = build()
    with open(os.path.join(HERE, "decode_edges.json"), "w") as f:
        f.write(dumps(doc))
    print("wrote decode_edges.json: %d cases, %d decode" % (len(doc["cases"]), sum(c["ok"] for c in doc["cases"])))


if __name__ == "__main__":
    main()
