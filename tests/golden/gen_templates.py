"""Generate tests/golden/templates.json from the CPU oracle (oracle/ed25519_ref.py).
Run: python tests/golden/gen_templates.py

Templated messages (include/edc.h, edc_tmpl_*): message i = heads[tpl[i]] + hole_i + tails[tpl[i]].
Each case holds a template set, the items (template index, hole, key and signature), and what the
oracle says about the MATERIALISED messages: k of every item, the batch verdict and [8]*check for
the fixed z seed, and Item::verify_single's code per item. DATA only.
"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "oracle"))
import ed25519_ref as o  # noqa: E402

Z_SEED = bytes([0x35]) * 32
NKEYS = 5
# total message lengths at the SHA-512 block boundaries (the hash covers 64 + len bytes: the block
# count changes at 47 -> 48 and 175 -> 176) and at the 16-byte staging boundaries
TOTALS = [0, 1, 15, 16, 17, 47, 48, 111, 112, 175, 176, 300]


def stream(label, n):
    out, c = b"", 0
    while len(out) < n:
        out += hashlib.sha512(b"templates/" + label.encode() + c.to_bytes(4, "little")).digest()
        c += 1
    return out[:n]


def finish(name, heads, tails, tpl, holes, flip=None):
    """Sign the materialised messages; flip = (item, byte of its hole) corrupted AFTER signing."""
    seeds = [stream("key%d" % j, 32) for j in range(NKEYS)]
    keys = [o.public_key(s) for s in seeds]
    key_idx = [(7 * i + 3) % NKEYS for i in range(len(tpl))]
    msgs = [heads[t] + h + tails[t] for t, h in zip(tpl, holes)]
    sigs = [o.sign(seeds[j], m) for j, m in zip(key_idx, msgs)]
    if flip is not None:
        i, b = flip
        holes = list(holes)
        holes[i] = holes[i][:b] + bytes([holes[i][b] ^ 1]) + holes[i][b + 1:]
        msgs = [heads[t] + h + tails[t] for t, h in zip(tpl, holes)]
    vks = [keys[j] for j in key_idx]
    items = list(zip(vks, sigs, msgs))
    code, check8 = o.batch_verify_seeded(items, Z_SEED)
    return {
        "name": name,
        "heads": [h.hex() for h in heads], "tails": [t.hex() for t in tails],
        "tpl": tpl, "holes": [h.hex() for h in holes],
        "keys": [k.hex() for k in keys], "key_idx": key_idx, "sigs": [s.hex() for s in sigs],
        "k": [o.challenge(s[:32], vk, m).to_bytes(32, "little").hex() for vk, s, m in items],
        "batch_code": code, "check8": check8.hex() if check8 is not None else None,
        "single": [o.verify(vk, s, m) for vk, s, m in items],
    }


def votes(flip=None):
    """32 votes of 120 bytes from 4 templates (a length-prefix variant, a nil vote with an empty
    tail) with a 12-byte hole, as a canonical vote's timestamp."""
    heads = [stream("vote-head%d" % t, n) for t, n in enumerate([70, 71, 70, 108])]
    tails = [stream("vote-tail%d" % t, n) for t, n in enumerate([38, 37, 38, 0])]
    tpl = [(0 if i % 8 else 1 + (i // 8) % 3) for i in range(32)]
    holes = [stream("vote-hole%d" % i, 12) for i in range(32)]
    return finish("votes" if flip is None else "votes_flipped", heads, tails, tpl, holes, flip)


def lengths():
    """Every total in TOTALS by several splits: all hole, all head, all tail, head + tail with an
    empty hole, and heads / tails of 15, 16 and 17 bytes around a hole (empty when they add up)."""
    shapes = [(0, 0)]
    for L in TOTALS:
        shapes += [(L, 0), (0, L), (L // 2, L - L // 2)]
    shapes += [(15, 0), (16, 0), (17, 0), (0, 15), (0, 16), (0, 17), (15, 17), (16, 16), (17, 15)]
    shapes = list(dict.fromkeys(shapes))
    heads = [stream("len-head%d" % t, hl) for t, (hl, tl) in enumerate(shapes)]
    tails = [stream("len-tail%d" % t, tl) for t, (hl, tl) in enumerate(shapes)]
    tpl, holes = [], []
    for L in TOTALS:
        for t, (hl, tl) in enumerate(shapes):
            if hl + tl == L or (hl + tl < L and (hl, tl) in shapes[-9:]) or (hl, tl) == (0, 0):
                tpl.append(t)
                holes.append(stream("len-hole%d-%d" % (L, t), L - hl - tl))
    return finish("lengths", heads, tails, tpl, holes)


def main():
    cases = [votes(), votes(flip=(10, 5)), lengths()]
    out = {"z_seed": Z_SEED.hex(), "cases": cases}
    with open(os.path.join(HERE, "templates.json"), "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    print("wrote templates.json:", {c["name"]: len(c["tpl"]) for c in cases})


if __name__ == "__main__":
    main()
