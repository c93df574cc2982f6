"""Generate tests/golden/commits.json from the CPU oracle (oracle/ed25519_ref.py).
Run: python tests/golden/gen_commits.py        (a few minutes: the oracle is pure Python)

Commit sets (include/edc.h, edc_commits_*): n items in queue order cut into commits by nc + 1
offsets, verified as nc independent batch::Verifier's (reference src/batch.rs:110-217). Every item
is a vote of 120 bytes, heads[t] + hole + tails[t] with the 12-byte hole of a canonical vote's
timestamp and t the template of the item's commit, signed by validator (position in its commit)
mod 150.

The items are laid down by RULE (layout() / build() below, which need no oracle and are imported
by tests/test_gpu_commits.py), so the file stays small: it holds the layout, the items that are
not what the rule gives (corrupted ones, in full), and what the oracle says about the result:
  sig_sha256        SHA-256 over the oracle's signatures of the rule's items (Ed25519 signing is
                    deterministic: a test that signs again must arrive at these bytes)
  k_sha256          SHA-256 over k = H(R || A || M) mod l of every final item
  item_codes        Item::verify_single's code of every item that is not Ok (all others are Ok:
                    every single item was verified by the oracle)
  commit_verdicts   Verifier::verify of every commit ALONE (the oracle's batch equation with the
                    fixed z seed), empty commits included
The ZIP215 commit holds the 196 (vk, sig) pairs of zip215_small_order.json: A and R of small order
and s = 0 verify for every message, here the commit's templated votes; the oracle checked each.
DATA only.
"""
import hashlib
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))

Z_SEED = bytes([0x36]) * 32
NKEYS = 150
HEAD_LENS, TAIL_LENS, HOLE = [70, 71, 70, 108], [38, 37, 38, 0], 12
L_ORDER = 2**252 + 27742317777372353535851937790883648493


def stream(label, n):
    out, c = b"", 0
    while len(out) < n:
        out += hashlib.sha512(b"commits/" + label.encode() + c.to_bytes(4, "little")).digest()
        c += 1
    return out[:n]


def key_seeds():
    return [stream("key%d" % j, 32) for j in range(NKEYS)]


def templates():
    return ([stream("head%d" % t, n) for t, n in enumerate(HEAD_LENS)],
            [stream("tail%d" % t, n) for t, n in enumerate(TAIL_LENS)])


def layout(name):
    """{"data": label of the holes, "sizes": items per commit, "corpus_commit": index or None}."""
    if name == "valid":             # 2049 crosses the coefficient kernel's chunk of 2048
        return {"data": "valid", "sizes": [0, 1, 150, 7, 2049, 0], "corpus_commit": None}
    if name in ("mixed_a", "mixed_b"):
        # 4310 items: the fallback cuts them at items 2048 and 4096; the 20-item commit is items
        # 2040..2059 between a 44-item commit and a full one
        sizes = [0, 150, 196, 0, 150, 150, 150, 150] + [150] * 7 + [44, 20] + [150] * 15 + [0]
        return {"data": "mixed", "sizes": sizes, "corpus_commit": 2}
    if name == "tmap_small":        # commits far smaller than a workgroup's 256 items
        rnd = random.Random(600)
        sizes = [rnd.randrange(6) for _ in range(600)]
        sizes[0] = sizes[-1] = 0
        return {"data": "tmap_small", "sizes": sizes, "corpus_commit": None}
    if name == "tmap_big":          # one commit over many workgroups
        return {"data": "tmap_big", "sizes": [3000], "corpus_commit": None}
    raise KeyError(name)


SETS = ["valid", "mixed_a", "mixed_b", "tmap_small", "tmap_big"]


def build(name):
    """The rule's items of a set, without signatures: commit_off, commit_tpl, per item its
    validator (None inside the ZIP215 commit), template, hole and message."""
    lay = layout(name)
    heads, tails = templates()
    off = [0]
    for s in lay["sizes"]:
        off.append(off[-1] + s)
    commit_tpl = [c % 4 for c in range(len(lay["sizes"]))]
    validator, tpl, holes, msgs = [], [], [], []
    for c, s in enumerate(lay["sizes"]):
        for j in range(s):
            i = off[c] + j
            validator.append(None if c == lay["corpus_commit"] else j % NKEYS)
            tpl.append(commit_tpl[c])
            holes.append(stream("%s/hole%d" % (lay["data"], i), HOLE))
            msgs.append(heads[commit_tpl[c]] + holes[-1] + tails[commit_tpl[c]])
    return {"commit_off": off, "commit_tpl": commit_tpl, "validator": validator, "tpl": tpl, "holes": holes,
            "msgs": msgs, "corpus_commit": lay["corpus_commit"]}


def corpus():
    with open(os.path.join(HERE, "zip215_small_order.json")) as f:
        return [(bytes.fromhex(c["vk"]), bytes.fromhex(c["sig"])) for c in json.load(f)["cases"]]


def overrides(name, vks, sigs):
    """The corrupted items of a set: [(item, vk, sig)]."""
    def flip(i, byte, bit):
        return (i, vks[i], sigs[i][:byte] + bytes([sigs[i][byte] ^ bit]) + sigs[i][byte + 1:])
    if name not in ("mixed_a", "mixed_b"):
        return []
    with open(os.path.join(HERE, "decode.json")) as f:
        not_a_point = bytes.fromhex([c for c in json.load(f)["cases"] if not c["ok"]][0]["enc"])
    return [flip(346, 33, 1),                                               # first item of its commit
            flip(645, 40, 0x10),                                            # last item of its commit
            (700, not_a_point, sigs[700]),                                  # undecodable key
            (800, vks[800], sigs[800][:32] + L_ORDER.to_bytes(32, "little")),  # s = l
            flip(2047 if name == "mixed_a" else 2048, 5, 4)]                # either side of item 2048


def main():
    sys.path.insert(0, os.path.join(HERE, "..", "..", "oracle"))
    import ed25519_ref as o

    seeds = key_seeds()
    keys = [o.public_key(s) for s in seeds]
    signed, single, alone = {}, {}, {}

    def sign(j, m):
        if (j, m) not in signed:
            signed[(j, m)] = o.sign(seeds[j], m)
        return signed[(j, m)]

    def verify(item):
        if item not in single:
            single[item] = o.verify(*item)
        return single[item]

    def commit_alone(items):
        key = hashlib.sha256(b"".join(a + b + c for a, b, c in items)).digest()
        if key not in alone:
            alone[key] = o.batch_verify_seeded(items, Z_SEED)[0]
        return alone[key]

    out = {"z_seed": Z_SEED.hex(), "nkeys": NKEYS, "sets": {}}
    for name in SETS:
        b = build(name)
        n = len(b["msgs"])
        vks = [keys[j] if j is not None else None for j in b["validator"]]
        sigs = [sign(j, m) if j is not None else None for j, m in zip(b["validator"], b["msgs"])]
        if b["corpus_commit"] is not None:
            i0 = b["commit_off"][b["corpus_commit"]]
            for d, (vk, sig) in enumerate(corpus()):
                vks[i0 + d], sigs[i0 + d] = vk, sig
        sig_sha = hashlib.sha256(b"".join(sigs)).hexdigest()
        ov = overrides(name, vks, sigs)
        for i, vk, sig in ov:
            vks[i], sigs[i] = vk, sig
        items = list(zip(vks, sigs, b["msgs"]))
        codes = [verify(it) for it in items]
        verdicts = [commit_alone(items[a:e]) for a, e in zip(b["commit_off"], b["commit_off"][1:])]
        for c, (a, e) in enumerate(zip(b["commit_off"], b["commit_off"][1:])):
            assert verdicts[c] == (1 if any(codes[a:e]) else 0), (name, c)
        ks = b"".join(o.challenge(s[:32], vk, m).to_bytes(32, "little") for vk, s, m in items)
        out["sets"][name] = {
            "sizes": layout(name)["sizes"], "n": n,
            "overrides": [{"item": i, "vk": vk.hex(), "sig": sig.hex()} for i, vk, sig in ov],
            "sig_sha256": sig_sha, "k_sha256": hashlib.sha256(ks).hexdigest(),
            "item_codes": {str(i): c for i, c in enumerate(codes) if c},
            "commit_verdicts": verdicts, "n_bad_commits": sum(1 for v in verdicts if v),
        }
        print(name, "n =", n, "commits =", len(verdicts), "bad items =", out["sets"][name]["item_codes"], flush=True)
    with open(os.path.join(HERE, "commits.json"), "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
