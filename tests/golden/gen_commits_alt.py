"""Generate tests/golden/commits_alt.json from the CPU oracle (oracle/ed25519_ref.py).
Run: python tests/golden/gen_commits_alt.py        (a few minutes: the oracle is pure Python)

Templated commit sets with per-item template variants (include/edc.h, edc_tmpl_commits_*_alt and
edc_tmpl_commits_*_device): every commit owns the window [commit_tpl[c], commit_tpl[c] + ALT_SPAN)
of the template set and item i takes template commit_tpl[c] + item_alt[i].

The set of 8 is two heights x {block, nil} x {short, long length prefix}: template 4 h + a with
a = 0 block/short, 1 block/long, 2 nil/short, 3 nil/long. The sign bytes start with their own
length, so a non-empty head's first byte is (message length - 1) and a template fixes its hole's
length: HOLE_OF_ALT = 12, 13, 11, 0 bytes. Template 3 has an empty head, template 6 an empty tail.

The items are laid down by RULE (layout() / build() below, which need no oracle and are imported by
the tests), so the file stays small. It holds, per set, the layout and SHA-256 of the variant bytes,
of the per-item template array and of the materialised messages; for the sets that carry
signatures (SIGNED) also
  sig_sha256        SHA-256 over the oracle's signatures of the rule's items (Ed25519 signing is
                    deterministic: a test that signs again must arrive at these bytes)
  overrides         the corrupted items, in full
  item_codes        Item::verify_single's code (the oracle's verify) of every item that is not Ok;
                    every single item was verified by the oracle
  commit_verdicts   1 iff one of the commit's items has a non-zero code, and for `mixed` also
                    checked against Verifier::verify of every commit ALONE (the oracle's batch
                    equation with the fixed z seed)
DATA only.
"""
import hashlib
import json
import os
import struct
import sys

HERE = os.path.dirname(os.path.abspath(__file__))

Z_SEED = bytes([0x41]) * 32
NKEYS = 150
ALT_SPAN = 4
HOLE_OF_ALT = [12, 13, 11, 0]
HEAD_LENS = [70, 70, 46, 0, 71, 71, 47, 38]
TAIL_LENS = [38, 38, 30, 50, 37, 37, 0, 12]
L_ORDER = 2**252 + 27742317777372353535851937790883648493
MAP_ITEMS = 2048                    # items per workgroup of the map kernel

# total n -> items per commit. Boundaries inside a lane's 8 items (3, 5, 2045, 1001) and on
# workgroup boundaries (2048, 4096); empty commits first, last, in between and next to a boundary.
EDGE = {
    1: [0, 1, 0],
    7: [3, 0, 4],
    8: [5, 3],
    9: [4, 0, 0, 5],
    2047: [2040, 7],
    2048: [1001, 0, 1047],
    2049: [2048, 1],
    4100: [0, 2045, 3, 0, 2048, 4, 0],
}
SETS = ["small", "mixed"] + ["edge%d" % n for n in EDGE]
SIGNED = ["mixed", "edge4100"]


def stream(label, n):
    out, c = b"", 0
    while len(out) < n:
        out += hashlib.sha512(b"commits_alt/" + label.encode() + c.to_bytes(4, "little")).digest()
        c += 1
    return out[:n]


def key_seeds():
    return [stream("key%d" % j, 32) for j in range(NKEYS)]


def templates():
    heads, tails = [], []
    for t, (hl, tl) in enumerate(zip(HEAD_LENS, TAIL_LENS)):
        total = hl + HOLE_OF_ALT[t % ALT_SPAN] + tl
        h = stream("head%d" % t, hl)
        heads.append(bytes([(total - 1) & 0xFF]) + h[1:] if hl else b"")
        tails.append(stream("tail%d" % t, tl))
    return heads, tails


def layout(name):
    """Items per commit."""
    if name == "small":             # commits far smaller than a lane's 8 items; empty first, last and in runs
        sizes = [x % 6 for x in stream("small/sizes", 600)]
        for c in [0, 1, 2, 100, 101, 102, 103, 300, 301, 598, 599]:
            sizes[c] = 0
        return sizes
    if name == "mixed":
        sizes = [x % 13 for x in stream("mixed/sizes", 40)]
        sizes[0] = sizes[20] = sizes[39] = 0
        return sizes
    if name.startswith("edge"):
        return list(EDGE[int(name[4:])])
    raise KeyError(name)


def build(name, messages=True):
    """The rule's items of a set, without signatures: commit_off, commit_tpl, per item its variant,
    template, validator, hole and message (holes and messages only when asked for)."""
    sizes = layout(name)
    heads, tails = templates()
    off = [0]
    for s in sizes:
        off.append(off[-1] + s)
    n = off[-1]
    commit_tpl = [ALT_SPAN * (c % 2) for c in range(len(sizes))]
    alt = [0 if x < 160 else 1 if x < 208 else 2 if x < 240 else 3 for x in stream(name + "/alt", n)]
    tpl, validator, holes, msgs = [], [], [], []
    for c, s in enumerate(sizes):
        for j in range(s):
            i = off[c] + j
            tpl.append(commit_tpl[c] + alt[i])
            validator.append(j % NKEYS)
            if messages:
                holes.append(stream("%s/hole%d" % (name, i), HOLE_OF_ALT[alt[i]]))
                msgs.append(heads[tpl[i]] + holes[i] + tails[tpl[i]])
    return {"sizes": sizes, "commit_off": off, "commit_tpl": commit_tpl, "alt": alt, "tpl": tpl,
            "validator": validator, "holes": holes, "msgs": msgs}


def digests(b):
    d = {"alt_sha256": hashlib.sha256(bytes(b["alt"])).hexdigest(),
         "tpl_sha256": hashlib.sha256(struct.pack("<%dH" % len(b["tpl"]), *b["tpl"])).hexdigest()}
    if b["msgs"] or not b["tpl"]:
        d["msg_sha256"] = hashlib.sha256(b"".join(b["msgs"])).hexdigest()
    return d


def bad_items(name, b):
    """The items `overrides` corrupts: (first item of a commit, last item of a commit, the item that
    gets an undecodable key, the item that gets s = l)."""
    if name != "mixed":
        return None
    off = b["commit_off"]
    full = [c for c, s in enumerate(b["sizes"]) if s >= 3]
    return off[full[1]], off[full[4] + 1] - 1, off[full[7]] + 1, off[full[10]]


def overrides(name, b, vks, sigs):
    """The corrupted items of a set: [(item, vk, sig)]."""
    def flip(i, byte, bit):
        return (i, vks[i], sigs[i][:byte] + bytes([sigs[i][byte] ^ bit]) + sigs[i][byte + 1:])
    if name != "mixed":
        return []
    first, last, key, sl = bad_items(name, b)
    with open(os.path.join(HERE, "decode.json")) as f:
        not_a_point = bytes.fromhex([c for c in json.load(f)["cases"] if not c["ok"]][0]["enc"])
    return [flip(first, 33, 1), flip(last, 40, 0x10), (key, not_a_point, sigs[key]),
            (sl, vks[sl], sigs[sl][:32] + L_ORDER.to_bytes(32, "little"))]


def main():
    sys.path.insert(0, os.path.join(HERE, "..", "..", "oracle"))
    import ed25519_ref as o

    seeds = key_seeds()
    keys = [o.public_key(s) for s in seeds]
    out = {"z_seed": Z_SEED.hex(), "nkeys": NKEYS, "alt_span": ALT_SPAN, "sets": {}}
    for name in SETS:
        b = build(name, messages=name in SIGNED)
        s = {"sizes": b["sizes"], "n": len(b["tpl"])}
        s.update(digests(b))
        if name in SIGNED:
            vks = [keys[j] for j in b["validator"]]
            sigs = [o.sign(seeds[j], m) for j, m in zip(b["validator"], b["msgs"])]
            s["sig_sha256"] = hashlib.sha256(b"".join(sigs)).hexdigest()
            ov = overrides(name, b, vks, sigs)
            for i, vk, sig in ov:
                vks[i], sigs[i] = vk, sig
            items = list(zip(vks, sigs, b["msgs"]))
            codes = [o.verify(*it) for it in items]
            spans = list(zip(b["commit_off"], b["commit_off"][1:]))
            verdicts = [1 if any(codes[a:e]) else 0 for a, e in spans]
            if name == "mixed":
                assert verdicts == [o.batch_verify_seeded(items[a:e], Z_SEED)[0] for a, e in spans]
            s.update({"overrides": [{"item": i, "vk": vk.hex(), "sig": sig.hex()} for i, vk, sig in ov],
                      "item_codes": {str(i): c for i, c in enumerate(codes) if c},
                      "commit_verdicts": verdicts, "n_bad_commits": sum(verdicts)})
        out["sets"][name] = s
        print(name, "n =", s["n"], "commits =", len(b["sizes"]), "bad items =", s.get("item_codes"), flush=True)
    with open(os.path.join(HERE, "commits_alt.json"), "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
