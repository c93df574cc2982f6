"""Model of the header hashes (include/edc.h, "Header hashes"): hashlib only. The RECURSIVE RFC 6962
root over leaves of any length, the byte rule, the four rules of edc_header_bind, and a seeded
generator of CometBFT-shaped headers (14 leaves) that carry validator-set roots and link to each
other. The validator-set roots come from tests/valhash_model.py.

Run as a script, it writes tests/golden/header.json: a few dozen headers over a small history, with
their roots and the outcome of every rule, some of them broken on purpose, so that a change of the
model itself shows up in review."""
import hashlib
import json
import os
import random

import valhash_model as vm

NONE = 0xFFFFFFFF
MAX_LEAVES = 64
BAD_HASH, BAD_VALS, BAD_NEXT, BAD_LINK = 1, 2, 4, 8
# the leaf lengths on both sides of every SHA-256 block boundary of 00 | leaf, and a long one
LENGTHS = [0, 1, 3, 54, 55, 56, 63, 64, 65, 118, 119, 120, 127, 128, 182, 183, 300]


def sha256(b):
    return hashlib.sha256(bytes(b)).digest()


def mth(leaves):
    """RFC 6962 section 2.1, by its recursive definition"""
    n = len(leaves)
    if n == 0:
        return sha256(b"")
    if n == 1:
        return sha256(b"\x00" + leaves[0])
    k = 1
    while k * 2 < n:
        k *= 2
    return sha256(b"\x01" + mth(leaves[:k]) + mth(leaves[k:]))


def rule(leaves, L, P, src):
    """does the byte rule (leaf L, position P, source src) hold for a header?"""
    return L < len(leaves) and len(leaves[L]) >= P + 32 and leaves[L][P:P + 32] == src


def bind(headers, expect=None, vals=None, nexts=None, link=None, set_roots=None, vals_at=(7, 2), next_at=(8, 2),
         link_at=(4, 2)):
    """-> (bad, n_bad, roots) as edc_header_bind defines them; set_roots[v] = the root of version v"""
    roots = [mth(h) for h in headers]
    skip = lambda x: x is None or x == NONE
    bad = []
    for i, h in enumerate(headers):
        f = 0
        if expect is not None and expect[i] != roots[i]:
            f |= BAD_HASH
        if vals is not None and not skip(vals[i]) and not rule(h, vals_at[0], vals_at[1], set_roots[vals[i]]):
            f |= BAD_VALS
        if nexts is not None and not skip(nexts[i]) and not rule(h, next_at[0], next_at[1], set_roots[nexts[i]]):
            f |= BAD_NEXT
        if link is not None and not skip(link[i]) and not rule(h, link_at[0], link_at[1], roots[link[i]]):
            f |= BAD_LINK
        bad.append(f)
    return bad, sum(1 for f in bad if f), roots


def blob(b):
    return b"\x0a" + bytes([len(b)]) + bytes(b) if b else b""


def shaped(rnd, height, last_hash, vals_root, next_root):
    """one CometBFT-shaped header: 14 leaves, the hashes at position 2 of the leaves 4, 7 and 8"""
    r32 = lambda: bytes(rnd.randrange(256) for _ in range(32))
    return [
        b"\x08\x0b",
        blob(b"model-chain"),
        b"\x08" + vm.uvarint(height) if height else b"",
        b"\x08" + vm.uvarint(1700000000 + height) + b"\x10" + vm.uvarint(rnd.randrange(1, 10 ** 9)),
        blob(last_hash) + b"\x12\x24\x08\x01\x12\x20" + r32(),
        blob(r32()), blob(r32()), blob(vals_root), blob(next_root), blob(r32()),
        blob(bytes(rnd.randrange(256) for _ in range(rnd.choice([0, 8, 32])))), blob(r32()), blob(r32()),
        blob(bytes(rnd.randrange(256) for _ in range(20))),
    ]


def chain(rnd, n, set_roots=None, first_height=1):
    """n shaped headers, header i carrying the root of header i - 1 and the set roots of the versions
    i % nv and (i + 1) % nv -> (headers, vals, nexts, link); link[0] is None"""
    nv = len(set_roots) if set_roots else 0
    pick = lambda v: set_roots[v] if nv else bytes(rnd.randrange(256) for _ in range(32))
    headers, last = [], bytes(rnd.randrange(256) for _ in range(32))
    for i in range(n):
        headers.append(shaped(rnd, first_height + i, last, pick(i % nv if nv else 0), pick((i + 1) % nv if nv else 0)))
        last = mth(headers[-1])
    vals = [i % nv for i in range(n)] if nv else None
    nexts = [(i + 1) % nv for i in range(n)] if nv else None
    return headers, vals, nexts, [None] + list(range(n - 1))


def random_leaves(rnd, count, lengths=LENGTHS):
    return [bytes(rnd.randrange(256) for _ in range(rnd.choice(lengths))) for _ in range(count)]


def flip(b, i, bit=0x01):
    return b[:i] + bytes([b[i] ^ bit]) + b[i + 1:]


def golden():
    rnd = random.Random("header golden")
    keys = vm.make_keys(5, b"header")
    N = vm.NOT_MEMBER
    base = [10, 20, N, 5, 0]
    updates = [[(2, 7)], [(0, N), (4, 3)], [(1, 21)]]
    set_roots = vm.history_roots(keys, base, updates)
    headers, vals, nexts, link = chain(rnd, 24, set_roots)
    # headers that are no CometBFT headers: other leaf counts, every rule skipped
    for count in (0, 1, 2, 3, 5, 9, 17):
        headers.append(random_leaves(rnd, count, [0, 1, 40, 55, 56, 120]))
        vals.append(None)
        nexts.append(None)
        link.append(None)
    # broken on purpose: a wrong validators_hash, a wrong next one, a link to the wrong header, a
    # header linked to itself, a short leaf 7
    headers[3][7] = flip(headers[3][7], 2)
    headers[9][8] = flip(headers[9][8], 33, 0x80)
    link[12] = 10
    link[15] = 15
    headers[20][7] = headers[20][7][:33]
    expect = [mth(h) for h in headers]
    expect[6] = flip(expect[6], 31)
    bad, n_bad, roots = bind(headers, expect, vals, nexts, link, set_roots)
    return {
        "keys": [k.hex() for k in keys], "base": base, "updates": [[list(pw) for pw in u] for u in updates],
        "headers": [[x.hex() for x in h] for h in headers], "expect": [e.hex() for e in expect],
        "vals": vals, "nexts": nexts, "link": link, "roots": [r.hex() for r in roots], "bad": bad, "n_bad": n_bad,
    }


if __name__ == "__main__":
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "header.json")
    with open(path, "w") as f:
        json.dump(golden(), f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", path)
