"""Model of the validator-set hashes (include/edc.h, "Validator-set hashes"): hashlib and Python
integers only. Address, order, leaf and uvarint, the RECURSIVE RFC 6962 root, and a small replayer
of a validator-set history (base plus updates -> members and powers at a version).

Run as a script, it writes tests/golden/valhash.json: roots of a few small sets, so that a change of
the model itself shows up in review."""
import hashlib
import json
import os

NOT_MEMBER = 0xFFFFFFFFFFFFFFFF
MAX_POWER = (1 << 63) - 1


def sha256(b):
    return hashlib.sha256(bytes(b)).digest()


def uvarint(x):
    assert 0 <= x < 1 << 64
    out = bytearray()
    while x >= 0x80:
        out.append((x & 0x7F) | 0x80)
        x >>= 7
    out.append(x)
    return bytes(out)


def address(key):
    assert len(key) == 32
    return sha256(key)[:20]


def leaf(key, power):
    assert len(key) == 32 and 0 <= power <= MAX_POWER
    return b"\x0a\x22\x0a\x20" + bytes(key) + (b"\x10" + uvarint(power) if power > 0 else b"")


def ordered(members):
    """members: (position, key, power) -> the same, power descending, address ascending, position ascending"""
    return sorted(members, key=lambda m: (-m[2], address(m[1]), m[0]))


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


def root(members):
    return mth([leaf(k, w) for _, k, w in ordered(members)])


def replay(base, updates):
    """base: one power (or NOT_MEMBER / None) per position; updates: per version 1..nv a list of
    (position, power) -> the powers by position at every version 0..nv"""
    cur = [NOT_MEMBER if w is None else w for w in base]
    states = [list(cur)]
    for upd in updates:
        for p, w in upd:
            cur[p] = NOT_MEMBER if w is None else w
        states.append(list(cur))
    return states


def members_at(keys, state):
    return [(p, keys[p], w) for p, w in enumerate(state) if w != NOT_MEMBER]


def history_roots(keys, base, updates):
    return [root(members_at(keys, s)) for s in replay(base, updates)]


def make_keys(n, tag=b"valhash"):
    """n distinct 32-byte strings (the hashes never decode a key, so any bytes serve)"""
    return [sha256(tag + i.to_bytes(4, "little")) for i in range(n)]


def golden():
    keys = make_keys(17)
    out = {"keys": [k.hex() for k in keys], "roots": {}, "uvarint": {}, "address0": address(keys[0]).hex()}
    for n in range(18):
        out["roots"][str(n)] = root([(p, keys[p], 10 + (p * 7) % 5) for p in range(n)]).hex()
    for x in (0, 1, 127, 128, (1 << 14) - 1, 1 << 14, MAX_POWER):
        out["uvarint"][str(x)] = uvarint(x).hex()
    return out


if __name__ == "__main__":
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "valhash.json")
    with open(path, "w") as f:
        json.dump(golden(), f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", path)
