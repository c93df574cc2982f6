"""Mixed-order keys: A = [a]B + T with T in the 8-torsion, under signatures with s != 0. A plain
helper (no fixtures): tests/golden/gen_mixed_order.py writes tests/golden/mixed_order.json from it,
tests/test_mixed_order_vectors.py checks that file on the CPU, tests/test_gpu_mixed_order.py feeds
it to the kernels.

Construction. With A = [a]B + T_t, R = [r]B + T_u, any k and s = (r + k a) mod l,
[s]B - [k]A - R = -(k T_t + T_u): a torsion point, zero only when k T_t cancels T_u. The cofactored
equation [8]([s]B - [k]A - R) = 0 of ZIP215 holds for every (t, u, k); the cofactorless one holds for
the k mod 8 that cancel and no others. A defect s <- s + delta moves the item's term by [delta]B, so a
batch with weights z has check = [-sum z_i delta_i]B + torsion and [8]check = [8 (-sum z_i delta_i)]B:
integers alone. Everything here is Python integers and oracle/ed25519_ref.py; nothing comes from the
code under test."""
import hashlib

import scalar_edges as se

o = se.o
L = o.L
SEED = hashlib.sha512(b"mixed-order/z-seed").digest()[:32]
NSECRETS = 3
TORSION = [o.decompress(e) for e in o.eight_torsion_encodings()]       # [i]T: orders 1 8 4 8 2 8 4 8
TORSION_ORDER = [1, 8, 4, 8, 2, 8, 4, 8]
# (t, u) of the prehashed items: T_t of order 2 (t = 4), 4 (t = 2, 6), 8 (t = 1, 3, 5, 7) and the
# honest control (t = 0), against R with and without torsion
PRE_PAIRS = [(4, 0), (4, 4), (4, 1), (2, 0), (2, 6), (6, 3), (1, 0), (1, 7), (3, 5), (5, 2), (7, 4), (0, 5)]
FIXED_K = [8, L - 1, L - 8]


def _h(label, i):
    return int.from_bytes(hashlib.sha512(b"mixed-order/%s/%d" % (label.encode(), i)).digest(), "little")


def secret(j):
    return _h("key", j) % (L - 1) + 1


_KEYS = {}


def key(j, t):
    """(a_j, compress([a_j]B + T_t)); the key's position in the fixture is 8 j + t."""
    if (j, t) not in _KEYS:
        _KEYS[j, t] = (secret(j), o.compress(o.add(se.base_mul(secret(j)), TORSION[t])))
    return _KEYS[j, t]


def keys():
    return [key(j, t)[1] for j in range(NSECRETS) for t in range(8)]


def _R(r, u):
    return o.compress(o.add(se.base_mul(r), TORSION[u]))


def message_items():
    """[(key position, sig, msg)]: all 64 (t, u), item 8 t + u, the secrets in rotation, messages
    of 0..126 bytes."""
    out = []
    for i in range(64):
        t, u, j = i // 8, i % 8, i % NSECRETS
        a, A = key(j, t)
        msg = hashlib.sha512(b"mixed-order/msg/%d" % i).digest() * 2
        msg = msg[:(i * 2) % 127]
        r = _h("r-msg", i) % L
        R = _R(r, u)
        k = o.challenge(R, A, msg)
        out.append((8 * j + t, R + se.sc((r + k * a) % L), msg))
    return out


def pair_ks(pi):
    """The k of a prehashed pair: one large k of every residue mod 8, then 8, l - 1, l - 8."""
    return [8 * (_h("k/%d" % pi, res) % ((L - 8) // 8)) + res for res in range(8)] + FIXED_K


def prehashed_items():
    """[(key position, sig, k)]: len(pair_ks) items per pair of PRE_PAIRS, pair after pair."""
    out = []
    for pi, (t, u) in enumerate(PRE_PAIRS):
        j = pi % NSECRETS
        a, _ = key(j, t)
        for ki, k in enumerate(pair_ks(pi)):
            r = _h("r-pre/%d" % pi, ki) % L
            out.append((8 * j + t, _R(r, u) + se.sc((r + k * a) % L), se.sc(k)))
    return out


# name -> (form, [(position, delta)]): every batch is the whole item list of its form in order
BATCHES = {
    "msg_valid": ("msg", []),
    "msg_defect": ("msg", [(5, 1), (42, L - 1)]),                       # (t, u) = (0, 5) and (5, 2)
    "pre_valid": ("pre", []),
    "pre_one_defect": ("pre", [(83, 8)]),                               # pair (1, 7), k = 6 mod 8
    "pre_defects": ("pre", [(2, 1), (37, L - 8), (64, (1 << 128) + 1), (131, 1 << 252)]),
}


def with_defects(items, defects):
    """The items (any third column) with s <- s + delta mod l at the defects' positions."""
    out = list(items)
    for pos, delta in defects:
        a, sig, c = out[pos]
        s = (int.from_bytes(sig[32:], "little") + delta) % L
        out[pos] = (a, sig[:32] + se.sc(s), c)
    return out


def defect_check8(z, defects):
    """compress([8 (-sum z_i delta_i) mod l]B): the torsion of A and R drops out under the cofactor."""
    c = -sum(z[pos] * delta for pos, delta in defects) % L
    return o.compress(se.base_mul(8 * c % L))


def expected(n, defects):
    """(per-item codes, batch code, check8) of a batch of n constructed items with these defects."""
    bad = {pos for pos, _ in defects}
    z = o.z_values(SEED, n)
    return [int(i in bad) for i in range(n)], int(bool(defects)), defect_check8(z, defects)


# ---------------------------------------------------------------- reading the fixture
def fixture_items(fx, form):
    """[(vk, sig, msg or k)] of the stored message ("msg") or prehashed ("pre") items."""
    ks = [bytes.fromhex(k) for k in fx["keys"]]
    return [(ks[j], bytes.fromhex(sig), bytes.fromhex(c)) for j, sig, c in fx[form + "_items"]]


def fixture_batch(fx, name):
    """(form, items with the defects applied, codes, (code, check8)) of a stored batch."""
    b = fx["batches"][name]
    defects = [(pos, int.from_bytes(bytes.fromhex(d), "little")) for pos, d in b["defects"]]
    items = with_defects(fixture_items(fx, b["form"]), defects)
    return b["form"], items, b["codes"], (b["code"], bytes.fromhex(b["check8"]))
