"""Edge scalars for the device's integer scalar layer: the families, the construction of valid items
that carry them, and a census proving that the inputs reach the edges. A plain helper (no fixtures):
tests/golden/gen_scalar_edges.py writes tests/golden/scalar_edges.json from it,
tests/test_scalar_edge_vectors.py checks that file on the CPU, tests/test_gpu_scalar_edges.py feeds
it to the kernels.

Construction. With a secret integer a, A = [a]B, any canonical s and k and a small-order point T,
the item (vk = A, sig = compress([(s - k a) mod l]B + T) || s, k) verifies under ZIP215, so a test
chooses s and k freely. In a batch with weights z_i the coefficient of a key is sum z_i k_i mod l
and that of B is -sum z_i s_i mod l; l is prime, so the last k of a key and the last s of the batch
are solved to make them any target, and R is built last. Everything here is Python integers and
oracle/ed25519_ref.py; nothing comes from the code under test."""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import ed25519_ref as o  # noqa: E402

L = o.L
M128 = (1 << 128) - 1
PLAN_C = (8, 9, 12, 13, 16)
B_TARGETS = [0, 1, L - 1, 1 << 252, (1 << 252) - 1, 1 << 128, M128]
SEED = hashlib.sha512(b"scalar-edges/z-seed").digest()[:32]
NKEYS_PER_ITEM = 4          # the per-item lists rotate over the first keys
TORSION = [o.decompress(e) for i, e in enumerate(o.eight_torsion_encodings()) if i in (0, 1, 5)]


# ---------------------------------------------------------------- the recodings, restated (census only)
def plan_windows(c, hi, hi_windows=True):
    """make_plan's rule: ws = ceil(128 / c) balanced windows over bits 0..127 (the first 128 % ws one
    bit wider), then wh = ceil(125 / hi) balanced windows over bits 128..252. -> ([(off, bits)], ws)"""
    wins, off = [], 0
    for span, width in ((128, c),) + (((125, hi),) if hi_windows else ()):
        cnt = -(-span // width)
        for i in range(cnt):
            bits = span // cnt + (1 if i < span % cnt else 0)
            wins.append((off, bits))
            off += bits
    return wins, -(-128 // c)


def plan_digits(s, wins):
    """Signed digits with a carry into the next window; the last window keeps raw + carry (up to
    2^bits). -> (digits, carry into each window)"""
    digits, cins, carry = [], [], 0
    for i, (off, bits) in enumerate(wins):
        raw = ((s >> off) & ((1 << bits) - 1)) + carry
        cins.append(carry)
        if i + 1 < len(wins) and raw >= 1 << (bits - 1):
            digits.append(raw - (1 << bits))
            carry = 1
        else:
            digits.append(raw)
            carry = 0
    return digits, cins


def radix_digits(s, width, npos):
    """Signed radix-2^width digits in [-(2^(width-1) - 1), 2^(width-1)], no carry out of the top
    position (radix16: width 4, 64 positions; radix256: width 8, 32). -> (digits, carry outs)"""
    digits, couts, carry = [], [], 0
    for j in range(npos):
        v = ((s >> (width * j)) & ((1 << width) - 1)) + carry
        carry = 1 if j + 1 < npos and v > 1 << (width - 1) else 0
        digits.append(v - (carry << width))
        couts.append(carry)
    return digits, couts


def longest_run(bits):
    best = cur = 0
    for b in bits:
        cur = cur + 1 if b else 0
        best = max(best, cur)
    return best


# ---------------------------------------------------------------- families
def _fit(v):
    """Below l with the pattern kept: bits from 252 up are cleared, never a reduction mod l."""
    v &= (1 << 256) - 1
    return v if v < L else v & ((1 << 252) - 1)


def _rep(byte, n=32):
    return int.from_bytes(bytes([byte]) * n, "little")


def _plans():
    return [(c, hi) for c in PLAN_C for hi in dict.fromkeys((8, c))]


FIXED = [0, 1, 2, 8, L - 1, L - 2, (L - 1) // 2, (L + 1) // 2, 1 << 252, (1 << 252) + 1, (1 << 252) - 1,
         1 << 128, (1 << 128) + 1, (1 << 128) - 1, 1 << 127]


def full_scalars():
    """The full-width family: distinct scalars < l, in a fixed order."""
    out = list(FIXED)
    offs = sorted({off for c, hi in _plans() for off, _ in plan_windows(c, hi)[0]})
    for off in offs:
        out += [1 << off, (1 << off) - 1]
        if off:
            out.append((1 << (off - 1)) + (1 << off) - 1)
    for c, hi in _plans():
        wins = plan_windows(c, hi)[0]
        out.append(sum(1 << (off + w - 1) for off, w in wins))                   # every window 2^(w-1)
        out.append(sum(((1 << (w - 1)) - 1) << off for off, w in wins))          # every window 2^(w-1) - 1
        out.append((1 << 253) - 1)                                               # every window all ones
    out += [_rep(0x88), _rep(0x77), _rep(0x99), _rep(0x88) + 1]                  # nibble runs, 88..89
    out += [_rep(0x80), _rep(0x7F), _rep(0x81), _rep(0x80) + 1]                  # byte runs, 80..80 81
    for start in (0, 15):
        for n in (1, 2, 4, 8, 16, 31):
            out.append(((1 << (8 * n)) - 1) << (8 * start))
    out += [0x0F << 248, (0x10 << 248) | ((1 << 124) - 1)]                       # top byte 0x0f, 0x10
    return list(dict.fromkeys(_fit(v) for v in out))


def z_scalars():
    """The 128-bit family."""
    out = [0, 1, M128, 1 << 127, (1 << 127) - 1]
    out += [v & M128 for v in full_scalars()]
    for c in (8, 16):            # top window all ones and the bit below it: digit 2^c
        wins, ws = plan_windows(c, c)
        off, bits = wins[ws - 1]
        out.append((((1 << bits) - 1) << off) | (1 << (off - 1)))
    return list(dict.fromkeys(out))


def scramble(n, label):
    return sorted(range(n), key=lambda i: hashlib.sha512(b"scalar-edges/%s/%d" % (label.encode(), i)).digest())


# ---------------------------------------------------------------- construction
_POW2_B = [o.B_POINT]


def base_mul(k):
    """[k]B from the doublings of B (additions only)."""
    acc, i = o.IDENTITY, 0
    while k >> i:
        if len(_POW2_B) <= i:
            _POW2_B.append(o.double(_POW2_B[-1]))
        if (k >> i) & 1:
            acc = o.add(acc, _POW2_B[i])
        i += 1
    return acc


def secret(j):
    return int.from_bytes(hashlib.sha512(b"scalar-edges/key/%d" % j).digest(), "little") % (L - 1) + 1


_KEYS = {}


def key(j):
    """(a_j, compress([a_j]B))"""
    if j not in _KEYS:
        _KEYS[j] = (secret(j), o.compress(base_mul(secret(j))))
    return _KEYS[j]


def sc(v, n=32):
    return v.to_bytes(n, "little")


def make_item(j, s, k, t):
    """(key index, sig, k) that verifies: R = [(s - k a_j) mod l]B + TORSION[t]."""
    a, _ = key(j)
    R = o.add(base_mul((s - k * a) % L), TORSION[t % len(TORSION)])
    return (j, o.compress(R) + sc(s), sc(k))


def shift_R(sig, delta=1):
    """The signature with R replaced by R + [delta]B."""
    return o.compress(o.add(o.decompress(sig[:32]), base_mul(delta))) + sig[32:]


NEAR_KINDS = ("s+1", "s-1", "k+1", "k-1", "R+B")


def near_miss(item, kind):
    """An invalid neighbour of a valid item. s + 1 is left unreduced (l - 1 -> l, a non-canonical s);
    the others wrap mod l so that k stays a canonical scalar."""
    j, sig, k = item
    s, kk = int.from_bytes(sig[32:], "little"), int.from_bytes(k, "little")
    if kind == "s+1":
        return (j, sig[:32] + sc(s + 1), k)
    if kind == "s-1":
        return (j, sig[:32] + sc((s - 1) % L), k)
    if kind == "k+1":
        return (j, sig, sc((kk + 1) % L))
    if kind == "k-1":
        return (j, sig, sc((kk - 1) % L))
    assert kind == "R+B"
    return (j, shift_R(sig), k)


def per_item_pairs():
    """(s, k) of the per-item lists: the family against itself on a fixed scramble, then every fixed
    value against every fixed value."""
    fam = full_scalars()
    perm = scramble(len(fam), "pairs")
    return [(fam[i], fam[perm[i]]) for i in range(len(fam))] + [(s, k) for s in FIXED for k in FIXED]


def per_item_items():
    return [make_item(i % NKEYS_PER_ITEM, s, k, i) for i, (s, k) in enumerate(per_item_pairs())]


# ---------------------------------------------------------------- batches
def batch_layouts():
    """[(name, B target, key targets, items per key)]: one batch per B target, the full family spread
    over them as key-coefficient targets, some keys with several items (key 0 of the first batch:
    64 maximal items and its solver); last, a batch whose every coefficient is 0."""
    fam = full_scalars()
    nb = len(B_TARGETS)
    out = []
    for b, bt in enumerate(B_TARGETS):
        targets = fam[b::nb]
        sizes = [65 if b == 0 else 5, 4, 3, 3, 2, 2, 2, 2] + [1] * (len(targets) - 8)
        out.append(("b%d" % b, bt, targets, sizes))
    out.append(("all_zero", 0, [0] * 6, [4, 3, 2, 1, 1, 1]))
    return out


class _Cycle:
    def __init__(self, seq, at=0):
        self.seq, self.at = seq, at

    def next(self, nonzero=False):
        while True:
            v = self.seq[self.at % len(self.seq)]
            self.at += 1
            if v or not nonzero:
                return v


def solve(z, ks, ss, solver_of_key, targets, bt):
    """Set the k of every key's solver item and the s of the last item so that the key coefficients
    are `targets` and the B coefficient is `bt`. solver_of_key: (items of the key, its solver) per key."""
    ks, ss = list(ks), list(ss)
    for (members, last), c in zip(solver_of_key, targets):
        rest = sum(z[i] * ks[i] for i in members if i != last) % L
        ks[last] = (c - rest) * pow(z[last], L - 2, L) % L
    n = len(z)
    rest = sum(z[i] * ss[i] for i in range(n - 1)) % L
    ss[n - 1] = (-bt - rest) * pow(z[n - 1], L - 2, L) % L
    return ks, ss


def build_batches():
    """Every batch as a dict of Python values (see gen_scalar_edges.py for the stored form)."""
    fam, zfam = full_scalars(), z_scalars()
    zc = _Cycle(zfam)
    kc = _Cycle([fam[i] for i in scramble(len(fam), "batch-k")])
    scy = _Cycle([fam[i] for i in scramble(len(fam), "batch-s")])
    out = []
    for bi, (name, bt, targets, sizes) in enumerate(batch_layouts()):
        m = len(targets)
        key_of = []                                   # queue order: the other items key by key in rounds,
        for r in range(max(sizes) - 1):               # then one solver item per key
            key_of += [j for j in range(m) if r < sizes[j] - 1]
        nfree = len(key_of)
        key_of += list(range(m))
        n = len(key_of)
        maximal = name == "b0"
        z, ks, ss = [], [], []
        for i, j in enumerate(key_of):
            if i < nfree and maximal and j == 0:      # z = 2^128 - 1, k = s = l - 1
                z.append(M128), ks.append(L - 1), ss.append(L - 1)
            else:
                z.append(zc.next(nonzero=i >= nfree)), ks.append(kc.next()), ss.append(scy.next())
        groups = [([i for i in range(n) if key_of[i] == j], nfree + j) for j in range(m)]
        zs = o.z_values(SEED, n)
        variants = {}
        for tag, zz in (("z", z), ("seeded", zs)):
            k2, s2 = solve(zz, ks, ss, groups, targets, bt)
            items = [make_item(j, s2[i], k2[i], i + bi) for i, j in enumerate(key_of)]
            # the twin: one item's R moved by [delta]B -> check = [z delta]B + sum z_i T_i
            pos = next(i for i in range(n // 3, n) if zz[i] % L)
            delta = 1 + bi
            tors = o.IDENTITY
            for i in range(n):
                tors = o.add(tors, o.scalar_mul(zz[i] % 8, TORSION[(i + bi) % len(TORSION)]))
            variants[tag] = {"z": list(zz), "items": items, "twin_pos": pos,
                             "twin_sig": shift_R(items[pos][1], delta),
                             "valid_check": tors,
                             "twin_check": o.add(base_mul(zz[pos] * delta % L), tors)}
        zero = [i for i in range(nfree) if z[i] == 0]
        out.append({"name": name, "b_target": bt, "key_targets": list(targets), "nkeys": m, "nfree": nfree,
                    "zero_z_pos": zero[0] if zero else None, "variants": variants})
    return out


# ---------------------------------------------------------------- reading the fixture
def rows_items(fx, rows):
    """[(vk, sig, k)] of stored [key index, sig, k] rows."""
    return [(bytes.fromhex(fx["keys"][j]), bytes.fromhex(sig), bytes.fromhex(k)) for j, sig, k in rows]


def variant_items(fx, b, tag):
    """(items, z) of a stored batch for caller-drawn z ("z") or z from the fixture's seed ("seeded")."""
    items = rows_items(fx, b["z"]["items"])
    if tag == "z":
        return items, [int.from_bytes(bytes.fromhex(z), "little") for z in b["z"]["z"]]
    items = items[:b["nfree"]] + rows_items(fx, b["seeded"]["solvers"])
    return items, o.z_values(bytes.fromhex(fx["seed"]), len(items))


def twin_of(items, v):
    """The perturbed twin of a variant v = b["z"] or b["seeded"]: one R moved."""
    out = list(items)
    vk, _, k = out[v["twin_pos"]]
    out[v["twin_pos"]] = (vk, bytes.fromhex(v["twin_sig"]), k)
    return out


# ---------------------------------------------------------------- big-int evaluation (the expected values' check)
def affine(pt):
    zi = pow(pt[2], o.P - 2, o.P)
    return pt[0] * zi % o.P, pt[1] * zi % o.P


def batch_check(items, z):
    """The reference's batch equation over prehashed items [(vk, sig, k)] (oracle.batch_verify with
    the caller's k): the check point before the cofactor, or None when something does not decode."""
    groups = {}
    for (vk, sig, k), zi in zip(items, z):
        groups.setdefault(bytes(vk), []).append((int.from_bytes(k, "little"), bytes(sig), zi))
    b_coeff, scalars, points = 0, [], []
    for vk, sigs in groups.items():
        A = o.decompress(vk)
        if A is None:
            return None
        a_coeff = 0
        for k, sig, zi in sigs:
            R = o.decompress(sig[:32])
            s = o.scalar_from_canonical_bytes(sig[32:])
            if R is None or s is None:
                return None
            b_coeff = (b_coeff - zi * s) % L
            a_coeff = (a_coeff + zi * k) % L
            scalars.append(zi)
            points.append(R)
        scalars.append(a_coeff)
        points.append(A)
    scalars.append(b_coeff)
    points.append(o.B_POINT)
    return o.multiscalar_mul(scalars, points)


def coefficients(items, z):
    """({vk: key coefficient}, B coefficient) of a batch, as integers."""
    keys, b = {}, 0
    for (vk, sig, k), zi in zip(items, z):
        keys[vk] = (keys.get(vk, 0) + zi * int.from_bytes(k, "little")) % L
        b = (b - zi * int.from_bytes(sig[32:], "little")) % L
    return keys, b


# ---------------------------------------------------------------- census
def census(per_item, batches):
    """Which named edges the inputs reach. per_item: [(vk, sig, k)]; batches: [(items, z)] with the
    z the device will see. Guards the inputs only: never an expected value."""
    c = {}
    ks = [int.from_bytes(k, "little") for _, _, k in per_item]
    ss = [int.from_bytes(sig[32:], "little") for _, sig, _ in per_item]
    d16 = [radix_digits(k, 4, 64) for k in ks]
    d256 = [radix_digits(s, 8, 32) for s in ss]
    c["radix16_plus8"] = any(8 in d for d, _ in d16)
    c["radix16_minus7"] = any(-7 in d for d, _ in d16)
    c["radix16_in_range"] = all(-7 <= x <= 8 for d, _ in d16 for x in d)
    c["radix256_plus128"] = any(128 in d for d, _ in d256)
    c["radix256_minus127"] = any(-127 in d for d, _ in d256)
    c["radix256_in_range"] = all(-127 <= x <= 128 for d, _ in d256 for x in d)
    c["carry_chain_62_nibbles"] = max(longest_run(co) for _, co in d16) >= 62
    c["carry_chain_31_bytes"] = max(longest_run(co) for _, co in d256) >= 31
    zs = [zi for _, z in batches for zi in z]
    coefs = []
    for items, z in batches:
        keys, b = coefficients(items, z)
        coefs.append((set(keys.values()), b))
    for name, v in (("0", 0), ("l-1", L - 1), ("2^252", 1 << 252)):
        c["key_coefficient_" + name] = any(v in keys for keys, _ in coefs)
        c["b_coefficient_" + name] = any(v == b for _, b in coefs)
    full = [v for keys, b in coefs for v in list(keys) + [b]]
    for cc in PLAN_C:
        wins, ws = plan_windows(cc, cc)
        top_bits = wins[ws - 1][1]
        zd = [plan_digits(zi, wins[:ws]) for zi in zs]
        fd = [plan_digits(v, wins) for v in full]
        if cc in (8, 16):
            c["top_short_digit_2^%d" % cc] = top_bits == cc and any(d[-1] == 1 << cc for d, _ in zd)
        inner = [(x, bits) for d, _ in zd + fd for x, (_, bits) in list(zip(d, wins))[:len(d) - 1]]
        c["inner_digit_min_c%d" % cc] = any(x == -(1 << (bits - 1)) for x, bits in inner)
        c["inner_digit_max_c%d" % cc] = any(x == (1 << (bits - 1)) - 1 for x, bits in inner)
        c["carry_into_top_full_c%d" % cc] = any(ci[-1] for _, ci in fd)
        # split coefficients: both halves are short terms
        halves = [h for v in full for h in (v & M128, v >> 128)]
        c["split_top_digit_2^bits_c%d" % cc] = any(plan_digits(h, wins[:ws])[0][-1] == 1 << top_bits for h in halves)
    c["split_lo_zero"] = any(v and v & M128 == 0 for v in full)
    c["split_hi_zero"] = any(v and v >> 128 == 0 for v in full)
    c["split_lo_all_ones"] = any(v & M128 == M128 for v in full)
    c["every_full_scalar_a_key_coefficient"] = set(full_scalars()) <= set().union(*(keys for keys, _ in coefs))
    c["z_zero"] = 0 in zs
    c["every_z_placed"] = set(z_scalars()) <= set(zs)
    return c
