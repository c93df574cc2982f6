"""Bucket-occupancy shapes for the Pippenger MSM (edc_msm.hip k_msm_sort / k_msm_accum_dma): batch
weights z chosen so that every bin of a plan holds what the test wants -- one bucket over all 256
lanes, two far-apart buckets with the boundary on a lane start, a Zipf tail, empty siblings, bins of
exactly 10240 entries -- the expected check point of such a batch, and a census proving from the plan
that the shape was reached. A plain helper (no fixtures): tests/test_bucket_shape_census.py checks it
on the CPU, tests/test_gpu_bucket_shapes.py feeds it to the kernels.

Expected value. For items that verify apart from defects s'_i = s_i + delta_i the batch equation
leaves check = [c]B with c = -sum z_i delta_i mod l, whatever the z. Everything here is Python
integers, hashlib and oracle/ed25519_ref.py; nothing comes from the code under test."""
import functools
import hashlib

import scalar_edges as se

o = se.o
L = se.L
M128 = se.M128
NKEYS = 8
NBASE = 512
MAX_BINS = 8192


# ---------------------------------------------------------------- base items
def key_seed(j):
    return hashlib.sha512(b"bucket-shapes/key/%d" % j).digest()[:32]


def message(i):
    """0..90 bytes."""
    out, need, ctr = b"", i % 91, 0
    while len(out) < need:
        out += hashlib.sha512(b"bucket-shapes/msg/%d/%d" % (i, ctr)).digest()
        ctr += 1
    return out[:need]


def signing_inputs(n=NBASE):
    """(seeds, msgs, seed index per message) of the base list."""
    return [key_seed(j) for j in range(NKEYS)], [message(i) for i in range(n)], [i % NKEYS for i in range(n)]


def sign_reference(n=NBASE):
    """The base list signed on the CPU (RFC 8032 is deterministic, so a device signer gives the same
    bytes): ed25519_ref.sign with [a]B computed once per key and additions of B's doublings."""
    seeds, msgs, idx = signing_inputs(n)
    keys = []
    for seed in seeds:
        a, prefix = o.expand_seed(seed)
        keys.append((a, prefix, o.compress(se.base_mul(a))))
    vks, sigs = [], []
    for m, j in zip(msgs, idx):
        a, prefix, A = keys[j]
        r = o.scalar_from_hash(hashlib.sha512(prefix + m).digest())
        R = o.compress(se.base_mul(r))
        s = (r + o.challenge(R, A, m) * a) % L
        vks.append(A)
        sigs.append(R + se.sc(s))
    return vks, sigs, msgs


def prehash(vks, sigs, msgs):
    """[(vk, sig, k)] with k = SHA-512(R || A || M) mod l."""
    return [(bytes(vk), bytes(sig), se.sc(int.from_bytes(hashlib.sha512(sig[:32] + vk + m).digest(), "little") % L))
            for vk, sig, m in zip(vks, sigs, msgs)]


def negated_twin(item):
    """(vk, enc(-R) || -s, -k): [-s]B = -R + [-k]A. None when R has x = 0 (-R = R)."""
    vk, sig, k = item
    R = o.decompress(sig[:32])
    if R is None or R[0] * pow(R[2], o.P - 2, o.P) % o.P == 0:
        return None
    s, kk = int.from_bytes(sig[32:], "little"), int.from_bytes(k, "little")
    return (vk, sig[:31] + bytes([sig[31] ^ 0x80]) + se.sc(-s % L), se.sc(-kk % L))


def with_defects(items, defects):
    """The items with s'_i = s_i + delta_i mod l at the positions of `defects` ({position: delta})."""
    out = list(items)
    for pos, delta in defects.items():
        vk, sig, k = out[pos]
        out[pos] = (vk, sig[:32] + se.sc((int.from_bytes(sig[32:], "little") + delta) % L), k)
    return out


def torsion_item(j=0, t=1):
    """A valid item whose R is a point of order 8: k = 1, s = a_j, R = T."""
    T = o.decompress(o.eight_torsion_encodings()[t])
    assert o.point_order(T) == "8"
    a, vk = se.key(j)
    return (vk, o.compress(T) + se.sc(a), se.sc(1))


def expected(z, defects):
    """(code, compress([8c]B), (x, y) of [c]B as 32-byte strings) for c = -sum z_i delta_i mod l."""
    c = -sum(z[pos] * delta for pos, delta in defects.items()) % L
    pt = se.base_mul(c)
    x, y = se.affine(pt)
    return (1 if c else 0), o.compress(se.base_mul(8 * c % L)), (se.sc(x), se.sc(y))


# ---------------------------------------------------------------- plans and the census
def plan_dict(c, hi, parts=1, nsub=None, split=False):
    """make_plan / batch_plan with explicit parts, restated in the form Engine.last_plan() reports."""
    wins, ws = se.plan_windows(c, hi, hi_windows=not split)
    bits = [b for _, b in wins]
    top = (ws - 1, len(wins) - 1)
    nslice = [-(-(1 << (b if w in top else b - 1)) // 256) for w, b in enumerate(bits)]
    nsub = list(nsub) if nsub else [1] * len(bits)
    bpr = sum(s * u for s, u in zip(nslice, nsub))
    while parts > 1 and bpr * parts > MAX_BINS:
        parts //= 2
    return {"bits": bits, "nslice": nslice, "nsub": nsub, "nwin": len(bits), "nwin_short": ws, "nranges": parts,
            "sum_ranges": int(parts > 1), "bins_per_range": bpr}


def per_sig_auto_nsub(n, entries):
    """batch_plan's sub-bin rule for n < 2^13 items with one key term per signature (9-bit windows of
    one slice each): 2 n + 1 entries expected in a short window, n + 1 in a high one."""
    def p2(x):
        p = 1
        while p * 2 <= x and p < 64:
            p *= 2
        return p
    return [p2((2 * n + 1) / entries)] * 15 + [p2((n + 1) / entries)] * 14


def plan_wins(plan):
    off, wins = 0, []
    for b in plan["bits"]:
        wins.append((off, b))
        off += b
    return wins


def terms(items, z, per_sig=False, split=False):
    """[(scalar, short?)] in term order: B, the R_i, then the keys (grouped: first appearance; the
    device's order differs, so census() is exact only where term_digits does not look at the index
    of a key term). Split coefficients: B lo, R_i, key lo, B hi, key hi, all short."""
    keys, b = se.coefficients(items, z)
    if per_sig:
        kc = [zi * int.from_bytes(k, "little") % L for (_, _, k), zi in zip(items, z)]
    else:
        kc = list(keys.values())
    rs = [(zi, True) for zi in z]
    if split:
        assert not per_sig
        return [(b & M128, True)] + rs + [(v & M128, True) for v in kc] + [(b >> 128, True)] + [(v >> 128, True) for v in kc]
    return [(b, False)] + rs + [(v, False) for v in kc]


def census_exact(plan, per_sig):
    return per_sig or (set(plan["nsub"]) == {1} and not plan["sum_ranges"])


def census(plan, tlist):
    """{(part, window, slice, sub-bin): 256 bucket counts} of the occupied bins, by term_get /
    term_digits / plan_digit."""
    wins, ws = plan_wins(plan), plan["nwin_short"]
    nparts = plan["nranges"] if plan["sum_ranges"] else 1
    bins, memo = {}, {}
    for t, (s, short) in enumerate(tlist):
        if not s:
            continue
        if (s, short) not in memo:
            memo[s, short] = se.plan_digits(s, wins[:ws] if short else wins)[0]
        for w, d in enumerate(memo[s, short]):
            if d:
                b = abs(d) - 1
                assert (b >> 8) < plan["nslice"][w]
                key = (t % nparts, w, b >> 8, t & (plan["nsub"][w] - 1))
                bins.setdefault(key, [0] * 256)[b & 255] += 1
    return bins


def all_bins(plan):
    nparts = plan["nranges"] if plan["sum_ranges"] else 1
    return [(p, w, s, u) for p in range(nparts) for w in range(plan["nwin"]) for s in range(plan["nslice"][w])
            for u in range(plan["nsub"][w])]


def bin_stats(counts):
    """What the accumulation's lanes meet in a bin with these bucket counts. Lane t walks the sorted
    positions [E t >> 8, E (t+1) >> 8).
    max_lanes: the most lanes with a non-empty range that one bucket covers;
    ends: {(e - lo, hi - e)} for every bucket end e < E, [lo, hi) the range of the lane owning e:
          (0, .) the end is a lane start, (1, .) one past it, (., 1) one before the next;
    crossed: the most empty buckets passed in one step inside a lane's range;
    empty_inside: the most lanes with an empty range [lo, lo) whose lo lies inside one bucket's span."""
    E = sum(counts)
    lo = [(E * t) >> 8 for t in range(257)]
    owner = [0] * E
    for t in range(256):
        for q in range(lo[t], lo[t + 1]):
            owner[q] = t
    spans, at = [], 0
    for b, c in enumerate(counts):
        if c:
            spans.append((b, at, at + c))
            at += c
    st = {"E": E, "occupied": len(spans), "max_lanes": 0, "ends": set(), "crossed": 0, "empty_inside": 0,
          "largest": max(counts)}
    for i, (b, s, e) in enumerate(spans):
        t0, t1 = owner[s], owner[e - 1]
        live = sum(1 for t in range(t0, t1 + 1) if lo[t] < lo[t + 1])
        st["max_lanes"] = max(st["max_lanes"], live)
        st["empty_inside"] = max(st["empty_inside"], sum(1 for t in range(256) if lo[t] == lo[t + 1] and s <= lo[t] < e))
        if e < E:
            t = owner[e]
            st["ends"].add((e - lo[t], lo[t + 1] - e))
            if e > lo[t]:
                st["crossed"] = max(st["crossed"], spans[i + 1][0] - b - 1)
    return st


# ---------------------------------------------------------------- z families
def short_wins(c):
    wins, ws = se.plan_windows(c, c)
    return tuple(wins[:ws])


def z_of(digits, wins):
    """The 128-bit z whose windows recode to exactly these signed digits."""
    z = sum(d << off for d, (off, _) in zip(digits, wins))
    assert 0 <= z <= M128 and se.plan_digits(z, wins)[0] == list(digits), digits
    return z


def d_one(w, bits, top):
    return 1


def d_max(w, bits, top):
    """The largest magnitude: bucket 255 of the window's last slice (2^bits unsigned on top,
    -2^(bits-1) below it)."""
    return (1 << bits) if top else -(1 << (bits - 1))


def d_mid(w, bits, top):
    """Bucket 77 of a middle slice."""
    nslice = -(-(1 << (bits if top else bits - 1)) // 256)
    return 256 * (nslice // 2) + 78


def d_far(w, bits, top):
    """The last bucket of slice 0 (bucket 255, or 127 where an 8-bit signed window has only 128)."""
    if top or bits >= 10:
        return 256
    return -256 if bits == 9 else -128


def uniform_z(dfn, wins):
    return z_of([dfn(w, bits, w + 1 == len(wins)) for w, (_, bits) in enumerate(wins)], wins)


def one_bucket(n, dfn, wins):
    return [uniform_z(dfn, wins)] * n


def two_buckets(n, n1, wins):
    return [uniform_z(d_one, wins)] * n1 + [uniform_z(d_far, wins)] * (n - n1)


def _draws(label, i):
    h = hashlib.sha512(b"bucket-shapes/%s/%d" % (label.encode(), i)).digest()
    return [int.from_bytes(h[4 * w:4 * w + 4], "little") / 2.0**32 for w in range(16)]


_ZIPF = {}


def zipf_bucket(u, nb):
    """Bucket b < nb with probability proportional to 1 / (b + 1)."""
    if nb not in _ZIPF:
        tot, acc, cum = sum(1.0 / (b + 1) for b in range(nb)), 0.0, []
        for b in range(nb):
            acc += 1.0 / (b + 1) / tot
            cum.append(acc)
        _ZIPF[nb] = cum
    cum = _ZIPF[nb]
    a, b = 0, nb - 1
    while a < b:
        m = (a + b) // 2
        if cum[m] < u:
            a = m + 1
        else:
            b = m
    return a


@functools.lru_cache(maxsize=None)
def zipf_digits(label, i, wins):
    """Positive magnitudes in slice 0 (below 2^(bits-1), so nothing carries)."""
    u = _draws(label, i)
    return [zipf_bucket(u[w], min(256, (1 << (bits - 1)) - 1)) + 1 for w, (_, bits) in enumerate(wins)]


def zipf(n, wins, label="zipf"):
    return [z_of(zipf_digits(label, i, wins), wins) for i in range(n)]


def prefix(n, cnt, dfn, wins):
    """Item i carries digit dfn(i, w) in window w while i < cnt[w], else 0 (non-negative digits)."""
    return [z_of([dfn(i, w) if i < cnt[w] else 0 for w in range(len(wins))], wins) for i in range(n)]


def comb(n, r, m, label="comb"):
    """z_i != 0 only where the term index 1 + i = r mod m; pseudo-random 128-bit values there."""
    return [int.from_bytes(hashlib.sha512(b"bucket-shapes/%s/%d" % (label.encode(), i)).digest()[:16], "little") | 1
            if (1 + i) % m == r else 0 for i in range(n)]


# ---------------------------------------------------------------- cases
class Case:
    """One batch and the plan it runs under. shape: set_msm_shape's (bits, parts), None = the
    automatic plan of n < 2^13 items with `entries` per bin; grouping: set_key_grouping's mode;
    split: the keys are registered, so the coefficients are cut at bit 128. make(base, wins) ->
    (items, z); prop(case, plan, bins) asserts what the case exists for."""

    def __init__(self, name, n, shape, make, prop, grouping=0, entries=0, split=False, msgs=False):
        self.name, self.n, self.shape, self.make, self.prop = name, n, shape, make, prop
        self.grouping, self.entries, self.split, self.msgs = grouping, entries, split, msgs
        self.per_sig = grouping == 2
        self.c = shape[0] if shape else 9
        self.wins = short_wins(self.c)

    def cpu_plans(self):
        """The plans the device may choose: grouped batches of >= 4096 items put the high bits in
        8-bit windows when the context's hint says "few keys"."""
        if self.shape is None:
            assert self.per_sig and self.n < 1 << 13
            return [plan_dict(9, 9, nsub=per_sig_auto_nsub(self.n, self.entries))]
        c, parts = self.shape
        his = [c] + ([8] if self.n >= 4096 and not self.per_sig and not self.split and c != 8 else [])
        return [plan_dict(c, hi, parts, split=self.split) for hi in his]

    def check_plan(self, plan):
        """The reported plan is the one the case asked for, and one the census is exact for."""
        ref = self.cpu_plans()
        keys = ("bits", "nslice", "nsub", "nwin", "nwin_short", "nranges", "sum_ranges", "bins_per_range")
        assert any(all(plan[k] == r[k] for k in keys) for r in ref), (self.name, plan)
        assert plan["per_sig"] == self.per_sig and plan["split"] == self.split and not plan["fold"], (self.name, plan)
        assert census_exact(plan, self.per_sig), (self.name, plan)

    def terms(self, items, z):
        return terms(items, z, self.per_sig, self.split)


_BUILT = {}


def build(case, base):
    """(items, z, position of an item inside the longest bucket), built once per case."""
    if case.name not in _BUILT:
        items, z = case.make(base, case.wins)
        assert len(items) == len(z) == case.n, case.name
        d0 = [se.plan_digits(zi, case.wins)[0][0] if zi else 0 for zi in z]
        live = [d for d in d0 if d]
        top = max(set(live), key=live.count) if live else 0
        _BUILT[case.name] = (items, z, d0.index(top))
    return _BUILT[case.name]


def tile(base, n):
    return [base[i % len(base)] for i in range(n)]


def variants(case, base):
    """[(tag, items, z, defects)]: clean, a defect inside the longest bucket, a defect in the last item."""
    items, z, long_pos = build(case, base)
    out = [("clean", items, z, {})]
    for tag, pos in (("defect_long", long_pos), ("defect_last", case.n - 1)):
        defects = {pos: 1 + pos}
        out.append((tag, with_defects(items, defects), z, defects))
    return out


def _stats(bins):
    return {k: bin_stats(v) for k, v in bins.items()}


def _fit(case, items, p, build_z, correct):
    """Fixed point of a size parameter p: build_z(p) -> z; correct(bins, p) -> the p that would meet
    the shape, p itself once it is met. The B and key coefficients move with z, so the few entries
    they add to a bin are only known once z is."""
    for _ in range(40):
        z = build_z(p)
        q = correct(census(case.cpu_plans()[0], case.terms(items, z)), p)
        if q == p:
            return z
        p = q
    raise AssertionError("no fixed point for " + case.name)


# properties -------------------------------------------------------
def p_single_bucket(E, lanes=None, empty_inside=False):
    def prop(case, plan, bins):
        hits = [s for s in _stats(bins).values() if s["E"] == E and s["occupied"] == 1]
        assert hits, (case.name, E)
        if lanes:
            assert any(s["max_lanes"] == lanes for s in hits), case.name
        if empty_inside:
            assert any(s["empty_inside"] > 0 for s in hits), case.name
    return prop


def p_long_bucket(lanes):
    def prop(case, plan, bins):
        assert max(s["max_lanes"] for s in _stats(bins).values()) >= lanes, case.name
    return prop


def p_boundary(offset):
    """Window 0: the end of bucket 0 on a lane start (0), one past it (1) or one before it (-1); off
    the start, the lane then steps over the >= 200 empty buckets between the two in one go."""
    def prop(case, plan, bins):
        s = bin_stats(bins[0, 0, 0, 0])
        e = bins[0, 0, 0, 0][0]
        lo = [(s["E"] * t) >> 8 for t in range(257)]
        t = max(u for u in range(256) if lo[u] <= e)
        size = lo[t + 1] - lo[t]
        assert size >= 3 and e - lo[t] == (offset if offset >= 0 else size - 1), (case.name, e, lo[t])
        assert (e - lo[t], lo[t + 1] - e) in s["ends"] and t == 100, case.name
        if offset and case.c >= 13:
            assert max(x["crossed"] for x in _stats(bins).values()) >= 200, case.name
    return prop


def p_zipf(case, plan, bins):
    """One long bucket, single-entry buckets and empties in the same bin; an end on a lane start
    somewhere and a lane that crosses buckets mid-range."""
    st = _stats(bins)
    assert any(s["max_lanes"] >= 20 and s["occupied"] < 200 and s["crossed"] >= 1 for s in st.values()), case.name
    assert any(1 in bins[k] and 0 in bins[k] and s["largest"] >= s["E"] // 8 for k, s in st.items()), case.name


def p_all_empty(case, plan, bins):
    assert not bins and all_bins(plan), case.name


def p_one_entry(case, plan, bins):
    """One R term, B and one key: no bin holds more than three entries. With 16-bit windows the three
    fall into different slices (bins of one entry); with 8-bit windows a window is one bin of three
    (short) or two (high) entries."""
    st = _stats(bins)
    es = {s["E"] for s in st.values()}
    assert max(es) <= 3 and {k[1] for k in st} >= set(range(plan["nwin_short"])), case.name
    assert 1 in es if case.c == 16 else {2, 3} <= es, case.name


def p_siblings(case, plan, bins):
    """Every occupied slice keeps all its entries in one sub-bin; its siblings are empty."""
    assert max(plan["nsub"]) >= 16, case.name
    slices = {}
    for (p, w, s, u) in bins:
        slices.setdefault((p, w, s), set()).add(u)
    assert slices and all(len(v) == 1 for v in slices.values()), case.name
    assert len(bins) * 16 <= len(all_bins(plan)), case.name


def p_subbins_uneven(case, plan, bins):
    """The sub-bins of a slice all hold entries, in different numbers."""
    st = _stats(bins)
    per = [st[k]["E"] for k in st if k[1] == 0]
    assert max(plan["nsub"]) >= 16 and len(per) == plan["nsub"][0] and len(set(per)) > 1, case.name
    assert any(s["max_lanes"] >= 10 for s in st.values()), case.name


def p_big(case, plan, bins):
    """Past the sort's register-resident entries: bins of exactly 10240, 10241 and more."""
    es = {s["E"] for s in _stats(bins).values()}
    assert 10240 in es and 10241 in es and max(es) >= case.n > 10241, (case.name, sorted(es)[-4:])


def p_none(case, plan, bins):
    assert bins, case.name


SORT_REG_ENTRIES = 40 * 256       # k_msm_sort keeps this many entries of a bin in registers


def make_cases():
    """Every case of the GPU test, in a fixed order."""
    out = []

    def add(*a, **k):
        out.append(Case(*a, **k))

    # one bucket per bin: E < 256 (lanes with empty ranges inside the span), 256, 257
    for n in (1, 2, 3, 100, 255, 256, 257):
        add("one_mid_c16_n%d" % n, n, (16, 1), lambda base, wins, n=n: (tile(base, n), one_bucket(n, d_mid, wins)),
            p_single_bucket(n, lanes=min(n, 256), empty_inside=n in (100, 255)))
    add("one_d1_c8_n300", 300, (8, 1), lambda base, wins: (tile(base, 300), one_bucket(300, d_one, wins)), p_long_bucket(240))
    add("one_max_c9_n300", 300, (9, 1), lambda base, wins: (tile(base, 300), one_bucket(300, d_max, wins)), p_long_bucket(240))
    add("one_max_c13_n257", 257, (13, 1), lambda base, wins: (tile(base, 257), one_bucket(257, d_max, wins)),
        p_single_bucket(257, lanes=256))

    # two far-apart buckets, the boundary on / next to a lane start
    def two(name, n, shape, offset):
        def make(base, wins):
            items = tile(base, n)

            def correct(bins, n1):
                counts = bins[0, 0, 0, 0]
                E = sum(counts)
                lo, hi = (E * 100) >> 8, (E * 101) >> 8
                goal = lo + (offset if offset >= 0 else hi - lo - 1)
                return goal - (counts[0] - n1)            # bucket 0 also holds what B and the keys put there
            return items, _fit(case, items, n * 100 // 256, lambda n1: two_buckets(n, n1, wins), correct)
        case = Case(name, n, shape, make, p_boundary(offset))
        out.append(case)
    two("two_c16_on", 900, (16, 1), 0)
    two("two_c16_after", 900, (16, 1), 1)
    two("two_c16_before", 900, (16, 1), -1)
    two("two_c9_on", 900, (9, 1), 0)

    # Zipf occupancy
    add("zipf_c9_n600", 600, (9, 1), lambda base, wins: (tile(base, 600), zipf(600, wins)), p_zipf)
    add("zipf_c13_n600", 600, (13, 1), lambda base, wins: (tile(base, 600), zipf(600, wins)), p_zipf)
    add("zipf_c11_p16_n600", 600, (11, 16), lambda base, wins: (tile(base, 600), zipf(600, wins)), p_none, grouping=2)
    add("zipf_c8_n300_msgs", 300, (8, 1), lambda base, wins: (tile(base, 300), zipf(300, wins)), p_zipf, msgs=True)
    add("zipf_c13_n600_split", 600, (13, 1), lambda base, wins: (tile(base, 600), zipf(600, wins)), p_zipf, split=True)

    # sub-bins: one sibling takes everything; uneven siblings under Zipf digits
    add("comb_auto_n4096", 4096, None, lambda base, wins: (tile(base, 4096), comb(4096, 0, 32)), p_siblings,
        grouping=2, entries=256)
    add("zipf_auto_n4099", 4099, None, lambda base, wins: (tile(base, 4099), zipf(4099, wins)), p_subbins_uneven,
        grouping=2, entries=256)

    # empty bins
    add("all_zero_c9_n64", 64, (9, 1), lambda base, wins: (tile(base, 64), [0] * 64), p_all_empty)
    for c in (16, 8):
        add("one_nonzero_c%d_n64" % c, 64, (c, 1),
            lambda base, wins: (tile(base, 64), [0] * 37 + [uniform_z(d_one, wins)] + [0] * 26), p_one_entry)

    # sums through the identity, doublings, torsion
    def cancel(base, wins):
        items = []
        for it in base:
            tw = negated_twin(it)
            if tw is not None and len(items) < 128:
                items += [it, tw]
        return items, one_bucket(128, d_mid, wins)
    add("cancel_c9_n128", 128, (9, 1), cancel, p_long_bucket(100))
    for c in (9, 16):
        add("repeat_c%d_n64" % c, 64, (c, 1), lambda base, wins: ([base[5]] * 64, one_bucket(64, d_mid, wins)),
            p_long_bucket(60))
    add("torsion_c9_n64", 64, (9, 1),
        lambda base, wins: ([torsion_item()] * 8 + tile(base, 56), one_bucket(64, d_one, wins)), p_long_bucket(60))

    # past the sort's registers: E = 10240, 10241 and n
    def big(name, dfn_of):
        n = 10300

        def make(base, wins):
            items = tile(base, n)
            dfn = dfn_of(wins)
            goal = {0: SORT_REG_ENTRIES, 1: SORT_REG_ENTRIES + 1}

            def correct(bins, cnt):
                new = dict(cnt)
                for w, g in goal.items():
                    new[w] += g - sum(bins[0, w, (dfn(0, w) - 1) >> 8, 0])
                return new
            start = {w: goal.get(w, n - 700 * (w - 2)) for w in range(len(wins))}
            return items, _fit(case, items, start, lambda cnt: prefix(n, cnt, dfn, wins), correct)
        case = Case(name, n, (16, 1), make, p_big)
        out.append(case)
    big("big_c16_one", lambda wins: lambda i, w: d_mid(w, wins[w][1], w + 1 == len(wins)))
    big("big_c16_zipf", lambda wins: lambda i, w: zipf_digits("big", i, wins)[w])
    return out


CASES = make_cases()
BY_NAME = {c.name: c for c in CASES}


def reduce_regime(nbin):
    """Which bin reduction a pipelined batch of nbin bins runs (edc_msm.hip launch_msm_bucket)."""
    return "quad" if nbin <= 128 else "lanes64" if nbin < 256 else "lanes32"
