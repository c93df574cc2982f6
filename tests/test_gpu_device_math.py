"""GPU: the device builds of the field and point arithmetic (csrc/fe25519.h, ge25519.h, ge_quad.h,
ge_row.h) on chosen limb inputs, through the test-only library tests/native/libedc_devcheck.so
(tests/native/devcheck.hip, one entry point dc_run), against Python integers mod p = 2^255 - 19 and
the oracle's point addition.

Whole signatures only ever feed these layers random points in random limb forms, and
tests/test_native_math.py runs the plain C path g++ sees, not the device's v_mad_u64_u32 / DPP /
permlane code. Here every operation gets limbs at the documented bounds (reduced: < 2^29 + 2^19;
lazy sum: twice that; mul input: < 2^30.41; lazy difference against a reduced partner), single-limb
extremes, multiples of p in shifted limb forms, small-order points, P + P and P + (-P) through the
additions, projective and non-canonical limb forms. Field elements travel as nine raw limbs, so
the reduced-output promise is asserted limb by limb. Nothing the code under test computes is used
as an expected value."""
import ctypes
import functools
import os
import random
from array import array

import pytest

from conftest import ROOT, golden

pytestmark = pytest.mark.gpu

P = 2**255 - 19
M29 = (1 << 29) - 1
RED = (1 << 29) + (1 << 19)          # reduced: every limb < RED
LAZY = 2 * RED                       # lazy sum of two reduced elements: every limb < LAZY
MULIN = int(2**30.41)                # documented mul-input bound: every limb < MULIN
TOPS = {"red": RED - 1, "lazy": LAZY - 1, "mulin": MULIN - 1}
# fe_sub's bias K = 4p + 2^263 - 4864 (fe25519.h EDC_SUB_K*)
SUB_K = [0x80000000 - 76 - 4864] + [0x80000000 - 4] * 7 + [0x80000000 + 0x2000000 - 4]
D2 = 2 * (-121665 * pow(121666, P - 2, P)) % P

OP = {
    "fe_mul": 0, "fe_sqr": 1, "fe_sub": 2, "fe_lsub_mul": 3, "fe_mul_lsub": 4, "fe_add_c": 5, "fe_carry": 6,
    "fe_mul_small": 7, "fe_canon": 8, "fe_invert": 9, "fe_pow_p58": 10, "fe_flags": 11,
    "rf_mul": 20, "rf_sqr": 21, "rf_sub": 22, "rf_add_c": 23, "rf_carry": 24,
    "row_dbl_k": 30, "row_add": 31, "row_horner": 32,
    "quad_dbl": 40, "quad_add_cached": 41, "quad_madd": 42, "quad_add": 43, "quad_dbl_d": 44, "quad_add_d": 45,
    "ge_madd_pos": 50, "ge_madd_neg": 51, "ge_dbl_t": 52, "ge_dbl_not": 53, "ge_add_cached": 54,
}
# words per case (in, out)
WORDS = {
    "fe_mul": (18, 9), "fe_sqr": (9, 9), "fe_sub": (18, 9), "fe_lsub_mul": (27, 9), "fe_mul_lsub": (27, 9),
    "fe_add_c": (18, 9), "fe_carry": (9, 9), "fe_mul_small": (10, 9), "fe_canon": (9, 9), "fe_invert": (9, 9),
    "fe_pow_p58": (9, 9), "fe_flags": (18, 1),
    "rf_mul": (18, 16), "rf_sqr": (9, 16), "rf_sub": (18, 16), "rf_add_c": (18, 16), "rf_carry": (9, 16),
    "row_dbl_k": (37, 36), "row_add": (72, 100), "row_horner": (73, 36),
    "quad_dbl": (36, 144), "quad_add_cached": (72, 144), "quad_madd": (72, 144), "quad_add": (72, 144),
    "quad_dbl_d": (36, 144), "quad_add_d": (72, 144),
    "ge_madd_pos": (72, 36), "ge_madd_neg": (72, 36), "ge_dbl_t": (36, 36), "ge_dbl_not": (36, 36),
    "ge_add_cached": (72, 36),
}
CHAIN_K = (1, 2, 3, 8, 16)


def test_sub_bias_is_a_multiple_of_p():
    assert val(SUB_K) % P == 0 and min(SUB_K) >= MULIN


# ---------------------------------------------------------------- plumbing

@pytest.fixture(scope="module")
def dc(engine):
    """dc_run of the test-only device library. The engine fixture comes first: it loads torch's HIP
    runtime and libedc.so, so this library binds to the same runtime."""
    so = os.path.join(ROOT, "tests", "native", "libedc_devcheck.so")
    assert os.path.exists(so), "tests/native/libedc_devcheck.so is not built (run __graft_entry__.build())"
    lib = ctypes.CDLL(so)
    lib.dc_run.restype = ctypes.c_int
    lib.dc_run.argtypes = [ctypes.c_int, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p,
                           ctypes.c_uint32]
    return lib


_results = {}


def run(dc, name, cases, key=None):
    """cases: one flat word list per case. Returns one output word list per case. A result is kept
    under `key` so that tests sharing inputs share the launch."""
    if key is not None and (name, key) in _results:
        return _results[(name, key)]
    iw, ow = WORDS[name]
    n = len(cases)
    assert 0 < n <= 1 << 16 and all(len(c) == iw for c in cases), (name, n)
    flat = array("I", [w for c in cases for w in c])
    out = array("I", bytes(4 * n * ow))
    rc = dc.dc_run(OP[name], n, flat.buffer_info()[0], iw, out.buffer_info()[0], ow)
    assert rc == 0, (name, rc)
    res = [out[i * ow:(i + 1) * ow].tolist() for i in range(n)]
    if key is not None:
        _results[(name, key)] = res
    return res


def limbs(v):
    """normalized radix-2^29 limbs; limb 8 takes everything from bit 232 up"""
    return [(v >> (29 * i)) & M29 for i in range(8)] + [v >> 232]


def val(ls):
    return sum(x << (29 * i) for i, x in enumerate(ls))


def first_bad(pred, n):
    return [i for i in range(n) if not pred(i)][:4]


# ---------------------------------------------------------------- field vectors

def _shifted_forms(base, bound, rnd, steps=6):
    """the construction of test_fe_is_zero_lazy_limbs: move 2^29 down from limb i+1 into limb i while
    every limb stays below `bound`"""
    forms = [list(base)]
    for _ in range(steps):
        f = list(forms[-1])
        i = rnd.randrange(8)
        if f[i + 1] > 0 and f[i] + (1 << 29) < bound:
            f[i + 1] -= 1
            f[i] += 1 << 29
        forms.append(f)
    return forms


@functools.lru_cache(maxsize=None)
def field_vectors():
    """(tag, limbs) with every limb < MULIN; the tag's prefix names the bound the vector respects"""
    rnd = random.Random(0xFE25519)
    v = []
    for name, top in TOPS.items():
        v.append((f"{name}:all", [top] * 9))
        v.append((f"{name}:low8", [top] * 8 + [0]))
        v.append((f"{name}:top1", [0] * 8 + [top]))
        for i in range(9):
            v.append((f"{name}:only{i}", [top if j == i else 0 for j in range(9)]))
            v.append((f"{name}:allbut{i}", [0 if j == i else top for j in range(9)]))
        for _ in range(150):
            v.append((f"{name}:near", [top - rnd.randrange(1 << 12) for _ in range(9)]))
        for _ in range(400):
            v.append((f"{name}:rand", [rnd.randrange(top + 1) for _ in range(9)]))
    for r in (0, 1, P - 1, 19, 2**255 - 20):
        for k in (0, 1, 2, 3, 31, 63, 64, 127, 169):
            base = limbs(r + k * P)
            if base[8] < MULIN:
                name = "red" if base[8] < RED else "mulin"
                v.append((f"{name}:cong{r % P if r < 20 else -1}+{k}p", base))
    k = 0
    while True:                                     # every multiple of p the lazy bound can hold
        base = limbs(k * P)
        if base[8] >= MULIN:
            break
        for n, f in enumerate(_shifted_forms(base, MULIN, rnd)):
            v.append((f"mulin:{k}p/form{n}", f))
        k += 1
    assert k > 150
    assert all(0 <= x < MULIN for _, ls in v for x in ls)
    return tuple((t, tuple(ls)) for t, ls in v)


@functools.lru_cache(maxsize=None)
def reduced_vectors():
    return tuple((t, ls) for t, ls in field_vectors() if max(ls) < RED)


@functools.lru_cache(maxsize=None)
def pair_cases():
    """(tag, a, b) for the two-operand ops, both operands inside the mul-input bound: a fixed
    scramble of the vector list, every extreme against every extreme of the same bound, and the
    asymmetric pairs (a lazy difference at its largest against a reduced partner, both orders)."""
    vec = field_vectors()
    n = len(vec)
    cases = [(f"{ta} x {tb}", a, b) for i, (ta, a) in enumerate(vec) for tb, b in [vec[(i * 5 + 1) % n]]]
    for name, top in TOPS.items():
        ext = [(t, ls) for t, ls in vec if t.startswith(name + ":") and t.split(":")[1] in ("all", "low8", "top1")]
        ext += [(t, ls) for t, ls in vec if t.startswith(name + ":only") or t.startswith(name + ":allbut")]
        for ta, a in ext:
            for tb, b in ext[:3]:
                cases.append((f"{ta} x {tb}", a, b))
    return tuple(cases)


@functools.lru_cache(maxsize=None)
def asym_cases():
    """one operand a lazy difference a + K - b (a a lazy sum < 2^30 + 2^20, limbs up to 2^31.61), the
    other reduced: fe_mul's asymmetric bound (fe25519.h fe_sub_lazy)"""
    rnd = random.Random(0xA5)
    red = reduced_vectors()
    lz = [[LAZY - 1 + k for k in SUB_K], [k for k in SUB_K]]
    lz += [[rnd.randrange(LAZY) + k - rnd.randrange(RED) for k in SUB_K] for _ in range(300)]
    lz += [[LAZY - 1 - rnd.randrange(1 << 12) + k for k in SUB_K] for _ in range(100)]
    cases = []
    for i, a in enumerate(lz):
        partners = [("red:all", (RED - 1,) * 9), red[(i * 11 + 3) % len(red)]]
        for tb, b in partners:
            cases.append((f"asym:lazydiff{i} x {tb}", tuple(a), b))
            cases.append((f"asym:{tb} x lazydiff{i}", b, tuple(a)))
    assert all(x < 2**31.61 for _, a, b in cases for x in a + b)
    return tuple(cases)


def check_field(name, tags, outs, expected, reduced=True, lanes16=False):
    """value mod p, the reduced-output promise, and for the row layout zeros on lanes 9..15"""
    n = len(tags)
    assert len(outs) == n == len(expected)
    wrong = first_bad(lambda i: val(outs[i][:9]) % P == expected[i] % P, n)
    assert not wrong, (name, "value mod p", [(tags[i], outs[i][:9]) for i in wrong])
    if reduced:
        wrong = first_bad(lambda i: max(outs[i][:9]) < RED, n)
        assert not wrong, (name, "limb >= 2^29 + 2^19", [(tags[i], outs[i][:9]) for i in wrong])
    if lanes16:
        wrong = first_bad(lambda i: not any(outs[i][9:]), n)
        assert not wrong, (name, "lanes 9..15 not 0", [(tags[i], outs[i]) for i in wrong])


def mul_cases():
    return pair_cases() + asym_cases()


@pytest.mark.parametrize("layer", ["fe", "rf"])
def test_mul(dc, layer):
    cs = mul_cases()
    outs = run(dc, f"{layer}_mul", [a + b for _, a, b in cs], key="mul")
    check_field(f"{layer}_mul", [t for t, _, _ in cs], outs, [val(a) * val(b) for _, a, b in cs], lanes16=layer == "rf")


def test_rf_mul_fe_mul_parity(dc):
    """The two independent products on the same limbs: each is held against the integers first, so a
    disagreement names the side that left them; then the two against each other."""
    cs = mul_cases()
    words = [a + b for _, a, b in cs]
    fe_out = run(dc, "fe_mul", words, key="mul")
    rf_out = run(dc, "rf_mul", words, key="mul")
    exp = [val(a) * val(b) % P for _, a, b in cs]
    fe_bad = first_bad(lambda i: val(fe_out[i]) % P == exp[i], len(cs))
    rf_bad = first_bad(lambda i: val(rf_out[i][:9]) % P == exp[i], len(cs))
    assert not fe_bad, ("fe_mul left the integers", [cs[i] for i in fe_bad])
    assert not rf_bad, ("rf_mul left the integers", [cs[i] for i in rf_bad])
    diff = first_bad(lambda i: val(fe_out[i]) % P == val(rf_out[i][:9]) % P, len(cs))
    assert not diff, ("rf_mul != fe_mul", [cs[i] for i in diff])


@pytest.mark.parametrize("layer", ["fe", "rf"])
def test_sqr(dc, layer):
    vec = field_vectors()
    outs = run(dc, f"{layer}_sqr", [list(a) for _, a in vec])
    check_field(f"{layer}_sqr", [t for t, _ in vec], outs, [val(a) ** 2 for _, a in vec], lanes16=layer == "rf")


@functools.lru_cache(maxsize=None)
def sub_cases():
    """a anywhere inside the mul-input bound; b at 0, at the reduced top, and scrambled"""
    vec = field_vectors()
    n = len(vec)
    zero, redtop = (0,) * 9, (RED - 1,) * 9
    cs = []
    for i, (t, a) in enumerate(vec):
        cs.append((f"{t} - 0", a, zero))
        cs.append((f"{t} - red:all", a, redtop))
        tb, b = vec[(i * 7 + 2) % n]
        cs.append((f"{t} - {tb}", a, b))
    return tuple(cs)


@pytest.mark.parametrize("layer", ["fe", "rf"])
def test_sub(dc, layer):
    cs = sub_cases()
    outs = run(dc, f"{layer}_sub", [a + b for _, a, b in cs])
    check_field(f"{layer}_sub", [t for t, _, _ in cs], outs, [val(a) - val(b) for _, a, b in cs], lanes16=layer == "rf")


@pytest.mark.parametrize("layer", ["fe", "rf"])
def test_add_c(dc, layer):
    """carried add: documented for reduced operands; any pair inside the mul-input bound still sums
    below 2^32, which is all the carry round needs"""
    cs = pair_cases()
    outs = run(dc, f"{layer}_add_c", [a + b for _, a, b in cs])
    check_field(f"{layer}_add_c", [t for t, _, _ in cs], outs, [val(a) + val(b) for _, a, b in cs],
                lanes16=layer == "rf")


@pytest.mark.parametrize("layer", ["fe", "rf"])
def test_carry(dc, layer):
    """limbs < 2^32 in, reduced out: the field vectors plus the 32-bit extremes"""
    rnd = random.Random(0xCA)
    top = (1 << 32) - 1
    vec = list(field_vectors()) + [("u32:all", (top,) * 9), ("u32:low8", (top,) * 8 + (0,)),
                                   ("u32:top1", (0,) * 8 + (top,))]
    vec += [(f"u32:only{i}", tuple(top if j == i else 0 for j in range(9))) for i in range(9)]
    vec += [("u32:near", tuple(top - rnd.randrange(1 << 12) for _ in range(9))) for _ in range(100)]
    vec += [("u32:rand", tuple(rnd.getrandbits(32) for _ in range(9))) for _ in range(400)]
    outs = run(dc, f"{layer}_carry", [list(a) for _, a in vec])
    check_field(f"{layer}_carry", [t for t, _ in vec], outs, [val(a) for _, a in vec], lanes16=layer == "rf")


@functools.lru_cache(maxsize=None)
def lsub_cases():
    """(tag, a, b, c) for fe_mul(fe_sub_lazy(a, b), c) and its mirror: a up to the mul-input top, b at
    0, at the reduced top and random reduced, the partner c reduced (at its top and scrambled)"""
    vec, red = field_vectors(), reduced_vectors()
    zero, redtop = (0,) * 9, (RED - 1,) * 9
    cs = []
    for name, top in TOPS.items():
        for b in (zero, redtop):
            cs.append((f"({name}:all - {'0' if b is zero else 'red:all'}) * red:all", (top,) * 9, b, redtop))
    for i, (t, a) in enumerate(vec):
        tb, b = [("0", zero), ("red:all", redtop), red[(i * 3 + 1) % len(red)]][i % 3]
        tc, c = red[(i * 7 + 2) % len(red)] if i % 4 else ("red:all", redtop)
        cs.append((f"({t} - {tb}) * {tc}", a, b, c))
    return tuple(cs)


@pytest.mark.parametrize("name", ["fe_lsub_mul", "fe_mul_lsub"])
def test_lazy_sub_products(dc, name):
    cs = lsub_cases()
    outs = run(dc, name, [a + b + c for _, a, b, c in cs])
    check_field(name, [t for t, *_ in cs], outs, [(val(a) - val(b)) * val(c) for _, a, b, c in cs])


def test_fe_mul_small(dc):
    vec = field_vectors()
    consts = [0, 1, 2, 19, 38, 1216, 4864, (1 << 13) - 1]
    rnd = random.Random(0x5A)
    cs = [(f"{t} * {c}", a, c) for i, (t, a) in enumerate(vec)
          for c in [consts[i % len(consts)] if i % 2 else rnd.randrange(1 << 13)]]
    cs += [(f"{name}:all * 8191", (top,) * 9, (1 << 13) - 1) for name, top in TOPS.items()]
    outs = run(dc, "fe_mul_small", [a + (c,) for _, a, c in cs])
    check_field("fe_mul_small", [t for t, _, _ in cs], outs, [val(a) * c for _, a, c in cs])


def test_fe_canon(dc):
    """canonical bytes: the output limbs are exactly the normalized limbs of the value mod p"""
    vec = field_vectors()
    outs = run(dc, "fe_canon", [list(a) for _, a in vec])
    wrong = first_bad(lambda i: outs[i] == limbs(val(vec[i][1]) % P), len(vec))
    assert not wrong, [(vec[i], outs[i]) for i in wrong]
    assert all(val(o).to_bytes(32, "little") == (val(a) % P).to_bytes(32, "little") for o, (_, a) in zip(outs, vec))


def test_fe_invert_and_pow_p58(dc):
    vec = field_vectors()
    tags = [t for t, _ in vec]
    words = [list(a) for _, a in vec]
    check_field("fe_invert", tags, run(dc, "fe_invert", words), [pow(val(a), P - 2, P) for _, a in vec])
    check_field("fe_pow_p58", tags, run(dc, "fe_pow_p58", words), [pow(val(a), (P - 5) // 8, P) for _, a in vec])


def test_fe_flags(dc):
    """fe_is_zero | fe_is_negative << 1 | fe_eq(a, b) << 2; b is another limb form of a's value for
    two cases in three"""
    vec = field_vectors()
    n = len(vec)
    cs = []
    for i, (t, a) in enumerate(vec):
        if i % 3 == 0:
            tb, b = vec[(i * 5 + 1) % n]
        else:
            k = (i * 13) % 160
            tb, b = f"same+{k}p", tuple(limbs(val(a) % P + k * P))
            assert b[8] < MULIN
        cs.append((f"{t} | {tb}", a, b))
    outs = run(dc, "fe_flags", [a + b for _, a, b in cs])
    exp = [int(val(a) % P == 0) | ((val(a) % P) & 1) << 1 | int((val(a) - val(b)) % P == 0) << 2 for _, a, b in cs]
    wrong = first_bad(lambda i: outs[i][0] == exp[i], len(cs))
    assert not wrong, [(cs[i], outs[i][0], exp[i]) for i in wrong]
    assert {e & 1 for e in exp} == {0, 1} and {e >> 2 for e in exp} == {0, 1}


# ---------------------------------------------------------------- point vectors

def reslice(v, rnd):
    """a non-canonical reduced limb form of v: v + k p with limb 8 still reduced, then 2^29 pushed
    down wherever the lower limb stays reduced"""
    v %= P
    k = rnd.randrange((RED << 232) // P - 1)
    f = limbs(v + k * P)
    assert f[8] < RED
    for i in rnd.sample(range(8), 8):
        if f[i + 1] > 0 and f[i] + (1 << 29) < RED:
            f[i + 1] -= 1
            f[i] += 1 << 29
    assert val(f) % P == v and max(f) < RED
    return f


def point_words(aff, form, rnd):
    """36 words X | Y | Z | T for the affine point: 'affine' (Z = 1, canonical limbs), 'affine-resliced'
    (Z = 1, X, Y, T in non-canonical reduced forms), 'scaled' (all four times a random lambda) or
    'scaled-resliced'"""
    x, y = aff
    lam = 1 if form.startswith("affine") else rnd.randrange(2, P)
    coords = [x * lam % P, y * lam % P, lam, x * y * lam % P]
    if form.endswith("resliced"):
        return sum((reslice(c, rnd) if not (form.startswith("affine") and i == 2) else limbs(c)
                    for i, c in enumerate(coords)), [])
    return sum((limbs(c) for c in coords), [])


def ext(aff):
    x, y = aff
    return (x, y, 1, x * y % P)


def affine(pt):
    X, Y, Z, _ = pt
    zi = pow(Z, P - 2, P)
    return (X * zi % P, Y * zi % P)


@functools.lru_cache(maxsize=None)
def source_points():
    """affine points: the valid golden decodings, the eight small-order points, identity, basepoint"""
    from conftest import load_oracle
    oracle = load_oracle()
    small = []
    for e in golden("zip215_small_order.json")["encodings"]:
        a = affine(oracle.decompress(bytes.fromhex(e)))
        if a not in small:
            small.append(a)
    assert len(small) == 8 and all(oracle.is_identity(oracle.scalar_mul(8, ext(a))) for a in small)
    pts = [affine(oracle.decompress(bytes.fromhex(c["enc"]))) for c in golden("decode.json")["cases"] if c["ok"]]
    ident, base = (0, 1), affine(oracle.B_POINT)
    return oracle, tuple(small), tuple(dict.fromkeys(pts + [ident, base]))


FORMS = ("affine", "affine-resliced", "scaled", "scaled-resliced")


@functools.lru_cache(maxsize=None)
def dbl_cases():
    """(tag, affine P, 36 words): every small-order point and a spread of the others in every form"""
    _, small, pts = source_points()
    rnd = random.Random(0xDB1)
    cs = []
    for i, a in enumerate(small):
        for f in FORMS:
            cs.append((f"small{i}/{f}", a, tuple(point_words(a, f, rnd))))
    for i, a in enumerate(pts):
        for f in FORMS:
            cs.append((f"pt{i}/{f}", a, tuple(point_words(a, f, rnd))))
    return tuple(cs)


@functools.lru_cache(maxsize=None)
def add_cases(q_affine):
    """(tag, affine P, affine Q, 72 words). q_affine: Q is given with Z = 1 (mixed additions)."""
    oracle, small, pts = source_points()
    rnd = random.Random(0xADD + q_affine)
    ident = (0, 1)
    pforms = FORMS
    qforms = FORMS[:2] if q_affine else FORMS
    pairs = []
    for n in range(200):
        pairs.append((f"rand{n}", rnd.choice(pts), rnd.choice(pts)))
    for i, a in enumerate(pts[::3]):
        pairs.append((f"P+P{i}", a, a))
        pairs.append((f"P-P{i}", a, affine(oracle.neg(ext(a)))))
        pairs.append((f"0+P{i}", ident, a))
        pairs.append((f"P+0{i}", a, ident))
    for i, a in enumerate(small):
        for j, b in enumerate(small):
            pairs.append((f"small{i}+small{j}", a, b))
    cs = []
    for n, (t, a, b) in enumerate(pairs):
        fa, fb = pforms[n % len(pforms)], qforms[(n // len(pforms)) % len(qforms)]
        cs.append((f"{t}/{fa}/{fb}", a, b, tuple(point_words(a, fa, rnd) + point_words(b, fb, rnd))))
    # the same limbs on both sides (not only the same point)
    for i, a in enumerate(small + pts[:8]):
        w = point_words(a, qforms[i % len(qforms)], rnd)
        cs.append((f"same-limbs{i}", a, a, tuple(w + w)))
    return tuple(cs)


def check_point(name, tag, w, want, with_t=True):
    """36 output limbs against the oracle's affine (x, y), projectively"""
    assert max(w) < RED, (name, tag, "limb >= 2^29 + 2^19", w)
    X, Y, Z, T = (val(w[9 * i:9 * i + 9]) % P for i in range(4))
    x, y = want
    assert Z != 0, (name, tag, "Z == 0")
    assert X == x * Z % P, (name, tag, "X != x Z")
    assert Y == y * Z % P, (name, tag, "Y != y Z")
    if with_t:
        assert T * Z % P == X * Y % P, (name, tag, "T Z != X Y")
    else:
        assert not any(w[27:]), (name, tag, "T not zero")
    return X, Y, Z, T


def check_quad(name, tag, w, want):
    copies = [w[36 * i:36 * i + 36] for i in range(4)]
    assert copies[1] == copies[0] and copies[2] == copies[0] and copies[3] == copies[0], (name, tag, "lanes differ")
    return check_point(name, tag, copies[0], want)


def expected_double(oracle, a, k=1):
    pt = ext(a)
    for _ in range(k):
        pt = oracle.double(pt)
    return affine(pt)


def test_lane_doubling(dc):
    oracle = source_points()[0]
    cs = dbl_cases()
    words = [list(w) for _, _, w in cs]
    for name, with_t in (("ge_dbl_t", True), ("ge_dbl_not", False)):
        outs = run(dc, name, words)
        for (t, a, _), o in zip(cs, outs):
            check_point(name, t, o, expected_double(oracle, a), with_t)


def test_doubling_layouts(dc):
    """quad_dbl, quad_dbl_d and row_dbl against the oracle, and the headers' promise that the three
    layouts hold the same field element in every coordinate"""
    oracle = source_points()[0]
    cs = dbl_cases()
    words = [list(w) for _, _, w in cs]
    got = {}
    for name in ("quad_dbl", "quad_dbl_d"):
        outs = run(dc, name, words)
        got[name] = [check_quad(name, t, o, expected_double(oracle, a)) for (t, a, _), o in zip(cs, outs)]
    outs = run(dc, "row_dbl_k", [w + [1] for w in words], key="k1")
    got["row_dbl"] = [check_point("row_dbl", t, o, expected_double(oracle, a)) for (t, a, _), o in zip(cs, outs)]
    for i, (t, _, _) in enumerate(cs):
        assert got["quad_dbl"][i] == got["quad_dbl_d"][i], (t, "quad_dbl_d != quad_dbl")
        assert got["quad_dbl"][i] == got["row_dbl"][i], (t, "row_dbl != quad_dbl")


@pytest.mark.parametrize("k", CHAIN_K)
def test_row_repeated_doubling(dc, k):
    oracle = source_points()[0]
    cs = dbl_cases()
    outs = run(dc, "row_dbl_k", [list(w) + [k] for _, _, w in cs], key=f"k{k}")
    for (t, a, _), o in zip(cs, outs):
        check_point(f"row_dbl x{k}", t, o, expected_double(oracle, a, k))


def expected_sum(oracle, a, b, k=0):
    pt = ext(a)
    for _ in range(k):
        pt = oracle.double(pt)
    return affine(oracle.add(pt, ext(b)))


def test_lane_additions(dc):
    oracle = source_points()[0]
    cs = add_cases(False)
    outs = run(dc, "ge_add_cached", [list(w) for *_, w in cs])
    for (t, a, b, _), o in zip(cs, outs):
        check_point("ge_add_cached", t, o, expected_sum(oracle, a, b))
    cs = add_cases(True)
    words = [list(w) for *_, w in cs]
    for name, sign in (("ge_madd_pos", False), ("ge_madd_neg", True)):
        outs = run(dc, name, words)
        for (t, a, b, _), o in zip(cs, outs):
            check_point(name, t, o, expected_sum(oracle, a, affine(oracle.neg(ext(b))) if sign else b))


def test_quad_madd(dc):
    oracle = source_points()[0]
    cs = add_cases(True)
    outs = run(dc, "quad_madd", [list(w) for *_, w in cs])
    for (t, a, b, _), o in zip(cs, outs):
        check_quad("quad_madd", t, o, expected_sum(oracle, a, b))


def test_addition_layouts(dc):
    """quad_add_cached, quad_add, quad_add_d and row_add against the oracle; the replicated quad, the
    distributed quad and the row layout hold the same field element in every coordinate; and
    row_cached's four rows are (Y - X, Y + X, Z, 2d T) with zeros on lanes 9..15"""
    oracle = source_points()[0]
    cs = add_cases(False)
    words = [list(w) for *_, w in cs]
    got = {}
    for name in ("quad_add_cached", "quad_add", "quad_add_d"):
        outs = run(dc, name, words)
        got[name] = [check_quad(name, t, o, expected_sum(oracle, a, b)) for (t, a, b, _), o in zip(cs, outs)]
    outs = run(dc, "row_add", words)
    got["row_add"] = [check_point("row_add", t, o[:36], expected_sum(oracle, a, b)) for (t, a, b, _), o in zip(cs, outs)]
    for i, (t, *_) in enumerate(cs):
        assert got["quad_add_cached"][i] == got["quad_add"][i], (t, "quad_add != quad_add_cached")
        assert got["quad_add_cached"][i] == got["quad_add_d"][i], (t, "quad_add_d != quad_add_cached")
        assert got["quad_add_cached"][i] == got["row_add"][i], (t, "row_add != quad_add_cached")
    for (t, _, _, w), o in zip(cs, outs):
        qx, qy, qz, qt = (val(w[36 + 9 * i:36 + 9 * i + 9]) for i in range(4))
        rows = [o[36 + 16 * i:36 + 16 * i + 16] for i in range(4)]
        want = [(qy - qx) % P, (qy + qx) % P, qz % P, D2 * qt % P]
        for r, e in zip(rows, want):
            assert val(r[:9]) % P == e, ("row_cached", t, rows)
            assert max(r[:9]) < RED and not any(r[9:]), ("row_cached", t, rows)


@pytest.mark.parametrize("k", CHAIN_K)
def test_row_horner_step(dc, k):
    """k doublings of P, then + Q: one step of horner_row / the tail of k_msm_slice"""
    oracle = source_points()[0]
    cs = add_cases(False)
    outs = run(dc, "row_horner", [list(w) + [k] for *_, w in cs])
    for (t, a, b, _), o in zip(cs, outs):
        check_point(f"row_horner k={k}", t, o, expected_sum(oracle, a, b, k))


# ---------------------------------------------------------------- arguments

def test_arguments(dc):
    buf = array("I", bytes(4 * 256))
    p = buf.buffer_info()[0]
    assert dc.dc_run(OP["fe_mul"], 0, None, 18, None, 9) == 0
    assert dc.dc_run(OP["row_add"], 0, p, 72, p, 100) == 0
    for bad_op in (-1, 12, 19, 25, 33, 46, 55, 1000):
        assert dc.dc_run(bad_op, 1, p, 18, p, 9) < 0
    assert dc.dc_run(OP["fe_mul"], 1, p, 17, p, 9) < 0
    assert dc.dc_run(OP["fe_mul"], 1, p, 18, p, 10) < 0
    assert dc.dc_run(OP["fe_mul"], 0, p, 9, p, 9) < 0
    assert dc.dc_run(OP["rf_mul"], 1, p, 18, p, 9) < 0
    assert dc.dc_run(OP["fe_mul"], (1 << 16) + 1, p, 18, p, 9) < 0
    assert dc.dc_run(OP["fe_mul"], 1, None, 18, p, 9) < 0
    assert all(w == 0 for w in buf)


def test_partial_last_block_and_neighbours(dc):
    """ncase that fills no whole block: every case still gets its own result (a value leaking across
    a row or quad boundary, or a slot past ncase being written, would show), and the same case gives
    the same words wherever it sits in the wave"""
    cs = mul_cases()[:37]
    words = [a + b for _, a, b in cs]
    whole = run(dc, "rf_mul", [a + b for _, a, b in mul_cases()], key="mul")
    part = run(dc, "rf_mul", words)
    assert part == whole[:37]
    moved = run(dc, "rf_mul", words[5:6] * 3 + words[:9])
    assert moved[0] == moved[1] == moved[2] == whole[5] and moved[3:] == whole[:9]
    dcs = dbl_cases()[:21]
    outs = run(dc, "quad_dbl_d", [list(w) for _, _, w in dcs])
    assert outs == run(dc, "quad_dbl_d", [list(w) for _, _, w in dbl_cases()])[:21]
    outs = run(dc, "row_dbl_k", [list(w) + [2] for _, _, w in dcs][:5])
    assert outs == run(dc, "row_dbl_k", [list(w) + [2] for _, _, w in dbl_cases()], key="k2")[:5]
