"""GPU: the device's integer scalar layer on chosen edge scalars (tests/golden/scalar_edges.json;
construction and census in tests/scalar_edges.py, checked on the CPU by test_scalar_edge_vectors.py).

The signed-window recodings (radix16_* and radix256_* of edc_single.hip, plan_digit / term_digits of
the Pippenger windows), the split of a coefficient at bit 128 and the coefficient pipeline of
edc_prep.hip (mul_128x256, the 64-bit limb sums, reduce_limb_sums, sc_reduce_wide, sc_sub,
sc_is_canonical) otherwise only ever see uniformly random scalars. Here valid prehashed items carry
chosen s and k, and batches carry chosen z, key coefficients and B coefficients: long carry ripples,
digits on their thresholds, coefficients equal to 0, l - 1 and 2^252, z = 0, z whose top window
becomes 2^bits. Every comparison is for equality with the big-integer oracle's stored values:
verdicts, [8]*check and the affine check point before the cofactor."""
import ctypes
import functools

import pytest

from conftest import golden

import scalar_edges as se

pytestmark = pytest.mark.gpu

FX = golden("scalar_edges.json")
KEYS = [bytes.fromhex(k) for k in FX["keys"]]
BATCHES = FX["batches"]
SEED = bytes.fromhex(FX["seed"])
IDENTITY = bytes([1]) + bytes(31)
P = 2**255 - 19
SHAPES = [(0, 0), (8, 1), (9, 1), (13, 1), (16, 1), (16, 2), (11, 16)]
NAMES = ("valid", "twin")


@pytest.fixture()
def knobs(engine):
    yield engine
    engine.set_msm_shape(0, 0)
    engine.set_key_grouping(0)
    engine.set_key_split(0)
    engine.keycache_clear()
    assert engine.lib.edc_set_fallback_shape(engine.ctx, 128, 9) == 0


def _cols(items):
    return [v for v, _, _ in items], [s for _, s, _ in items], [k for _, _, k in items]


def _zbytes(z):
    return b"".join(zi.to_bytes(16, "little") for zi in z)


@functools.lru_cache(maxsize=None)
def _case(bi, tag, name):
    """(items, z, (code, check8), (x, y)) of batch bi: tag "z" / "seeded", name "valid" / "twin"."""
    b = BATCHES[bi]
    items, z = se.variant_items(FX, b, tag)
    if name == "twin":
        items = se.twin_of(items, b[tag])
    e = b[tag][name]
    return items, z, (e["code"], bytes.fromhex(e["check8"])), (bytes.fromhex(e["x"]), bytes.fromhex(e["y"]))


def _all_cases(tag):
    return [(BATCHES[bi]["name"] + "/" + name,) + _case(bi, tag, name) for bi in range(len(BATCHES)) for name in NAMES]


def _affine(partial):
    X, Y, Z = (int.from_bytes(partial[32 * i:32 * i + 32], "little") for i in range(3))
    zi = pow(Z, P - 2, P)
    return (X * zi % P).to_bytes(32, "little"), (Y * zi % P).to_bytes(32, "little")


# ---------------------------------------------------------------- per-item paths
@pytest.fixture(scope="module")
def per_item():
    """(valid rows, rows interleaved with one near-miss each, the expected codes of the latter)."""
    rows = [(j, bytes.fromhex(sig), bytes.fromhex(k)) for j, sig, k in FX["per_item"]]
    mixed, expect = [], []
    for i, row in enumerate(rows):
        mixed += [row, se.near_miss(row, se.NEAR_KINDS[i % len(se.NEAR_KINDS)])]
        expect += [0, 1]
    return rows, mixed, expect


def _row_cols(rows):
    return [KEYS[j] for j, _, _ in rows], [s for _, s, _ in rows], [k for _, _, k in rows]


@pytest.mark.parametrize("cache", [False, True], ids=["single", "comb"])
def test_verify_each(knobs, per_item, cache):
    """k_verify_single, and k_verify_comb once the keys are registered."""
    _, mixed, expect = per_item
    if cache:
        knobs.keycache_load(KEYS[:se.NKEYS_PER_ITEM])
    assert knobs.verify_prehashed_each(*_row_cols(mixed)) == expect


@pytest.mark.parametrize("cache", [False, True], ids=["quad", "comb"])
def test_fallback_one_range(knobs, per_item, cache):
    """Below 2048 items the grouped fallback is one range; it fails, so every item goes through
    k_verify_quad (k_verify_comb with the keys registered)."""
    _, mixed, expect = per_item
    assert len(mixed) < 2048
    if cache:
        knobs.keycache_load(KEYS[:se.NKEYS_PER_ITEM])
    code, verdicts, nbad, _ = knobs.batch_verify_prehashed_fallback(*_row_cols(mixed), SEED)
    assert code == 1 and verdicts == expect and nbad == sum(expect)


@pytest.mark.parametrize("bits,cache", [(8, False), (13, False), (8, True)])
def test_fallback_two_ranges(knobs, per_item, bits, cache):
    """4096 items in two ranges with one near-miss each: the per-(range, key) and per-range B terms
    go through the range MSM, the items of the failing ranges through the per-item kernels."""
    rows, _, _ = per_item
    tiled = [rows[i % len(rows)] for i in range(4096)]
    expect = [0] * 4096
    for pos, kind in ((1000, "k+1"), (3000, "R+B")):
        tiled[pos] = se.near_miss(tiled[pos], kind)
        expect[pos] = 1
    assert knobs.lib.edc_set_fallback_shape(knobs.ctx, 2, bits) == 0
    if cache:
        knobs.keycache_load(KEYS[:se.NKEYS_PER_ITEM])
    code, verdicts, nbad, c8 = knobs.batch_verify_prehashed_fallback(*_row_cols(tiled), SEED)
    assert code == 1 and verdicts == expect and nbad == 2 and c8 != IDENTITY


# ---------------------------------------------------------------- the batch equation
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "c%d_p%d" % s)
def test_batch_equation_shapes(knobs, shape):
    """Every batch and its twin, caller z: the host call, the device call with d_z, and
    submit + wait with the check point before the cofactor; then z from the seed."""
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda:0")
    lib = knobs.lib
    knobs.set_msm_shape(*shape)
    for cid, items, z, exp, xy in _all_cases("z"):
        vks, sigs, ks = _cols(items)
        assert knobs.batch_verify_prehashed(vks, sigs, ks, z=_zbytes(z), want_check8=True) == exp, cid
        d = [torch.tensor(list(b"".join(x)), dtype=torch.uint8, device=dev) for x in (vks, sigs, ks)]
        d_z = torch.tensor(list(_zbytes(z)), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        ptr = [t.data_ptr() for t in d]
        c8 = ctypes.create_string_buffer(32)
        code = lib.edc_batch_verify_prehashed_device(knobs.ctx, len(items), *ptr, None, 0, d_z.data_ptr(), c8)
        assert (code, c8.raw) == exp, cid
        t = lib.edc_batch_submit_prehashed_device(knobs.ctx, len(items), *ptr, None, 0, d_z.data_ptr(), 1)
        assert t >= 0, cid
        c8, part, bad = ctypes.create_string_buffer(32), ctypes.create_string_buffer(128), ctypes.c_int(-1)
        code = lib.edc_batch_wait(knobs.ctx, t, c8, part, ctypes.byref(bad))
        assert (code, c8.raw) == exp and bad.value == 0, cid
        assert _affine(part.raw) == xy, cid
    for cid, items, z, exp, xy in _all_cases("seeded"):
        vks, sigs, ks = _cols(items)
        assert knobs.batch_verify_prehashed(vks, sigs, ks, z_seed=SEED, want_check8=True) == exp, cid
        t = knobs.batch_submit_prehashed(vks, sigs, ks, SEED, want_check8=True)
        assert knobs.batch_wait(t, want_check8=True) == exp, cid


@pytest.mark.parametrize("mode", [1, 2, 3])
def test_key_grouping_modes(knobs, mode):
    """Grouped keys, one key term per signature (z_i k_i mod l reduced per item) and the on-device
    overflow path."""
    knobs.set_key_grouping(mode)
    for tag, zkw in (("z", None), ("seeded", {"z_seed": SEED})):
        for cid, items, z, exp, _ in _all_cases(tag):
            kw = zkw or {"z": _zbytes(z)}
            assert knobs.batch_verify_prehashed(*_cols(items), want_check8=True, **kw) == exp, (cid, tag)


class _Draw:
    """Caller-drawn z for verify_detailed: 16 bytes per item in queue order."""

    def __init__(self, z):
        self.z, self.at = _zbytes(z), 0

    def fill_bytes(self, n):
        self.at += n
        return self.z[self.at - n:self.at]


def _queue3(sv, items):
    vks, sigs, ks = _cols(items)
    n = len(items)
    for a, b in ((0, n // 3), (n // 3, 2 * n // 3), (2 * n // 3, n)):
        sv.queue_many(vks[a:b], sigs[a:b], ks=ks[a:b])
    assert sv.batch_size == n


def test_stream_verifier_caller_z(knobs, edc):
    for cid, items, z, exp, _ in _all_cases("z"):
        sv = edc.batch.StreamVerifier(knobs)
        try:
            _queue3(sv, items)
            assert sv.verify_detailed(_Draw(z)) == exp, cid
        finally:
            sv.close()


def test_eager_verifier_seeded(knobs, edc):
    """The eager verifier takes no caller z: the k of every key was solved against z_values(seed)."""
    for cid, items, _, exp, _ in _all_cases("seeded"):
        sv = edc.batch.StreamVerifier(knobs)
        try:
            sv.set_fold(1)
            sv.begin_eager(SEED)
            _queue3(sv, items)
            assert sv.verify_detailed(None) == exp, cid
            assert sv.folded[0] > 0, cid
        finally:
            sv.close()


@pytest.mark.parametrize("key_split", [0, 1], ids=["split", "set_key_split_1"])
def test_split_coefficients(knobs, edc, key_split):
    """With the batch's keys registered the coefficients are cut at bit 128: the cut sees lo = 0,
    hi = 0, lo = 2^128 - 1 and 2^252. last_split proves which plan ran."""
    knobs.keycache_load(KEYS)
    knobs.set_key_split(key_split)
    for cid, items, z, exp, _ in _all_cases("z"):
        sv = edc.batch.StreamVerifier(knobs)
        try:
            _queue3(sv, items)
            assert sv.verify_detailed(_Draw(z)) == exp, cid
            assert sv.last_split == (0 if key_split else 1), cid
        finally:
            sv.close()
        for _ in range(2):       # the one-call path plans its split from the previous batch
            assert knobs.batch_verify_prehashed(*_cols(items), z=_zbytes(z), want_check8=True) == exp, cid


def test_zero_z_item_contributes_nothing(knobs):
    """An invalid item under z = 0 does not change the verdict (its k and s still pass the canonical
    checks): the batch stays Ok with the identity as [8]*check."""
    seen = 0
    for bi, b in enumerate(BATCHES):
        p = b["zero_z_pos"]
        if p is None:
            continue
        items, z, exp, _ = _case(bi, "z", "valid")
        assert z[p] == 0 and exp == (0, IDENTITY)
        for kind in ("R+B", "k+1", "s-1"):
            bad = list(items)
            j = KEYS.index(bad[p][0])
            _, sig, k = se.near_miss((j, bad[p][1], bad[p][2]), kind)
            bad[p] = (bad[p][0], sig, k)
            assert knobs.batch_verify_prehashed(*_cols(bad), z=_zbytes(z), want_check8=True) == exp, (b["name"], kind)
            assert knobs.verify_prehashed_each(*_cols(bad)) == [int(i == p) for i in range(len(bad))]
        seen += 1
    assert seen
