"""GPU: every verification path on mixed-order keys (tests/golden/mixed_order.json; construction in
tests/mixed_order.py, checked on the CPU by test_mixed_order_vectors.py), and the point decoder on
edge encodings (tests/golden/decode_edges.json).

A mixed-order key A = [a]B + T_t lies outside both the prime-order and the torsion subgroup. Under a
valid signature with s != 0, [s]B - [k]A - R is the torsion point -(k T_t + T_u): only the final
multiplication by the cofactor makes the item verify, for every k mod 8, and only it makes [c mod l]A
(the reduced key coefficient of a batch), the comb table of a registered key, its [2^128]A multiple
and a shard's partial agree with [c]A. ZIP215 promises one verdict from every path, so every result
here is held to the fixture exactly: per-item codes (k_verify_single, k_verify_comb, k_verify_quad),
(code, [8]*check) of the batch in every grouping mode with keys unregistered, registered and split,
shard partials recombined, and the cached, incremental and commit-set forms."""
import ctypes
import functools

import pytest

from conftest import golden

import mixed_order as mo

pytestmark = pytest.mark.gpu

FX = golden("mixed_order.json")
EDGES = golden("decode_edges.json")["cases"]
SEED = bytes.fromhex(FX["seed"])
KEYS = [bytes.fromhex(k) for k in FX["keys"]]
NAMES = sorted(FX["batches"])
IDENTITY = bytes([1]) + bytes(31)


@functools.lru_cache(maxsize=None)
def _batch(name):
    """(form, items [(vk, sig, msg or k)], per-item codes, (code, check8))"""
    return mo.fixture_batch(FX, name)


@pytest.fixture()
def knobs(engine):
    yield engine
    engine.set_msm_shape(0, 0)
    engine.set_key_grouping(0)
    engine.set_key_split(0)
    engine.keycache_clear()


def _register(eng):
    u, ok = eng.keycache_load(KEYS)
    assert u == len(KEYS) and all(ok)


def _cols(items):
    return [a for a, _, _ in items], [b for _, b, _ in items], [c for _, _, c in items]


def _dev(form, items):
    """The items in device memory: [vk, sig, msg, msg_off] or [vk, sig, k] tensors."""
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda:0")
    vks, sigs, cs = _cols(items)
    d = [torch.tensor(list(b"".join(x)) or [0], dtype=torch.uint8, device=dev) for x in (vks, sigs, cs)]
    if form == "msg":
        offs = [0]
        for m in cs:
            offs.append(offs[-1] + len(m))
        d.append(torch.tensor(offs, dtype=torch.int64, device=dev))
    torch.cuda.synchronize()
    return d


def _ptrs(d):
    return [t.data_ptr() for t in d]


def _host_call(eng, form, items):
    fn = eng.batch_verify if form == "msg" else eng.batch_verify_prehashed
    return fn(*_cols(items), z_seed=SEED, want_check8=True)


def _host_submit_wait(eng, form, items):
    fn = eng.batch_submit if form == "msg" else eng.batch_submit_prehashed
    return eng.batch_wait(fn(*_cols(items), SEED, want_check8=True), want_check8=True)


def _device_call(eng, form, d, n):
    fn = eng.lib.edc_batch_verify_device if form == "msg" else eng.lib.edc_batch_verify_prehashed_device
    c8 = ctypes.create_string_buffer(32)
    code = fn(eng.ctx, n, *_ptrs(d), SEED, 0, None, c8)
    return code, c8.raw


def _device_submit_wait(eng, form, d, n, z_base=0):
    """-> ((code, check8), partial, bad) of submit + wait on device-resident items at global index z_base."""
    fn = eng.lib.edc_batch_submit_device if form == "msg" else eng.lib.edc_batch_submit_prehashed_device
    t = fn(eng.ctx, n, *_ptrs(d), SEED, z_base, None, 1)
    assert t >= 0
    c8, part, bad = ctypes.create_string_buffer(32), ctypes.create_string_buffer(128), ctypes.c_int(-1)
    code = eng.lib.edc_batch_wait(eng.ctx, t, c8, part, ctypes.byref(bad))
    return (code, c8.raw), part.raw, bad.value


def _each(eng, form, items, d=None):
    """Per-item codes: edc_verify_each_device for messages, edc_verify_prehashed_each for prehashed items."""
    if form == "pre":
        return eng.verify_prehashed_each(*_cols(items))
    torch = pytest.importorskip("torch")
    d = d or _dev(form, items)
    out = torch.full((len(items),), 7, dtype=torch.uint8, device=d[0].device)
    torch.cuda.synchronize()
    assert eng.lib.edc_verify_each_device(eng.ctx, len(items), *_ptrs(d), out.data_ptr()) == 0
    return out.cpu().tolist()


def _fallback(eng, form, items):
    """(code, per-item codes, number invalid, check8) of the batch with its grouped fallback."""
    if form == "pre":
        return eng.batch_verify_prehashed_fallback(*_cols(items), SEED)
    d = _dev(form, items)
    n = len(items)
    v, cnt, c8 = ctypes.create_string_buffer(n), ctypes.c_int(0), ctypes.create_string_buffer(32)
    rc = eng.lib.edc_batch_verify_fallback_device(eng.ctx, n, *_ptrs(d), SEED, v, ctypes.byref(cnt), c8)
    return rc, list(v.raw), cnt.value, c8.raw


# ---------------------------------------------------------------- per-item kernels
@pytest.mark.parametrize("cache", [False, True], ids=["single", "comb"])
@pytest.mark.parametrize("name", NAMES)
def test_verify_each(knobs, name, cache):
    """k_verify_single on [1..8](-A) of a mixed-order A; k_verify_comb on its 512 comb records once
    the keys are registered."""
    form, items, codes, _ = _batch(name)
    if cache:
        _register(knobs)
    assert _each(knobs, form, items) == codes


@pytest.mark.parametrize("cache", [False, True], ids=["quad", "comb"])
@pytest.mark.parametrize("name", NAMES)
def test_batch_with_fallback(knobs, name, cache):
    """The batch and, when a defect fails it, the grouped fallback: below 2048 items it is one range,
    so every item goes through k_verify_quad (k_verify_comb with the keys registered). The batch
    verdict, the per-item codes and the count agree as ZIP215 requires."""
    form, items, codes, (code, c8) = _batch(name)
    assert len(items) < 2048
    if cache:
        _register(knobs)
    assert _fallback(knobs, form, items) == (code, codes, sum(codes), c8)
    assert code == int(any(codes))


# ---------------------------------------------------------------- the batch equation
@pytest.mark.parametrize("keys", ["unregistered", "split", "unsplit"])
@pytest.mark.parametrize("grouping", [0, 2, 3])
def test_batch_every_entry(knobs, grouping, keys):
    """Every batch through the host call, the device call and submit + wait (host and device), in
    grouping modes 0 (keys grouped: sum z k mod l per mixed-order key), 2 (one key term per
    signature) and 3 (grouping abandoned on the device), with the keys unregistered, registered
    with coefficients split at bit 128 onto the cached [2^128]A, and registered without the split."""
    knobs.set_key_grouping(grouping)
    if keys != "unregistered":
        _register(knobs)
        knobs.set_key_split(0 if keys == "split" else 1)
    for rep in range(2 if keys == "split" else 1):      # the one-call path plans its split from the previous batch
        for name in NAMES:
            form, items, _, exp = _batch(name)
            d = _dev(form, items)
            tag = (name, rep)
            assert _host_call(knobs, form, items) == exp, tag
            assert _device_call(knobs, form, d, len(items)) == exp, tag
            assert _host_submit_wait(knobs, form, items) == exp, tag
            got, _, bad = _device_submit_wait(knobs, form, d, len(items))
            assert got == exp and bad == 0, tag


@pytest.mark.parametrize("shape", [(8, 1), (13, 1), (16, 2)], ids=lambda s: "c%d_p%d" % s)
def test_batch_window_shapes(knobs, shape):
    """Other Pippenger window widths and parts, keys unregistered and registered (split)."""
    knobs.set_msm_shape(*shape)
    for registered in (False, True):
        if registered:
            _register(knobs)
        for name in NAMES:
            form, items, _, exp = _batch(name)
            for _ in range(2 if registered else 1):
                assert _host_call(knobs, form, items) == exp, (name, registered)


@pytest.mark.parametrize("key_split", [0, 1], ids=["split", "set_key_split_1"])
def test_incremental_verifier_registered_keys(knobs, edc, key_split):
    """The incremental verifier with every key registered; last_split proves which plan ran."""
    _register(knobs)
    knobs.set_key_split(key_split)
    for name in NAMES:
        form, items, codes, exp = _batch(name)
        sv = edc.batch.StreamVerifier(knobs)
        try:
            _queue3(sv, form, items)
            assert sv.verify_detailed(SEED) == exp, name
            assert sv.last_split == (0 if key_split else 1), name
            assert sv.verify_with_fallback(SEED) == (exp[0], codes, exp[1]), name
        finally:
            sv.close()


# ---------------------------------------------------------------- shards
@pytest.mark.parametrize("registered", [False, True], ids=["unregistered", "registered"])
@pytest.mark.parametrize("nshards", [2, 4])
def test_shards_recombine(knobs, nshards, registered):
    """Each shard's partial keeps its torsion residue (no cofactor before the combine); the partials
    of 2 and 4 shards at global z offsets sum to the whole batch's [8]*check. Messages through
    edc_batch_partial_device, prehashed items through submit + wait's partial."""
    if registered:
        _register(knobs)
    for name in NAMES:
        form, items, _, exp = _batch(name)
        n = len(items)
        bounds = [n * s // nshards for s in range(nshards + 1)]
        parts, bad_any = [], 0
        for lo, hi in zip(bounds, bounds[1:]):
            d = _dev(form, items[lo:hi])
            if form == "msg":
                part, flag = ctypes.create_string_buffer(128), ctypes.c_int(-1)
                assert knobs.lib.edc_batch_partial_device(knobs.ctx, hi - lo, *_ptrs(d), SEED, lo, None, part,
                                                          ctypes.byref(flag)) == 0
                part, flag = part.raw, flag.value
            else:
                _, part, flag = _device_submit_wait(knobs, form, d, hi - lo, z_base=lo)
            assert flag == 0
            parts.append(part)
            bad_any |= flag
        assert knobs.combine_partials(parts, bad_any) == exp, name
        assert knobs.combine_partials(parts[::-1], bad_any) == exp, name


# ---------------------------------------------------------------- compositions
def _queue3(sv, form, items):
    vks, sigs, cs = _cols(items)
    n = len(items)
    for a, b in ((0, n // 3), (n // 3, 2 * n // 3), (2 * n // 3, n)):
        kw = {"msgs": cs[a:b]} if form == "msg" else {"ks": cs[a:b]}
        sv.queue_many(vks[a:b], sigs[a:b], **kw)
    assert sv.batch_size == n


@pytest.mark.parametrize("eager", [False, True], ids=["lazy", "eager"])
def test_incremental_verifier(knobs, edc, eager):
    """Queued in three pieces; in eager mode the [z]R terms (R with torsion) are folded at queue time."""
    for name in NAMES:
        form, items, codes, exp = _batch(name)
        sv = edc.batch.StreamVerifier(knobs)
        try:
            if eager:
                sv.set_fold(1)
                sv.begin_eager(SEED)
            _queue3(sv, form, items)
            assert sv.verify_detailed(None if eager else SEED) == exp, name
            if not eager:
                assert sv.verify_with_fallback(SEED) == (exp[0], codes, exp[1]), name
        finally:
            sv.close()


def test_verified_signature_cache(knobs):
    """Feed, then batch again: the valid items become hits, a defect makes its item a miss again, and
    hits and misses give the verdicts of the uncached paths. The misses alone are the batch, drawing
    z in their own queue order."""
    knobs.sigcache_create(1024)
    try:
        for valid, form, kw in (("msg_valid", "msg", "msgs"), ("pre_valid", "pre", "ks")):
            _, items, codes, _ = _batch(valid)
            vks, sigs, cs = _cols(items)
            n = len(items)
            if form == "msg":
                assert knobs.batch_verify_cached(vks, sigs, z_seed=SEED, **{kw: cs}) == (0, IDENTITY, n)
            else:
                assert knobs.verify_each_cached(vks, sigs, **{kw: cs}) == (codes, n)
            assert knobs.batch_verify_cached(vks, sigs, z_seed=SEED, **{kw: cs}) == (0, IDENTITY, 0)
            assert knobs.verify_each_cached(vks, sigs, **{kw: cs}) == (codes, 0)
            for name in NAMES:
                f, bad_items, bad_codes, _ = _batch(name)
                defects = [(pos, int.from_bytes(bytes.fromhex(d), "little")) for pos, d in FX["batches"][name]["defects"]]
                if f != form or not defects:
                    continue
                vks, sigs, cs = _cols(bad_items)
                z = mo.o.z_values(SEED, len(defects))
                c8 = mo.defect_check8(z, [(m, delta) for m, (_, delta) in enumerate(sorted(defects))])
                assert knobs.batch_verify_cached(vks, sigs, z_seed=SEED, **{kw: cs}) == (1, c8, len(defects)), name
                assert knobs.verify_each_cached(vks, sigs, **{kw: cs}) == (bad_codes, len(defects)), name
    finally:
        knobs.sigcache_create(0)


@pytest.mark.parametrize("registered", [False, True], ids=["unregistered", "registered"])
def test_commit_set(knobs, registered):
    """Two commits of 16 votes each, mixed-order validators among honest ones (the message items of
    t = 0, 1 and of t = 4, 5): both valid, then the second with one defect. Message and prehashed forms."""
    if registered:
        _register(knobs)
    for valid, bad, pos, kw in (("msg_valid", "msg_defect", 42, "msgs"), ("pre_valid", "pre_defects", 37, "ks")):
        lo = pos - pos % 16
        good_items, bad_items = _batch(valid)[1], _batch(bad)[1]
        assert _batch(bad)[2][lo:lo + 16] == [int(lo + i == pos) for i in range(16)]
        for second, verdicts in ((good_items, [0, 0]), (bad_items, [0, 1])):
            vks, sigs, cs = _cols(good_items[:16] + second[lo:lo + 16])
            codes = [0] * 16 + [int(verdicts[1] and lo + i == pos) for i in range(16)]
            got = knobs.commits_verify([0, 16, 32], sigs, SEED, vks=vks, **{kw: cs})
            assert got == (verdicts[1], verdicts, codes, sum(verdicts)), (bad, verdicts)


# ---------------------------------------------------------------- decode edges
ENCS = [bytes.fromhex(c["enc"]) for c in EDGES]


def test_decompress_edges(engine):
    got = engine.decompress(ENCS)
    for c, (ok, x, y) in zip(EDGES, got):
        assert ok == c["ok"], c["enc"]
        if ok:
            assert (x.hex(), y.hex()) == (c["x"], c["y"]), c["enc"]


def test_key_ingestion_edges(knobs):
    """edc_vk_validate and the key cache's per-key ok flags on every edge encoding."""
    assert knobs.vk_validate(ENCS) == [0 if c["ok"] else 2 for c in EDGES]
    _, ok = knobs.keycache_load(ENCS)
    assert ok == [c["ok"] for c in EDGES]


def test_verify_each_on_edge_encodings(knobs, oracle):
    """Every rejected encoding once as A (MalformedPublicKey) and once as R (InvalidSignature), and
    a dozen accepted edge encodings as A under a signature made for another key (InvalidSignature,
    not MalformedPublicKey). The expected codes are the oracle's."""
    vk, sig, msg = _batch("msg_valid")[1][0]
    rejected = [e for e, c in zip(ENCS, EDGES) if not c["ok"]]
    accepted = [e for e, c in zip(ENCS, EDGES) if c["ok"]]
    accepted = accepted[::max(1, len(accepted) // 12)][:12]
    assert len(rejected) >= 14 and len(accepted) == 12
    items = [(e, sig, msg) for e in rejected] + [(vk, e + sig[32:], msg) for e in rejected]
    items += [(e, sig, msg) for e in accepted] + [(vk, sig, msg)]
    expect = [2] * len(rejected) + [1] * len(rejected) + [1] * 12 + [0]
    assert [oracle.verify(*it) for it in items] == expect
    assert _each(knobs, "msg", items) == expect
