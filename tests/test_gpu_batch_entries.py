"""GPU: the plain batch entries against one another (include/edc.h): edc_batch_verify[_z|_device],
the prehashed forms, the six submit entries behind edc_batch_wait, the four fallback entries and the
per-item entries, on the same items, and what each of them accepts and refuses.

Every expected value is another entry's result in the same test; the entries themselves are held to
the oracle's fixtures in test_gpu_parity.py and test_gpu_prehashed.py. The shapes sit on the edges
the host code has: 0, 1, the quad / single threshold of the per-item pass (EDC_QUAD_VERIFY_MAX, read
from the source the library is built from), one k_coef workgroup (COEF_CHUNK) and three fallback
ranges. The chunked host path (n >= 2^16) has test_gpu_hostchunk.py. The last case is the
incremental verifier's fallback where the grouped fallback has to redo the batch's prefix."""
import ctypes
import os
import random
import re

import pytest

from conftest import PKG_DIR, golden

pytestmark = pytest.mark.gpu


def _constant(path, pattern):
    """the one number of `pattern` in a source file of the library (the default build's value)"""
    with open(os.path.join(PKG_DIR, "csrc", path)) as f:
        m = re.search(pattern, f.read())
    assert m, (path, pattern)
    return int(m.group(1))


QMAX = 1 << _constant("edc_api.hip", r"#define EDC_QUAD_VERIFY_MAX \(1u << (\d+)\)")
CHUNK = _constant("edc_common.h", r"constexpr uint32_t COEF_CHUNK = (\d+);")
NS = [0, 1, QMAX, QMAX + 1, CHUNK - 1, CHUNK + 1, 2 * CHUNK + 3]
SEED = bytes(range(7, 39))
NKEYS = 37
L = (1 << 252) + 27742317777372353535851937790883648493
ARG = -2


def _up(b, shift=0):
    import torch
    t = torch.frombuffer(bytearray(bytes(shift) + bytes(b) + bytes(16)), dtype=torch.uint8).to("cuda:0")
    torch.cuda.synchronize()
    return t[shift:]


def _flip(sig, at=40):
    return sig[:at] + bytes([sig[at] ^ 4]) + sig[at + 1:]


class Items:
    """n items signed by NKEYS signers in turn; forged: positions whose signature has one s bit flipped."""

    def __init__(self, eng, keys, n, forged=()):
        self.n = n
        self.who = [i % NKEYS for i in range(n)]
        self.msgs = [b"batch entries %d of %d" % (i, n) + b"." * (i % 5) for i in range(n)]
        self.vks, self.sigs = eng.sign([keys.seeds[w] for w in self.who], self.msgs) if n else ([], [])
        for i in forged:
            self.sigs[i] = _flip(self.sigs[i])
        self._ks = self._dev = None
        self.eng = eng

    @property
    def ks(self):
        if self._ks is None:
            self._ks = self.eng.challenge(self.vks, self.sigs, self.msgs)
        return self._ks

    def dev(self):
        if self._dev is None:
            import torch
            off = [0]
            for m in self.msgs:
                off.append(off[-1] + len(m))
            self._dev = dict(vk=_up(b"".join(self.vks)), sig=_up(b"".join(self.sigs)), msg=_up(b"".join(self.msgs)),
                             off=torch.tensor(off, dtype=torch.int64, device="cuda:0"), k=_up(b"".join(self.ks)))
            torch.cuda.synchronize()
        return {x: t.data_ptr() for x, t in self._dev.items()}


class Keys:
    def __init__(self, eng):
        rnd = random.Random("batch entries keys")
        self.seeds = [rnd.randbytes(32) for _ in range(NKEYS)]
        self.keys, _ = eng.sign(self.seeds, [b""] * NKEYS)


@pytest.fixture(scope="module")
def eng(edc):
    pytest.importorskip("torch")
    e = edc.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def cached(edc, keys):
    """a second context with the signers registered (the indexed submits) and an empty signature table"""
    e = edc.Engine(0)
    e.keycache_load(keys.keys)
    e.sigcache_create(1 << 16)
    yield e
    e.close()


@pytest.fixture(scope="module")
def keys(eng):
    return Keys(eng)


@pytest.fixture(scope="module")
def items(eng, keys):
    cache = {}

    def get(n, forged=()):
        if (n, forged) not in cache:
            cache[(n, forged)] = Items(eng, keys, n, forged)
        return cache[(n, forged)]
    return get


def _wait(eng, t):
    assert t >= 0, eng.lib.edc_last_error(eng.ctx)
    c8 = ctypes.create_string_buffer(32)
    return eng.lib.edc_batch_wait(eng.ctx, t, c8, None, None), c8.raw


def _sync_device(eng, name, *a):
    c8 = ctypes.create_string_buffer(32)
    return getattr(eng.lib, name)(eng.ctx, *a, c8), c8.raw


# ---------------------------------------------------------------- 1. / 2. the batch forms
@pytest.mark.parametrize("n,forge", [(n, False) for n in NS] + [(n, True) for n in NS if n],
                         ids=lambda v: {False: "valid", True: "forged"}.get(v, str(v)) if isinstance(v, bool) else str(v))
def test_batch_forms_agree(eng, cached, oracle, items, n, forge):
    it = items(n, tuple(sorted({0, n - 1})) if forge else ())
    D = it.dev()
    z = b"".join(v.to_bytes(16, "little") for v in oracle.z_values(SEED, n))
    lib, ctx = eng.lib, eng.ctx
    got = {
        "verify": eng.batch_verify(it.vks, it.sigs, it.msgs, z_seed=SEED, want_check8=True),
        "verify_z": eng.batch_verify(it.vks, it.sigs, it.msgs, z=z, want_check8=True),
        "verify_device": _sync_device(eng, "edc_batch_verify_device", n, D["vk"], D["sig"], D["msg"], D["off"], SEED, 0, None),
        "prehashed": eng.batch_verify_prehashed(it.vks, it.sigs, it.ks, z_seed=SEED, want_check8=True),
        "prehashed_device": _sync_device(eng, "edc_batch_verify_prehashed_device", n, D["vk"], D["sig"], D["k"], SEED, 0, None),
        "submit": eng.batch_wait(eng.batch_submit(it.vks, it.sigs, it.msgs, SEED, want_check8=True), True),
        "submit_prehashed": eng.batch_wait(eng.batch_submit_prehashed(it.vks, it.sigs, it.ks, SEED, want_check8=True), True),
        "submit_device": _wait(eng, lib.edc_batch_submit_device(ctx, n, D["vk"], D["sig"], D["msg"], D["off"], SEED, 0, None, 1)),
        "submit_prehashed_device": _wait(eng, lib.edc_batch_submit_prehashed_device(ctx, n, D["vk"], D["sig"], D["k"], SEED, 0, None, 1)),
        "submit_indexed": cached.batch_wait(cached.batch_submit_indexed(it.who, it.sigs, it.msgs, SEED, want_check8=True), True),
        "submit_prehashed_indexed": cached.batch_wait(
            cached.batch_submit_prehashed_indexed(it.who, it.sigs, it.ks, SEED, want_check8=True), True),
    }
    want = got["verify"]
    assert want[0] == (1 if forge else 0) and (forge or n or want[1] == bytes([1]) + bytes(31))
    for name, res in got.items():
        assert tuple(res) == tuple(want), (name, n)


# ---------------------------------------------------------------- 3. the fallback forms
def _bad_items(eng, keys, items, n, forged):
    """the forged items of `forged`, an undecodable key at 2 and a non-canonical s (s + l) at 5"""
    it = items(n, forged)
    bad_key = bytes.fromhex(next(c["enc"] for c in golden("decode.json")["cases"] if not c["ok"]))
    vks, sigs = list(it.vks), list(it.sigs)
    vks[2] = bad_key
    s = int.from_bytes(sigs[5][32:], "little") + L
    sigs[5] = sigs[5][:32] + s.to_bytes(32, "little")
    out = Items(eng, keys, 0)
    out.n, out.who, out.msgs, out.vks, out.sigs = n, it.who, it.msgs, vks, sigs
    return out


def _each_forms(eng, cached, it):
    import torch
    D = it.dev()
    out = torch.full((max(it.n, 1),), 7, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    assert eng.lib.edc_verify_each_device(eng.ctx, it.n, D["vk"], D["sig"], D["msg"], D["off"], out.data_ptr()) == 0
    res = {"each": eng.verify_each(it.vks, it.sigs, it.msgs), "each_device": out.cpu().tolist()[:it.n],
           "prehashed_each": eng.verify_prehashed_each(it.vks, it.sigs, it.ks)}
    for form in ("msgs", "ks"):
        cached.sigcache_clear()
        codes, miss = cached.verify_each_cached(it.vks, it.sigs, **{form: getattr(it, form)})
        assert miss == it.n
        res["sigcache_each_" + form] = codes
    cached.sigcache_clear()
    return res


@pytest.mark.parametrize("n", [CHUNK + 1, 2 * CHUNK + 3])
def test_fallback_forms_agree(eng, cached, keys, items, n):
    forged = tuple(sorted({0, CHUNK // 2, CHUNK - 1, n - CHUNK // 3, n - 1}))       # range ends, a middle, both batch ends
    it = _bad_items(eng, keys, items, n, forged)
    D = it.dev()
    each = _each_forms(eng, cached, it)
    codes = each["each"]
    assert [i for i, c in enumerate(codes) if c] == sorted(set(forged) | {2, 5})
    for name, res in each.items():
        assert res == codes, name

    def raw(e, name, *a, tail=()):
        v, cnt, c8 = ctypes.create_string_buffer(n), ctypes.c_int(-1), ctypes.create_string_buffer(32)
        rc = getattr(e.lib, name)(e.ctx, n, *a, SEED, v, ctypes.byref(cnt), c8, *tail)
        return rc, list(v.raw), cnt.value, c8.raw

    miss = ctypes.c_size_t(0)
    cached.sigcache_clear()
    got = {
        "fallback_device": raw(eng, "edc_batch_verify_fallback_device", D["vk"], D["sig"], D["msg"], D["off"]),
        "prehashed_fallback": eng.batch_verify_prehashed_fallback(it.vks, it.sigs, it.ks, SEED),
        "prehashed_fallback_device": raw(eng, "edc_batch_verify_prehashed_fallback_device", D["vk"], D["sig"], D["k"]),
        "sigcache_fallback_device": raw(cached, "edc_sigcache_batch_verify_fallback_device", D["vk"], D["sig"], None, None, D["k"],
                                        tail=(ctypes.byref(miss),)),
    }
    cached.sigcache_clear()
    assert miss.value == n
    want = got["fallback_device"]
    assert want[:3] == (1, codes, len(forged) + 2)
    for name, res in got.items():
        assert tuple(res) == want, name


# ---------------------------------------------------------------- 4. the per-item forms
@pytest.mark.parametrize("n", [QMAX, QMAX + 1])
def test_each_forms_agree(eng, cached, keys, items, n):
    it = _bad_items(eng, keys, items, n, (0, n - 1))
    each = _each_forms(eng, cached, it)
    assert [i for i, c in enumerate(each["each"]) if c] == [0, 2, 5, n - 1]
    for name, res in each.items():
        assert res == each["each"], name


# ---------------------------------------------------------------- 5. what each entry accepts and refuses
def _err(e):
    return e.lib.edc_last_error(e.ctx).decode()


def test_empty_batches(eng):
    c8 = ctypes.create_string_buffer(32)
    assert eng.lib.edc_batch_verify_z(eng.ctx, 0, None, None, None, (ctypes.c_uint64 * 1)(0), None, c8) == 0      # null z
    assert c8.raw == bytes([1]) + bytes(31)
    assert eng.lib.edc_batch_verify_z(eng.ctx, 1, b"\0" * 32, b"\0" * 64, b"\0", (ctypes.c_uint64 * 2)(0, 0), None, c8) == ARG
    c8 = ctypes.create_string_buffer(32)
    assert eng.lib.edc_batch_verify_prehashed(eng.ctx, 0, None, None, None, SEED, None, c8) == 0                 # reads no input
    assert c8.raw == bytes([1]) + bytes(31)


def test_refusals_write_nothing_and_take_no_ticket(edc, keys, items):
    it = items(CHUNK - 1)
    D = it.dev()
    vk, sig, k = b"".join(it.vks), b"".join(it.sigs), b"".join(it.ks)
    n = it.n
    e = edc.Engine(0)
    try:
        e.keycache_load(keys.keys)
        e.sigcache_create(1 << 12)
        lib, ctx = e.lib, e.ctx
        odd_k, odd_z = _up(k, shift=8).data_ptr(), _up(bytes(16 * n), shift=8).data_ptr()
        good = e.batch_verify(it.vks, it.sigs, it.msgs, z_seed=SEED, want_check8=True)

        def ticket():
            t = lib.edc_batch_submit_prehashed_device(ctx, n, D["vk"], D["sig"], D["k"], SEED, 0, None, 1)
            assert _wait(e, t) == tuple(good)
            return t

        # misaligned d_k / d_z: refused before the device is touched
        for dk, dz in ((odd_k, None), (D["k"], odd_z)):
            c8 = ctypes.create_string_buffer(b"\x77" * 32, 32)
            assert lib.edc_batch_verify_prehashed_device(ctx, n, D["vk"], D["sig"], dk, SEED, 0, dz, c8) == ARG
            assert c8.raw == b"\x77" * 32 and _err(e) == "d_k / d_z must be 16-byte aligned"
            t0 = ticket()
            assert lib.edc_batch_submit_prehashed_device(ctx, n, D["vk"], D["sig"], dk, SEED, 0, dz, 1) == ARG
            assert _err(e) == "d_k / d_z must be 16-byte aligned"
            assert ticket() == t0 + 1
        v, cnt, c8 = ctypes.create_string_buffer(b"\x77" * n, n), ctypes.c_int(0x77), ctypes.create_string_buffer(b"\x77" * 32, 32)
        assert lib.edc_batch_verify_prehashed_fallback_device(ctx, n, D["vk"], D["sig"], odd_k, SEED, v, ctypes.byref(cnt), c8) == ARG
        assert (v.raw, cnt.value, c8.raw) == (b"\x77" * n, 0x77, b"\x77" * 32) and _err(e) == "d_k must be 16-byte aligned"

        # an index past the registered list: refused before a slot is claimed
        past = [NKEYS] + it.who[1:]
        for submit, last in ((e.batch_submit_indexed, it.msgs), (e.batch_submit_prehashed_indexed, it.ks)):
            t0 = ticket()
            with pytest.raises(edc.EngineError, match="edc error -2: key index outside the registered key list"):
                submit(past, it.sigs, last, SEED)
            assert ticket() == t0 + 1
            assert e.batch_wait(submit(it.who, it.sigs, last, SEED, want_check8=True), True) == good

        # a k that is no canonical scalar: the per-item entries refuse it on the host, the batch entries at the wait
        for bad in (b"\xff" * 32, L.to_bytes(32, "little")):
            ks = list(it.ks)
            ks[n // 2] = bad
            kb = b"".join(ks)
            out = ctypes.create_string_buffer(b"\x77" * n, n)
            assert lib.edc_verify_prehashed_each(ctx, n, vk, sig, kb, out) == ARG
            assert out.raw == b"\x77" * n and _err(e) == "prehashed k is not a canonical scalar"
            miss = ctypes.c_size_t(0x77)
            assert lib.edc_sigcache_verify_each(ctx, n, vk, sig, None, None, kb, out, ctypes.byref(miss)) == ARG
            assert (out.raw, miss.value) == (b"\x77" * n, 0x77) and _err(e) == "prehashed k is not a canonical scalar"
            at_wait = "edc error -2: prehashed k is not a canonical scalar \\(must be < l"
            with pytest.raises(edc.EngineError, match=at_wait):
                e.batch_verify_prehashed(it.vks, it.sigs, ks, z_seed=SEED)
            with pytest.raises(edc.EngineError, match=at_wait):
                e.batch_wait(e.batch_submit_prehashed(it.vks, it.sigs, ks, SEED))
            with pytest.raises(edc.EngineError, match=at_wait):
                e.batch_verify_prehashed_fallback(it.vks, it.sigs, ks, SEED)
        assert e.verify_prehashed_each(it.vks, it.sigs, it.ks) == [0] * n

        # the slots: a synchronous call needs slot 0, a submission the slot of the next ticket
        assert lib.edc_set_slots(ctx, 2) == 0                                         # two slots, the next ticket is 0
        held = [e.batch_submit(it.vks, it.sigs, it.msgs, SEED, want_check8=True) for _ in range(2)]
        assert held == [0, 1]
        c8 = ctypes.create_string_buffer(b"\x77" * 32, 32)
        assert lib.edc_batch_verify_prehashed_device(ctx, n, D["vk"], D["sig"], D["k"], SEED, 0, None, c8) == ARG
        assert c8.raw == b"\x77" * 32 and _err(e) == "slot 0 busy: wait for submitted batches first"
        for name in ("edc_batch_submit_device", "edc_batch_submit_prehashed_device"):
            a = (D["msg"], D["off"]) if name == "edc_batch_submit_device" else (D["k"],)
            assert getattr(lib, name)(ctx, n, D["vk"], D["sig"], *a, SEED, 0, None, 1) == ARG
            assert _err(e) == "all slots in flight: wait for the oldest ticket first"
        with pytest.raises(edc.EngineError, match="all slots in flight"):
            e.batch_submit_prehashed(it.vks, it.sigs, it.ks, SEED)
        assert [e.batch_wait(t, True) for t in held] == [good, good]
        assert ticket() == held[1] + 1
    finally:
        e.close()


# ---------------------------------------------------------------- 6. the verifier's fallback after a redone prefix
def _item_cap(n):
    """csrc/devbuf.h: what a fresh verifier's slot holds once n items are queued in one call"""
    return 1024 if n < 1024 else n + n // 8


def _ranges(n, ranges):
    """fallback_geometry of edc_api.hip for a range target below its cap: (items per range, G)"""
    rsize = -(-(-(-n // ranges)) // CHUNK) * CHUNK
    return rsize, -(-n // rsize)


def test_verifier_fallback_after_a_redone_prefix(edc):
    """With every key distinct (m = n) the per-(range, key) sums of the grouped fallback need G * m
    slots, and a verifier's slot has item_cap(n): from the first n with two ranges on, G * m > cap_n,
    so fallback_ranges redoes the prefix with one key term per signature on the verifier's own slot
    and the verifier has to rebuild its grouped key state before the next verify."""
    ranges = 2
    n = next(n for n in range(1, 4 * CHUNK) if _ranges(n, ranges)[1] * n > _item_cap(n))
    assert n == CHUNK + 1 and _ranges(n, ranges) == (CHUNK, 2)
    e = edc.Engine(0)
    try:
        assert e.lib.edc_set_fallback_shape(e.ctx, ranges, 9) == 0
        rnd = random.Random("batch entries redo")
        msgs = [b"redo %d" % i for i in range(n)]
        vks, sigs = e.sign([rnd.randbytes(32) for _ in range(n)], msgs)
        assert len(set(vks)) == n
        good = e.batch_verify(vks, sigs, msgs, z_seed=SEED, want_check8=True)
        sigs[n - 7] = _flip(sigs[n - 7])
        codes = e.verify_each(vks, sigs, msgs)
        assert codes == [0] * (n - 7) + [1] + [0] * 6
        want = e.batch_verify(vks, sigs, msgs, z_seed=SEED, want_check8=True)
        sv = edc.batch.StreamVerifier(e)
        assert not sv.cached
        sv.queue_many(vks, sigs, msgs=msgs)
        assert sv.verify_with_fallback(SEED) == (1, codes, want[1])
        assert sv.verify_detailed(SEED) == want and want[0] == 1 and want != good     # the grouped key state is back
        assert sv.verify_with_fallback(SEED) == (1, codes, want[1])
        sv.close()
    finally:
        e.close()
