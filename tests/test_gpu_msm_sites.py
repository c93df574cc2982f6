"""GPU: the six places of edc_api.hip that enqueue the MSM chain (binning, sort, accumulation, tail)
on a slot's workspace (MsmWs, edc_launch.h), each driven once per engine at the smallest shape that
reaches its own code: the one-batch path (enqueue_prefix / enqueue_batch), the multi launch
(enqueue_multi), the chunked host path (enqueue_host_chunked), the grouped fallback
(fallback_ranges), the eager fold (verifier_fold) and the incremental verify
(verifier_enqueue_verify).

Every case is checked two ways: verdict and [8]*check byte for byte against edc_batch_verify_device
on the same items and z seed, and the verdict against oracle/ed25519_ref.py. The oracle evaluates
the batch equation itself up to 2,049 items per batch (about half a second). Beyond that, at 2^16
and at the fallback's 4,097 items, its verdict comes from what it can evaluate in a few seconds and
from ZIP215's agreement of batch and single verification, which the oracle's own fixtures hold it
to: a batch holding an item that oracle.verify rejects is invalid, and every item of a batch whose
equation holds under the oracle verifies singly."""
import ctypes
import os
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

SEED = bytes(range(0x40, 0x60))
IDENTITY = bytes([1]) + bytes(31)
MLEN = 32
CHUNK = 2048          # COEF_CHUNK (edc_common.h)
HOST_CHUNK_MIN = 1 << 16


class Work:
    """n items of bench.make_workload on the device (signers = 0: distinct keys), 32-byte messages;
    forged: positions whose signature has one bit of s flipped"""

    def __init__(self, env, eng, n, signers, forged=()):
        torch, bench, edc = env
        self.n, self.forged = n, tuple(forged)
        self.vk, self.sig, self.msg, self.off = bench.make_workload(edc, eng, torch, torch.device("cuda:0"), n, signers,
                                                                    MLEN, 0)
        for i in self.forged:
            self.sig[64 * i + 40] ^= 4
        torch.cuda.synchronize()
        self._host = None

    def host(self):
        """(vks, sigs, msgs) as lists of bytes"""
        if self._host is None:
            n = self.n
            hv, hs = self.vk[:32 * n].cpu().numpy().tobytes(), self.sig[:64 * n].cpu().numpy().tobytes()
            hm = self.msg[:MLEN * n].cpu().numpy().tobytes()
            self._host = ([hv[32 * i:32 * i + 32] for i in range(n)], [hs[64 * i:64 * i + 64] for i in range(n)],
                          [hm[MLEN * i:MLEN * i + MLEN] for i in range(n)])
        return self._host

    def items(self, lo=0, hi=None):
        return list(zip(*(col[lo:hi] for col in self.host())))

    def device(self, eng, lo=0, hi=None, z_base=0):
        """edc_batch_verify_device over items [lo, hi) with z drawn from z_base on: (code, check8).
        Messages have one length, so the first hi - lo + 1 offsets are the range's own."""
        hi = self.n if hi is None else hi
        c8 = ctypes.create_string_buffer(32)
        rc = eng.lib.edc_batch_verify_device(eng.ctx, hi - lo, self.vk.data_ptr() + 32 * lo, self.sig.data_ptr() + 64 * lo,
                                             self.msg.data_ptr() + MLEN * lo, self.off.data_ptr(), SEED, z_base, None, c8)
        return rc, c8.raw


@pytest.fixture(scope="module")
def env(edc):
    torch = pytest.importorskip("torch")
    sys.path.insert(0, ROOT)
    import bench
    return torch, bench, edc


@pytest.fixture(scope="module")
def eng(env):
    e = env[2].Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def work(env, eng):
    cache = {}

    def get(n, signers, forged=()):
        key = (n, signers, tuple(forged))
        if key not in cache:
            cache[key] = Work(env, eng, n, signers, forged)
        return cache[key]
    return get


def _oracle_batch(oracle, w, lo=0, hi=None, z_base=0):
    hi = w.n if hi is None else hi
    return oracle.batch_verify(w.items(lo, hi), oracle.z_values(SEED, hi - lo, z_base))


def _check(got, dev, orc, forged):
    """got / dev: (code, check8) of the site and of the device path; orc: the oracle's (code, check8)"""
    assert tuple(got) == tuple(dev)
    assert got[0] == orc[0] == (1 if forged else 0)
    if orc[1] is not None:
        assert got[1] == orc[1]
    assert (got[1] == IDENTITY) == (not forged) and got[1] != bytes(32)


# ---------------------------------------------------------------- 1. the one-batch path
@pytest.mark.parametrize("n,signers", [(33, 5), (CHUNK + 1, 5), (CHUNK + 1, 0)], ids=["33-grouped", "2049-grouped", "2049-distinct"])
@pytest.mark.parametrize("forge", [False, True], ids=["valid", "forged"])
def test_one_batch(eng, oracle, work, n, signers, forge):
    w = work(n, signers, (n - 2,) if forge else ())
    vks, sigs, msgs = w.host()
    got = eng.batch_verify(vks, sigs, msgs, z_seed=SEED, want_check8=True)        # host form, staged in one piece
    t = eng.lib.edc_batch_submit_device(eng.ctx, n, w.vk.data_ptr(), w.sig.data_ptr(), w.msg.data_ptr(), w.off.data_ptr(),
                                        SEED, 0, None, 1)                          # a pipelined slot
    assert t >= 0, eng.lib.edc_last_error(eng.ctx)
    assert tuple(eng.batch_wait(t, True)) == tuple(got)
    _check(got, w.device(eng), _oracle_batch(oracle, w), forge)


# ---------------------------------------------------------------- 2. the multi launch
def test_multi_launch(eng, oracle, work):
    nb, n_per = 2, CHUNK
    w = work(nb * n_per, 5, (n_per + 77,))                                        # batch 1 holds the wrong signature
    t = eng.batch_submit_multi_device(nb, n_per, w.vk.data_ptr(), w.sig.data_ptr(), w.msg.data_ptr(), w.off.data_ptr(), SEED,
                                      0, want_check8=True)
    rc, verdicts, c8s, _, bad = eng.batch_wait_multi(t, nb)
    assert rc == 1 and verdicts == [0, 1] and bad == [0, 0]
    for b in range(nb):
        lo, hi = b * n_per, (b + 1) * n_per
        _check((verdicts[b], c8s[b]), w.device(eng, lo, hi, z_base=lo), _oracle_batch(oracle, w, lo, hi, z_base=lo), b == 1)


# ---------------------------------------------------------------- 3. the chunked host path
def test_host_chunked(eng, oracle, work):
    n = HOST_CHUNK_MIN
    # the path taken is the chunked one: host buffers, n at its threshold, the A/B switch unset
    assert n >= HOST_CHUNK_MIN and os.environ.get("EDC_HOST_CHUNKS", "1")[0] != "0"
    bad = n - 3                                                                     # in the last chunk
    w = work(n, 150, (bad,))
    hv, hs = w.vk[:32 * n].cpu().numpy().tobytes(), w.sig[:64 * n].cpu().numpy().tobytes()
    hm = w.msg[:MLEN * n].cpu().numpy().tobytes()
    ho = (ctypes.c_uint64 * (n + 1))(*range(0, MLEN * (n + 1), MLEN))
    kb = ctypes.create_string_buffer(32 * n)
    eng._check(eng.lib.edc_challenge(eng.ctx, n, hv, hs, hm, ho, kb))
    dev = w.device(eng)
    item = (hv[32 * bad:32 * bad + 32], hs[64 * bad:64 * bad + 64], hm[MLEN * bad:MLEN * bad + MLEN])
    orc = (1 if oracle.verify(*item) else 0, None)                                  # one rejected item: an invalid batch
    c8 = ctypes.create_string_buffer(32)
    rc = eng.lib.edc_batch_verify(eng.ctx, n, hv, hs, hm, ho, SEED, c8)
    _check((rc, c8.raw), dev, orc, True)
    c8 = ctypes.create_string_buffer(32)
    rc = eng.lib.edc_batch_verify_prehashed(eng.ctx, n, hv, hs, kb.raw, SEED, None, c8)
    _check((rc, c8.raw), dev, orc, True)


# ---------------------------------------------------------------- 4. the grouped fallback
def test_grouped_fallback(env, oracle):
    torch, bench, edc = env
    n, ranges, bits = 2 * CHUNK + 1, 3, 9                                           # ranges of 2,048; the last holds one item
    bad = CHUNK + 500                                                               # in range 1
    e = edc.Engine(0)
    try:
        assert e.lib.edc_set_fallback_shape(e.ctx, ranges, bits) == 0
        w = Work(env, e, n, 5, (bad,))
        codes, cnt, c8 = ctypes.create_string_buffer(n), ctypes.c_int(-1), ctypes.create_string_buffer(32)
        rc = e.lib.edc_batch_verify_fallback_device(e.ctx, n, w.vk.data_ptr(), w.sig.data_ptr(), w.msg.data_ptr(),
                                                    w.off.data_ptr(), SEED, codes, ctypes.byref(cnt), c8)
        dev = w.device(e)
        # the oracle's per-item codes: it rejects item `bad`, accepts the items at the range ends, and
        # its batch equation holds over all the others, so each of them verifies singly
        items = w.items()
        want = [0] * n
        want[bad] = oracle.verify(*items[bad])
        assert want[bad] == 1
        for i in (0, CHUNK - 1, CHUNK, 2 * CHUNK - 1, 2 * CHUNK):
            assert oracle.verify(*items[i]) == 0
        rest = items[:bad] + items[bad + 1:]
        assert oracle.batch_verify_seeded(rest, SEED)[0] == 0
        assert list(codes.raw) == want and cnt.value == 1
        _check((rc, c8.raw), dev, (1, None), True)
    finally:
        e.close()


# ---------------------------------------------------------------- 5. the eager fold
@pytest.mark.parametrize("forge", [False, True], ids=["valid", "forged"])
def test_eager_fold(env, eng, oracle, work, forge):
    edc = env[2]
    calls, per = 3, 64
    w = work(calls * per, 5, (per + 9,) if forge else ())                          # in the second queue call
    vks, sigs, msgs = w.host()
    plain, eager = edc.batch.StreamVerifier(eng), edc.batch.StreamVerifier(eng)
    try:
        eager.set_fold(per)
        eager.begin_eager(SEED)
        for c in range(calls):
            a, b = c * per, (c + 1) * per
            plain.queue_many(vks[a:b], sigs[a:b], msgs=msgs[a:b])
            eager.queue_many(vks[a:b], sigs[a:b], msgs=msgs[a:b])
        got = eager.verify_detailed()
        assert eager.folded[1] >= 1 and eager.folded[0] >= per
        assert tuple(plain.verify_detailed(SEED)) == tuple(got)
        _check(got, w.device(eng), _oracle_batch(oracle, w), forge)
    finally:
        plain.close()
        eager.close()


# ---------------------------------------------------------------- 6. the incremental verify
def test_verifier_verify_plain(env, eng, oracle, work):
    w = work(33, 5)
    vks, sigs, msgs = w.host()
    sv = env[2].batch.StreamVerifier(eng)
    try:
        for a, b in ((0, 20), (20, 33)):
            sv.queue_many(vks[a:b], sigs[a:b], msgs=msgs[a:b])
        got = sv.verify_detailed(SEED)
        assert sv.last_split == 0
        _check(got, w.device(eng), _oracle_batch(oracle, w), False)
    finally:
        sv.close()


def test_verifier_verify_split(env, oracle):
    """with the signers in the key cache the verify takes the split plan (verifier_split holds from
    one queued item on: tests/test_gpu_verifier_keycache.py runs it on the golden batches)"""
    edc = env[2]
    e = edc.Engine(0)
    try:
        w = Work(env, e, 33, 5, (7,))
        vks, sigs, msgs = w.host()
        dev = w.device(e)                                                           # before the cache: the wide plan
        e.keycache_load(list(dict.fromkeys(vks)))
        sv = edc.batch.StreamVerifier(e)
        sv.queue_many(vks[:20], sigs[:20], msgs=msgs[:20])
        sv.queue_many(vks[20:], sigs[20:], msgs=msgs[20:])
        got = sv.verify_detailed(SEED)
        assert sv.last_split == 1
        _check(got, dev, _oracle_batch(oracle, w), True)
        sv.close()
    finally:
        e.close()
