"""CPU: the verified-signature cache's C ABI and Python surface (include/edc.h, edc_sigcache_*).
The header declares and the library exports every entry, each is listed in ABI_SYMBOLS, a NULL
context is an argument error everywhere, and the header states what a hit is worth. No compute
calls (no GPU here)."""
import ctypes
import os
import re

from conftest import ROOT

SYMBOLS = ["edc_sigcache_create", "edc_sigcache_clear", "edc_sigcache_advance", "edc_sigcache_stats",
           "edc_sigcache_lookup_device", "edc_sigcache_batch_verify_device", "edc_sigcache_batch_verify",
           "edc_sigcache_batch_verify_fallback_device", "edc_sigcache_verify_each"]


def _header():
    return open(os.path.join(ROOT, "include", "edc.h")).read()


def test_header_library_and_abi_list(edc):
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    declared = set(re.findall(r"\b(edc_[a-z0-9_]+)\s*\(", code))
    lib = edc.load_library()
    for s in SYMBOLS:
        assert s in declared, f"include/edc.h does not declare {s}"
        assert hasattr(lib, s), f"libedc.so does not export {s}"
        assert s in edc.ABI_SYMBOLS
    assert sorted(s for s in declared if s.startswith("edc_sigcache_")) == sorted(SYMBOLS)


def test_null_context_is_an_argument_error(edc):
    lib = edc.load_library()
    buf, seed = ctypes.create_string_buffer(128), bytes(32)
    out6 = (ctypes.c_uint64 * 6)()
    off = (ctypes.c_uint64 * 2)(0, 0)
    miss, cnt = ctypes.c_size_t(0), ctypes.c_int(0)
    assert lib.edc_sigcache_create(None, 1024, 0) == -2
    assert lib.edc_sigcache_clear(None) == -2
    assert lib.edc_sigcache_advance(None) == -2
    assert lib.edc_sigcache_stats(None, out6) == -2
    assert lib.edc_sigcache_lookup_device(None, 0, None, None, None, None) == -2
    assert lib.edc_sigcache_batch_verify_device(None, 0, None, None, None, None, None, seed, buf,
                                                ctypes.byref(miss)) == -2
    assert lib.edc_sigcache_batch_verify(None, 0, b"\0", b"\0", b"\0", off, None, seed, buf, ctypes.byref(miss)) == -2
    assert lib.edc_sigcache_batch_verify(None, 0, b"\0", b"\0", None, None, b"\0", seed, buf, ctypes.byref(miss)) == -2
    assert lib.edc_sigcache_batch_verify_fallback_device(None, 0, None, None, None, None, None, seed, buf,
                                                         ctypes.byref(cnt), buf, ctypes.byref(miss)) == -2
    assert lib.edc_sigcache_verify_each(None, 0, b"\0", b"\0", b"\0", off, None, buf, ctypes.byref(miss)) == -2


def test_python_surface(edc):
    for name in ("sigcache_create", "sigcache_clear", "sigcache_advance", "sigcache_stats", "sigcache_lookup",
                 "batch_verify_cached", "batch_verify_cached_fallback", "verify_each_cached"):
        assert callable(getattr(edc.Engine, name)), name
    assert callable(edc.batch.Verifier.verify_cached)
    assert callable(edc.batch.Item.verify_single_many_cached)
    # z drawn by a caller's RNG object cannot follow the miss list: refused before any engine call
    v = edc.batch.Verifier()
    try:
        v.verify_cached(object())
        raise AssertionError("expected ValueError")
    except ValueError:
        pass


def test_header_states_soundness():
    doc = " ".join(_header().replace("*", " ").split())
    m = re.search(r"Soundness\. A hit means.*?never shared", doc)
    assert m, "include/edc.h: the Soundness paragraph of the verified-signature cache is missing"
    par = m.group(0)
    for phrase in ("byte-identical (vk, sig, k)", "batch whose equation held", "fresh and secret",
                   "would not verify on their own", "caller vouches for k", "per context"):
        assert phrase in par, phrase
    for ref in ("src/batch.rs:127-217", "src/batch.rs:104-107", "src/verification_key.rs:225-258"):
        assert ref in doc, ref
