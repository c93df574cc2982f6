"""CPU: the incremental verifier's C ABI and Python surface exist (no compute calls, no GPU)."""
import os
import re

from conftest import ROOT

VERIFIER_SYMBOLS = ["edc_verifier_create", "edc_verifier_destroy", "edc_verifier_queue", "edc_verifier_queue_prehashed",
                    "edc_verifier_queue_device", "edc_verifier_size", "edc_verifier_verify",
                    "edc_verifier_verify_fallback", "edc_verifier_reset"]


def _header_verifier_symbols():
    src = open(os.path.join(ROOT, "include", "edc.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(edc_verifier_[a-z0-9_]+)\s*\(", src)))


def test_header_declares_the_verifier_entries():
    assert _header_verifier_symbols() == sorted(VERIFIER_SYMBOLS)


def test_library_exports_every_verifier_symbol(edc):
    lib = edc.load_library()
    for s in _header_verifier_symbols():
        assert hasattr(lib, s), f"libedc.so does not export {s}"
        assert s in edc.ABI_SYMBOLS


def test_null_verifier_is_an_argument_error(edc):
    """Every entry checks its handle before touching the GPU."""
    lib = edc.load_library()
    assert lib.edc_verifier_create(None, 16) is None
    assert lib.edc_verifier_size(None) == 0
    assert lib.edc_verifier_queue(None, 0, None, None, None, None) == -2
    assert lib.edc_verifier_queue_prehashed(None, 0, None, None, None) == -2
    assert lib.edc_verifier_queue_device(None, 0, None, None, None, None, None) == -2
    assert lib.edc_verifier_verify(None, bytes(32), None, None) == -2
    assert lib.edc_verifier_verify_fallback(None, bytes(32), None, None, None) == -2
    assert lib.edc_verifier_reset(None) == -2
    lib.edc_verifier_destroy(None)


def test_stream_verifier_surface(edc):
    sv = edc.batch.StreamVerifier
    for name in ["queue", "queue_many", "batch_size", "verify", "verify_detailed", "verify_with_fallback", "reset",
                 "close"]:
        assert hasattr(sv, name), name
    assert isinstance(sv.batch_size, property)
    # batch.Verifier keeps its host-list shape beside it
    assert hasattr(edc.batch.Verifier, "queue") and not hasattr(edc.batch.Verifier, "reset")
